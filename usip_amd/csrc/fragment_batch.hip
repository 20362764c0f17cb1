// usip_amd/csrc/fragment_batch.hip -- evaluation batches built on the device from indoor fragments resident in HBM (SURVEY 8
// f-27).  Replaces RedwoodLoader.__getitem__ and Match3DEvalLoader.__getitem__ (csrc/fragment_batch_math.h has the
// semantics).  Four launches on one stream, no host synchronisation:
//   fragment_clouds_kernel  one thread per cloud of the stage's 2P = 2 ceil(B / 2): its fragment id and first FPS index into
//                           the workspace; thread 0 also writes the one identity table
//   cloud_points_kernel     csrc/cloud_stage.h with FragmentView: one thread per slot of each cloud, a pure gather of the
//                           bank row; threads j < n_sub also write FPS candidate j
//   fps_kernel              usip_fps_f32 (csrc/fps.hip) on the candidates, unchanged
//   cloud_nodes_kernel      one thread per node: the candidate FPS chose
// With B odd the last cloud repeats the last fragment into row B2 - 1 of buffers that hold B2 clouds: nothing is written
// past them.  Src = PhiloxFragmentDraws (usip_fragment_batch_build_f32) or ExplicitFragmentDraws
// (usip_fragment_batch_apply_f32).  Every float is written by exactly one thread.
#include "cloud_stage.h"
#include "fragment_batch_math.h"

using namespace usip_fragment_batch;

namespace {

struct Workspace : CloudWorkspace {     // table [1][T_SIZE]
    int32_t* cloud_frag;                // [2P], cloud q = c * P + p
};

template <class Src>
__global__ __launch_bounds__(64) void fragment_clouds_kernel(usip_pairs_recipe r, Src src, const int32_t* __restrict__ ids,
                                                             int P, int B, int num_fragments, Workspace w)
{
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= 2 * P) return;
    const int c = q / P, p = q - c * P;
    w.cloud_frag[q] = clampi(ids[position(P, B, p, c)], 0, num_fragments - 1);
    w.first[q] = src.first(p, c, r.n_sub);
    if (q == 0) identity_table(w.table);
}

// parts: 0 the table, 1 candidates, 2 first indices, 3 FPS picks, 4 cloud fragment ids, 5 = the total
void workspace_layout(const usip_pairs_recipe& r, int B, char* base, Workspace* w, long long parts[6])
{
    const int P = (B + 1) / 2;
    cloud_workspace_layout(r, P, 1, base, w, parts);                     // one table for all
    parts[5] = parts[4] + align256((long long)2 * P * 4);
    if (w) w->cloud_frag = (int32_t*)(base + parts[4]);
}

template <class Src>
int launch(const usip_pairs_recipe& recipe, const Src& src, const usip_fragment_batch_bank& b, const int32_t* ids, int B,
           const usip_fragment_batch_out& out, void* workspace, hipStream_t stream)
{
    const usip_pairs_recipe r = stage_recipe(recipe);
    const int P = (B + 1) / 2;
    Workspace w;
    long long parts[6];
    workspace_layout(r, B, (char*)workspace, &w, parts);
    USIP_LAUNCH(fragment_clouds_kernel<Src>, dim3(usip_ceil_div(2 * P, 64)), dim3(64), 0, stream, r, src, ids, P, B,
                b.num_fragments, w);
    USIP_LAUNCH_CHECK();
    const FragmentView v{w.table, b.offsets, w.cloud_frag, b.num_fragments};
    const long long half = P;
    const CloudOut o{{out.pc, out.pc + half * 3 * r.N}, {out.sn, out.sn + half * r.Cs * r.N},
                     {out.node, out.node + half * 3 * r.M}, out.rows, out.node_slots};
    return cloud_stage_launch(r, src, v, b.rows, P, o, w, stream);
}

}  // namespace

extern "C" long long usip_fragment_batch_workspace_bytes(const usip_pairs_recipe* recipe, int B)
{
    return usip_fragment_batch_workspace_offset(recipe, B, 5);
}

extern "C" long long usip_fragment_batch_workspace_offset(const usip_pairs_recipe* recipe, int B, int part)
{
    if (!fragment_recipe_ok(recipe) || B < 0 || part < 0 || part > 5) return USIP_EINVAL;
    long long parts[6];
    workspace_layout(*recipe, B, nullptr, nullptr, parts);
    return parts[part];
}

extern "C" int usip_fragment_batch_build_f32(const usip_pairs_recipe* recipe, const usip_fragment_batch_bank* bank,
                                             const int32_t* ids, const int32_t* ids_host, int B, uint64_t seed,
                                             uint64_t step, const usip_fragment_batch_out* out, void* workspace,
                                             void* stream)
{
    const int rc = fragment_args_ok(recipe, bank, ids, ids_host, B, out);
    if (rc != 1) return rc;
    if (!workspace) return USIP_EINVAL;
    PhiloxFragmentDraws src;
    src.s = {seed, step, 0};
    src.ids = ids;
    src.P = (B + 1) / 2;
    src.B = B;
    src.num_fragments = bank->num_fragments;
    return launch(*recipe, src, *bank, ids, B, *out, workspace, (hipStream_t)stream);
}

extern "C" int usip_fragment_batch_apply_f32(const usip_pairs_recipe* recipe, const usip_fragment_batch_draws* draws,
                                             const usip_fragment_batch_bank* bank, const int32_t* ids,
                                             const int32_t* ids_host, int B, const usip_fragment_batch_out* out,
                                             void* workspace, void* stream)
{
    const int rc = fragment_args_ok(recipe, bank, ids, ids_host, B, out);
    if (rc != 1) return rc;
    if (!workspace || !fragment_draws_ok(draws)) return USIP_EINVAL;
    ExplicitFragmentDraws src;
    src.d = *draws;
    src.P = (B + 1) / 2;
    src.B = B;
    src.N = recipe->N;
    src.n_sub = recipe->n_sub;
    return launch(*recipe, src, *bank, ids, B, *out, workspace, (hipStream_t)stream);
}
