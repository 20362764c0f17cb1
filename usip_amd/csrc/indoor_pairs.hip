// usip_amd/csrc/indoor_pairs.hip -- indoor descriptor training batches built on the device from recorded frame pairs resident
// in HBM.  Replaces SceneNNDescriptorLoader.__getitem__ in DataLoader workers (csrc/indoor_pairs_math.h has
// the semantics).  Four launches on one stream, no host synchronisation:
//   indoor_tables_kernel  one thread per pair: the sample's mode, the pair's draws -> ONE float64 table for both clouds
//                         (pair_table without height scaling, the mode's scale and shift rules), the outputs R, scale,
//                         shift, and both clouds' frame ids and first FPS indices into the workspace
//   cloud_points_kernel   csrc/cloud_stage.h with IndoorView: one thread per slot of each of the 2P clouds; the anchor's
//                         row is moved by the sample's ICP matrix in float64 before anything else, the positive takes the
//                         transform; threads j < n_sub also write FPS candidate j (the anchor's: the move, rounded)
//   fps_kernel            usip_fps_f32 (csrc/fps.hip) on the candidates, unchanged
//   cloud_nodes_kernel    one thread per node: the anchor's recomputed in float64 from its bank row
// Src = PhiloxIndoorDraws (usip_indoor_pairs_build_f32) or ExplicitIndoorDraws (usip_indoor_pairs_apply_f32); neither makes
// or reads a jitter draw.  Every float is written by exactly one thread.
#include "cloud_stage.h"
#include "indoor_pairs_math.h"

using namespace usip_indoor_pairs;

namespace {

struct Workspace : CloudWorkspace {     // table [P][T_SIZE]
    int32_t* cloud_frame;               // [2P], cloud q = c * P + p
};

template <class Src>
__global__ __launch_bounds__(64) void indoor_tables_kernel(usip_indoor_pairs_recipe r, Src src, IndoorBank bank,
                                                           const int32_t* __restrict__ sample_ids, int P, Workspace w,
                                                           usip_indoor_pairs_out out)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    const int s = bank.sample(sample_ids[p]);
    double* T = w.table + (long long)p * T_SIZE;
    indoor_table(r, bank.mode(r.mode, s), src, p, T);
    for (int c = 0; c < 2; ++c) {
        w.first[c * P + p] = src.first(p, c, r.cloud.n_sub);
        w.cloud_frame[c * P + p] = bank.frame(s, c);
    }
    for (int i = 0; i < 9; ++i) out.R[p * 9 + i] = (float)T[T_RD + i];
    out.scale[p] = (float)T[T_DSCALE];
    for (int k = 0; k < 3; ++k) out.shift[p * 3 + k] = (float)T[T_DSHIFT + k];
}

// parts: 0 tables, 1 candidates, 2 first indices, 3 FPS picks, 4 cloud frame ids, 5 = the total
void workspace_layout(const usip_pairs_recipe& r, int P, char* base, Workspace* w, long long parts[6])
{
    cloud_workspace_layout(r, P, P, base, w, parts);                     // one table per pair
    parts[5] = parts[4] + align256((long long)2 * P * 4);
    if (w) w->cloud_frame = (int32_t*)(base + parts[4]);
}

template <class Src>
int launch(const usip_indoor_pairs_recipe& r, const Src& src, const usip_indoor_pairs_bank& b, const int32_t* sample_ids,
           int P, const usip_indoor_pairs_out& out, void* workspace, hipStream_t stream)
{
    Workspace w;
    long long parts[6];
    workspace_layout(r.cloud, P, (char*)workspace, &w, parts);
    const IndoorBank bank{b.rows, b.offsets, b.pairs, b.icp, b.sample_mode, b.num_frames, b.num_samples};
    USIP_LAUNCH(indoor_tables_kernel<Src>, dim3(usip_ceil_div(P, 64)), dim3(64), 0, stream, r, src, bank, sample_ids, P, w,
                out);
    USIP_LAUNCH_CHECK();
    const IndoorView v{w.table, b.rows, b.offsets, w.cloud_frame, b.icp, sample_ids, b.num_frames, b.num_samples,
                       r.icp_moves_normals};
    const CloudOut o{{out.pc[0], out.pc[1]}, {out.sn[0], out.sn[1]}, {out.node[0], out.node[1]}, out.rows, out.node_slots};
    return cloud_stage_launch(stage_recipe(r), src, v, b.rows, P, o, w, stream);
}

}  // namespace

extern "C" long long usip_indoor_pairs_workspace_bytes(const usip_indoor_pairs_recipe* recipe, int P)
{
    return usip_indoor_pairs_workspace_offset(recipe, P, 5);
}

extern "C" long long usip_indoor_pairs_workspace_offset(const usip_indoor_pairs_recipe* recipe, int P, int part)
{
    if (!indoor_recipe_ok(recipe) || P < 0 || part < 0 || part > 5) return USIP_EINVAL;
    long long parts[6];
    workspace_layout(recipe->cloud, P, nullptr, nullptr, parts);
    return parts[part];
}

extern "C" int usip_indoor_pairs_build_f32(const usip_indoor_pairs_recipe* recipe, const usip_indoor_pairs_bank* bank,
                                           const int32_t* sample_ids, int P, uint64_t seed, uint64_t step,
                                           long long pair_base, const usip_indoor_pairs_out* out, void* workspace,
                                           void* stream)
{
    const int rc = indoor_args_ok(recipe, bank, sample_ids, P, out);
    if (rc != 1) return rc;
    if (!workspace) return USIP_EINVAL;
    const PhiloxIndoorDraws src{{seed, step, pair_base}};
    return launch(*recipe, src, *bank, sample_ids, P, *out, workspace, (hipStream_t)stream);
}

extern "C" int usip_indoor_pairs_apply_f32(const usip_indoor_pairs_recipe* recipe, const usip_indoor_pairs_draws* draws,
                                           const usip_indoor_pairs_bank* bank, const int32_t* sample_ids, int P,
                                           const usip_indoor_pairs_out* out, void* workspace, void* stream)
{
    const int rc = indoor_args_ok(recipe, bank, sample_ids, P, out);
    if (rc != 1) return rc;
    if (!workspace || !indoor_draws_ok(draws)) return USIP_EINVAL;
    const usip_pairs_recipe& c = recipe->cloud;
    const ExplicitIndoorDraws src{{}, ExplicitDraws{draws->cloud, c.N, c.n_sub, c.M, c.Cs}};
    return launch(*recipe, src, *bank, sample_ids, P, *out, workspace, (hipStream_t)stream);
}
