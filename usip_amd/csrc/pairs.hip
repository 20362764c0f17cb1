// usip_amd/csrc/pairs.hip -- training pairs built on the device from scans resident in HBM.
//
// Replaces the reference's per-pair CPU work in DataLoader workers (KittiLoader / OxfordLoader .__getitem__ with augment
// and transform_pc_pytorch; csrc/pairs_math.h has the semantics).  Four launches on one stream, no host synchronisation:
//   pairs_params_kernel   one thread per pair: the pair's draws -> float64 table (augment rotations, scale, shift, height
//                         scale, the transform's f32 R / scale / shift), the outputs R, scale, shift, and the two first
//                         FPS indices
//   cloud_points_kernel   csrc/cloud_stage.h with PairView: one thread per slot of each of the 2P clouds, pc [3][N] /
//                         sn [Cs][N] written transposed (coalesced along the slot); threads j < n_sub also write the
//                         un-augmented FPS candidate j [3][n_sub]
//   fps_kernel            usip_fps_f32 (csrc/fps.hip) on the candidates, unchanged
//   cloud_nodes_kernel    one thread per node: the chosen candidate, augment with its own jitter, transform
// Src = PhiloxDraws (usip_pairs_build_f32) or ExplicitDraws (usip_pairs_apply_f32): one arithmetic for both.
#include "cloud_stage.h"

using namespace usip_pairs;

namespace {

template <class Src>
__global__ __launch_bounds__(64) void pairs_params_kernel(usip_pairs_recipe r, Src src, int P, double* __restrict__ table,
                                                          int32_t* __restrict__ first, float* __restrict__ R,
                                                          float* __restrict__ scale, float* __restrict__ shift)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    double* T = table + (long long)p * T_SIZE;
    pair_table(r, src, p, T);
    for (int c = 0; c < 2; ++c) first[c * P + p] = src.first(p, c, r.n_sub);
    for (int i = 0; i < 9; ++i) R[p * 9 + i] = (float)T[T_RD + i];
    scale[p] = (float)T[T_DSCALE];
    for (int k = 0; k < 3; ++k) shift[p * 3 + k] = (float)T[T_DSHIFT + k];
}

bool out_ok(const usip_pairs_out* o)
{
    return o && o->pc[0] && o->pc[1] && o->sn[0] && o->sn[1] && o->node[0] && o->node[1] && o->R && o->scale && o->shift;
}

template <class Src>
int launch(const usip_pairs_recipe& r, const Src& src, const float* bank, const int64_t* offsets, int num_scans,
           const int32_t* scan_ids, int P, const usip_pairs_out& out, void* workspace, hipStream_t stream)
{
    CloudWorkspace w;
    long long parts[5];
    cloud_workspace_layout(r, P, P, (char*)workspace, &w, parts);          // one table per pair
    USIP_LAUNCH(pairs_params_kernel<Src>, dim3(usip_ceil_div(P, 64)), dim3(64), 0, stream, r, src, P, w.table, w.first,
                out.R, out.scale, out.shift);
    USIP_LAUNCH_CHECK();
    const PairView v{w.table, offsets, scan_ids, num_scans};
    const CloudOut o{{out.pc[0], out.pc[1]}, {out.sn[0], out.sn[1]}, {out.node[0], out.node[1]}, out.rows, out.node_slots};
    return cloud_stage_launch(r, src, v, bank, P, o, w, stream);
}

int check_args(const usip_pairs_recipe* r, const float* bank, const int64_t* offsets, int num_scans,
               const int32_t* scan_ids, int P, long long min_rows, const usip_pairs_out* out, void* workspace)
{
    if (!recipe_ok(r) || P < 0 || num_scans < 1) return USIP_EINVAL;
    if (min_rows < 1 || (r->require_full && min_rows < r->N)) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!bank || !offsets || !scan_ids || !workspace || !out_ok(out)) return USIP_EINVAL;
    return 1;
}

}  // namespace

extern "C" long long usip_pairs_workspace_bytes(const usip_pairs_recipe* recipe, int P)
{
    return usip_pairs_workspace_offset(recipe, P, 4);
}

extern "C" long long usip_pairs_workspace_offset(const usip_pairs_recipe* recipe, int P, int part)
{
    if (!recipe_ok(recipe) || P < 0 || part < 0 || part > 4) return USIP_EINVAL;
    long long parts[5];             // 0 table, 1 candidates, 2 first indices, 3 FPS picks, 4 = the total
    cloud_workspace_layout(*recipe, P, P, nullptr, nullptr, parts);
    return parts[part];
}

extern "C" int usip_pairs_build_f32(const usip_pairs_recipe* recipe, const float* bank, const int64_t* offsets,
                                    int num_scans, const int32_t* scan_ids, int P, long long min_rows, uint64_t seed,
                                    uint64_t step, long long pair_base, const usip_pairs_out* out, void* workspace,
                                    void* stream)
{
    const int rc = check_args(recipe, bank, offsets, num_scans, scan_ids, P, min_rows, out, workspace);
    if (rc != 1) return rc;
    const PhiloxDraws src{{seed, step, pair_base}};
    return launch(*recipe, src, bank, offsets, num_scans, scan_ids, P, *out, workspace, (hipStream_t)stream);
}

extern "C" int usip_pairs_apply_f32(const usip_pairs_recipe* recipe, const usip_pairs_draws* draws, const float* bank,
                                    const int64_t* offsets, int num_scans, const int32_t* scan_ids, int P,
                                    long long min_rows, const usip_pairs_out* out, void* workspace, void* stream)
{
    const int rc = check_args(recipe, bank, offsets, num_scans, scan_ids, P, min_rows, out, workspace);
    if (rc != 1) return rc;
    if (!draws || !draws->rows || !draws->cand || !draws->first || !draws->params ||
        (recipe->train && (!draws->jit_pc || !draws->jit_sn || !draws->jit_node)))
        return USIP_EINVAL;
    const ExplicitDraws src{*draws, recipe->N, recipe->n_sub, recipe->M, recipe->Cs};
    return launch(*recipe, src, bank, offsets, num_scans, scan_ids, P, *out, workspace, (hipStream_t)stream);
}
