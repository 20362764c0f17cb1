// usip_amd/csrc/desc_pairs.hip -- descriptor training batches built on the device from posed scans resident in HBM
// (SURVEY 8 f-8).  Replaces KittiDescriptorLoader.__getitem__ in DataLoader workers and the host-side O(B^2)
// mine_negative_sample (csrc/desc_pairs_math.h has the semantics).  Five launches on one stream, no host synchronisation:
//   desc_select_kernel   one thread per pair: the positive scan by the reference's
//                        narrowing search, both poses, the anchor's sequence, the two clouds' float64 tables and first FPS
//                        indices, every cloud's scan id into the workspace
//   desc_mine_kernel     one thread per anchor (one workgroup): the negative mined from the poses, and the count of rows
//                        without a candidate (an integer summed in LDS, one store)
//   cloud_points_kernel  csrc/cloud_stage.h with CloudView (the scan id read from the workspace, a table per cloud, no
//                        transform): one thread per slot of each of the 2P clouds, pc [3][N] / sn [Cs][N] written
//                        transposed (coalesced along the slot); threads j < n_sub also write FPS candidate j
//   fps_kernel           usip_fps_f32 (csrc/fps.hip) on the un-augmented candidates, unchanged
//   cloud_nodes_kernel   one thread per node: the chosen candidate, augment with its own jitter
// Src = PhiloxDescDraws (usip_desc_pairs_build_f32) or ExplicitDescDraws (usip_desc_pairs_apply_f32): one arithmetic.
#include "cloud_stage.h"
#include "desc_pairs_math.h"

using namespace usip_desc_pairs;

namespace {

struct Workspace : CloudWorkspace {     // table [2P][T_SIZE], cloud q = c * P + p
    int32_t* cloud_scan;                // [2P]
};

template <class Src>
__global__ __launch_bounds__(64) void desc_select_kernel(usip_desc_pairs_recipe r, Src src, PosedBank bank,
                                                         const int32_t* __restrict__ scan_ids, int P, Workspace w,
                                                         usip_desc_pairs_out out)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    {
        const int a = bank.scan(scan_ids[p]);
        const int pos = select_positive(bank, r.positive_radius, src, p, a);
        w.cloud_scan[p] = a;
        w.cloud_scan[P + p] = pos;
        out.pos_id[p] = pos;
        out.anc_seq[p] = bank.seq(a);
        for (int i = 0; i < 16; ++i) {
            out.anc_pose[p * 16 + i] = (float)bank.poses[(long long)a * 16 + i];
            out.pos_pose[p * 16 + i] = (float)bank.poses[(long long)pos * 16 + i];
        }
        const double us = src.scale_u(p);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            double u[CLOUD_U];
            src.cloud_params(p, c, u);
            cloud_table(r.cloud, us, u, w.table + (long long)(c * P + p) * T_SIZE);
            w.first[c * P + p] = src.first(p, c, r.cloud.n_sub);
        }
    }
}

template <class Src>
__global__ __launch_bounds__(PT) void desc_mine_kernel(double thr, Src src, PosedBank bank,
                                                       const int32_t* __restrict__ scan_ids, int P,
                                                       int64_t* __restrict__ neg_idx, int32_t* __restrict__ neg_fail)
{
    __shared__ int fails;
    if (threadIdx.x == 0) fails = 0;
    __syncthreads();
    int my_fails = 0;
    for (int p = threadIdx.x; p < P; p += PT) {
        int fail;
        neg_idx[p] = mine_negative(bank, thr, src, scan_ids, P, p, fail);
        my_fails += fail;
    }
    if (my_fails) atomicAdd(&fails, my_fails);              // an integer in LDS
    __syncthreads();
    if (threadIdx.x == 0) neg_fail[0] = fails;
}

// parts: 0 tables, 1 candidates, 2 first indices, 3 FPS picks, 4 cloud scan ids, 5 = the total
void workspace_layout(const usip_pairs_recipe& r, int P, char* base, Workspace* w, long long parts[6])
{
    cloud_workspace_layout(r, P, 2 * P, base, w, parts);                 // one table per cloud
    parts[5] = parts[4] + align256((long long)2 * P * 4);
    if (w) w->cloud_scan = (int32_t*)(base + parts[4]);
}

template <class Src>
int launch(const usip_desc_pairs_recipe& r, const Src& src, const usip_desc_pairs_bank& b, const int32_t* scan_ids, int P,
           const usip_desc_pairs_out& out, void* workspace, hipStream_t stream)
{
    Workspace w;
    long long parts[6];
    workspace_layout(r.cloud, P, (char*)workspace, &w, parts);
    const PosedBank bank{b.rows, b.offsets, b.poses, b.seq_of, b.seq_start, b.num_scans, b.num_seq};
    USIP_LAUNCH(desc_select_kernel<Src>, dim3(usip_ceil_div(P, 64)), dim3(64), 0, stream, r, src, bank, scan_ids, P, w, out);
    USIP_LAUNCH_CHECK();
    if (r.mine) {
        USIP_LAUNCH(desc_mine_kernel<Src>, dim3(1), dim3(PT), 0, stream, r.negative_radius, src, bank, scan_ids, P,
                    out.neg_idx, out.neg_fail);
        USIP_LAUNCH_CHECK();
    }
    const CloudView v{w.table, b.offsets, w.cloud_scan, b.num_scans};
    const CloudOut o{{out.pc[0], out.pc[1]}, {out.sn[0], out.sn[1]}, {out.node[0], out.node[1]}, out.rows, out.node_slots};
    return cloud_stage_launch(r.cloud, src, v, b.rows, P, o, w, stream);
}

}  // namespace

extern "C" long long usip_desc_pairs_workspace_bytes(const usip_desc_pairs_recipe* recipe, int P)
{
    return usip_desc_pairs_workspace_offset(recipe, P, 5);
}

extern "C" long long usip_desc_pairs_workspace_offset(const usip_desc_pairs_recipe* recipe, int P, int part)
{
    if (!desc_recipe_ok(recipe) || P < 0 || part < 0 || part > 5) return USIP_EINVAL;
    long long parts[6];
    workspace_layout(recipe->cloud, P, nullptr, nullptr, parts);
    return parts[part];
}

extern "C" int usip_desc_pairs_build_f32(const usip_desc_pairs_recipe* recipe, const usip_desc_pairs_bank* bank,
                                         const int32_t* scan_ids, int P, uint64_t seed, uint64_t step, long long pair_base,
                                         const usip_desc_pairs_out* out, void* workspace, void* stream)
{
    const int rc = desc_args_ok(recipe, bank, scan_ids, P, out);
    if (rc != 1) return rc;
    if (!workspace) return USIP_EINVAL;
    const PhiloxDescDraws src{{seed, step, pair_base}};
    return launch(*recipe, src, *bank, scan_ids, P, *out, workspace, (hipStream_t)stream);
}

extern "C" int usip_desc_pairs_apply_f32(const usip_desc_pairs_recipe* recipe, const usip_desc_pairs_draws* draws,
                                         const usip_desc_pairs_bank* bank, const int32_t* scan_ids, int P,
                                         const usip_desc_pairs_out* out, void* workspace, void* stream)
{
    const int rc = desc_args_ok(recipe, bank, scan_ids, P, out);
    if (rc != 1) return rc;
    if (!workspace || !desc_draws_ok(recipe, draws)) return USIP_EINVAL;
    const usip_pairs_recipe& c = recipe->cloud;
    const ExplicitDescDraws src{ExplicitDraws{draws->cloud, c.N, c.n_sub, c.M, c.Cs}, draws->params, draws->tries,
                                draws->neg_pick, draws->T};
    return launch(*recipe, src, *bank, scan_ids, P, *out, workspace, (hipStream_t)stream);
}
