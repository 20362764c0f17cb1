// usip_amd/csrc/desc_pairs.hip -- descriptor training batches built on the device from posed scans resident in HBM
// (SURVEY 8 f-8).  Replaces KittiDescriptorLoader.__getitem__ in DataLoader workers and the host-side O(B^2)
// mine_negative_sample (csrc/desc_pairs_math.h has the semantics).  Five launches on one stream, no host synchronisation:
//   desc_select_kernel   one thread per pair: the positive scan by the reference's
//                        narrowing search, both poses, the anchor's sequence, the two clouds' float64 tables and first FPS
//                        indices, every cloud's scan id into the workspace
//   desc_mine_kernel     one thread per anchor (one workgroup): the negative mined from the poses, and the count of rows
//                        without a candidate (an integer summed in LDS, one store)
//   desc_points_kernel   one thread per slot of each of the 2P clouds, the scan id read from the workspace: slot -> scan row
//                        through the keyed bijection, one 32-byte row load, augment, pc [3][N] / sn [Cs][N] written
//                        transposed (coalesced along the slot); threads j < n_sub also write FPS candidate j
//   fps_kernel           usip_fps_f32 (csrc/fps.hip) on the un-augmented candidates, unchanged
//   desc_nodes_kernel    one thread per node: the chosen candidate, augment with its own jitter
// Src = PhiloxDescDraws (usip_desc_pairs_build_f32) or ExplicitDescDraws (usip_desc_pairs_apply_f32): one arithmetic.
#include "common.h"
#include "desc_pairs_math.h"

using namespace usip_desc_pairs;

namespace {

constexpr int PT = 256;

struct Workspace {
    double* table;          // [2P][T_SIZE], cloud q = c * P + p
    float* cand_xyz;
    int32_t* first;
    int32_t* fps;
    int32_t* cloud_scan;    // [2P]
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

template <class Src>
__global__ __launch_bounds__(PT) void desc_points_kernel(usip_pairs_recipe r, Src src, PosedBank bank, int P, Workspace w,
                                                         usip_desc_pairs_out out)
{
    const int j = blockIdx.x * PT + threadIdx.x, q = blockIdx.y, c = q / P, p = q - c * P;
    const int N = r.N;
    if (j >= N) return;
    const int s = bank.scan(w.cloud_scan[q]);
    const long long o0 = bank.offsets[s], n = bank.offsets[s + 1] - o0;
    if (n < N) return;                                   // refused on the host (min_rows)
    if (j < r.n_sub) {
        const int slot = src.cand(p, c, N, j);
        const long long crow = src.row(p, c, n, N, slot);
        const float* cp = bank.rows + (o0 + crow) * r.row_len;
        float* cd = w.cand_xyz + (long long)q * 3 * r.n_sub;
        for (int k = 0; k < 3; ++k) cd[(long long)k * r.n_sub + j] = cp[k];
    }
    const double* T = w.table + (long long)q * T_SIZE;
    const long long row = src.row(p, c, n, N, j);
    const float* rp = bank.rows + (o0 + row) * r.row_len;
    float xyz[3], sv[MAX_CS];
    load_row(r, rp, xyz, sv);
    double zp[4] = {0, 0, 0, 0}, zs[MAX_CS];
    for (int k = 0; k < MAX_CS; ++k) zs[k] = 0.0;
    if (r.train) {
        src.jit_pc(p, c, N, j, zp);
        src.jit_sn(p, c, N, r.Cs, j, zs);
    }
    float o[3];
    finish_xyz(r, T, 0, xyz, zp, r.pc_sigma, r.pc_clip, true, o);
    finish_sn(r, T, 0, sv, zs);
    float* pc = out.pc[c] + (long long)p * 3 * N;
    float* sn = out.sn[c] + (long long)p * r.Cs * N;
    for (int k = 0; k < 3; ++k) pc[(long long)k * N + j] = o[k];
    for (int k = 0; k < r.Cs; ++k) sn[(long long)k * N + j] = sv[k];
    if (out.rows) out.rows[(long long)q * N + j] = (int32_t)row;
}

template <class Src>
__global__ __launch_bounds__(PT) void desc_nodes_kernel(usip_pairs_recipe r, Src src, int P, Workspace w,
                                                        usip_desc_pairs_out out)
{
    const int m = blockIdx.x * PT + threadIdx.x, q = blockIdx.y, c = q / P, p = q - c * P;
    const int M = r.M, ns = r.n_sub;
    if (m >= M) return;
    const double* T = w.table + (long long)q * T_SIZE;
    const int ci = clampi(w.fps[(long long)q * M + m], 0, ns - 1);
    const float* cd = w.cand_xyz + (long long)q * 3 * ns;
    const float xyz[3] = {cd[ci], cd[ns + ci], cd[2 * ns + ci]};
    double z[4] = {0, 0, 0, 0};
    if (r.train) src.jit_node(p, c, M, m, z);
    float o[3];
    finish_xyz(r, T, 0, xyz, z, r.node_sigma, r.node_clip, false, o);
    float* node = out.node[c] + (long long)p * 3 * M;
    for (int k = 0; k < 3; ++k) node[(long long)k * M + m] = o[k];
    if (out.node_slots) out.node_slots[(long long)q * M + m] = src.cand(p, c, r.N, ci);
}

long long align256(long long b) { return (b + 255) & ~255LL; }

// parts: 0 tables, 1 candidates, 2 first indices, 3 FPS picks, 4 cloud scan ids, 5 = the total
long long workspace_layout(const usip_pairs_recipe& r, int P, char* base, Workspace* w, long long* parts = nullptr)
{
    long long o = 0;
    const long long t = o; o += align256((long long)2 * P * T_SIZE * 8);
    const long long cx = o; o += align256((long long)2 * P * 3 * r.n_sub * 4);
    const long long fi = o; o += align256((long long)2 * P * 4);
    const long long fp = o; o += align256((long long)2 * P * r.M * 4);
    const long long cs = o; o += align256((long long)2 * P * 4);
    if (parts) { parts[0] = t; parts[1] = cx; parts[2] = fi; parts[3] = fp; parts[4] = cs; parts[5] = o; }
    if (w) {
        w->table = (double*)(base + t);
        w->cand_xyz = (float*)(base + cx);
        w->first = (int32_t*)(base + fi);
        w->fps = (int32_t*)(base + fp);
        w->cloud_scan = (int32_t*)(base + cs);
    }
    return o;
}

template <class Src>
int launch(const usip_desc_pairs_recipe& r, const Src& src, const usip_desc_pairs_bank& b, const int32_t* scan_ids, int P,
           const usip_desc_pairs_out& out, void* workspace, hipStream_t stream)
{
    Workspace w;
    workspace_layout(r.cloud, P, (char*)workspace, &w);
    const PosedBank bank{b.rows, b.offsets, b.poses, b.seq_of, b.seq_start, b.num_scans, b.num_seq};
    const usip_pairs_recipe& c = r.cloud;
    USIP_LAUNCH(desc_select_kernel<Src>, dim3(usip_ceil_div(P, 64)), dim3(64), 0, stream, r, src, bank, scan_ids, P, w, out);
    USIP_LAUNCH_CHECK();
    if (r.mine) {
        USIP_LAUNCH(desc_mine_kernel<Src>, dim3(1), dim3(PT), 0, stream, r.negative_radius, src, bank, scan_ids, P,
                    out.neg_idx, out.neg_fail);
        USIP_LAUNCH_CHECK();
    }
    USIP_LAUNCH(desc_points_kernel<Src>, dim3(usip_ceil_div(c.N, PT), 2 * P), dim3(PT), 0, stream, c, src, bank, P, w, out);
    USIP_LAUNCH_CHECK();
    const int rc = usip_fps_f32(w.cand_xyz, w.first, w.fps, 2 * P, c.n_sub, c.M, stream);
    if (rc != USIP_OK) return rc;
    USIP_LAUNCH(desc_nodes_kernel<Src>, dim3(usip_ceil_div(c.M, PT), 2 * P), dim3(PT), 0, stream, c, src, P, w, out);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

}  // namespace

extern "C" long long usip_desc_pairs_workspace_bytes(const usip_desc_pairs_recipe* recipe, int P)
{
    if (!desc_recipe_ok(recipe) || P < 0) return USIP_EINVAL;
    return workspace_layout(recipe->cloud, P, nullptr, nullptr);
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
    const PhiloxDescDraws src{seed, step, pair_base};
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
