// usip_amd/csrc/pairs.hip -- training pairs built on the device from scans resident in HBM.
//
// Replaces the reference's per-pair CPU work in DataLoader workers (KittiLoader / OxfordLoader .__getitem__ with augment
// and transform_pc_pytorch; csrc/pairs_math.h has the semantics).  Four launches on one stream, no host synchronisation:
//   pairs_params_kernel   one thread per pair: the pair's draws -> float64 table (augment rotations, scale, shift, height
//                         scale, the transform's f32 R / scale / shift), the outputs R, scale, shift, and the two first
//                         FPS indices
//   pairs_points_kernel   one thread per slot of each of the 2P clouds: slot -> scan row through the keyed bijection (or
//                         the fix_idx layout), one 32-byte row load, augment + transform, pc [3][N] / sn [Cs][N] written
//                         transposed (coalesced along the slot); threads j < n_sub also write the un-augmented FPS
//                         candidate j [3][n_sub]
//   fps_kernel            usip_fps_f32 (csrc/fps.hip) on the candidates, unchanged
//   pairs_nodes_kernel    one thread per node: the chosen candidate, augment with its own jitter, transform
// Src = PhiloxDraws (usip_pairs_build_f32) or ExplicitDraws (usip_pairs_apply_f32): one arithmetic for both.
#include "common.h"
#include "pairs_math.h"

using namespace usip_pairs;

namespace {

constexpr int PT = 256;

struct Bank {
    const float* rows;
    const int64_t* offsets;
    const int32_t* scan_ids;
    int num_scans;

    __device__ __forceinline__ void scan(int p, long long& o0, long long& n) const
    {
        int s = scan_ids[p];
        s = s < 0 ? 0 : (s >= num_scans ? num_scans - 1 : s);
        o0 = offsets[s];
        n = offsets[s + 1] - o0;
    }
};

template <class Src>
__global__ __launch_bounds__(64) void pairs_params_kernel(usip_pairs_recipe r, Src src, int P, double* __restrict__ table,
                                                          int32_t* __restrict__ first, float* __restrict__ R,
                                                          float* __restrict__ scale, float* __restrict__ shift)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    double u[USIP_PAIRS_NPARAM];
    src.params(p, u);
    double* T = table + (long long)p * T_SIZE;
    pair_table(r, u, T);
    for (int c = 0; c < 2; ++c) first[c * P + p] = src.first(p, c, r.n_sub);
    for (int i = 0; i < 9; ++i) R[p * 9 + i] = (float)T[T_RD + i];
    scale[p] = (float)T[T_DSCALE];
    for (int k = 0; k < 3; ++k) shift[p * 3 + k] = (float)T[T_DSHIFT + k];
}

template <class Src>
__global__ __launch_bounds__(PT) void pairs_points_kernel(usip_pairs_recipe r, Src src, Bank bank, int P,
                                                          const double* __restrict__ table, usip_pairs_out out,
                                                          float* __restrict__ cand_xyz)
{
    const int j = blockIdx.x * PT + threadIdx.x, q = blockIdx.y, c = q / P, p = q - c * P;
    const int N = r.N;
    if (j >= N) return;
    long long o0, n;
    bank.scan(p, o0, n);
    if (n < 1) return;                                   // refused on the host (min_rows)
    const double* T = table + (long long)p * T_SIZE;
    const long long row = src.row(p, c, n, N, j);
    const float* rp = bank.rows + (o0 + row) * r.row_len;
    float xyz[3], s[MAX_CS];
    load_row(r, rp, xyz, s);
    raw_xyz(T, rp, xyz);
    double zp[4] = {0, 0, 0, 0}, zs[MAX_CS];
    for (int k = 0; k < MAX_CS; ++k) zs[k] = 0.0;
    if (r.train) {
        src.jit_pc(p, c, N, j, zp);
        src.jit_sn(p, c, N, r.Cs, j, zs);
    }
    float o[3];
    finish_xyz(r, T, c, xyz, zp, r.pc_sigma, r.pc_clip, true, o);
    finish_sn(r, T, c, s, zs);
    float* pc = out.pc[c] + (long long)p * 3 * N;
    float* sn = out.sn[c] + (long long)p * r.Cs * N;
    for (int k = 0; k < 3; ++k) pc[(long long)k * N + j] = o[k];
    for (int k = 0; k < r.Cs; ++k) sn[(long long)k * N + j] = s[k];
    if (out.rows) out.rows[(long long)q * N + j] = (int32_t)row;
    if (j < r.n_sub) {
        const int slot = src.cand(p, c, N, j);
        const long long crow = src.row(p, c, n, N, slot);
        float cx[3];
        raw_xyz(T, bank.rows + (o0 + crow) * r.row_len, cx);
        float* cd = cand_xyz + (long long)q * 3 * r.n_sub;
        for (int k = 0; k < 3; ++k) cd[(long long)k * r.n_sub + j] = cx[k];
    }
}

template <class Src>
__global__ __launch_bounds__(PT) void pairs_nodes_kernel(usip_pairs_recipe r, Src src, int P, const double* __restrict__ table,
                                                         const float* __restrict__ cand_xyz, const int32_t* __restrict__ fps,
                                                         usip_pairs_out out)
{
    const int m = blockIdx.x * PT + threadIdx.x, q = blockIdx.y, c = q / P, p = q - c * P;
    const int M = r.M, ns = r.n_sub;
    if (m >= M) return;
    const double* T = table + (long long)p * T_SIZE;
    int ci = fps[(long long)q * M + m];
    ci = ci < 0 ? 0 : (ci >= ns ? ns - 1 : ci);
    const float* cd = cand_xyz + (long long)q * 3 * ns;
    const float xyz[3] = {cd[ci], cd[ns + ci], cd[2 * ns + ci]};
    double z[4] = {0, 0, 0, 0};
    if (r.train) src.jit_node(p, c, M, m, z);
    float o[3];
    finish_xyz(r, T, c, xyz, z, r.node_sigma, r.node_clip, false, o);
    float* node = out.node[c] + (long long)p * 3 * M;
    for (int k = 0; k < 3; ++k) node[(long long)k * M + m] = o[k];
    if (out.node_slots) out.node_slots[(long long)q * M + m] = src.cand(p, c, r.N, ci);
}

long long align256(long long b) { return (b + 255) & ~255LL; }

struct Workspace {
    double* table;
    float* cand_xyz;
    int32_t* first;
    int32_t* fps;
};

// parts: 0 table, 1 candidates, 2 first indices, 3 FPS picks, 4 = the total (usip_pairs_workspace_offset)
long long workspace_layout(const usip_pairs_recipe& r, int P, char* base, Workspace* w, long long* parts = nullptr)
{
    long long o = 0;
    const long long t = o; o += align256((long long)P * T_SIZE * 8);
    const long long cx = o; o += align256((long long)2 * P * 3 * r.n_sub * 4);
    const long long fi = o; o += align256((long long)2 * P * 4);
    const long long fp = o; o += align256((long long)2 * P * r.M * 4);
    if (parts) { parts[0] = t; parts[1] = cx; parts[2] = fi; parts[3] = fp; parts[4] = o; }
    if (w) {
        w->table = (double*)(base + t);
        w->cand_xyz = (float*)(base + cx);
        w->first = (int32_t*)(base + fi);
        w->fps = (int32_t*)(base + fp);
    }
    return o;
}

bool out_ok(const usip_pairs_out* o)
{
    return o && o->pc[0] && o->pc[1] && o->sn[0] && o->sn[1] && o->node[0] && o->node[1] && o->R && o->scale && o->shift;
}

template <class Src>
int launch(const usip_pairs_recipe& r, const Src& src, const float* bank, const int64_t* offsets, int num_scans,
           const int32_t* scan_ids, int P, const usip_pairs_out& out, void* workspace, hipStream_t stream)
{
    Workspace w;
    workspace_layout(r, P, (char*)workspace, &w);
    const Bank b{bank, offsets, scan_ids, num_scans};
    USIP_LAUNCH(pairs_params_kernel<Src>, dim3(usip_ceil_div(P, 64)), dim3(64), 0, stream, r, src, P, w.table, w.first,
                out.R, out.scale, out.shift);
    USIP_LAUNCH_CHECK();
    USIP_LAUNCH(pairs_points_kernel<Src>, dim3(usip_ceil_div(r.N, PT), 2 * P), dim3(PT), 0, stream, r, src, b, P, w.table,
                out, w.cand_xyz);
    USIP_LAUNCH_CHECK();
    const int rc = usip_fps_f32(w.cand_xyz, w.first, w.fps, 2 * P, r.n_sub, r.M, stream);
    if (rc != USIP_OK) return rc;
    USIP_LAUNCH(pairs_nodes_kernel<Src>, dim3(usip_ceil_div(r.M, PT), 2 * P), dim3(PT), 0, stream, r, src, P, w.table,
                w.cand_xyz, w.fps, out);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
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
    if (!recipe_ok(recipe) || P < 0) return USIP_EINVAL;
    return workspace_layout(*recipe, P, nullptr, nullptr);
}

extern "C" long long usip_pairs_workspace_offset(const usip_pairs_recipe* recipe, int P, int part)
{
    if (!recipe_ok(recipe) || P < 0 || part < 0 || part > 4) return USIP_EINVAL;
    long long parts[5];
    workspace_layout(*recipe, P, nullptr, nullptr, parts);
    return parts[part];
}

extern "C" int usip_pairs_build_f32(const usip_pairs_recipe* recipe, const float* bank, const int64_t* offsets,
                                    int num_scans, const int32_t* scan_ids, int P, long long min_rows, uint64_t seed,
                                    uint64_t step, long long pair_base, const usip_pairs_out* out, void* workspace,
                                    void* stream)
{
    const int rc = check_args(recipe, bank, offsets, num_scans, scan_ids, P, min_rows, out, workspace);
    if (rc != 1) return rc;
    const PhiloxDraws src{seed, step, pair_base};
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
