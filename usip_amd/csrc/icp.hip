// usip_amd/csrc/icp.hip -- trimmed point-to-point ICP between downsampled fragments on the device: the
// refinement of the reference's second log writer (evaluation/matlab/eval_indoor/3dmatch/writeLogReconputeAlign.m), batched
// over pairs.  csrc/icp_math.h has the decisions, which the host twin (csrc/icp_cpu.cpp) shares; include/usip_hip.h (f-13)
// is the contract.  The loop is a fixed sequence of launches: every workgroup first reads its pair's state in device
// memory and leaves when the pair has stopped, the fit kernel writes that state, the host never reads it.  No launch
// synchronises, no floating-point atomics, every index read from memory is clamped.
//
//   icp_init_kernel      one lane per pair: the start pose, the state, zeros in every output.
//   icp_nearest_kernel   the exact nearest row of fragment 1 for every moved row of fragment 2.  A workgroup owns 256
//                        queries, one per lane; fragment 1's rows, sorted along x, are staged in LDS as float64 in tiles of
//                        256 with their row indices and walked outward in both directions from the tile at the queries'
//                        smallest x.  A direction ends at the tile no lane needs: a lane needs a tile unless the tile's
//                        nearest x is farther from the lane's own x than the lane's best (icp_math.h bound_met()).
//   icp_trim_kernel      one workgroup per pair: the m-th smallest d2 by a radix select over the 64-bit patterns, eight
//                        digits of eight bits, the histogram in LDS (integer atomics); then the rank among equal values
//                        by a ballot scan in ascending row order.  The cut (d2*, i*), not a list.
//   icp_fit_kernel       one workgroup per pair: two lane-strided passes over the kept rows (centroids, then B[10]), the
//                        tree; every lane solves (8 Jacobi sweeps) and lane 0 advances the pose, the histories, the state.
//   icp_final_kernel     one workgroup per pair: the hits within the radius, the root mean kept d2.
// Under the point-to-plane metric the same sequence launches csrc/icp_plane.hip's icp_fit_plane_kernel in
// icp_fit_kernel's place; csrc/icp_state.h is what the two files share.
#include <vector>
#include "icp_state.h"
#include "tile_walk.h"

using namespace usip_reg;
using namespace usip_frag;
using namespace usip_icp;
using namespace usip_bank;
using usip_walk::block_minmax;
using usip_walk::walk_outward;

namespace {

static_assert(LANES == usip_walk::WALK_TILE && TILE == usip_walk::WALK_TILE, "icp_nearest_kernel walks tile_walk.h's tiles");
constexpr int WAVES = usip_walk::WALK_WAVES;

// the bank and, per fragment at its offset, the local row indices ascending along x
struct SortedBank : Bank {
    const int32_t* perm1;
};

// Exclusive scan of one flag per lane over the workgroup; the caller puts a barrier between two calls.
__device__ __forceinline__ int block_scan(bool flag, int* wave_tot, int* total)
{
    const unsigned long long mask = __ballot(flag);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wave_tot[w] = __popcll(mask);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) {
        const int c = wave_tot[k];
        before += k < w ? c : 0;
        all += c;
    }
    *total = all;
    return before + usip_mbcnt(mask);
}

__global__ __launch_bounds__(64) void icp_init_kernel(Bank bank, Pairs pr, const double* __restrict__ Rt0,
                                                      const uint8_t* __restrict__ mask, int P, double* __restrict__ Rt,
                                                      int32_t* __restrict__ state, double* __restrict__ hist,
                                                      int32_t* __restrict__ iterations, uint8_t* __restrict__ converged,
                                                      double* __restrict__ rmse, int32_t* __restrict__ hits,
                                                      double* __restrict__ ratio)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    const int n1 = range_of(bank, pr.frag1, p, pr.Lmax).n, n2 = range_of(bank, pr.frag2, p, pr.Lmax).n;
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[(long long)p * 12 + k] = Rt0[(long long)p * 12 + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) hist[(long long)p * 6 + k] = 0.0;
    state[p] = (mask && mask[p] == 0) || n1 < 1 || n2 < 1 ? NOT_REFINED : RUNNING;
    iterations[p] = 0;
    converged[p] = 0;
    rmse[p] = 0.0;
    hits[p] = 0;
    ratio[2 * p] = 0.0;
    ratio[2 * p + 1] = 0.0;
}

// state NULL: every pair with mask[p] != 0 (mask NULL: every pair); otherwise the running pairs, or, in the final pass,
// the refined ones.
__global__ __launch_bounds__(LANES) void icp_nearest_kernel(SortedBank bank, Pairs pr, const double* __restrict__ Rt_all,
                                                            const uint8_t* __restrict__ mask,
                                                            const int32_t* __restrict__ order2,
                                                            const int32_t* __restrict__ state, int final_pass,
                                                            int32_t* __restrict__ idx, double* __restrict__ d2out,
                                                            unsigned long long* __restrict__ visits)
{
    __shared__ double tile[2][3][TILE];
    __shared__ int trow[2][TILE];
    __shared__ double sRt[12];
    __shared__ double slots[WAVES];
    const int p = blockIdx.y, l = threadIdx.x;
    if (state) {
        const int st = state[p];
        if (final_pass ? st == NOT_REFINED : st != RUNNING) return;    // workgroup-uniform, here and below
    } else if (mask && mask[p] == 0) {
        return;
    }
    const Range r1 = range_of(bank, pr.frag1, p, pr.Lmax), r2 = range_of(bank, pr.frag2, p, pr.Lmax);
    const int n1 = r1.n, n2 = r2.n;
    if ((int)blockIdx.x * TILE >= n2 || n1 < 1) return;
    if (l < 12) sRt[l] = Rt_all[(long long)p * 12 + l];
    __syncthreads();
    double Rt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = sRt[k];
    const int row_len = bank.row_len;
    const float* rows1 = bank.rows + r1.first * row_len;
    const int32_t* perm = bank.perm1 + r1.first;

    const int s = blockIdx.x * TILE + l;
    const bool live = s < n2;
    const int i = live ? (order2 ? clamp_index(order2[(long long)p * pr.Lmax + s], n2) : s) : 0;
    const float* b = bank.rows + (r2.first + i) * row_len;
    const double b0 = (double)b[0], b1 = (double)b[1], b2 = (double)b[2];
    const double qx = xform(Rt, 0, b0, b1, b2), qy = xform(Rt, 1, b0, b1, b2), qz = xform(Rt, 2, b0, b1, b2);
    const double inf = (double)__builtin_inff();
    double xlo = live ? qx : inf, unused = 0.0;
    block_minmax<true, false>(xlo, unused, slots);

    const auto x_at = [&](int at) { return (double)rows1[(long long)safe_index(perm[at], n1) * row_len]; };
    const usip_walk::Tiles<decltype(x_at)> tiles(n1, x_at);
    const int start = tiles.start(xlo);
    double best = inf;
    int brow = 0x7fffffff;
    unsigned long long evaluated = 0;
    bool need[2];
    walk_outward(
        tiles, start - 1, start,
        [&](int left, int right) {
            need[0] = left >= 0 && live && !bound_met(qx - tiles.near_x(0, left), best);
            need[1] = right < tiles.tiles && live && !bound_met(tiles.near_x(1, right) - qx, best);
            const int end_left = __syncthreads_or(need[0]) ? 0 : usip_walk::END_LEFT;  // (also: every lane is done with the tiles)
            return end_left | (__syncthreads_or(need[1]) ? 0 : usip_walk::END_RIGHT);
        },
        [&](int side, int t) {
            const int row = safe_index(perm[min(t * TILE + l, n1 - 1)], n1);
            const float* a = rows1 + (long long)row * row_len;
            tile[side][0][l] = (double)a[0];
            tile[side][1][l] = (double)a[1];
            tile[side][2][l] = (double)a[2];
            trow[side][l] = row;
        },
        [&](int side, int, int m) {
            if (!need[side]) return;
            evaluated += (unsigned long long)m;
            for (int c = 0; c < m; ++c) {
                const double d2 = sqdist3(qx, qy, qz, tile[side][0][c], tile[side][1][c], tile[side][2][c]);
                const int row = trow[side][c];
                if (better(d2, row, best, brow)) { best = d2; brow = row; }
            }
        });
    if (live) {
        idx[(long long)p * pr.Lmax + i] = brow;
        d2out[(long long)p * pr.Lmax + i] = best;
    }
    if (visits) {                                                      // integers: the order of the additions is free
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) evaluated += __shfl_xor(evaluated, off);
        if ((l & 63) == 0 && evaluated) atomicAdd(&visits[p], evaluated);
    }
}

__global__ __launch_bounds__(LANES) void icp_trim_kernel(Bank bank, Pairs pr, const int32_t* __restrict__ state,
                                                         int final_pass, double inlier_ratio,
                                                         const unsigned long long* __restrict__ d2bits,
                                                         unsigned long long* __restrict__ cut_bits,
                                                         int32_t* __restrict__ cut_i, double* __restrict__ cut_d2_out,
                                                         int32_t* __restrict__ cut_i_out, int slot, int slots)
{
    __shared__ unsigned hist[256];
    __shared__ int s_wave[WAVES];
    __shared__ int s_i;
    const int p = blockIdx.x, l = threadIdx.x;
    const int st = state[p];
    if (final_pass ? st == NOT_REFINED : st != RUNNING) return;
    const int n2 = range_of(bank, pr.frag2, p, pr.Lmax).n;             // >= 1: the state says so
    const unsigned long long* v = d2bits + (long long)p * pr.Lmax;
    unsigned long long prefix = 0;
    int remaining = trim_count(inlier_ratio, n2);
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        hist[l] = 0;
        __syncthreads();
        for (int i = l; i < n2; i += LANES) {
            const unsigned long long b = v[i];
            if (pass == 0 || (b >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(unsigned)(b >> shift) & 255u], 1u);
        }
        __syncthreads();
        unsigned digit = 255;
        for (unsigned d = 0; d < 256; ++d) {                           // every lane walks the same counts
            const int c = (int)hist[d];
            if (remaining <= c) { digit = d; break; }
            remaining -= c;
        }
        prefix |= (unsigned long long)digit << shift;
        __syncthreads();
    }
    // `remaining` is now the rank of the cut among the rows at exactly d2*, in ascending row order
    if (l == 0) s_i = n2 - 1;
    int seen = 0;
    for (int base = 0; base < n2; base += LANES) {
        const int i = base + l;
        const bool eq = i < n2 && v[i] == prefix;
        int total;
        const int at = seen + block_scan(eq, s_wave, &total);
        if (eq && at == remaining - 1) s_i = i;
        seen += total;
        __syncthreads();
        if (seen >= remaining) break;
    }
    if (l == 0) {
        cut_bits[p] = prefix;
        cut_i[p] = s_i;
        if (cut_d2_out) {
            cut_d2_out[(long long)p * slots + slot] = double_of(prefix);
            cut_i_out[(long long)p * slots + slot] = s_i;
        }
    }
}

__global__ __launch_bounds__(LANES) void icp_fit_kernel(Bank bank, Pairs pr, const int32_t* __restrict__ idx,
                                                        const unsigned long long* __restrict__ d2bits,
                                                        const unsigned long long* __restrict__ cut_bits,
                                                        const int32_t* __restrict__ cut_i, double inlier_ratio,
                                                        double tol_t, double tol_c, int32_t* __restrict__ state,
                                                        double* __restrict__ Rt_all, double* __restrict__ hist_all,
                                                        int32_t* __restrict__ iterations, uint8_t* __restrict__ converged)
{
    __shared__ double part[LANES][10];
    const int p = blockIdx.x, l = threadIdx.x;
    if (state[p] != RUNNING) return;
    const Range r1 = range_of(bank, pr.frag1, p, pr.Lmax), r2 = range_of(bank, pr.frag2, p, pr.Lmax);
    const int n1 = r1.n, n2 = r2.n, row_len = bank.row_len;
    const double m = (double)trim_count(inlier_ratio, n2);
    const unsigned long long cut = cut_bits[p];
    const int icut = cut_i[p];
    const unsigned long long* v = d2bits + (long long)p * pr.Lmax;
    const int32_t* nn = idx + (long long)p * pr.Lmax;
    const float* rows1 = bank.rows + r1.first * row_len;
    const float* rows2 = bank.rows + r2.first * row_len;

    double s[6] = {0, 0, 0, 0, 0, 0};
    for (int i = l; i < n2; i += LANES)
        if (kept(v[i], i, cut, icut)) {
            const float* a = rows1 + (long long)clamp_index(nn[i], n1) * row_len;
            const float* b = rows2 + (long long)i * row_len;
#pragma unroll
            for (int k = 0; k < 3; ++k) { s[k] += (double)a[k]; s[3 + k] += (double)b[k]; }
        }
#pragma unroll
    for (int k = 0; k < 10; ++k) part[l][k] = k < 6 ? s[k] : 0.0;
    tree_sum<6>(part, l);
    double ca[3], cb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ca[k] = part[0][k] / m; cb[k] = part[0][3 + k] / m; }
    __syncthreads();

    double B[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = l; i < n2; i += LANES)
        if (kept(v[i], i, cut, icut)) {
            const float* a = rows1 + (long long)clamp_index(nn[i], n1) * row_len;
            const float* b = rows2 + (long long)i * row_len;
            const double x[3] = {(double)a[0] - ca[0], (double)a[1] - ca[1], (double)a[2] - ca[2]};
            const double y[3] = {(double)b[0] - cb[0], (double)b[1] - cb[1], (double)b[2] - cb[2]};
            accumulate(B, x, y);
        }
#pragma unroll
    for (int k = 0; k < 10; ++k) part[l][k] = B[k];
    tree_sum<10>(part, l);
#pragma unroll
    for (int k = 0; k < 10; ++k) B[k] = part[0][k];
    double Rn[12];
    transform_from(B, ca, cb, Rn);                                     // every lane: the same instructions on the same values
    if (l == 0) advance(finite12(Rn), Rn, p, tol_t, tol_c, state, Rt_all, hist_all, iterations, converged);
}

__global__ __launch_bounds__(LANES) void icp_final_kernel(Bank bank, Pairs pr, const int32_t* __restrict__ state,
                                                          const unsigned long long* __restrict__ d2bits,
                                                          const unsigned long long* __restrict__ cut_bits,
                                                          const int32_t* __restrict__ cut_i, double inlier_ratio,
                                                          double radius, double r2hi, double* __restrict__ rmse,
                                                          int32_t* __restrict__ hits, double* __restrict__ ratio)
{
    __shared__ double part[LANES][10];
    const int p = blockIdx.x, l = threadIdx.x;
    if (state[p] == NOT_REFINED) return;
    const int n1 = range_of(bank, pr.frag1, p, pr.Lmax).n, n2 = range_of(bank, pr.frag2, p, pr.Lmax).n;
    const unsigned long long cut = cut_bits[p];
    const int icut = cut_i[p];
    const unsigned long long* v = d2bits + (long long)p * pr.Lmax;
    double sum = 0.0;
    int mine = 0;
    for (int i = l; i < n2; i += LANES) {
        const double d2 = double_of(v[i]);
        if (kept(v[i], i, cut, icut)) sum += d2;
        mine += within(d2, radius, r2hi) ? 1 : 0;
    }
    part[l][0] = sum;
    part[l][1] = (double)mine;                                         // counts below 2^24: exact in any order
    tree_sum<2>(part, l);
    if (l != 0) return;
    const int h = (int)part[0][1];
    const double total = part[0][0];
    hits[p] = h;
    ratio[2 * p] = (double)h / (double)n1;
    ratio[2 * p + 1] = (double)h / (double)n2;
    rmse[p] = sqrt(total / (double)trim_count(inlier_ratio, n2));
}

long long align256(long long v) { return (v + 255) / 256 * 256; }

struct Workspace {
    long long idx, d2, cut_bits, cut_i, state, hist, bytes;
    Workspace(int P, int Lmax)
    {
        long long at = 0;
        d2 = at;       at += align256((long long)P * Lmax * 8);
        idx = at;      at += align256((long long)P * Lmax * 4);
        cut_bits = at; at += align256((long long)P * 8);
        hist = at;     at += align256((long long)P * 6 * 8);
        cut_i = at;    at += align256((long long)P * 4);
        state = at;    at += align256((long long)P * 4);
        bytes = at;
    }
};

}  // namespace

extern "C" long long usip_icp_workspace_bytes(int P, int Lmax)
{
    if (P < 0 || P > 65535 || Lmax < 1 || Lmax > (1 << 24)) return USIP_EINVAL;
    return Workspace(P, Lmax).bytes;
}

extern "C" int usip_icp_nearest_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags,
                                    long long total_rows, const int32_t* perm1, const int32_t* frag1, const int32_t* frag2,
                                    const double* Rt, const uint8_t* mask, const int32_t* order2, int P, int Lmax,
                                    int32_t* idx, double* d2, unsigned long long* visits, void* stream)
{
    if (!(bank_ok(rows, row_len, offsets, num_frags, total_rows, P, Lmax) && perm1)) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!frag1 || !frag2 || !Rt || !idx || !d2) return USIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(idx, 0, (size_t)P * Lmax * sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(d2, 0, (size_t)P * Lmax * sizeof(double), st);
    if (e == hipSuccess && visits) e = hipMemsetAsync(visits, 0, (size_t)P * sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    const SortedBank bank{{rows, offsets, row_len, num_frags, total_rows}, perm1};
    const Pairs pr{frag1, frag2, Lmax};
    USIP_LAUNCH(icp_nearest_kernel, dim3(usip_ceil_div(Lmax, TILE), P), dim3(LANES), 0, st, bank, pr, Rt, mask, order2,
                (const int32_t*)nullptr, 0, idx, d2, visits);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

// Both entries of the loop: everything but the fit's launch is one sequence, whatever the metric.  fit_sums: the plane
// metric's optional record.
static int refine_loop(bool plane, const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                       const int32_t* perm1, const int32_t* frag1, const int32_t* frag2, const double* Rt0,
                       const uint8_t* mask, const int32_t* order2, int P, int Lmax, double inlier_ratio, int max_iterations,
                       double tol_t, double tol_c, double align_radius, void* workspace, long long workspace_bytes, double* Rt,
                       int32_t* iterations, uint8_t* converged, double* rmse, int32_t* hits, double* ratio, double* cut_d2,
                       int32_t* cut_i_out, unsigned long long* visits, double* stage_ms, double* fit_sums, void* stream)
{
    if (!(bank_ok(rows, row_len, offsets, num_frags, total_rows, P, Lmax) && perm1) || (plane && row_len < 6))
        return USIP_EINVAL;
    if (!(inlier_ratio > 0.0 && inlier_ratio <= 1.0) || max_iterations < 0 || max_iterations > MAX_ITERATIONS ||
        !(tol_t >= 0.0) || !(tol_c >= 0.0) || !(align_radius > 0.0))
        return USIP_EINVAL;
    if (stage_ms) stage_ms[0] = stage_ms[1] = stage_ms[2] = stage_ms[3] = 0.0;
    if (P == 0) return USIP_OK;
    const Workspace ws(P, Lmax);
    if (!frag1 || !frag2 || !Rt0 || !workspace || workspace_bytes < ws.bytes || !Rt || !iterations || !converged || !rmse ||
        !hits || !ratio || (cut_d2 == nullptr) != (cut_i_out == nullptr))
        return USIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)workspace;
    int32_t* idx = (int32_t*)(w + ws.idx);
    double* d2 = (double*)(w + ws.d2);
    unsigned long long* d2bits = (unsigned long long*)(w + ws.d2);
    unsigned long long* cut_bits = (unsigned long long*)(w + ws.cut_bits);
    int32_t* cut_i = (int32_t*)(w + ws.cut_i);
    int32_t* state = (int32_t*)(w + ws.state);
    double* hist = (double*)(w + ws.hist);
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)ws.bytes, st);     // rows no query names read as zeros, never as junk
    if (e == hipSuccess && visits) e = hipMemsetAsync(visits, 0, (size_t)P * sizeof(unsigned long long), st);
    const int slots = max_iterations + 1;
    if (e == hipSuccess && cut_d2) e = hipMemsetAsync(cut_d2, 0, (size_t)P * slots * sizeof(double), st);
    if (e == hipSuccess && cut_d2) e = hipMemsetAsync(cut_i_out, 0, (size_t)P * slots * sizeof(int32_t), st);
    if (e == hipSuccess && fit_sums && max_iterations > 0)
        e = hipMemsetAsync(fit_sums, 0, (size_t)P * max_iterations * PLANE_SUMS * sizeof(double), st);
    if (e != hipSuccess) return (int)e;
    const SortedBank bank{{rows, offsets, row_len, num_frags, total_rows}, perm1};
    const Pairs pr{frag1, frag2, Lmax};
    const dim3 grid(usip_ceil_div(Lmax, TILE), P);
    USIP_LAUNCH(icp_init_kernel, dim3(usip_ceil_div(P, 64)), dim3(64), 0, st, bank, pr, Rt0, mask, P, Rt, state, hist,
                iterations, converged, rmse, hits, ratio);
    USIP_LAUNCH_CHECK();
    // stage_ms (a measurement, tools/icp_bench.py): an event after every launch, read once all are enqueued; the events
    // are destroyed on every way out, and an event that could not be made or recorded is the call's error
    struct Marks {
        std::vector<hipEvent_t> ev;
        hipError_t err = hipSuccess;
        ~Marks() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    } marks;
    const auto mark = [&]() {
        if (!stage_ms || marks.err != hipSuccess) return;
        hipEvent_t ev;
        marks.err = hipEventCreate(&ev);
        if (marks.err != hipSuccess) return;
        marks.ev.push_back(ev);
        marks.err = hipEventRecord(ev, st);
    };
    mark();
    for (int round = 0; round <= max_iterations; ++round) {
        const int final_pass = round == max_iterations ? 1 : 0;
        USIP_LAUNCH(icp_nearest_kernel, grid, dim3(LANES), 0, st, bank, pr, (const double*)Rt, (const uint8_t*)nullptr,
                    order2, (const int32_t*)state, final_pass, idx, d2, visits);
        USIP_LAUNCH_CHECK();
        mark();
        USIP_LAUNCH(icp_trim_kernel, dim3(P), dim3(LANES), 0, st, bank, pr, (const int32_t*)state, final_pass, inlier_ratio,
                    (const unsigned long long*)d2bits, cut_bits, cut_i, cut_d2, cut_i_out, round, slots);
        USIP_LAUNCH_CHECK();
        mark();
        if (!final_pass && plane) {
            const int rc = launch_fit_plane(bank, pr, P, idx, d2bits, cut_bits, cut_i, tol_t, tol_c, state, Rt, hist,
                                            iterations, converged, fit_sums, max_iterations, st);
            if (rc != USIP_OK) return rc;
        } else if (!final_pass) {
            USIP_LAUNCH(icp_fit_kernel, dim3(P), dim3(LANES), 0, st, bank, pr, (const int32_t*)idx,
                        (const unsigned long long*)d2bits, (const unsigned long long*)cut_bits, (const int32_t*)cut_i,
                        inlier_ratio, tol_t, tol_c, state, Rt, hist, iterations, converged);
        } else {
            USIP_LAUNCH(icp_final_kernel, dim3(P), dim3(LANES), 0, st, bank, pr, (const int32_t*)state,
                        (const unsigned long long*)d2bits, (const unsigned long long*)cut_bits, (const int32_t*)cut_i,
                        inlier_ratio, align_radius, radius_sq_hi(align_radius), rmse, hits, ratio);
        }
        USIP_LAUNCH_CHECK();
        mark();
    }
    if (stage_ms) {
        if (marks.err == hipSuccess) marks.err = hipEventSynchronize(marks.ev.back());
        for (size_t k = 0; marks.err == hipSuccess && k + 1 < marks.ev.size(); ++k) {
            float ms = 0.f;
            marks.err = hipEventElapsedTime(&ms, marks.ev[k], marks.ev[k + 1]);
            stage_ms[k / 3 == (size_t)max_iterations ? 3 : k % 3] += (double)ms;
        }
        if (marks.err != hipSuccess) return (int)marks.err;
    }
    return USIP_OK;
}

extern "C" int usip_icp_refine_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags,
                                   long long total_rows, const int32_t* perm1, const int32_t* frag1, const int32_t* frag2,
                                   const double* Rt0, const uint8_t* mask, const int32_t* order2, int P, int Lmax,
                                   double inlier_ratio, int max_iterations, double tol_t, double tol_c, double align_radius,
                                   void* workspace, long long workspace_bytes, double* Rt, int32_t* iterations,
                                   uint8_t* converged, double* rmse, int32_t* hits, double* ratio,
                                   double* cut_d2, int32_t* cut_i_out, unsigned long long* visits, double* stage_ms,
                                   void* stream)
{
    return refine_loop(false, rows, row_len, offsets, num_frags, total_rows, perm1, frag1, frag2, Rt0, mask, order2, P, Lmax,
                       inlier_ratio, max_iterations, tol_t, tol_c, align_radius, workspace, workspace_bytes, Rt, iterations,
                       converged, rmse, hits, ratio, cut_d2, cut_i_out, visits, stage_ms, nullptr, stream);
}

extern "C" int usip_icp_refine_plane_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags,
                                         long long total_rows, const int32_t* perm1, const int32_t* frag1,
                                         const int32_t* frag2, const double* Rt0, const uint8_t* mask, const int32_t* order2,
                                         int P, int Lmax, double inlier_ratio, int max_iterations, double tol_t, double tol_c,
                                         double align_radius, void* workspace, long long workspace_bytes, double* Rt,
                                         int32_t* iterations, uint8_t* converged, double* rmse, int32_t* hits, double* ratio,
                                         double* cut_d2, int32_t* cut_i_out, unsigned long long* visits, double* stage_ms,
                                         double* fit_sums, void* stream)
{
    return refine_loop(true, rows, row_len, offsets, num_frags, total_rows, perm1, frag1, frag2, Rt0, mask, order2, P, Lmax,
                       inlier_ratio, max_iterations, tol_t, tol_c, align_radius, workspace, workspace_bytes, Rt, iterations,
                       converged, rmse, hits, ratio, cut_d2, cut_i_out, visits, stage_ms, fit_sums, stream);
}
