// usip_amd/csrc/ground_truth.hip -- a fragment scene's ground truth on the device: the per-pair work of
// evaluation/matlab/eval_indoor/3dmatch/getGtInfoLog.m.  csrc/ground_truth_math.h has the semantics and the arithmetic, which
// the host twin (csrc/ground_truth_cpu.cpp) shares; include/usip_hip.h (f-18) is the contract.  No launch synchronises, no
// floating-point atomics, every index read from memory is clamped.
//
//   gt_reach_kernel         a workgroup owns 256 rows of fragment 2, moved by the pair's pose, in the order of their moved x;
//                           fragment 1's tiles of 256 rows, sorted along x, are staged in LDS as float64 and walked outward
//                           from the tile at the queries' x range (csrc/tile_walk.h), every lane at the same LDS address.  A
//                           lane keeps its smallest d2 -- one walk answers both radii.  A side ends when the x-gap alone
//                           reaches `far` (fragments_math.h beyond()); a lane stops testing once its d2 is within `near`, the
//                           workgroup ends when no lane is left.  cls and key go through perm2 to the local row; the two
//                           counts are one integer atomic each per workgroup.
//   gt_ratio_kernel         hits over either fragment's length.
//   gt_information_kernel   one workgroup per pair: lane l adds the terms of the selected rows l, l + 256, ... at the moved
//                           point; registration_math.h's tree; lane 0 fills the 6 x 6.
#include "common.h"
#include "bank.h"
#include "ground_truth_math.h"
#include "tile_walk.h"

using namespace usip_gt;
using namespace usip_frag;
using namespace usip_bank;
using namespace usip_walk;
using usip_reg::clamp_count;
using usip_reg::clamp_index;
using usip_reg::tree_sum;

namespace {

static_assert(LANES == WALK_TILE, "gt_reach_kernel walks tile_walk.h's tiles");

struct Radii {
    double far, far2hi, near, near2hi;
};

__global__ __launch_bounds__(LANES) void gt_reach_kernel(Bank bank, const int32_t* __restrict__ frag1,
                                                         const int32_t* __restrict__ frag2,
                                                         const double* __restrict__ Rt_all, const int32_t* __restrict__ perm1,
                                                         const int32_t* __restrict__ perm2, const uint8_t* __restrict__ mask,
                                                         int Lmax, Radii rad, unsigned long long seed,
                                                         const int64_t* __restrict__ pair_ids, uint8_t* __restrict__ cls,
                                                         unsigned long long* __restrict__ key, int32_t* __restrict__ hits)
{
    __shared__ double tile[2][3][WALK_TILE];
    __shared__ double sRt[12];
    __shared__ double slots[2 * WALK_WAVES];
    const int p = blockIdx.y, l = threadIdx.x;
    if (mask && mask[p] == 0) return;                                  // workgroup-uniform, here and below
    const Range r1 = bank.range(frag1[p], Lmax), r2 = bank.range(frag2[p], Lmax);
    const int n1 = r1.n, n2 = r2.n;
    if ((int)blockIdx.x * WALK_TILE >= n2 || n1 < 1) return;           // cls 0 and key KEY_NONE are there already
    if (l < 12) sRt[l] = Rt_all[(long long)p * 12 + l];
    __syncthreads();
    double Rt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = sRt[k];
    const int row_len = bank.row_len;
    const float* rows1 = bank.rows + r1.first * row_len;
    const int32_t* pa = perm1 + r1.first;

    const int s = blockIdx.x * WALK_TILE + l;
    const bool live = s < n2;
    const int i = safe_index(perm2[(long long)p * Lmax + (live ? s : n2 - 1)], n2);
    const float* b = bank.rows + (r2.first + i) * row_len;
    const double b0 = (double)b[0], b1 = (double)b[1], b2 = (double)b[2];
    const double qx = xform(Rt, 0, b0, b1, b2), qy = xform(Rt, 1, b0, b1, b2), qz = xform(Rt, 2, b0, b1, b2);
    double xlo = qx, xhi = qx;
    block_minmax<true, true>(xlo, xhi, slots);                         // the x range of this workgroup's queries

    const auto x_at = [&](int at) { return (double)rows1[(long long)safe_index(pa[at], n1) * row_len]; };
    const Tiles<decltype(x_at)> tiles(n1, x_at);
    const int start = tiles.start(xlo);
    double best = (double)__builtin_inff();
    bool done = !live;                                                 // the lane has nothing left to learn
    walk_outward(
        tiles, start - 1, start,
        [&](int left, int right) {
            if (!__syncthreads_or(!done)) return END_LEFT | END_RIGHT;         // (also: every lane is done with the tiles)
            return (left >= 0 && beyond(xlo - tiles.near_x(0, left), rad.far) ? END_LEFT : 0) |
                   (right < tiles.tiles && beyond(tiles.near_x(1, right) - xhi, rad.far) ? END_RIGHT : 0);
        },
        [&](int side, int t) {
            const int row = safe_index(pa[min(t * WALK_TILE + l, n1 - 1)], n1);
            const float* a = rows1 + (long long)row * row_len;
            tile[side][0][l] = (double)a[0];
            tile[side][1][l] = (double)a[1];
            tile[side][2][l] = (double)a[2];
        },
        [&](int side, int, int m) {
            if (done) return;
            double least = best;                                       // (a local: the minimum stays in a register in the loop)
            for (int c = 0; c < m; ++c) {
                const double d2 = sqdist3(qx, qy, qz, tile[side][0][c], tile[side][1][c], tile[side][2][c]);
                least = d2 < least ? d2 : least;
            }
            best = least;
            done = within(best, rad.near, rad.near2hi);
        });
    const int c = live ? (int)reach_class(best, rad.far, rad.far2hi, rad.near, rad.near2hi) : 0;
    if (c) {
        cls[(long long)p * Lmax + i] = (uint8_t)c;
        if (c == 2) key[(long long)p * Lmax + i] = selection_key(seed, pair_ids ? (uint64_t)pair_ids[p] : (uint64_t)p, (uint64_t)i);
    }
    const int reached = __syncthreads_count(c >= 1), close = __syncthreads_count(c == 2);
    if (l == 0 && reached) atomicAdd(&hits[2 * p], reached);           // integers: the order of the additions is free
    if (l == 0 && close) atomicAdd(&hits[2 * p + 1], close);
}

__global__ __launch_bounds__(64) void gt_ratio_kernel(Bank bank, const int32_t* __restrict__ frag1,
                                                      const int32_t* __restrict__ frag2, int P, int Lmax,
                                                      const int32_t* __restrict__ hits, double* __restrict__ ratio)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    const int n1 = bank.range(frag1[p], Lmax).n, n2 = bank.range(frag2[p], Lmax).n;
    ratio[2 * p] = n1 > 0 ? (double)hits[2 * p] / (double)n1 : 0.0;
    ratio[2 * p + 1] = n2 > 0 ? (double)hits[2 * p] / (double)n2 : 0.0;
}

__global__ __launch_bounds__(LANES) void gt_information_kernel(Bank bank, const int32_t* __restrict__ frag2,
                                                               const double* __restrict__ Rt_all,
                                                               const int32_t* __restrict__ order,
                                                               const int32_t* __restrict__ count, int cap, int Lmax,
                                                               double* __restrict__ info)
{
    __shared__ double part[LANES][10];
    __shared__ double sRt[12];
    const int p = blockIdx.x, l = threadIdx.x;
    const Range r2 = bank.range(frag2[p], Lmax);
    const int n = r2.n >= 1 ? clamp_count(count, p, cap) : 0;          // workgroup-uniform
    if (l < 12) sRt[l] = Rt_all[(long long)p * 12 + l];
    __syncthreads();
    double Rt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = sRt[k];
    const float* rows2 = bank.rows + r2.first * bank.row_len;
    double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int mine = 0;
    for (int at = l; at < n; at += LANES) {
        const float* b = rows2 + (long long)clamp_index(order[(long long)p * cap + at], r2.n) * bank.row_len;
        const double b0 = (double)b[0], b1 = (double)b[1], b2 = (double)b[2];
        double t[9];
        gt_terms(xform(Rt, 0, b0, b1, b2), xform(Rt, 1, b0, b1, b2), xform(Rt, 2, b0, b1, b2), t);
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] += t[k];
        ++mine;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) part[l][k] = s[k];
    part[l][9] = (double)mine;                                         // counts up to 65536: exact in any order
    tree_sum<10>(part, l);
    if (l != 0) return;
    double sum[9], out[36];
#pragma unroll
    for (int k = 0; k < 9; ++k) sum[k] = part[0][k];
    info_fill(sum, (int)part[0][9], out);
#pragma unroll
    for (int k = 0; k < 36; ++k) info[(long long)p * 36 + k] = out[k];
}

}  // namespace

extern "C" int usip_gt_reach_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                                 const int32_t* perm1, const int32_t* frag1, const int32_t* frag2, const double* Rt,
                                 const int32_t* perm2, const uint8_t* mask, int P, int Lmax, double far_radius,
                                 double near_radius, uint64_t seed, const int64_t* pair_ids, uint8_t* cls, int32_t* hits,
                                 double* ratio, uint64_t* key, void* stream)
{
    if (!bank_ok(rows, row_len, offsets, num_frags, total_rows, P, Lmax) || !(near_radius > 0.0) ||
        !(far_radius > near_radius))
        return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!perm1 || !frag1 || !frag2 || !Rt || !perm2 || !cls || !hits || !ratio || !key) return USIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Bank bank{rows, offsets, row_len, num_frags, total_rows};
    const size_t slots = (size_t)P * (size_t)Lmax;
    hipError_t e = hipMemsetAsync(cls, 0, slots, st);
    if (e == hipSuccess) e = hipMemsetAsync(key, 0xff, slots * sizeof(uint64_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(hits, 0, (size_t)P * 2 * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const Radii rad{far_radius, radius_sq_hi(far_radius), near_radius, radius_sq_hi(near_radius)};
    USIP_LAUNCH(gt_reach_kernel, dim3(usip_ceil_div(Lmax, WALK_TILE), P), dim3(LANES), 0, st, bank, frag1, frag2, Rt, perm1,
                perm2, mask, Lmax, rad, (unsigned long long)seed, pair_ids, cls, (unsigned long long*)key, hits);
    USIP_LAUNCH_CHECK();
    USIP_LAUNCH(gt_ratio_kernel, dim3(usip_ceil_div(P, 64)), dim3(64), 0, st, bank, frag1, frag2, P, Lmax, hits, ratio);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_gt_information_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags,
                                       long long total_rows, const int32_t* frag2, const double* Rt, const int32_t* order,
                                       const int32_t* count, int P, int Lmax, int cap, double* info, void* stream)
{
    if (!bank_ok(rows, row_len, offsets, num_frags, total_rows, P, Lmax) || cap < 1 || cap > CAP_MAX) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!frag2 || !Rt || !order || !count || !info) return USIP_EINVAL;
    const Bank bank{rows, offsets, row_len, num_frags, total_rows};
    USIP_LAUNCH(gt_information_kernel, dim3(P), dim3(LANES), 0, (hipStream_t)stream, bank, frag2, Rt, order, count, cap, Lmax,
                info);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
