// usip_amd/csrc/fragments.hip -- indoor fragment registration on the device: the per-pair work of the
// Redwood / 3DMatch benchmark (evaluation/matlab/eval_indoor/3dmatch/register2Fragments.m).  csrc/fragments_math.h has
// the semantics and the arithmetic, which the host twin (csrc/fragments_cpu.cpp) shares.  RANSAC itself is not here: the
// pair's correspondences (up to 10240) go through csrc/registration.hip's one trial and one select kernel.  No launch
// synchronises, no floating-point atomics.
//
//   knn_counted_kernel<K>        one wave per query descriptor, nearest_counted_kernel's distance (an FMA chain over the
//                                channels, sqrtf); every lane keeps the K best of its candidates in registers, then K
//                                rounds of a wave-wide lexicographic (distance, index) minimum pop the answer in order.
//   match_union_kernel           one workgroup per pair: the keys i Mp + q of both lists in LDS (40 KB at the limit), a
//                                bitonic network whose comparators all point the same way (so a length that is no power of
//                                two needs no padding), adjacent-unique, a prefix scan, the rows in order.
//   information_kernel           one workgroup per pair: lane-strided partial sums of A'A's nine distinct terms, the tree.
//   overlap_keys_kernel          x of every fragment-2 point under the pair's estimate: what the caller sorts by.
//   overlap_kernel<XQ>           an existence query.  A workgroup owns 256 queries; database tiles of 256 points, sorted
//                                along x, are staged in LDS as float64 and walked outward from the tile at the queries' x
//                                range, every lane at the same LDS address.  A direction ends when the x-gap alone reaches
//                                the radius (fragments_math.h beyond()); a lane stops testing at its first hit, the
//                                workgroup ends when no lane is left.
#include "common.h"
#include "bank.h"
#include "fragments_math.h"
#include "tile_walk.h"

using namespace usip_reg;
using namespace usip_frag;
using namespace usip_bank;
using namespace usip_walk;

namespace {

static_assert(OTILE == WALK_TILE, "overlap_kernel walks tile_walk.h's tiles");
constexpr int UT = 1024;    // lanes of the union's workgroup

// ------------------------------------------------------------------------------------------------ top-k matching
constexpr int NJ = 4;       // candidates in flight per lane

template <int K>
__global__ __launch_bounds__(256) void knn_counted_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          const int32_t* __restrict__ a_count,
                                                          const int32_t* __restrict__ b_count, float* __restrict__ dist,
                                                          int32_t* __restrict__ idx, int32_t* __restrict__ valid, int C,
                                                          int Ma, int Nb)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bi = blockIdx.y;
    const int na = clamp_count(a_count, bi, Ma), nb = clamp_count(b_count, bi, Nb);
    if (blockIdx.x == 0 && threadIdx.x == 0) valid[bi] = nb < K ? nb : K;
    if (i >= Ma) return;
    const long long o = ((long long)bi * Ma + i) * K;
    if (i >= na || nb < 1) {                                           // padding rows: a defined value, never data
        if (lane < K) { dist[o + lane] = __builtin_inff(); idx[o + lane] = 0; }
        return;
    }
    const float* ab = a + (long long)bi * C * Ma;
    const float* bb = b + (long long)bi * C * Nb;
    TopK<K> list;
    list.clear();
    for (int j0 = 0; j0 < nb; j0 += 64 * NJ) {
        int jc[NJ];
        float s[NJ];
#pragma unroll
        for (int u = 0; u < NJ; ++u) { jc[u] = min(j0 + u * 64 + lane, nb - 1); s[u] = 0.f; }
        for (int c = 0; c < C; ++c) {
            const float av = ab[(long long)c * Ma + i];
#pragma unroll
            for (int u = 0; u < NJ; ++u) {
                const float df = av - bb[(long long)c * Nb + jc[u]];
                s[u] = __builtin_fmaf(df, df, s[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < NJ; ++u) {
            const int j = j0 + u * 64 + lane;
            if (j < nb) list.offer(sqrtf(s[u]), j);                    // ascending j per lane
        }
    }
#pragma unroll
    for (int r = 0; r < K; ++r) {
        float best = list.d[0];
        int bj = list.j[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_xor(best, off);
            const int oj = __shfl_xor(bj, off);
            if (od < best || (od == best && oj < bj)) { best = od; bj = oj; }
        }
        if (bj != 0x7fffffff && list.j[0] == bj) list.pop();           // one lane owns index bj
        if (lane == 0) {
            const bool have = bj != 0x7fffffff;
            dist[o + r] = have ? best : __builtin_inff();
            idx[o + r] = have ? bj : 0;
        }
    }
}

template <int K>
int launch_knn(const float* a, const float* b, const int32_t* a_count, const int32_t* b_count, float* dist, int32_t* idx,
               int32_t* valid, int B, int C, int Ma, int Nb, hipStream_t stream)
{
    USIP_LAUNCH(knn_counted_kernel<K>, dim3(usip_ceil_div(Ma, 4), B), dim3(256), 0, stream, a, b, a_count, b_count, dist,
                idx, valid, C, Ma, Nb);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

// ------------------------------------------------------------------------------------------------ union of the two lists
__device__ __forceinline__ void order(uint32_t* key, int i, int j, int total)
{
    if (j < total) {
        const uint32_t x = key[i], y = key[j];
        if (x > y) { key[i] = y; key[j] = x; }
    }
}

__global__ __launch_bounds__(UT) void match_union_kernel(const int32_t* __restrict__ nn12, const int32_t* __restrict__ nn21,
                                                         const int32_t* __restrict__ a_count,
                                                         const int32_t* __restrict__ p_count, int Ma, int Mp, int k,
                                                         int32_t* __restrict__ pairs, int32_t* __restrict__ count)
{
    __shared__ uint32_t key[UNION_MAX];
    __shared__ int scan[UT];
    const int p = blockIdx.x, l = threadIdx.x;
    const int Cmax = k * (Ma + Mp);
    const int na = clamp_count(a_count, p, Ma), np = clamp_count(p_count, p, Mp);
    const int k12 = np < k ? np : k, k21 = na < k ? na : k;            // the valid columns of either list
    const int n12 = na * k12, total = n12 + np * k21;                  // <= Cmax <= UNION_MAX
    const int32_t* A = nn12 + (long long)p * Ma * k;
    const int32_t* Q = nn21 + (long long)p * Mp * k;
    for (int e = l; e < n12; e += UT) {
        const int i = e / k12, c = e - i * k12;
        key[e] = (uint32_t)(i * Mp + clamp_index(A[(long long)i * k + c], Mp));
    }
    for (int e = l; e < total - n12; e += UT) {
        const int q = e / k21, c = e - q * k21;
        key[n12 + e] = (uint32_t)(clamp_index(Q[(long long)q * k + c], Ma) * Mp + q);
    }
    int n2 = 1;
    while (n2 < total) n2 <<= 1;
    // a bitonic network in its one-directional form: the first step of a merge pairs i with its mirror in the block, the
    // rest with i + s; the smaller key always goes to the lower index, so slots >= total stand for +inf and are skipped
    for (int size = 2; size <= n2; size <<= 1) {
        const int half = size >> 1;
        __syncthreads();
        for (int t = l; t < (n2 >> 1); t += UT) {
            const int blk = t / half, off = t - blk * half;
            const int i = blk * size + off;
            order(key, i, blk * size + size - 1 - off, total);
        }
        for (int s = half >> 1; s > 0; s >>= 1) {
            __syncthreads();
            for (int t = l; t < (n2 >> 1); t += UT) {
                const int blk = t / s, off = t - blk * s;
                const int i = blk * 2 * s + off;
                order(key, i, i + s, total);
            }
        }
    }
    __syncthreads();
    // adjacent-unique over contiguous segments, an inclusive scan of the segments' counts, then the rows
    const int per = (total + UT - 1) / UT;
    const int lo = min(l * per, total), hi = min(lo + per, total);
    int mine = 0;
    for (int e = lo; e < hi; ++e) mine += (e == 0 || key[e] != key[e - 1]) ? 1 : 0;
    scan[l] = mine;
    __syncthreads();
    for (int off = 1; off < UT; off <<= 1) {
        const int v = l >= off ? scan[l - off] : 0;
        __syncthreads();
        scan[l] += v;
        __syncthreads();
    }
    int at = scan[l] - mine;
    const int unique = scan[UT - 1];
    int32_t* out = pairs + (long long)p * Cmax * 2;
    for (int e = lo; e < hi; ++e)
        if (e == 0 || key[e] != key[e - 1]) {
            const int i = (int)(key[e] / (uint32_t)Mp);
            out[2LL * at] = i;
            out[2LL * at + 1] = (int)key[e] - i * Mp;
            ++at;
        }
    for (int e = unique + l; e < Cmax; e += UT) { out[2LL * e] = 0; out[2LL * e + 1] = 0; }
    if (l == 0) count[p] = unique;
}

// ------------------------------------------------------------------------------------------------ information matrix
__global__ __launch_bounds__(REFIT_LANES) void information_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                                  int Nmax, double* __restrict__ info)
{
    __shared__ double part[REFIT_LANES][INFO_W];
    __shared__ int s_n;
    const int p = blockIdx.x, l = threadIdx.x;
    const float* a = x + (long long)p * 3 * Nmax;
    const uint8_t* m = mask + (long long)p * Nmax;
    if (l == 0) s_n = 0;
    double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int mine = 0;
    for (int i = l; i < Nmax; i += REFIT_LANES)
        if (m[i]) {
            double t[9];
            info_terms((double)a[i], (double)a[(long long)Nmax + i], (double)a[2LL * Nmax + i], t);
#pragma unroll
            for (int k = 0; k < 9; ++k) s[k] += t[k];
            ++mine;
        }
#pragma unroll
    for (int k = 0; k < 9; ++k) part[l][k] = s[k];
    part[l][9] = 0.0;
    __syncthreads();
    if (mine) atomicAdd(&s_n, mine);
    tree_sum<9>(part, l);
    if (l != 0) return;
    double sum[9], out[36];
    for (int k = 0; k < 9; ++k) sum[k] = part[0][k];
    info_fill(sum, s_n, out);
    for (int k = 0; k < 36; ++k) info[(long long)p * 36 + k] = out[k];
}

// ------------------------------------------------------------------------------------------------ overlap
// the point at sorted position s of a fragment, moved by Rt when `moved`
__device__ __forceinline__ void sorted_point(const float* base, int row_len, const int32_t* perm, int s, int n, bool moved,
                                             const double* Rt, double* x, double* y, double* z)
{
    const float* r = base + (long long)safe_index(perm[s], n) * row_len;
    const double b0 = (double)r[0], b1 = (double)r[1], b2 = (double)r[2];
    *x = moved ? xform(Rt, 0, b0, b1, b2) : b0;
    *y = moved ? xform(Rt, 1, b0, b1, b2) : b1;
    *z = moved ? xform(Rt, 2, b0, b1, b2) : b2;
}

__global__ __launch_bounds__(256) void overlap_keys_kernel(Bank bank, const int32_t* __restrict__ frag2,
                                                           const double* __restrict__ Rt, int Lmax,
                                                           double* __restrict__ keys)
{
    const int p = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x;
    if (s >= Lmax) return;
    const Range f = bank.range(frag2[p], Lmax);
    double v = (double)__builtin_inff();                               // padding sorts last
    if (s < f.n) {
        const float* r = bank.rows + (f.first + s) * bank.row_len;
        v = xform(Rt + (long long)p * 12, 0, (double)r[0], (double)r[1], (double)r[2]);
    }
    keys[(long long)p * Lmax + s] = v;
}

// XQ false: the queries are fragment 1's points, the database fragment 2's moved by Rt (ratio[p][0]); XQ true: the
// converse (ratio[p][1]).  perm1 sorts every fragment of the bank along x (local indices, at the fragment's offset),
// perm2 [P][Lmax] sorts fragment 2 along the moved x (overlap_keys_kernel's values).
template <bool XQ>
__global__ __launch_bounds__(OTILE) void overlap_kernel(Bank bank, const int32_t* __restrict__ frag1,
                                                        const int32_t* __restrict__ frag2, const double* __restrict__ Rt_all,
                                                        const int32_t* __restrict__ perm1, const int32_t* __restrict__ perm2,
                                                        int Lmax, double radius, double r2hi, int32_t* __restrict__ hits)
{
    __shared__ double tile[2][3][OTILE];
    __shared__ double sRt[12];
    __shared__ double slots[2 * WALK_WAVES];
    const int p = blockIdx.y, l = threadIdx.x;
    const Range r1 = bank.range(frag1[p], Lmax), r2 = bank.range(frag2[p], Lmax);
    const int nq = XQ ? r2.n : r1.n, nd = XQ ? r1.n : r2.n;
    if (blockIdx.x * OTILE >= nq || nd < 1) return;                    // workgroup-uniform
    if (l < 12) sRt[l] = Rt_all[(long long)p * 12 + l];
    __syncthreads();
    double Rt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = sRt[k];
    const int32_t* pa = perm1 + r1.first;
    const int32_t* pb = perm2 + (long long)p * Lmax;
    const float* ra = bank.rows + r1.first * bank.row_len;
    const float* rb = bank.rows + r2.first * bank.row_len;
    const float* qrows = XQ ? rb : ra;
    const float* drows = XQ ? ra : rb;
    const int32_t* qperm = XQ ? pb : pa;
    const int32_t* dperm = XQ ? pa : pb;
    const int row_len = bank.row_len;

    const int q = blockIdx.x * OTILE + l;
    const bool live = q < nq;
    double xi, yi, zi;
    sorted_point(qrows, row_len, qperm, live ? q : nq - 1, nq, XQ, Rt, &xi, &yi, &zi);
    double xlo = xi, xhi = xi;
    block_minmax<true, true>(xlo, xhi, slots);                         // the x range of this workgroup's queries

    const auto x_at = [&](int s) {                                     // x of the database row at sorted position s
        const float* r = drows + (long long)safe_index(dperm[s], nd) * row_len;
        return !XQ ? xform(Rt, 0, (double)r[0], (double)r[1], (double)r[2]) : (double)r[0];
    };
    const Tiles<decltype(x_at)> tiles(nd, x_at);
    const int start = tiles.start(xlo);
    bool hit = false;
    walk_outward(
        tiles, start - 1, start,
        [&](int left, int right) {
            if (!__syncthreads_or(live && !hit)) return END_LEFT | END_RIGHT;  // (also: every lane is done with the tiles)
            return (left >= 0 && beyond(xlo - tiles.near_x(0, left), radius) ? END_LEFT : 0) |
                   (right < tiles.tiles && beyond(tiles.near_x(1, right) - xhi, radius) ? END_RIGHT : 0);
        },
        [&](int side, int t) {
            const int s = t * OTILE + l;
            double x, y, z;
            sorted_point(drows, row_len, dperm, s < nd ? s : nd - 1, nd, !XQ, Rt, &x, &y, &z);
            tile[side][0][l] = x;
            tile[side][1][l] = y;
            tile[side][2][l] = z;
        },
        [&](int side, int, int m) {
            bool found = hit || !live;                                 // (a local: the flag stays a lane mask in the loop)
            for (int c = 0; c < m && !found; ++c)
                found = within(sqdist3(xi, yi, zi, tile[side][0][c], tile[side][1][c], tile[side][2][c]), radius, r2hi);
            hit = found && live;
        });
    const int found = __syncthreads_count(live && hit);
    if (l == 0 && found) atomicAdd(&hits[2 * p + (XQ ? 1 : 0)], found);
}

__global__ __launch_bounds__(64) void overlap_ratio_kernel(Bank bank, const int32_t* __restrict__ frag1,
                                                           const int32_t* __restrict__ frag2, int P, int Lmax,
                                                           const int32_t* __restrict__ hits, double* __restrict__ ratio)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    const int n1 = bank.range(frag1[p], Lmax).n, n2 = bank.range(frag2[p], Lmax).n;
    ratio[2 * p] = n1 > 0 ? (double)hits[2 * p] / (double)n1 : 0.0;
    ratio[2 * p + 1] = n2 > 0 ? (double)hits[2 * p + 1] / (double)n2 : 0.0;
}

}  // namespace

extern "C" int usip_knn_nd_counted_f32(const float* a, const float* b, const int32_t* a_count, const int32_t* b_count, int k,
                                       float* dist, int32_t* idx, int32_t* valid, int B, int C, int Ma, int Nb, void* stream)
{
    if (B < 0 || B > 65535 || C < 1 || Ma < 0 || Nb < 1 || k < 1 || k > KMAX) return USIP_EINVAL;
    if ((long long)B * Ma == 0) return USIP_OK;
    if (!a || !b || !a_count || !b_count || !dist || !idx || !valid) return USIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    switch (k) {
#define USIP_TOPK_CASE(k_) case k_: return launch_knn<k_>(a, b, a_count, b_count, dist, idx, valid, B, C, Ma, Nb, st)
        USIP_TOPK_CASE(1); USIP_TOPK_CASE(2); USIP_TOPK_CASE(3); USIP_TOPK_CASE(4);
        USIP_TOPK_CASE(5); USIP_TOPK_CASE(6); USIP_TOPK_CASE(7); USIP_TOPK_CASE(8);
#undef USIP_TOPK_CASE
    }
    return USIP_EINVAL;
}

extern "C" int usip_match_union_i32(const int32_t* nn12, const int32_t* nn21, const int32_t* a_count, const int32_t* p_count,
                                    int P, int Ma, int Mp, int k, int32_t* pairs, int32_t* count, void* stream)
{
    if (P < 0 || P > 65535 || Ma < 1 || Mp < 1 || k < 1 || k > KMAX) return USIP_EINVAL;
    if ((long long)k * ((long long)Ma + Mp) > UNION_MAX) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!nn12 || !nn21 || !a_count || !p_count || !pairs || !count) return USIP_EINVAL;
    USIP_LAUNCH(match_union_kernel, dim3(P), dim3(UT), 0, (hipStream_t)stream, nn12, nn21, a_count, p_count, Ma, Mp, k,
                pairs, count);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_information_f32(const float* x, const uint8_t* mask, int P, int Nmax, double* info, void* stream)
{
    if (P < 0 || P > 65535 || Nmax < 1 || Nmax > NMAX) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!x || !mask || !info) return USIP_EINVAL;
    USIP_LAUNCH(information_kernel, dim3(P), dim3(REFIT_LANES), 0, (hipStream_t)stream, x, mask, Nmax, info);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_overlap_keys_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags,
                                     long long total_rows, const int32_t* frag2, const double* Rt, int P, int Lmax,
                                     double* keys, void* stream)
{
    if (!bank_ok(rows, row_len, offsets, num_frags, total_rows, P, Lmax)) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!frag2 || !Rt || !keys) return USIP_EINVAL;
    const Bank bank{rows, offsets, row_len, num_frags, total_rows};
    USIP_LAUNCH(overlap_keys_kernel, dim3(usip_ceil_div(Lmax, 256), P), dim3(256), 0, (hipStream_t)stream, bank, frag2, Rt,
                Lmax, keys);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_overlap_ratio_f32(const float* rows, int row_len, const int64_t* offsets, int num_frags,
                                      long long total_rows, const int32_t* frag1, const int32_t* frag2, const double* Rt,
                                      const int32_t* perm1, const int32_t* perm2, int P, int Lmax, double radius,
                                      int32_t* hits, double* ratio, void* stream)
{
    if (!bank_ok(rows, row_len, offsets, num_frags, total_rows, P, Lmax) || !(radius > 0.0)) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!frag1 || !frag2 || !Rt || !perm1 || !perm2 || !hits || !ratio) return USIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Bank bank{rows, offsets, row_len, num_frags, total_rows};
    const hipError_t e = hipMemsetAsync(hits, 0, (size_t)P * 2 * sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const double r2hi = radius_sq_hi(radius);
    const dim3 grid(usip_ceil_div(Lmax, OTILE), P);
    USIP_LAUNCH(overlap_kernel<false>, grid, dim3(OTILE), 0, st, bank, frag1, frag2, Rt, perm1, perm2, Lmax, radius, r2hi,
                hits);
    USIP_LAUNCH_CHECK();
    USIP_LAUNCH(overlap_kernel<true>, grid, dim3(OTILE), 0, st, bank, frag1, frag2, Rt, perm1, perm2, Lmax, radius, r2hi,
                hits);
    USIP_LAUNCH_CHECK();
    USIP_LAUNCH(overlap_ratio_kernel, dim3(usip_ceil_div(P, 64)), dim3(64), 0, st, bank, frag1, frag2, P, Lmax, hits, ratio);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
