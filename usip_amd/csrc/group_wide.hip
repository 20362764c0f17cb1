// usip_amd/csrc/group_wide.hip -- neighbourhoods wider than 256 samples (256 < K <= 1024, K % 4 == 0) on gfx950.
//
// group_max4_kernel<L> (group.hip) gives a row to L = K/4 <= 64 lanes and bn_bwd_reduce_kernel<true, .> (shared_mlp.hip)
// a neighbourhood to K/4 lanes of a power-of-two shuffle, so both end at K = 256.  The indoor descriptor groups 448 points
// per keypoint.  Here a row (a neighbourhood) belongs to a whole wave and a lane owns the float4s l, l + 64, l + 128, ... of
// it: NP = ceil(K / 256) passes, the last of which leaves the lanes past K/4 - 64 (NP - 1) idle.
//
//   group_max_wide       pooled / arg / yarg exactly as group_max / group_max_act (group.hip's header comment and
//                        pool_order.h: a NaN ranks above everything, the first k wins, -0.0 and +0.0 tie)
//   bn_bwd_reduce_wide   partial / gsum exactly as bn_bwd_reduce_kernel<true, .>, in a summation order of its own
#include "common.h"
#include "pool_order.h"
#include "bn_reduce_common.h"

namespace {

// One wave per row, RPW rows per wave with all NP * RPW 16-B loads issued before the first is used (non-temporal: the
// tensor is next read in backward): 2 - 4 KiB in flight per wave, what group.hip's comment on group_max4_kernel found
// this pass to need.  Inside a lane k only grows (pass after pass, x y z w), so pool_gt keeps the first k; across lanes the
// (value, k) rule of group_max4_kernel runs over a 64-lane butterfly -- the rule is symmetric, every lane ends with the row's
// answer and lane 0 stores it.  A lower k may sit on a higher lane (k = 100: lane 25, k = 260: lane 1): only k decides.
template <int NP, bool NANS>
__global__ __launch_bounds__(256) void group_max_wide_kernel(
    const float* __restrict__ z, float* __restrict__ pooled, int32_t* __restrict__ arg, long long rows,
    const float* __restrict__ coef, int relu, int C, int M, float* __restrict__ zarg, int K4)
{
    constexpr int RPW = NP == 2 ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long row0 = ((long long)blockIdx.x * 4 + wave) * RPW;
    float4 v[RPW][NP];
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const float* zr = z + min(row0 + j, rows - 1) * K4 * 4;         // clamped: branch-free loads
#pragma unroll
        for (int p = 0; p < NP; ++p) v[j][p] = usip_load_stream4(zr + min(lane + 64 * p, K4 - 1) * 4);
    }
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const long long row = row0 + j;
        float s0 = 1.f, s1 = 0.f;
        if (coef) {
            const int ch = (int)((min(row, rows - 1) / M) % C);         // wave-uniform
            s0 = coef[ch]; s1 = coef[C + ch];
        }
        float best = 0.f, braw = 0.f;
        int bk = 0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int f = lane + 64 * p;
            if (p > 0 && f >= K4) continue;                             // (pass 0 is whole: K4 > 64)
            float4 w = v[j][p];
            if (coef) {
                w.x = __builtin_fmaf(w.x, s0, s1); w.y = __builtin_fmaf(w.y, s0, s1);
                w.z = __builtin_fmaf(w.z, s0, s1); w.w = __builtin_fmaf(w.w, s0, s1);
                if (relu) { w.x = fmaxf(w.x, 0.f); w.y = fmaxf(w.y, 0.f); w.z = fmaxf(w.z, 0.f); w.w = fmaxf(w.w, 0.f); }
            }
            if (p == 0 || pool_gt<NANS>(w.x, best)) { best = w.x; bk = f * 4; braw = v[j][p].x; }
            if (pool_gt<NANS>(w.y, best)) { best = w.y; bk = f * 4 + 1; braw = v[j][p].y; }
            if (pool_gt<NANS>(w.z, best)) { best = w.z; bk = f * 4 + 2; braw = v[j][p].z; }
            if (pool_gt<NANS>(w.w, best)) { best = w.w; bk = f * 4 + 3; braw = v[j][p].w; }
        }
        if constexpr (NANS) pool_hide_nan(best, bk);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(best, off);
            const int ok = __shfl_xor(bk, off);
            const float orw = __shfl_xor(braw, off);
            if (ov > best || (ov == best && ok < bk)) { best = ov; bk = ok; braw = orw; }
        }
        if (lane == 0 && row < rows) {
            if constexpr (NANS) {                           // without coef braw IS the NaN; with it, fma(braw, s0, s1) was
                if (bk < 0) { bk += POOL_NAN; best = coef ? __builtin_nanf("") : braw; }
            }
            pooled[row] = best;
            arg[row] = bk;
            if (zarg) zarg[row] = braw;
        }
    }
}

// One workgroup per (cloud, channel) row, as bn_bwd_reduce_kernel; wave w of the four walks the neighbourhoods w, w + 4, ...
// whole.  A lane's float4s are the pooling kernel's; all 2 NP loads of a neighbourhood are issued before the first is used
// (ordinary loads: the pair (dZ, Y) is next read by the data / weight gradient kernels).
// Order, fixed: a lane adds its passes' (d0 + d1) + (d2 + d3) in pass order into gd (and the y's into gy), the 64 lanes
// combine gd / gy by the xor butterfly 32, 16, ..., 1 and lane 0 stores; s1 takes each pass's quad sum, s2 the fma chain
// d0..d3 of each pass and mx the maximum, per lane across the wave's neighbourhoods, and end in bn_bwd_block_reduce.
template <int NP>
__global__ __launch_bounds__(256) void bn_bwd_reduce_wide_kernel(
    const float* __restrict__ dZ, const float* __restrict__ Y, const float* __restrict__ coef,
    const float* __restrict__ mean, const float* __restrict__ invstd, float* __restrict__ partial,
    float* __restrict__ gsum, int relu, int C, int P, int nrows, int K, int want_max)
{
    const long long rowid = blockIdx.x;
    const int ch = (int)(rowid % C);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float* dz = dZ + rowid * P;
    const float* y = Y + rowid * P;
    const float sc = coef[ch], sh = coef[C + ch], mu = mean[ch], is = invstd[ch];
    const int K4 = K / 4, G = P / K;
    float* g0 = gsum + rowid * G;
    float* g1 = gsum + ((long long)nrows + rowid) * G;
    float s1 = 0.f, s2 = 0.f, mx = 0.f;
    // UNR neighbourhoods of the wave in flight (NP = 2: two, i.e. 8 KiB per wave; the workgroups are few -- nb * C -- and each
    // wave would otherwise wait on 4 KiB at a time); they are reduced one after the other, in the order w, w + 4, ...
    constexpr int UNR = NP == 2 ? 2 : 1;
    for (int gb = wave; gb < G; gb += 4 * UNR) {
        float4 yq[UNR][NP], dq[UNR][NP];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int g = min(gb + 4 * u, G - 1);                           // clamped: branch-free loads
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int off = g * K + min(lane + 64 * p, K4 - 1) * 4;
                yq[u][p] = *reinterpret_cast<const float4*>(y + off);
                dq[u][p] = *reinterpret_cast<const float4*>(dz + off);
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int g = gb + 4 * u;                                       // (wave-uniform)
            if (g >= G) break;
            float gd = 0.f, gy = 0.f;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                if (p > 0 && lane + 64 * p >= K4) continue;
                const float4 yv = yq[u][p];
                const float4 dv = dq[u][p];
                const float d0 = (!relu || __builtin_fmaf(yv.x, sc, sh) > 0.f) ? dv.x : 0.f;
                const float d1 = (!relu || __builtin_fmaf(yv.y, sc, sh) > 0.f) ? dv.y : 0.f;
                const float d2 = (!relu || __builtin_fmaf(yv.z, sc, sh) > 0.f) ? dv.z : 0.f;
                const float d3 = (!relu || __builtin_fmaf(yv.w, sc, sh) > 0.f) ? dv.w : 0.f;
                const float qd = (d0 + d1) + (d2 + d3);
                const float qy = (yv.x + yv.y) + (yv.z + yv.w);
                gd = p == 0 ? qd : gd + qd;
                gy = p == 0 ? qy : gy + qy;
                mx = fmaxf(fmaxf(mx, fmaxf(fabsf(d0), fabsf(d1))), fmaxf(fabsf(d2), fabsf(d3)));
                s1 += qd;
                s2 = __builtin_fmaf(d0, (yv.x - mu) * is, s2);
                s2 = __builtin_fmaf(d1, (yv.y - mu) * is, s2);
                s2 = __builtin_fmaf(d2, (yv.z - mu) * is, s2);
                s2 = __builtin_fmaf(d3, (yv.w - mu) * is, s2);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                gd += __shfl_xor(gd, off);
                gy += __shfl_xor(gy, off);
            }
            if (lane == 0) { g0[g] = gd; g1[g] = gy; }
        }
    }
    bn_bwd_block_reduce(s1, s2, mx, partial, rowid, nrows, want_max);
}

}  // namespace

extern "C" int usip_group_max_wide_f32(const float* y, const float* coef, int relu, float* pooled, int32_t* arg,
                                       float* yarg, int B, int C, int M, int K, void* stream)
{
    const long long rows = (long long)B * C * M;
    if (B < 0 || C < 1 || M < 0 || K % 4 != 0 || K <= 256 || K > 1024) return USIP_EINVAL;
    if (rows == 0) return USIP_OK;
    if (!y || !pooled || !arg || (reinterpret_cast<uintptr_t>(y) & 15u)) return USIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int np = (K + 255) / 256, rpw = np == 2 ? 2 : 1;
    const long long blocks = (rows + 4 * rpw - 1) / (4 * rpw);
    if (blocks > 0x7fffffffLL) return USIP_EINVAL;
    const bool nans = !(coef && relu);                       // what passed through fmaxf(., 0) cannot be NaN
#define USIP_GMW(NP_)                                                                                              \
    if (np == NP_) {                                                                                               \
        if (nans)                                                                                                  \
            USIP_LAUNCH((group_max_wide_kernel<NP_, true>), dim3((unsigned)blocks), dim3(256), 0, st, y, pooled, arg, rows, \
                        coef, relu, C, M, yarg, K / 4);                                                            \
        else                                                                                                       \
            USIP_LAUNCH((group_max_wide_kernel<NP_, false>), dim3((unsigned)blocks), dim3(256), 0, st, y, pooled, arg, rows, \
                        coef, relu, C, M, yarg, K / 4);                                                            \
    }
    USIP_GMW(2) USIP_GMW(3) USIP_GMW(4)
#undef USIP_GMW
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_bn_backward_reduce_wide_f32(const float* dZ, const float* Y, const float* coef_fwd,
                                                const float* mean, const float* invstd, const float* gamma,
                                                int relu, float* partial, float* dgamma, float* dbeta,
                                                float* coef4, float* gsum, int group,
                                                int nb, int C, int P, int want_bound, void* stream)
{
    if (nb < 1 || C < 1 || P < 1 || !dZ || !Y || !partial || !gsum || !coef_fwd || !mean || !invstd) return USIP_EINVAL;
    if (group % 4 != 0 || group <= 256 || group > 1024 || P % group != 0 ||
        (reinterpret_cast<uintptr_t>(dZ) & 15u) || (reinterpret_cast<uintptr_t>(Y) & 15u))
        return USIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)nb * C;
    if (rows > 0x7fffffffLL) return USIP_EINVAL;
    const int np = (group + 255) / 256;
#define USIP_BNW(NP_)                                                                                              \
    if (np == NP_)                                                                                                 \
        USIP_LAUNCH((bn_bwd_reduce_wide_kernel<NP_>), dim3((unsigned)rows), dim3(256), 0, st, dZ, Y, coef_fwd, mean, \
                    invstd, partial, gsum, relu, C, P, (int)rows, group, want_bound);
    USIP_BNW(2) USIP_BNW(3) USIP_BNW(4)
#undef USIP_BNW
    USIP_LAUNCH_CHECK();
    USIP_LAUNCH(bn_bwd_finalize_kernel, dim3(usip_ceil_div(C, 64)), dim3(64), 0, st, partial, nb, C,
                (double)nb * (double)P, gamma, coef_fwd, mean, invstd, dgamma, dbeta, coef4, want_bound);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
