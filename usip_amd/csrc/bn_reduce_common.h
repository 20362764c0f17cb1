// usip_amd/csrc/bn_reduce_common.h -- what the BatchNorm-backward reduction passes share (shared_mlp.hip, group_wide.hip):
// the block reduction that ends a (cloud, channel) row and the finalisation over the rows of a channel.
#pragma once
#include "common.h"

namespace {

// The end of a 256-thread workgroup's pass over one (cloud, channel) row: the per-lane sums s1, s2 and the per-lane maximum
// mx go down each wave, the four waves' results through LDS, and thread 0 writes partial[{0, 1, 2}][rowid] in a fixed order.
__device__ __forceinline__ void bn_bwd_block_reduce(float s1, float s2, float mx, float* __restrict__ partial,
                                                    long long rowid, int nrows, int want_max)
{
    __shared__ float red[3][4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); mx = fmaxf(mx, __shfl_down(mx, off));
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s1; red[1][threadIdx.x >> 6] = s2; red[2][threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[rowid] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        partial[nrows + rowid] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        if (want_max) partial[2LL * nrows + rowid] = fmaxf(fmaxf(red[2][0], red[2][1]), fmaxf(red[2][2], red[2][3]));
    }
}

// dgamma = sum2, dbeta = sum1, and the PRO_BN_BWD coefficients
//   dY = gamma*invstd * (dYhat - mean(dYhat) - yhat * mean(dYhat*yhat)) = a1*dYhat + q1*y + q0
__global__ __launch_bounds__(64) void bn_bwd_finalize_kernel(
    const float* __restrict__ partial, int nb, int C, double count, const float* __restrict__ gamma,
    const float* __restrict__ coef_fwd, const float* __restrict__ mean, const float* __restrict__ invstd,
    float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ coef4, int want_bound)
{
    const int ch = blockIdx.x * 64 + threadIdx.x;
    const long long nrows = (long long)nb * C;
    float bound = 0.f;
    if (ch < C) {
        double s1 = 0.0, s2 = 0.0;
        float mx = 0.f;
        int b = 0;
        // eight rows per pass, all loads issued before the first addition (one row per pass was a chain of nb load
        // latencies: 8-10 us at nb = 16); same order of additions
        for (; b + 7 < nb; b += 8) {
            float u[8], v[8], w[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                u[i] = partial[(long long)(b + i) * C + ch];
                v[i] = partial[nrows + (long long)(b + i) * C + ch];
                w[i] = want_bound ? partial[2 * nrows + (long long)(b + i) * C + ch] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) { s1 += (double)u[i]; s2 += (double)v[i]; mx = fmaxf(mx, w[i]); }
        }
        for (; b < nb; ++b) {
            s1 += (double)partial[(long long)b * C + ch];
            s2 += (double)partial[nrows + (long long)b * C + ch];
            if (want_bound) mx = fmaxf(mx, partial[2 * nrows + (long long)b * C + ch]);
        }
        if (dbeta) dbeta[ch] = (float)s1;
        if (dgamma) dgamma[ch] = (float)s2;
        if (coef4) {
            const float a1 = coef_fwd[ch], a0 = coef_fwd[C + ch];
            const float is = invstd[ch], mu = mean[ch];
            const float c1m = (float)(s1 / count), c2m = (float)(s2 / count);
            coef4[ch] = a1;
            coef4[C + ch] = a0;
            coef4[2 * C + ch] = -a1 * c2m * is;
            coef4[3 * C + ch] = a1 * (c2m * is * mu - c1m);
            // |dY| = |a1| |dYhat - c1m - yhat c2m| <= |a1| (max|dYhat| + |c1m| + |c2m| sqrt(n)):  |yhat| <= sqrt(n) for
            // batch statistics over n samples (n (y - mean)^2 <= n sum (y - mean)^2 = n^2 var)
            bound = fabsf(a1) * (mx + fabsf(c1m) + fabsf(c2m) * (float)sqrt(count));
        }
    }
    if (want_bound && coef4) {
        // row 4 of coef4 ([5][C]): entry i = bound of |dY| over the channels [64 i, 64 i + 64) -- what the split-fp16
        // kernels scale their streamed operand by (they take the max over the ceil(C/64) entries)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) bound = fmaxf(bound, __shfl_down(bound, off));
        if (threadIdx.x == 0) coef4[4 * C + blockIdx.x] = bound;
    }
    (void)gamma;
}

}  // namespace
