// usip_amd/csrc/registration.hip -- evaluation on the device: RANSAC registration of matched keypoints,
// keypoint repeatability and descriptor matching on ragged batches.  Replaces the reference's MATLAB evaluation
// (evaluation/matlab/eval_outdoor/kitti/evaluate_kitti.m with external/ransacfitRt.m, ransac.m, estimateRt.m,
// estimateRigidTransform.m, Utils.compareTransform; eval_repeatability/eval_rep.m); csrc/registration_math.h has the
// semantics and the arithmetic, which the host twin (csrc/registration_cpu.cpp) shares.  No launch synchronises.
// The RANSAC kernels also serve the indoor fragment evaluation (csrc/fragments.hip): up to NMAX = 10240
// correspondences per pair.  Each has a second form for pairs of one chunk (Nmax <= CHUNK), which the entry point picks:
// ransac_trials_resident_kernel and ransac_select_resident_kernel compute the same bits a few per cent faster at the
// outdoor evaluation's shapes.
//
//   ransac_trials_kernel   grid (T / 256, P), one lane per trial: triplet (read from memory) -> rigid fit (float64, 4x4
//                          Jacobi in registers); then the pair's 6 x count float32 coordinates go through LDS in chunks of
//                          CHUNK rows (24 KB) and every lane walks a chunk at the same LDS address (a broadcast read),
//                          keeping its hypothesis and a running inlier count across chunks.  A trial's score does not
//                          depend on the trials before it, so all T run in parallel.
//   ransac_select_kernel   one workgroup per pair: ransac.m's sequential loop over the T scores, evaluated per trial in
//                          parallel (the budget N is a function of the running maximum alone: a max-scan, one budget per
//                          trial, the first trial that ends the loop), the chosen hypothesis' inliers (the flags live
//                          in the mask it writes, so nothing per correspondence stays in registers), the refit over
//                          ALL inliers with sums in a fixed order (lane-strided partial sums, then a binary tree: no
//                          floating-point atomics, bit-reproducible and the host twin's order), compareTransform.
//   repeatability_kernel   grid (Ma / 256, P): R_gt pos + t_gt staged in LDS as float64 (CHUNK rows at a time), one lane per
//                          anchor keypoint;
//   repeat_count_kernel    one workgroup per pair: hits and ratio.
//   nearest_counted_kernel one wave per anchor descriptor, the arithmetic of nearest_nd_kernel (csrc/nearest.hip: an FMA
//                          chain over the channels, sqrtf, first index on ties) with per-frame counts on both sides.
#include "common.h"
#include "registration_math.h"

using namespace usip_reg;

namespace {

constexpr int RT = 256;

template <class Src>
__global__ __launch_bounds__(RT) void ransac_trials_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                           const int32_t* __restrict__ count, int Nmax, int T,
                                                           double threshold, Src src, int32_t* __restrict__ counts,
                                                           double* __restrict__ hyp, int32_t* __restrict__ drawn)
{
    __shared__ float pts[CHUNK][6];
    const int p = blockIdx.y, t = blockIdx.x * RT + threadIdx.x;
    const int n = clamp_count(count, p, Nmax);
    const float* a = x1 + (long long)p * 3 * Nmax;
    const float* b = x2 + (long long)p * 3 * Nmax;
    const long long o = (long long)p * T + t;
    if (n < 3) {                                          // ransacfitRt returns before any trial (workgroup-uniform)
        if (t < T) {
            counts[o] = 0;
            if (hyp) for (int k = 0; k < 12; ++k) hyp[o * 12 + k] = 0.0;
            if (drawn) for (int k = 0; k < 3; ++k) drawn[o * 3 + k] = 0;
        }
        return;
    }
    const bool live = t < T;
    int idx[3] = {0, 0, 0};
    double Rt[12];
    {
        if (live) src.get(p, t, n, T, idx);
        double x[3][3], y[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                x[k][c] = (double)a[(long long)c * Nmax + idx[k]];
                y[k][c] = (double)b[(long long)c * Nmax + idx[k]];
            }
        fit3(x, y, Rt);
    }
    int hits = 0;
    for (int base = 0; base < n; base += CHUNK) {
        const int m = min(CHUNK, n - base);
        __syncthreads();                                  // the previous chunk has been read
        for (int i = threadIdx.x; i < m; i += RT) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                pts[i][k] = a[(long long)k * Nmax + base + i];
                pts[i][3 + k] = b[(long long)k * Nmax + base + i];
            }
        }
        __syncthreads();
        for (int i = 0; i < m; ++i) {
            const double d = residual(Rt, (double)pts[i][0], (double)pts[i][1], (double)pts[i][2], (double)pts[i][3],
                                      (double)pts[i][4], (double)pts[i][5]);
            hits += d < threshold ? 1 : 0;
        }
    }
    if (!live) return;
    counts[o] = hits;
    if (hyp)
#pragma unroll
        for (int k = 0; k < 12; ++k) hyp[o * 12 + k] = Rt[k];
    if (drawn)
#pragma unroll
        for (int k = 0; k < 3; ++k) drawn[o * 3 + k] = idx[k];
}

// The pair fits one chunk (Nmax <= CHUNK, the outdoor evaluation): staged once, the triplet read from LDS, lanes beyond T
// gone after the one barrier.  Same values in the same order as ransac_trials_kernel, hence the same bits; kept because
// the chunked form measured 4 % slower at 8 pairs of 512.
template <class Src>
__global__ __launch_bounds__(RT) void ransac_trials_resident_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                           const int32_t* __restrict__ count, int Nmax, int T,
                                                           double threshold, Src src, int32_t* __restrict__ counts,
                                                           double* __restrict__ hyp, int32_t* __restrict__ drawn)
{
    __shared__ float pts[CHUNK][6];
    const int p = blockIdx.y, t = blockIdx.x * RT + threadIdx.x;
    const int n = clamp_count(count, p, Nmax);
    const float* a = x1 + (long long)p * 3 * Nmax;
    const float* b = x2 + (long long)p * 3 * Nmax;
    for (int i = threadIdx.x; i < n; i += RT) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            pts[i][k] = a[(long long)k * Nmax + i];
            pts[i][3 + k] = b[(long long)k * Nmax + i];
        }
    }
    __syncthreads();
    if (t >= T) return;
    const long long o = (long long)p * T + t;
    if (n < 3) {                                          // ransacfitRt returns before any trial
        counts[o] = 0;
        if (hyp) for (int k = 0; k < 12; ++k) hyp[o * 12 + k] = 0.0;
        if (drawn) for (int k = 0; k < 3; ++k) drawn[o * 3 + k] = 0;
        return;
    }
    int idx[3];
    src.get(p, t, n, T, idx);
    double x[3][3], y[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[k][c] = (double)pts[idx[k]][c];
            y[k][c] = (double)pts[idx[k]][3 + c];
        }
    double Rt[12];
    fit3(x, y, Rt);
    int hits = 0;
    for (int i = 0; i < n; ++i) {
        const double d = residual(Rt, (double)pts[i][0], (double)pts[i][1], (double)pts[i][2], (double)pts[i][3],
                                  (double)pts[i][4], (double)pts[i][5]);
        hits += d < threshold ? 1 : 0;
    }
    counts[o] = hits;
    if (hyp)
#pragma unroll
        for (int k = 0; k < 12; ++k) hyp[o * 12 + k] = Rt[k];
    if (drawn)
#pragma unroll
        for (int k = 0; k < 3; ++k) drawn[o * 3 + k] = idx[k];
}

template <class Src>
__global__ __launch_bounds__(REFIT_LANES) void ransac_select_kernel(const float* __restrict__ x1,
                                                                    const float* __restrict__ x2,
                                                                    const int32_t* __restrict__ count, int Nmax, int T,
                                                                    int max_trials, double threshold, Src src,
                                                                    const int32_t* __restrict__ counts,
                                                                    const double* __restrict__ gt, SelectOut out)
{
    __shared__ double part[REFIT_LANES][10];
    __shared__ double sRt[12], cen[6];
    __shared__ int scan[REFIT_LANES];
    __shared__ int s_exit, s_best, s_chosen, s_inl;
    const int p = blockIdx.x, l = threadIdx.x;
    const int n = clamp_count(count, p, Nmax);
    const float* a = x1 + (long long)p * 3 * Nmax;
    const float* b = x2 + (long long)p * 3 * Nmax;
    uint8_t* mask = out.inlier_mask + (long long)p * Nmax;
    if (l == 0) { s_exit = 0x7fffffff; s_best = 0; s_chosen = 0; s_inl = 0; }
    __syncthreads();

    int trialcount = 0;
    if (n > 3) {
        const int32_t* sc = counts + (long long)p * T;
        int carry = 0;
        for (int base = 0; base <= max_trials; base += REFIT_LANES) {
            const int t = base + l;
            scan[l] = t <= max_trials ? sc[t] : -1;
            __syncthreads();
            for (int off = 1; off < REFIT_LANES; off <<= 1) {          // inclusive max-scan
                const int v = l >= off ? scan[l - off] : -1;
                __syncthreads();
                scan[l] = max(scan[l], v);
                __syncthreads();
            }
            const int pm = max(carry, scan[l]);                        // ransac.m's bestscore after trial t
            if (t <= max_trials && (t + 1 > max_trials || !(trials_needed(pm, n) > (double)(t + 1))))
                atomicMin(&s_exit, t);
            carry = max(carry, scan[REFIT_LANES - 1]);
            __syncthreads();
            if (s_exit != 0x7fffffff) {
                if (t == s_exit) s_best = pm;
                break;
            }
        }
        __syncthreads();
        const int te = s_exit, best = s_best;
        for (int t = l; t <= te; t += REFIT_LANES)
            if (sc[t] == best) atomicMax(&s_chosen, t);                // ties: the later trial
        __syncthreads();
        trialcount = te + 1;
    }

    if (n >= 3 && l == 0) {
        int idx[3] = {0, 1, 2};
        if (n > 3) src.get(p, s_chosen, n, T, idx);
        double x[3][3], y[3][3];
        for (int k = 0; k < 3; ++k)
            for (int c = 0; c < 3; ++c) {
                x[k][c] = (double)a[(long long)c * Nmax + idx[k]];
                y[k][c] = (double)b[(long long)c * Nmax + idx[k]];
            }
        double Rt[12];
        fit3(x, y, Rt);
        for (int k = 0; k < 12; ++k) sRt[k] = Rt[k];
    }
    __syncthreads();

    // the chosen hypothesis' inlier set (count == 3: the three, unconditionally), kept in the mask: lane l owns the rows
    // l, l + 256, ... in every pass below, so it reads back only what it wrote itself
    int mine = 0;
    {
        double Rt[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Rt[k] = sRt[k];
        for (int i = l; i < Nmax; i += REFIT_LANES) {
            bool in = false;
            if (i < n && n >= 3)
                in = n == 3 || residual(Rt, (double)a[i], (double)a[(long long)Nmax + i], (double)a[2LL * Nmax + i],
                                        (double)b[i], (double)b[(long long)Nmax + i], (double)b[2LL * Nmax + i]) < threshold;
            mask[i] = in ? 1 : 0;
            mine += in ? 1 : 0;
        }
    }
    if (mine) atomicAdd(&s_inl, mine);
    __syncthreads();
    const int ninl = s_inl;
    const bool ok = ninl >= 3;
    if (!ok && mine)
        for (int i = l; i < n; i += REFIT_LANES) mask[i] = 0;

    if (ok) {                                                          // block-uniform
        // centroids: lane l adds its rows in index order, then the tree
#pragma unroll
        for (int k = 0; k < 10; ++k) part[l][k] = 0.0;
        for (int i = l; i < n; i += REFIT_LANES)
            if (mask[i]) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    part[l][c] += (double)a[(long long)c * Nmax + i];
                    part[l][3 + c] += (double)b[(long long)c * Nmax + i];
                }
            }
        tree_sum<6>(part, l);
        if (l < 6) cen[l] = part[0][l] / (double)ninl;
        __syncthreads();
        double B[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = l; i < n; i += REFIT_LANES)
            if (mask[i]) {
                double xc[3], yc[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    xc[c] = (double)a[(long long)c * Nmax + i] - cen[c];
                    yc[c] = (double)b[(long long)c * Nmax + i] - cen[3 + c];
                }
                accumulate(B, xc, yc);
            }
#pragma unroll
        for (int k = 0; k < 10; ++k) part[l][k] = B[k];
        tree_sum<10>(part, l);
    }
    if (l != 0) return;
    double Rt[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) {
        double Bs[10];
        for (int k = 0; k < 10; ++k) Bs[k] = part[0][k];
        const double cx[3] = {cen[0], cen[1], cen[2]}, cy[3] = {cen[3], cen[4], cen[5]};
        transform_from(Bs, cx, cy, Rt);
    }
    for (int k = 0; k < 12; ++k) out.Rt[(long long)p * 12 + k] = Rt[k];
    out.inliers[p] = ok ? ninl : 0;
    out.trialcount[p] = trialcount;
    out.valid[p] = ok ? 1 : 0;
    if (out.chosen) out.chosen[p] = s_chosen;
    if (gt) {
        double dt = 3.0, dd = 6.0;                                     // evaluate_kitti.m's catch values
        if (ok) compare(gt + (long long)p * 12, Rt, &dt, &dd);
        out.delta_t[p] = dt;
        out.delta_deg[p] = dd;
    }
}

// The pair fits one chunk (Nmax <= CHUNK): lane l keeps the flags of its CHUNK / 256 rows in registers and reads no mask
// back.  The scan, the tie rule and the refit's order are ransac_select_kernel's line for line, hence the same bits; kept
// because the mask-resident form measured 1 us (2 %) slower at 8 pairs of 512.
template <class Src>
__global__ __launch_bounds__(REFIT_LANES) void ransac_select_resident_kernel(const float* __restrict__ x1,
                                                                    const float* __restrict__ x2,
                                                                    const int32_t* __restrict__ count, int Nmax, int T,
                                                                    int max_trials, double threshold, Src src,
                                                                    const int32_t* __restrict__ counts,
                                                                    const double* __restrict__ gt, SelectOut out)
{
    __shared__ double part[REFIT_LANES][10];
    __shared__ double sRt[12], cen[6];
    __shared__ int scan[REFIT_LANES];
    __shared__ int s_exit, s_best, s_chosen, s_inl;
    const int p = blockIdx.x, l = threadIdx.x;
    const int n = clamp_count(count, p, Nmax);
    const float* a = x1 + (long long)p * 3 * Nmax;
    const float* b = x2 + (long long)p * 3 * Nmax;
    uint8_t* mask = out.inlier_mask + (long long)p * Nmax;
    if (l == 0) { s_exit = 0x7fffffff; s_best = 0; s_chosen = 0; s_inl = 0; }
    __syncthreads();

    int trialcount = 0;
    if (n > 3) {
        const int32_t* sc = counts + (long long)p * T;
        int carry = 0;
        for (int base = 0; base <= max_trials; base += REFIT_LANES) {
            const int t = base + l;
            scan[l] = t <= max_trials ? sc[t] : -1;
            __syncthreads();
            for (int off = 1; off < REFIT_LANES; off <<= 1) {          // inclusive max-scan
                const int v = l >= off ? scan[l - off] : -1;
                __syncthreads();
                scan[l] = max(scan[l], v);
                __syncthreads();
            }
            const int pm = max(carry, scan[l]);                        // ransac.m's bestscore after trial t
            if (t <= max_trials && (t + 1 > max_trials || !(trials_needed(pm, n) > (double)(t + 1))))
                atomicMin(&s_exit, t);
            carry = max(carry, scan[REFIT_LANES - 1]);
            __syncthreads();
            if (s_exit != 0x7fffffff) {
                if (t == s_exit) s_best = pm;
                break;
            }
        }
        __syncthreads();
        const int te = s_exit, best = s_best;
        for (int t = l; t <= te; t += REFIT_LANES)
            if (sc[t] == best) atomicMax(&s_chosen, t);                // ties: the later trial
        __syncthreads();
        trialcount = te + 1;
    }

    if (n >= 3 && l == 0) {
        int idx[3] = {0, 1, 2};
        if (n > 3) src.get(p, s_chosen, n, T, idx);
        double x[3][3], y[3][3];
        for (int k = 0; k < 3; ++k)
            for (int c = 0; c < 3; ++c) {
                x[k][c] = (double)a[(long long)c * Nmax + idx[k]];
                y[k][c] = (double)b[(long long)c * Nmax + idx[k]];
            }
        double Rt[12];
        fit3(x, y, Rt);
        for (int k = 0; k < 12; ++k) sRt[k] = Rt[k];
    }
    __syncthreads();

    // the chosen hypothesis' inlier set (count == 3: the three, unconditionally)
    bool in[CHUNK / REFIT_LANES];
    int mine = 0;
#pragma unroll
    for (int r = 0; r < CHUNK / REFIT_LANES; ++r) {
        const int i = r * REFIT_LANES + l;
        in[r] = false;
        if (i < n && n >= 3) {
            double Rt[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) Rt[k] = sRt[k];
            in[r] = n == 3 || residual(Rt, (double)a[i], (double)a[(long long)Nmax + i], (double)a[2LL * Nmax + i],
                                       (double)b[i], (double)b[(long long)Nmax + i], (double)b[2LL * Nmax + i]) < threshold;
        }
        mine += in[r] ? 1 : 0;
    }
    if (mine) atomicAdd(&s_inl, mine);
    __syncthreads();
    const int ninl = s_inl;
    const bool ok = ninl >= 3;
    for (int i = l; i < Nmax; i += REFIT_LANES) mask[i] = 0;
#pragma unroll
    for (int r = 0; r < CHUNK / REFIT_LANES; ++r) {
        const int i = r * REFIT_LANES + l;
        if (i < Nmax && in[r] && ok) mask[i] = 1;
    }

    if (ok) {                                                          // block-uniform
        // centroids: lane l adds its rows in index order, then the tree
#pragma unroll
        for (int k = 0; k < 10; ++k) part[l][k] = 0.0;
#pragma unroll
        for (int r = 0; r < CHUNK / REFIT_LANES; ++r) {
            const int i = r * REFIT_LANES + l;
            if (in[r]) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    part[l][c] += (double)a[(long long)c * Nmax + i];
                    part[l][3 + c] += (double)b[(long long)c * Nmax + i];
                }
            }
        }
        tree_sum<6>(part, l);
        if (l < 6) cen[l] = part[0][l] / (double)ninl;
        __syncthreads();
        double B[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < CHUNK / REFIT_LANES; ++r) {
            const int i = r * REFIT_LANES + l;
            if (in[r]) {
                double xc[3], yc[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    xc[c] = (double)a[(long long)c * Nmax + i] - cen[c];
                    yc[c] = (double)b[(long long)c * Nmax + i] - cen[3 + c];
                }
                accumulate(B, xc, yc);
            }
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) part[l][k] = B[k];
        tree_sum<10>(part, l);
    }
    if (l != 0) return;
    double Rt[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) {
        double Bs[10];
        for (int k = 0; k < 10; ++k) Bs[k] = part[0][k];
        const double cx[3] = {cen[0], cen[1], cen[2]}, cy[3] = {cen[3], cen[4], cen[5]};
        transform_from(Bs, cx, cy, Rt);
    }
    for (int k = 0; k < 12; ++k) out.Rt[(long long)p * 12 + k] = Rt[k];
    out.inliers[p] = ok ? ninl : 0;
    out.trialcount[p] = trialcount;
    out.valid[p] = ok ? 1 : 0;
    if (out.chosen) out.chosen[p] = s_chosen;
    if (gt) {
        double dt = 3.0, dd = 6.0;                                     // evaluate_kitti.m's catch values
        if (ok) compare(gt + (long long)p * 12, Rt, &dt, &dd);
        out.delta_t[p] = dt;
        out.delta_deg[p] = dd;
    }
}

__global__ __launch_bounds__(64) void compare_kernel(const double* __restrict__ gt, const double* __restrict__ Rt,
                                                     int P, double* __restrict__ delta_t, double* __restrict__ delta_deg)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= P) return;
    compare(gt + (long long)p * 12, Rt + (long long)p * 12, delta_t + p, delta_deg + p);
}

__global__ __launch_bounds__(RT) void repeatability_kernel(const float* __restrict__ anc, const int32_t* __restrict__ anc_count,
                                                           const float* __restrict__ pos, const int32_t* __restrict__ pos_count,
                                                           const double* __restrict__ gt, int Ma, int Mp,
                                                           double* __restrict__ min_dist)
{
    __shared__ double q[3][CHUNK];
    const int p = blockIdx.y, i = blockIdx.x * RT + threadIdx.x;
    const int na = clamp_count(anc_count, p, Ma), np = clamp_count(pos_count, p, Mp);
    const float* A = anc + (long long)p * 3 * Ma;
    const float* Q = pos + (long long)p * 3 * Mp;
    const double* G = gt + (long long)p * 12;
    const bool live = i < na;
    const double ax = live ? (double)A[i] : 0.0, ay = live ? (double)A[(long long)Ma + i] : 0.0,
                 az = live ? (double)A[2LL * Ma + i] : 0.0;
    double best = (double)__builtin_inff();
    for (int base = 0; base < np; base += CHUNK) {
        const int m = min(CHUNK, np - base);
        __syncthreads();
        for (int j = threadIdx.x; j < m; j += RT) {                    // Utils.apply_transform
            const double y0 = (double)Q[base + j], y1 = (double)Q[(long long)Mp + base + j], y2 = (double)Q[2LL * Mp + base + j];
#pragma unroll
            for (int c = 0; c < 3; ++c) q[c][j] = ((G[4 * c] * y0 + G[4 * c + 1] * y1) + G[4 * c + 2] * y2) + G[4 * c + 3];
        }
        __syncthreads();
        for (int j = 0; j < m; ++j) {
            const double d0 = ax - q[0][j], d1 = ay - q[1][j], d2 = az - q[2][j];
            const double d = (d0 * d0 + d1 * d1) + d2 * d2;
            best = d < best ? d : best;
        }
    }
    if (i < Ma) min_dist[(long long)p * Ma + i] = live ? sqrt(best) : (double)__builtin_inff();
}

__global__ __launch_bounds__(RT) void repeat_count_kernel(const double* __restrict__ min_dist, const int32_t* __restrict__ anc_count,
                                                          int Ma, double radius, int32_t* __restrict__ hits,
                                                          double* __restrict__ ratio)
{
    __shared__ int s_hits;
    const int p = blockIdx.x;
    const int na = clamp_count(anc_count, p, Ma);
    if (threadIdx.x == 0) s_hits = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < na; i += RT) mine += min_dist[(long long)p * Ma + i] < radius ? 1 : 0;
    if (mine) atomicAdd(&s_hits, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        hits[p] = s_hits;
        ratio[p] = na > 0 ? (double)s_hits / (double)na : 0.0;
    }
}

constexpr int NJ = 4;       // candidates in flight per lane

__global__ __launch_bounds__(256) void nearest_counted_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                              const int32_t* __restrict__ a_count,
                                                              const int32_t* __restrict__ b_count, float* __restrict__ min_d,
                                                              int32_t* __restrict__ arg, int C, int Ma, int Nb)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bi = blockIdx.y;
    if (i >= Ma) return;
    const int na = clamp_count(a_count, bi, Ma), nb = clamp_count(b_count, bi, Nb);
    const long long o = (long long)bi * Ma + i;
    if (i >= na || nb < 1) {                                           // padding rows: a defined value, never data
        if (lane == 0) { min_d[o] = __builtin_inff(); arg[o] = 0; }
        return;
    }
    const float* ab = a + (long long)bi * C * Ma;
    const float* bb = b + (long long)bi * C * Nb;
    float best = __builtin_inff();
    int bj = 0x7fffffff;
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
            if (j < nb) {
                const float d = sqrtf(s[u]);
                if (d < best) { best = d; bj = j; }                    // ascending j per lane: the first stays
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float od = __shfl_xor(best, off);
        const int oj = __shfl_xor(bj, off);
        if (od < best || (od == best && oj < bj)) { best = od; bj = oj; }
    }
    if (lane == 0) {
        min_d[o] = best;
        arg[o] = (bj == 0x7fffffff) ? 0 : bj;
    }
}

bool shape_ok(int P, int Nmax, int T) { return P >= 0 && P <= 65535 && Nmax >= 1 && Nmax <= NMAX && T >= 1; }

template <class Src>
int launch_trials(const float* x1, const float* x2, const int32_t* count, int P, int Nmax, int T, double threshold,
                  const Src& src, int32_t* counts, double* hyp, int32_t* drawn, hipStream_t stream)
{
    if (Nmax <= CHUNK)
        USIP_LAUNCH(ransac_trials_resident_kernel<Src>, dim3(usip_ceil_div(T, RT), P), dim3(RT), 0, stream, x1, x2, count,
                    Nmax, T, threshold, src, counts, hyp, drawn);
    else
        USIP_LAUNCH(ransac_trials_kernel<Src>, dim3(usip_ceil_div(T, RT), P), dim3(RT), 0, stream, x1, x2, count, Nmax, T,
                    threshold, src, counts, hyp, drawn);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

template <class Src>
int launch_select(const float* x1, const float* x2, const int32_t* count, int P, int Nmax, int T, int max_trials,
                  double threshold, const Src& src, const int32_t* counts, const double* gt, const SelectOut& out,
                  hipStream_t stream)
{
    if (Nmax <= CHUNK)
        USIP_LAUNCH(ransac_select_resident_kernel<Src>, dim3(P), dim3(REFIT_LANES), 0, stream, x1, x2, count, Nmax, T,
                    max_trials, threshold, src, counts, gt, out);
    else
        USIP_LAUNCH(ransac_select_kernel<Src>, dim3(P), dim3(REFIT_LANES), 0, stream, x1, x2, count, Nmax, T, max_trials,
                    threshold, src, counts, gt, out);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

}  // namespace

extern "C" int usip_ransac_trials_f32(const float* x1, const float* x2, const int32_t* count, int P, int Nmax, int T,
                                      double threshold, uint64_t seed, const int64_t* pair_ids, int32_t* counts,
                                      double* hypotheses, int32_t* triplets_out, void* stream)
{
    if (!shape_ok(P, Nmax, T)) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!x1 || !x2 || !count || !counts) return USIP_EINVAL;
    const PhiloxTriplets src{seed, pair_ids};
    return launch_trials(x1, x2, count, P, Nmax, T, threshold, src, counts, hypotheses, triplets_out, (hipStream_t)stream);
}

extern "C" int usip_ransac_trials_explicit_f32(const float* x1, const float* x2, const int32_t* count, int P, int Nmax,
                                               int T, double threshold, const int32_t* triplets, int32_t* counts,
                                               double* hypotheses, void* stream)
{
    if (!shape_ok(P, Nmax, T)) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!x1 || !x2 || !count || !counts || !triplets) return USIP_EINVAL;
    const ExplicitTriplets src{triplets};
    return launch_trials(x1, x2, count, P, Nmax, T, threshold, src, counts, hypotheses, nullptr, (hipStream_t)stream);
}

extern "C" int usip_ransac_select_f32(const float* x1, const float* x2, const int32_t* count, int P, int Nmax, int T,
                                      int max_trials, double threshold, uint64_t seed, const int64_t* pair_ids,
                                      const int32_t* triplets, const int32_t* counts, const double* gt, double* Rt,
                                      uint8_t* inlier_mask, int32_t* inliers, int32_t* trialcount, uint8_t* valid,
                                      int32_t* chosen, double* delta_t, double* delta_deg, void* stream)
{
    if (!shape_ok(P, Nmax, T) || max_trials < 0 || max_trials > T - 1) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!x1 || !x2 || !count || !counts || !Rt || !inlier_mask || !inliers || !trialcount || !valid) return USIP_EINVAL;
    if (gt && (!delta_t || !delta_deg)) return USIP_EINVAL;
    const SelectOut out{Rt, inlier_mask, inliers, trialcount, valid, chosen, delta_t, delta_deg};
    hipStream_t st = (hipStream_t)stream;
    if (triplets)
        return launch_select(x1, x2, count, P, Nmax, T, max_trials, threshold, ExplicitTriplets{triplets}, counts, gt, out,
                             st);
    return launch_select(x1, x2, count, P, Nmax, T, max_trials, threshold, PhiloxTriplets{seed, pair_ids}, counts, gt, out,
                         st);
}

extern "C" int usip_compare_transform_f64(const double* gt, const double* Rt, int P, double* delta_t, double* delta_deg,
                                          void* stream)
{
    if (P < 0) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!gt || !Rt || !delta_t || !delta_deg) return USIP_EINVAL;
    USIP_LAUNCH(compare_kernel, dim3(usip_ceil_div(P, 64)), dim3(64), 0, (hipStream_t)stream, gt, Rt, P, delta_t, delta_deg);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_repeatability_f32(const float* anc, const int32_t* anc_count, const float* pos,
                                      const int32_t* pos_count, const double* gt, double radius, int P, int Ma, int Mp,
                                      double* min_dist, int32_t* hits, double* ratio, void* stream)
{
    if (P < 0 || P > 65535 || Ma < 1 || Mp < 1) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!anc || !anc_count || !pos || !pos_count || !gt || !min_dist || !hits || !ratio) return USIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    USIP_LAUNCH(repeatability_kernel, dim3(usip_ceil_div(Ma, RT), P), dim3(RT), 0, st, anc, anc_count, pos, pos_count, gt,
                Ma, Mp, min_dist);
    USIP_LAUNCH_CHECK();
    USIP_LAUNCH(repeat_count_kernel, dim3(P), dim3(RT), 0, st, min_dist, anc_count, Ma, radius, hits, ratio);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_nearest_nd_counted_f32(const float* a, const float* b, const int32_t* a_count, const int32_t* b_count,
                                           float* min_d, int32_t* arg, int B, int C, int Ma, int Nb, void* stream)
{
    if (B < 0 || B > 65535 || C < 1 || Ma < 0 || Nb < 1) return USIP_EINVAL;
    if ((long long)B * Ma == 0) return USIP_OK;
    if (!a || !b || !a_count || !b_count || !min_d || !arg) return USIP_EINVAL;
    USIP_LAUNCH(nearest_counted_kernel, dim3(usip_ceil_div(Ma, 4), B), dim3(256), 0, (hipStream_t)stream, a, b, a_count,
                b_count, min_d, arg, C, Ma, Nb);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
