// usip_amd/csrc/icp_math.h -- the arithmetic of trimmed point-to-point ICP between downsampled fragments,
// shared by the kernels of csrc/icp.hip and the host twin of csrc/icp_cpu.cpp.  The convention is f-9's: float32 inputs,
// float64 arithmetic, sums in a fixed order.  The move (xform), the distance (sqdist3) and the radius test (within) are
// csrc/fragments_math.h's; the rigid fit (accumulate, transform_from), the clamps and the tree sum are
// csrc/registration_math.h's.  This header adds the decisions of the loop: which candidate is nearer, when a tile of the
// walk cannot hold a nearer one, which rows the trim keeps, when the pair stops.
//
// Reference semantics (evaluation/matlab/eval_indoor/3dmatch/writeLogReconputeAlign.m): pcdownsample 'gridAverage' 0.04 of
// both fragments, pcregrigid(moving, fixed, 'InlierRatio', 0.3, 'InitialTransform', estimate) -- point to point, 20
// iterations, Tolerance [0.01 0.009] over the last three iterations by default -- then the share of moved points with a
// fixed point at sqrt(d2) < 0.05.  pcregrigid is a MATLAB built-in: include/usip_hip.h (f-13) states this project's own
// contract, written from the documented behaviour.
#pragma once
#include "fragments_math.h"

namespace usip_icp {

constexpr int LANES = 256;              // lanes of every workgroup; the strided sums' width (= usip_reg::REFIT_LANES)
constexpr int TILE = 256;               // fragment-1 rows per LDS tile of the walk
constexpr int MAX_ITERATIONS = 64;
constexpr int PLANE_SUMS = 27;          // f-28's fit (csrc/icp_plane_math.h): H_00 H_01 .. H_05 H_11 .. H_55, then g_0 .. g_5
constexpr int RUNNING = 0, STOPPED = 1, NOT_REFINED = 2;               // a pair's state between the launches
static_assert(LANES == usip_reg::REFIT_LANES, "the fit's sums go through registration_math.h's tree");

// A non-negative float64 orders as its bit pattern does.
USIP_HD unsigned long long bits_of(double v)
{
    unsigned long long u;
    __builtin_memcpy(&u, &v, 8);
    return u;
}
USIP_HD double double_of(unsigned long long u)
{
    double v;
    __builtin_memcpy(&v, &u, 8);
    return v;
}

// The candidate (d2, row) replaces the best: nearer, or as near with the lower row index.
USIP_HD bool better(double d2, int row, double best, int best_row) { return d2 < best || (d2 == best && row < best_row); }

// Every row at least gap > 0 away along x is farther than best: d2 = (dx dx + ..) + .. >= fl(dx dx) >= fl(gap gap) > best.
// Strict: a row at exactly the best distance may carry a lower index and must still be seen.
USIP_HD bool bound_met(double gap, double best) { return gap > 0.0 && gap * gap > best; }

// m of the trim, 1 <= m <= n2 (n2 >= 1, 0 < inlier_ratio <= 1)
USIP_HD int trim_count(double inlier_ratio, int n2)
{
    const long long m = (long long)floor(inlier_ratio * (double)n2);
    return (int)(m < 1 ? 1 : (m > (long long)n2 ? (long long)n2 : m));
}

// (d2_i, i) <= (d2*, i*), on bit patterns
USIP_HD bool kept(unsigned long long b, int i, unsigned long long cut, int icut) { return b < cut || (b == cut && i <= icut); }

USIP_HD bool finite12(const double* Rt)
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) ok = ok && (Rt[k] - Rt[k] == 0.0);
    return ok;
}

// dt = |t - t'|, dc = |R - R'|_F: nine squared differences added in row-major order
USIP_HD void pose_delta(const double* a, const double* b, double* dt, double* dc)
{
    const double e0 = a[3] - b[3], e1 = a[7] - b[7], e2 = a[11] - b[11];
    *dt = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double d = a[4 * r + c] - b[4 * r + c];
            s += d * d;
        }
    *dc = sqrt(s);
}

// h holds the last three values, the newest in h[2]; the mean of the last min(k, 3)
USIP_HD void push(double* h, double v) { h[0] = h[1]; h[1] = h[2]; h[2] = v; }
USIP_HD double recent_mean(const double* h, int k)
{
    return k >= 3 ? ((h[0] + h[1]) + h[2]) / 3.0 : (k == 2 ? (h[1] + h[2]) / 2.0 : h[2]);
}

}  // namespace usip_icp
