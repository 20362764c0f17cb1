// usip_amd/csrc/fpfh_math.h -- the arithmetic of the FPFH baseline descriptor, shared by the kernels of
// csrc/fpfh.hip and the host twin of csrc/fpfh_cpu.cpp: both sides run the same float64 operations in the same order on the
// float32 points of a frame, so their results are equal bit for bit.  It sits over prepare_math.h (sqdist), iss_math.h (member,
// the limits) and harris_math.h (has_normal).  No libm call feeds a decision or a result: only sqrt and division, which are
// correctly rounded on both sides, and fabs.
//
// Reference semantics: the reference's scoring scripts name hand-crafted descriptors (eval_indoor/3dmatch/evaluate.m:
// descriptorName = 'my'; % 3dmatch, spin, fpfh) that it does not contain.  What follows is this project's own definition of
// Fast Point Feature Histograms (Rusu, Blodow, Beetz 2009), written after PCL's FPFHEstimation / computePairFeatures with the
// deviations of DESIGN 8o:
//   normals        f64 rows as csrc/harris_math.h has them; a point whose row is all zero or not finite HAS NO NORMAL: it is a
//                  member of nobody, its SPFH row is zero and its member count is 0
//   membership     usip_iss::member over usip_prep::sqdist: d2 < r * r (strict; r * r once, in float64).  The point itself is
//                  not its own neighbour: a query counts every row with a normal and d2 < r2 and takes one off for itself
//                  when sqdist(p_i, p_i) < r2 (which fails only for non-finite coordinates)
//   pair (i, j)    d = p_j - p_i, f4 = sqrt(d2).  f4 == 0: a member that adds to no bin.  a1 = (n_i . d) / f4, a2 = (n_j . d)
//                  / f4; |a1| < |a2|: n1 = n_j, n2 = n_i, d = -d, f3 = -a2; otherwise (equality too) n1 = n_i, n2 = n_j, f3 =
//                  a1.  v = d x n1; |v| == 0: no bin; else v /= |v|, w = n1 x v, f2 = v . n2, y = w . n2, x = n1 . n2.  Every
//                  dot product is (a0 b0 + a1 b1) + a2 b2.
//   bins           h2 = bin11(f2), h3 = bin11(f3): t = (11 (f + 1)) / 2 truncated, 0 when !(t > 0), 10 when t >= 10.
//                  h1 = the sector of the angle of (x, y) among the eleven of width 2 pi / 11 from -pi, WITHOUT an inverse
//                  tangent: the number of boundaries phi_k = -pi + 2 pi k / 11, k = 1 .. 10, at or below the angle, where with
//                  b_k = (cos phi_k, sin phi_k) as the float64 literals below and c_k = b_k.x * y - b_k.y * x
//                    k <= 5 (phi_k < 0):  y >= 0 || c_k >= 0          k >= 6 (phi_k > 0):  y >= 0 && c_k >= 0
//                  (0, 0) is the angle 0: bin 5.  A zero y of either sign with x < 0 is the angle pi: bin 10, where PCL's
//                  clamp puts it.
//   SPFH           the integer counts of the three histograms, i32 [33] = h1 | 11 + h2 | 22 + h3, and the member count
//   FPFH           of a keypoint q (any position) over the cloud points j with members_j > 0 and 0 < d2(q, j) < r2:
//                  acc[bin] += ((double)spfh_j[bin] * (100.0 / members_j)) * (1.0 / d2); lane l of 64 takes the sorted positions
//                  lo + l + 64 k ascending, lo = first_within(); then lanes fold by the xor-butterfly 32, 16, 8, 4, 2, 1; then
//                  each block of eleven is scaled by 100 / (its sum, bins ascending) when that is positive
#pragma once
#include "harris_math.h"

// On the device a lane keeps the 33 sums in 66 registers; the fence keeps the compiler from putting all 33 counts of a row in
// flight beside them (eleven at a time fit the budget of four waves per SIMD).  It moves no arithmetic.
#if defined(__HIP_DEVICE_COMPILE__)
#define USIP_FPFH_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define USIP_FPFH_FENCE() ((void)0)
#endif

namespace usip_fpfh {

using usip_harris::has_normal;
using usip_iss::member;
using usip_prep::TILE;

constexpr int BINS = 11, WIDTH = 33, LANES = 64;
constexpr int MMAX = 65535;                                            // keypoints per frame

USIP_HD bool bad_keypoints(int M) { return M < 1 || M > MMAX; }

USIP_HD int bin11(double f)
{
    const double t = (11.0 * (f + 1.0)) / 2.0;
    return !(t > 0.0) ? 0 : (t >= 10.0 ? 10 : (int)t);
}

USIP_HD int at_or_above(double bx, double by, double x, double y, bool low)
{
    const bool c = bx * y - by * x >= 0.0, up = y >= 0.0;
    return (low ? (up || c) : (up && c)) ? 1 : 0;
}

USIP_HD int sector11(double x, double y)
{
    if (x == 0.0 && y == 0.0) return 5;
    return at_or_above(-0x1.aeb8c8764f0b9p-1, -0x1.14cedf8bb580dp-1, x, y, true) +
           at_or_above(-0x1.a9628d9c712b4p-2, -0x1.d1bb48eee2c14p-1, x, y, true) +
           at_or_above(0x1.2375f640f44dap-3, -0x1.fac9e043842efp-1, x, y, true) +
           at_or_above(0x1.4f49e7f775887p-1, -0x1.82f19bb3a28a1p-1, x, y, true) +
           at_or_above(0x1.eb42a9bcd5058p-1, -0x1.207e7fd768dbcp-2, x, y, true) +
           at_or_above(0x1.eb42a9bcd5058p-1, 0x1.207e7fd768dbcp-2, x, y, false) +
           at_or_above(0x1.4f49e7f775887p-1, 0x1.82f19bb3a28a1p-1, x, y, false) +
           at_or_above(0x1.2375f640f44dap-3, 0x1.fac9e043842efp-1, x, y, false) +
           at_or_above(-0x1.a9628d9c712b1p-2, 0x1.d1bb48eee2c15p-1, x, y, false) +
           at_or_above(-0x1.aeb8c8764f0bbp-1, 0x1.14cedf8bb580ap-1, x, y, false);
}

USIP_HD double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

struct Bins { int h1, h2, h3; };

// The three bins of the pair (query i at p with normal ni, member j at (xj, yj, zj) with normal nj, d2 = sqdist(p, j));
// false: the pair adds to no bin.
USIP_HD bool pair_bins(double xi, double yi, double zi, float xj, float yj, float zj, double d2, double ni0, double ni1,
                       double ni2, double nj0, double nj1, double nj2, Bins& out)
{
    const double f4 = sqrt(d2);
    if (f4 == 0.0) return false;
    double d0 = (double)xj - xi, d1 = (double)yj - yi, e2 = (double)zj - zi;
    const double a1 = dot3(ni0, ni1, ni2, d0, d1, e2) / f4, a2 = dot3(nj0, nj1, nj2, d0, d1, e2) / f4;
    const bool swap = fabs(a1) < fabs(a2);
    const double p0 = swap ? nj0 : ni0, p1 = swap ? nj1 : ni1, p2 = swap ? nj2 : ni2;       // n1
    const double q0 = swap ? ni0 : nj0, q1 = swap ? ni1 : nj1, q2 = swap ? ni2 : nj2;       // n2
    const double f3 = swap ? -a2 : a1;
    if (swap) { d0 = -d0; d1 = -d1; e2 = -e2; }
    double v0 = d1 * p2 - e2 * p1, v1 = e2 * p0 - d0 * p2, v2 = d0 * p1 - d1 * p0;         // d x n1
    const double vn = sqrt(dot3(v0, v1, v2, v0, v1, v2));
    if (!(vn > 0.0)) return false;
    v0 /= vn;
    v1 /= vn;
    v2 /= vn;
    const double w0 = p1 * v2 - p2 * v1, w1 = p2 * v0 - p0 * v2, w2 = p0 * v1 - p1 * v0;   // n1 x v
    const double f2 = dot3(v0, v1, v2, q0, q1, q2);
    const double y = dot3(w0, w1, w2, q0, q1, q2), x = dot3(p0, p1, p2, q0, q1, q2);
    out.h1 = sector11(x, y);
    out.h2 = bin11(f2);
    out.h3 = bin11(f3);
    return true;
}

// what a query takes off its count for itself
USIP_HD int own(double xi, double yi, double zi, double r2)
{
    return member(usip_prep::sqdist(xi, yi, zi, (float)xi, (float)yi, (float)zi), r2) ? 1 : 0;
}

// The first sorted position s in [0, n) with qx - xs(s) < r (n when there is none): every row before it has dx = fl(qx - x_s)
// >= r, hence d2 >= fl(dx dx) >= fl(r r) = r2 (float64 rounding is monotone): no member.
template <class Xs>
USIP_HD int first_within(int n, double qx, double r, const Xs& xs)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (qx - xs(mid) < r) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// whether cloud point j at squared distance d2 from a keypoint adds its SPFH row
USIP_HD bool gathers(double d2, double r2, int32_t members_j) { return members_j > 0 && d2 > 0.0 && member(d2, r2); }

// one row to a lane's 33 sums
USIP_HD void add_row(double acc[WIDTH], const int32_t* row, int32_t members_j, double d2)
{
    const double scale = 100.0 / (double)members_j, w = 1.0 / d2;
#pragma unroll
    for (int h = 0; h < WIDTH; h += BINS) {
#pragma unroll
        for (int b = h; b < h + BINS; ++b) acc[b] += ((double)row[b] * scale) * w;
        USIP_FPFH_FENCE();
    }
}

// block H of eleven to the sum 100, where it has one
template <int H>
USIP_HD void normalise(double acc[WIDTH])
{
    double sum = 0.0;
#pragma unroll
    for (int b = 0; b < BINS; ++b) sum += acc[H * BINS + b];
    const bool some = sum > 0.0;
    const double scale = 100.0 / sum;
#pragma unroll
    for (int b = 0; b < BINS; ++b) acc[H * BINS + b] = some ? acc[H * BINS + b] * scale : 0.0;
}

}  // namespace usip_fpfh
