// usip_amd/csrc/spin_math.h -- the arithmetic of the spin-image baseline descriptor, shared by the kernels of
// csrc/spin.hip and the host twin of csrc/spin_cpu.cpp: both sides run the same float64 operations on the float32 points of a
// frame and add INTEGERS, so their results are equal bit for bit.  It sits over shot_math.h (angle, clamp_one, dot3,
// first_within, the keypoint limit), harris_math.h (has_normal, finite), iss_math.h (member, the limits) and prepare_math.h
// (sqdist).  Only + - * / sqrt fabs floor and comparisons feed a result: no libm call but floor, which is exact.
//
// Reference semantics: the reference's indoor scoring scripts name spin images (eval_indoor/3dmatch/evaluate.m:
// descriptorName = 'my'; % 3dmatch, spin, fpfh) and the reference does not contain them.  What follows is this project's own
// definition of spin images (Johnson, Hebert 1999), written after PCL's SpinImageEstimation with the deviations of DESIGN 8q:
//   axis           a row v of axes f64 [B][M][3] IS AN AXIS iff its three numbers are finite and v . v is positive and finite;
//                  a = v / sqrt(v . v), component by component.  Without an axis the keypoint's row is zeros and it has no
//                  member.
//   members        live rows with d2 > 0 and d2 < r * r (strict; r * r once, in float64; d2 = usip_prep::sqdist(q, p_j)).
//                  d = p_j - q, beta = d . a.  With a support angle s = support_angle_cos > 0: a row without a normal is
//                  skipped, and so is one with fabs(n_j . a) < s (a counter-directed normal passes); normals are used as
//                  given.  With s == 0 no normal is read.  Every dot product is (a0 b0 + a1 b1) + a2 b2.
//   rectangular    W = 8, bin = (r * 0.70710678118654757) / W (the cylinder inscribed in the search sphere).  alpha =
//                  sqrt(max(0, d2 - beta * beta)), u = alpha / bin, v = beta / bin.  The row is a member iff u < W, v < W and
//                  v > -W.  ab = (int)floor(u), bb = (int)floor(v) + W; the offsets are u - floor(u) and v - floor(v).
//   radial         bin = r / W, u = sqrt(d2) / bin; c = beta / sqrt(d2) clamped to [-1, 1], theta = angle(c, sqrt((1 - c) * (1 +
//                  c))) in [-pi / 2, pi / 2] (shot_math.h's inverse tangent: the arc sine of c), v = theta / ((pi / 2) / W).
//                  Every row of the sphere is a member.  THE BORDER RULE: a u that reaches W after rounding goes to ab = W - 1,
//                  a v that reaches W to bb = 2 W - 1, with the largest offset below 1 (2^20 - 1 quanta).
//   weights        INTEGERS with the quantum 2^-20 per axis: qa = (int64)(offset_a * 1048576.0) capped at 2^20 - 1 (an offset
//                  that rounds to 1, as -1e-30 - floor(-1e-30) does, takes the cap), qb likewise.  The cells (ab, bb), (ab + 1,
//                  bb), (ab, bb + 1), (ab + 1, bb + 1) get (2^20 - qa)(2^20 - qb), qa (2^20 - qb), (2^20 - qa) qb, qa qb: 2^40
//                  per member in all (a weight of 0 adds nothing).  column = row * (2 W + 1) + col: hist i64 [153], 9 rows of
//                  alpha by 17 columns of beta.  N <= 2^20, so a row's total stays below 2^61.  Integer sums do not depend on
//                  the order of the walk.
//   descriptor     spin_b = (double)hist_b / ((double)kp_members * 2^40): one division per column, the denominator exact;
//                  zeros when kp_members == 0.
#pragma once
#include "shot_math.h"

namespace usip_spin {

using usip_fpfh::bad_keypoints;
using usip_fpfh::dot3;
using usip_fpfh::first_within;
using usip_fpfh::LANES;
using usip_harris::finite;
using usip_harris::has_normal;
using usip_iss::member;
using usip_prep::TILE;
using usip_shot::angle;
using usip_shot::clamp_one;
using usip_shot::HALF_PI;

constexpr int W = 8, ROWS = W + 1, COLS = 2 * W + 1, WIDTH = ROWS * COLS, ADDS = 4;
constexpr int PER_LANE = (WIDTH + LANES - 1) / LANES;                  // columns of a lane when the row is written
constexpr int RECTANGULAR = 0, RADIAL = 1;
constexpr double QUANTUM = 1048576.0, SQRT_HALF = 0.70710678118654757, TOTAL = 1099511627776.0;
constexpr long long ONE = 1LL << 20;
constexpr double THETA_BIN = HALF_PI / W;                              // (exact: a power of two under pi / 2)

USIP_HD bool bad_support(double s) { return !(s >= 0.0) || !(s <= 1.0); }
USIP_HD bool bad_structure(int structure) { return structure != RECTANGULAR && structure != RADIAL; }

// The unit axis of a keypoint, or none
struct Axis {
    double a0, a1, a2;
    bool ok;
    USIP_HD Axis(double v0, double v1, double v2)
    {
        const double vv = dot3(v0, v1, v2, v0, v1, v2);
        ok = finite(v0) && finite(v1) && finite(v2) && vv > 0.0 && finite(vv);
        const double len = sqrt(vv);
        a0 = ok ? v0 / len : 0.0;
        a1 = ok ? v1 / len : 0.0;
        a2 = ok ? v2 / len : 0.0;
    }
};

// whether the support angle s > 0 keeps the row with the normal n
USIP_HD bool supported(const Axis& A, double s, double n0, double n1, double n2)
{
    return has_normal(n0, n1, n2) && !(fabs(dot3(n0, n1, n2, A.a0, A.a1, A.a2)) < s);
}

USIP_HD long long quanta(double offset)
{
    const long long q = (long long)(offset * QUANTUM);
    return q > ONE - 1 ? ONE - 1 : q;
}

// What one member adds: its four cells (ab, bb), (ab + 1, bb), (ab, bb + 1), (ab + 1, bb + 1) as columns, and their weights
struct Adds {
    int ab, bb;
    int col[ADDS];
    long long q[ADDS];
};

// The cells of the row at d = p_j - q with 0 < d2 < r2; false: outside the structure (the rectangular one only)
template <int STRUCTURE>
USIP_HD bool member_adds(const Axis& A, double r, double d2, double d0, double d1, double e2, Adds& out)
{
    const double beta = dot3(d0, d1, e2, A.a0, A.a1, A.a2);
    double u, v;
    if (STRUCTURE == RADIAL) {
        const double dist = sqrt(d2), c = clamp_one(beta / dist);
        u = dist / (r / (double)W);
        v = angle(c, sqrt((1.0 - c) * (1.0 + c))) / THETA_BIN;
    } else {
        const double bin = (r * SQRT_HALF) / (double)W, a2 = d2 - beta * beta;
        u = sqrt(a2 > 0.0 ? a2 : 0.0) / bin;
        v = beta / bin;
        if (!(u < (double)W && v < (double)W && v > -(double)W)) return false;
    }
    const double fu = floor(u), fv = floor(v);
    int ab = (int)fu, bb = (int)fv + W;
    long long qa = quanta(u - fu), qb = quanta(v - fv);
    if (ab >= W) {                                                     // the border rule (never taken by the rectangular test)
        ab = W - 1;
        qa = ONE - 1;
    }
    if (bb >= 2 * W) {
        bb = 2 * W - 1;
        qb = ONE - 1;
    }
    if (bb < 0) {                                                      // (|theta| <= pi / 2 keeps v >= -W: never taken)
        bb = 0;
        qb = 0;
    }
    if (ab < 0) {                                                      // (u >= 0: never taken; no column leaves the image)
        ab = 0;
        qa = 0;
    }
    out.ab = ab;
    out.bb = bb;
    out.col[0] = ab * COLS + bb;
    out.col[1] = (ab + 1) * COLS + bb;
    out.col[2] = ab * COLS + bb + 1;
    out.col[3] = (ab + 1) * COLS + bb + 1;
    out.q[0] = (ONE - qa) * (ONE - qb);
    out.q[1] = qa * (ONE - qb);
    out.q[2] = (ONE - qa) * qb;
    out.q[3] = qa * qb;
    return true;
}

// a column of the descriptor from its integer sum
USIP_HD double column(long long h, int32_t members) { return members > 0 ? (double)h / ((double)members * TOTAL) : 0.0; }

}  // namespace usip_spin
