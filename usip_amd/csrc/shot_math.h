// usip_amd/csrc/shot_math.h -- the arithmetic of the SHOT baseline descriptor, shared by the kernels of
// csrc/shot.hip and the host twin of csrc/shot_cpu.cpp: both sides run the same float64 operations in the same order on the
// float32 points of a frame, so their results are equal bit for bit.  It sits over fpfh_math.h (dot3, first_within, the
// keypoint limit), harris_math.h (has_normal, finite), iss_math.h (member, the limits) and prepare_math.h (sqdist,
// jacobi_rotate3, JACOBI_SWEEPS).  Only + - * / sqrt fabs and comparisons feed a result: no libm call.
//
// Reference semantics: the reference's outdoor scoring script is set to a SHOT result (evaluation/matlab/eval_outdoor/kitti/
// evaluate_kitti.m: .../kitti/shot/iss_256, FEATURE_DIM = 352) that the reference does not contain.  What follows is this
// project's own definition of SHOT-352 (Tombari, Salti, Di Stefano 2010), written after PCL's SHOTEstimation and
// SHOTLocalReferenceFrameEstimation with the deviations of DESIGN 8p:
//   membership     usip_iss::member over usip_prep::sqdist(q, p_j): d2 < r * r (strict; r * r once, in float64)
//   frame          over ALL live rows within r (no normal needed; a row at d2 == 0 counts): d = p_j - q, w = r - sqrt(d2),
//                  seven sums: w and wd0 d0, wd0 d1, wd0 d2, wd1 d1, wd1 d2, wd2 d2 with wda = w * da.  THE ORDER: 64 partial
//                  sums, partial l over the sorted positions lo + l + 64 k ascending, lo = first_within(); folded by s[l] +=
//                  s[l ^ off], off = 32 .. 1.  C = sums / sum w; JACOBI_SWEEPS sweeps of jacobi_rotate3 <0,1> <0,2> <1,2>; x =
//                  the column of the largest diagonal entry, z = of the smallest (the first of equal ones, either way).  The
//                  sign of x: the members with d . x >= 0 against those with d . x < 0 (integer counts); x is negated iff the
//                  first count is the smaller (a tie keeps it); z likewise; y = z cross x.  Fewer than 5 members, sum w not
//                  positive or a component that is not finite: NO FRAME, nine zeros.
//   histogram      members: rows with a normal, d2 < r2, d2 > 0.  x' = d . x, y' = d . y, z' = d . z, dist = sqrt(d2), c =
//                  n_j . z clamped to [-1, 1]; every dot is (a0 b0 + a1 b1) + a2 b2.
//   hard bins      t = (1 + c) * 5, cb = (int)(t + 0.5) in 0 .. 10; sh = dist > r / 2; el = z' > 0; az = sector8(x', y'):
//                  the sector of width pi / 4, counted from -pi, by signs and |x'| against |y'| alone.  THE TIE RULE: a
//                  boundary direction belongs to the sector that begins there, and the direction pi (y' == 0 of either sign,
//                  x' < 0) to sector 7; (0, 0) is the direction 0: sector 4.  So with y' >= 0: x' > 0 gives 4 when |y'| < |x'|
//                  and 5 otherwise; x' <= 0 gives 6 when |y'| > |x'| and 7 otherwise.  With y' < 0: x' < 0 gives 0 when |y'| <
//                  |x'| and 1 otherwise; x' >= 0 gives 2 when |y'| > |x'| and 3 otherwise.
//                  column = ((az * 2 + el) * 2 + sh) * 11 + cb
//   interpolation  four offsets from the centre of the member's own bin, each clamped to [-1/2, 1/2]:
//                  cosine     t - cb; neighbour cb + 1 (offset > 0) or cb - 1 (offset < 0) where that is in 0 .. 10
//                  radial     inner shell dist / (r / 2) - 1/2, neighbour the outer shell for an offset > 0; outer shell
//                             (dist - r / 2) / (r / 2) - 1/2, neighbour the inner shell for an offset < 0; none otherwise
//                  elevation  u = z' / dist clamped to [-1, 1], theta = angle(sqrt((1 - u) * (1 + u)), u) in [0, pi]; offset =
//                             (theta - centre) / (pi / 2), centre pi / 4 (el = 1) or 3 pi / 4 (el = 0); the neighbour is the
//                             other half for el = 1 and an offset > 0, for el = 0 and an offset < 0; none otherwise
//                  azimuth    phi = angle(y', x'); offset = (phi - (az - 3.5) * (pi / 4)) / (pi / 4); neighbour az + 1 (offset
//                             > 0) or az - 1 (offset < 0), modulo 8
//   weights        INTEGERS with the quantum 2^-32: q_k = (int64)(|offset_k| * 4294967296.0); the member's own column gets the
//                  sum over the four k of 2^32 - q_k, an existing neighbour column its q_k (a q_k of 0 adds nothing), a q_k
//                  towards a missing neighbour is dropped.  Integer sums do not depend on the order of the walk.
//   descriptor     h_b = (double)hist_b; s = sum h_b * h_b: 64 partial sums, partial l over the columns l + 64 k ascending,
//                  folded as above; shot_b = h_b / sqrt(s), zeros when s == 0.
//
// angle(y, x) is this project's own inverse tangent of two arguments, in (-pi, pi]: m = min(|x|, |y|), M = max(|x|, |y|); (0, 0)
// gives 0; t = m / M where m <= M * 0.41421356237309503, else t = (m - M) / (m + M) and pi / 4 is added (ONE division either
// way, |t| <= tan(pi / 8)); atan t = t * P(t * t), P the Taylor polynomial 1 - z / 3 + z^2 / 5 - ... + z^20 / 41 in Horner's
// order (the first dropped term is below 1e-18); then pi / 2 - a when |y| > |x|, pi - a when x < 0, -a when y < 0.  A zero of
// either sign is +0: angle(-0.0, x < 0) = +pi, where libm's atan2 gives -pi.  Finite arguments only.  Measured against
// np.arctan2 on 2 000 001 directions at random lengths plus the axes, the diagonals and signed zeros (tests/test_shot_cpu.py):
// the largest absolute difference is EPS_A = 4.4408920985006262e-16 (one unit in the last place of pi).
#pragma once
#include "fpfh_math.h"

namespace usip_shot {

using usip_fpfh::bad_keypoints;
using usip_fpfh::dot3;
using usip_fpfh::first_within;
using usip_fpfh::LANES;
using usip_harris::finite;
using usip_harris::has_normal;
using usip_iss::member;
using usip_prep::JACOBI_SWEEPS;
using usip_prep::TILE;

constexpr int WIDTH = 352, COSINES = 11, MIN_MEMBERS = 5, ADDS = 5;
constexpr int PER_LANE = (WIDTH + LANES - 1) / LANES;                  // columns of a lane in the descriptor's sum
constexpr double QUANTUM = 4294967296.0;
constexpr long long ONE = 1LL << 32;
constexpr double PI = 3.141592653589793, HALF_PI = 1.5707963267948966, QUARTER_PI = 0.7853981633974483;
constexpr double THREE_QUARTER_PI = 2.356194490192345, TAN_PI_8 = 0.41421356237309503;

// atan t for |t| <= tan(pi / 8): t * (1 - z / 3 + z^2 / 5 - ... + z^20 / 41), z = t * t
USIP_HD double atan_small(double t)
{
    const double z = t * t;
    double p = 1.0 / 41.0;
    p = p * z - 1.0 / 39.0;
    p = p * z + 1.0 / 37.0;
    p = p * z - 1.0 / 35.0;
    p = p * z + 1.0 / 33.0;
    p = p * z - 1.0 / 31.0;
    p = p * z + 1.0 / 29.0;
    p = p * z - 1.0 / 27.0;
    p = p * z + 1.0 / 25.0;
    p = p * z - 1.0 / 23.0;
    p = p * z + 1.0 / 21.0;
    p = p * z - 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z - 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z - 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z - 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z - 1.0 / 3.0;
    p = p * z + 1.0;
    return t * p;
}

USIP_HD double angle(double y, double x)
{
    const double ax = fabs(x), ay = fabs(y);
    const bool swap = ay > ax;
    const double hi = swap ? ay : ax, lo = swap ? ax : ay;
    double a = 0.0;
    if (hi > 0.0) {
        const bool upper = lo > hi * TAN_PI_8;
        const double num = upper ? lo - hi : lo, den = upper ? lo + hi : hi;
        a = atan_small(num / den);
        a = upper ? QUARTER_PI + a : a;
    }
    a = swap ? HALF_PI - a : a;
    a = x < 0.0 ? PI - a : a;
    return y < 0.0 ? -a : a;
}

USIP_HD int sector8(double x, double y)
{
    if (x == 0.0 && y == 0.0) return 4;
    const double ax = fabs(x), ay = fabs(y);
    if (y >= 0.0) return x > 0.0 ? (ay < ax ? 4 : 5) : (ay > ax ? 6 : 7);
    return x < 0.0 ? (ay < ax ? 0 : 1) : (ay > ax ? 2 : 3);
}

USIP_HD int column(int az, int el, int sh, int cb) { return ((az * 2 + el) * 2 + sh) * COSINES + cb; }

// The seven sums of one partial (named fields: no array, no index)
struct Sums {
    double w = 0.0, s00 = 0.0, s01 = 0.0, s02 = 0.0, s11 = 0.0, s12 = 0.0, s22 = 0.0;
    USIP_HD void add(double r, double d2, double d0, double d1, double e2)
    {
        const double wt = r - sqrt(d2), w0 = wt * d0, w1 = wt * d1, w2 = wt * e2;
        w += wt;
        s00 += w0 * d0;
        s01 += w0 * d1;
        s02 += w0 * e2;
        s11 += w1 * d1;
        s12 += w1 * e2;
        s22 += w2 * e2;
    }
    USIP_HD void fold(const Sums& o)
    {
        w += o.w;
        s00 += o.s00;
        s01 += o.s01;
        s02 += o.s02;
        s11 += o.s11;
        s12 += o.s12;
        s22 += o.s22;
    }
};

// The x and z axes before their signs are decided; ok: the keypoint can have a frame
struct Axes {
    double x0, x1, x2, z0, z1, z2;
    bool ok;
};

USIP_HD Axes axes_from(const Sums& S, int members)
{
    Axes A{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, members >= MIN_MEMBERS && S.w > 0.0};
    if (!A.ok) return A;
    const double c00 = S.s00 / S.w, c01 = S.s01 / S.w, c02 = S.s02 / S.w, c11 = S.s11 / S.w, c12 = S.s12 / S.w,
                 c22 = S.s22 / S.w;
    double a[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}};
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll 1
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        usip_prep::jacobi_rotate3<0, 1>(a, v);
        usip_prep::jacobi_rotate3<0, 2>(a, v);
        usip_prep::jacobi_rotate3<1, 2>(a, v);
    }
    const bool l1 = a[1][1] > a[0][0];                                 // the largest: the first of equal ones
    double e = l1 ? a[1][1] : a[0][0];
    A.x0 = l1 ? v[0][1] : v[0][0];
    A.x1 = l1 ? v[1][1] : v[1][0];
    A.x2 = l1 ? v[2][1] : v[2][0];
    const bool l2 = a[2][2] > e;
    A.x0 = l2 ? v[0][2] : A.x0;
    A.x1 = l2 ? v[1][2] : A.x1;
    A.x2 = l2 ? v[2][2] : A.x2;
    const bool s1 = a[1][1] < a[0][0];                                 // the smallest: the first of equal ones
    e = s1 ? a[1][1] : a[0][0];
    A.z0 = s1 ? v[0][1] : v[0][0];
    A.z1 = s1 ? v[1][1] : v[1][0];
    A.z2 = s1 ? v[2][1] : v[2][0];
    const bool s2 = a[2][2] < e;
    A.z0 = s2 ? v[0][2] : A.z0;
    A.z1 = s2 ? v[1][2] : A.z1;
    A.z2 = s2 ? v[2][2] : A.z2;
    return A;
}

// The votes of one member on the two signs
struct Votes {
    int32_t xp = 0, xn = 0, zp = 0, zn = 0;
    USIP_HD void add(const Axes& A, double d0, double d1, double e2)
    {
        const bool x = dot3(d0, d1, e2, A.x0, A.x1, A.x2) >= 0.0, z = dot3(d0, d1, e2, A.z0, A.z1, A.z2) >= 0.0;
        xp += x ? 1 : 0;
        xn += x ? 0 : 1;
        zp += z ? 1 : 0;
        zn += z ? 0 : 1;
    }
};

// out[9] = the rows x, y, z of the frame, or zeros
USIP_HD void frame_from(const Axes& A, const Votes& V, double out[9])
{
    const bool fx = V.xp < V.xn, fz = V.zp < V.zn;
    const double x0 = fx ? -A.x0 : A.x0, x1 = fx ? -A.x1 : A.x1, x2 = fx ? -A.x2 : A.x2;
    const double z0 = fz ? -A.z0 : A.z0, z1 = fz ? -A.z1 : A.z1, z2 = fz ? -A.z2 : A.z2;
    const double y0 = z1 * x2 - z2 * x1, y1 = z2 * x0 - z0 * x2, y2 = z0 * x1 - z1 * x0;
    const bool ok = A.ok && finite(x0) && finite(x1) && finite(x2) && finite(y0) && finite(y1) && finite(y2) && finite(z0) &&
                    finite(z1) && finite(z2);
    out[0] = ok ? x0 : 0.0;
    out[1] = ok ? x1 : 0.0;
    out[2] = ok ? x2 : 0.0;
    out[3] = ok ? y0 : 0.0;
    out[4] = ok ? y1 : 0.0;
    out[5] = ok ? y2 : 0.0;
    out[6] = ok ? z0 : 0.0;
    out[7] = ok ? z1 : 0.0;
    out[8] = ok ? z2 : 0.0;
}

// A frame as the histogram pass reads it: nine finite numbers whose x row is not all zero; anything else is NO FRAME
struct Lrf {
    double x0, x1, x2, y0, y1, y2, z0, z1, z2;
    USIP_HD bool exists() const
    {
        return has_normal(x0, x1, x2) && finite(y0) && finite(y1) && finite(y2) && finite(z0) && finite(z1) && finite(z2);
    }
};

USIP_HD bool describes(double d2, double r2, double n0, double n1, double n2)
{
    return d2 > 0.0 && member(d2, r2) && has_normal(n0, n1, n2);
}

USIP_HD double clamp_half(double d) { return d < -0.5 ? -0.5 : (d > 0.5 ? 0.5 : d); }
USIP_HD double clamp_one(double c) { return c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c); }
USIP_HD long long quanta(double d) { return (long long)(fabs(d) * QUANTUM); }

// What one member adds: col[0] its own column, col[1 .. 4] the cosine, radial, elevation and azimuth neighbours (-1: none)
struct Adds {
    int col[ADDS];
    long long q[ADDS];
};

USIP_HD void member_adds(const Lrf& L, double r, double d2, double d0, double d1, double e2, double n0, double n1, double n2,
                         Adds& out)
{
    const double dist = sqrt(d2), half = r / 2.0;
    const double xp = dot3(d0, d1, e2, L.x0, L.x1, L.x2), yp = dot3(d0, d1, e2, L.y0, L.y1, L.y2),
                 zp = dot3(d0, d1, e2, L.z0, L.z1, L.z2);
    const double c = clamp_one(dot3(n0, n1, n2, L.z0, L.z1, L.z2));
    const double t = (1.0 + c) * 5.0;
    const int cb = (int)(t + 0.5), sh = dist > half ? 1 : 0, el = zp > 0.0 ? 1 : 0, az = sector8(xp, yp);
    const double dcos = clamp_half(t - (double)cb);
    const double drad = clamp_half(sh ? (dist - half) / half - 0.5 : dist / half - 0.5);
    const double u = clamp_one(zp / dist);
    const double theta = angle(sqrt((1.0 - u) * (1.0 + u)), u);
    const double dele = clamp_half((theta - (el ? QUARTER_PI : THREE_QUARTER_PI)) / HALF_PI);
    const double dazi = clamp_half((angle(yp, xp) - ((double)az - 3.5) * QUARTER_PI) / QUARTER_PI);
    const long long qc = quanta(dcos), qr = quanta(drad), qe = quanta(dele), qa = quanta(dazi);
    const int nc = dcos > 0.0 ? cb + 1 : cb - 1;
    out.col[0] = column(az, el, sh, cb);
    out.q[0] = (((ONE - qc) + (ONE - qr)) + (ONE - qe)) + (ONE - qa);
    out.col[1] = qc > 0 && nc >= 0 && nc < COSINES ? column(az, el, sh, nc) : -1;
    out.q[1] = qc;
    out.col[2] = qr > 0 && (sh ? drad < 0.0 : drad > 0.0) ? column(az, el, 1 - sh, cb) : -1;
    out.q[2] = qr;
    out.col[3] = qe > 0 && (el ? dele > 0.0 : dele < 0.0) ? column(az, 1 - el, sh, cb) : -1;
    out.q[3] = qe;
    out.col[4] = qa > 0 ? column((az + (dazi > 0.0 ? 1 : 7)) & 7, el, sh, cb) : -1;
    out.q[4] = qa;
}

}  // namespace usip_shot
