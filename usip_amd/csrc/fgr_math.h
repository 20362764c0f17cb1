// usip_amd/csrc/fgr_math.h -- the arithmetic of Fast Global Registration (Zhou, Park, Koltun, ECCV 2016),
// shared by the kernels of csrc/fgr.hip and the host twin of csrc/fgr_cpu.cpp: both sides run the same float64 operations
// in the same order on float32 inputs, so they agree bit for bit.  include/usip_hip.h (f-12) is the contract; the
// reference's eval_indoor/fgr/fast_global_registration.cpp wraps an app.h it does not ship, so the definition is this
// project's own, written from the paper and its published constants.
//
//   mutual rows    (i, nn12[i]) for ascending i with nn21[nn12[i]] == i
//   normalisation  u = (x - mean) / scale, mean over ALL keypoints of a fragment, scale the largest centred norm of both
//   tuple test     trial t: three rows perm(0..2) of a PairsPerm bijection on [0, nc) keyed from the Philox4x64-10 block with
//                  key (seed, 0) and counter (t, TAG_FGR << 8, g, 0); accepted iff every edge keeps its length within 0.95
//   optimisation   64 Gauss-Newton steps under graduated non-convexity, 19 distinct sums per step (sums_of_row), a 6 x 6
//                  Cholesky in a fixed order, Rz Ry Rx from fgr_sincos
#pragma once
#include <math.h>
#include "pairs_rng.h"
#include "registration_math.h"

namespace usip_fgr {

constexpr uint32_t TAG_FGR = 10;        // continues the stream tags of csrc/pairs_rng.h (1-8) and csrc/registration_math.h (9)
constexpr int MMAX = 1024;              // keypoints per fragment, hence mutual rows per pair
constexpr int TRIALS_PER_ROW = 100;     // T = 100 nc
constexpr int TUPLE_CAP = 1000;         // accepted trials kept
constexpr int ROWS_MAX = 3 * TUPLE_CAP;
constexpr int MIN_ROWS = 10;            // fewer rows: the pair is invalid
constexpr double TUPLE_SCALE = 0.95;
constexpr int ITERATIONS = 64;
constexpr double DIV_FACTOR = 1.4, MAX_CORR_DIST = 0.025;
constexpr int LANES = 256;              // lane l sums its rows l, l + 256, ... in ascending order, then the binary tree
constexpr int NSUM = 19;                // the distinct ones of the 27 sums (see sums_of_row)
constexpr double PI = 3.141592653589793;

using usip_reg::clamp_count;

// The larger of two, NaN if either is one: the order of a reduction does not matter.
USIP_HD double max_nan(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }

USIP_HD bool finite(double v) { return v - v == 0.0; }

// sqrt((x x + y y) + z z) of a centred point
USIP_HD double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

// The binary tree over 256 partial sums, part[l] += part[l + s] for s = 128 .. 1 (usip_reg::tree_sum's pairing), on the
// host.  The device takes the strides 128 and 64 as (p[l] + p[l + 128]) + (p[l + 64] + p[l + 192]) in lane l of a wave and
// the strides 32 .. 1 by lane shuffles: the same additions of the same pairs.
inline double tree256(double* part)
{
    for (int s = LANES / 2; s > 0; s >>= 1)
        for (int l = 0; l < s; ++l) part[l] += part[l + s];
    return part[0];
}

// One edge of the tuple test: li, lj its lengths in normalised fragment 1 and 2.
USIP_HD bool edge_ok(const double* a1, const double* b1, const double* a2, const double* b2)
{
    const double li = norm3(a1[0] - b1[0], a1[1] - b1[1], a1[2] - b1[2]);
    const double lj = norm3(a2[0] - b2[0], a2[1] - b2[1], a2[2] - b2[2]);
    return li * TUPLE_SCALE < lj && lj < li / TUPLE_SCALE;
}
// u[k]: the normalised row k of the trial, fragment 1 in [0..3), fragment 2 in [3..6)
USIP_HD bool tuple_ok(const double* u0, const double* u1, const double* u2)
{
    return edge_ok(u0, u1, u0 + 3, u1 + 3) && edge_ok(u0, u2, u0 + 3, u2 + 3) && edge_ok(u1, u2, u1 + 3, u2 + 3);
}

// sin and cos for |x| <= pi, the same bits on host and device: n = rint(x 2/pi), r = (x - n pio2_hi) - n pio2_lo (exact
// products: n is at most 2 and pio2_hi has 33 significant bits), then the fdlibm kernel polynomials on |r| <= pi/4 in
// Horner form -- additions and multiplications only, never contracted.  Against numpy.sin / numpy.cos on 2 000 001 evenly
// spaced points of [-pi, pi] the largest absolute difference is 2.22e-16 for the sine and 1.11e-16 for the cosine (two
// and one units in the last place of a value below 1); tests/test_fgr_cpu.py holds both below 2.3e-16.
USIP_HD void fgr_sincos(double x, double* s, double* c)
{
    const double n = rint(x * 0.6366197723675814);
    const double r = (x - n * 1.57079632673412561417e+00) - n * 6.07710050650619224932e-11;
    const double z = r * r;
    const double ps = -1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 +
                      z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))));
    const double pc = 4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                      z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))));
    const double sr = r + (r * z) * ps;
    const double cr = (1.0 - 0.5 * z) + (z * z) * pc;
    const int q = (int)n & 3;
    *s = q == 0 ? sr : (q == 1 ? cr : (q == 2 ? -sr : -cr));
    *c = q == 0 ? cr : (q == 1 ? -sr : (q == 2 ? -cr : sr));
}

// The state of the optimisation: x1 = R x2 + t on normalised coordinates, row-major R.
struct Pose {
    double R[9], t[3];
};
USIP_HD void pose_identity(Pose& p)
{
    p.R[0] = 1; p.R[1] = 0; p.R[2] = 0; p.R[3] = 0; p.R[4] = 1; p.R[5] = 0; p.R[6] = 0; p.R[7] = 0; p.R[8] = 1;
    p.t[0] = 0; p.t[1] = 0; p.t[2] = 0;
}

USIP_HD double next_par(double par, int k) { return (k % 4 == 0 && par > MAX_CORR_DIST) ? par / DIV_FACTOR : par; }

// One row's terms added to the sums.  With q = R u2 + t, r = u1 - q, e = (r0 r0 + r1 r1) + r2 r2, w = par / (e + par),
// s = w w and the Jacobian rows J0 = [0, -q2, q1, -1, 0, 0], J1 = [q2, 0, -q0, 0, -1, 0], J2 = [-q1, q0, 0, 0, 0, -1], the 21
// upper entries of sum s J'J and the 6 of sum s J'r are 27 sums; six are sums of exact zeros (A03 A14 A25 A34 A35 A45) and
// A44, A55 repeat A33, so 19 are carried:
//    0 A00 = s (q1 q1 + q2 q2)    1 A01 = -s q0 q1    2 A02 = -s q0 q2    3 A04 = -s q2    4 A05 = s q1
//    5 A11 = s (q0 q0 + q2 q2)    6 A12 = -s q1 q2    7 A13 = s q2        8 A15 = -s q0
//    9 A22 = s (q0 q0 + q1 q1)   10 A23 = -s q1      11 A24 = s q0       12 A33 = s
//   13 b0 = s (q2 r1 - q1 r2)    14 b1 = s (q0 r2 - q2 r0)    15 b2 = s (q1 r0 - q0 r1)    16 17 18 b3..5 = -s r0..2
USIP_HD void sums_of_row(double S[NSUM], const Pose& p, const double* u, double par)
{
    const double q0 = ((p.R[0] * u[3] + p.R[1] * u[4]) + p.R[2] * u[5]) + p.t[0];
    const double q1 = ((p.R[3] * u[3] + p.R[4] * u[4]) + p.R[5] * u[5]) + p.t[1];
    const double q2 = ((p.R[6] * u[3] + p.R[7] * u[4]) + p.R[8] * u[5]) + p.t[2];
    const double r0 = u[0] - q0, r1 = u[1] - q1, r2 = u[2] - q2;
    const double e = (r0 * r0 + r1 * r1) + r2 * r2;
    const double w = par / (e + par);
    const double s = w * w;
    const double s0 = s * q0, s1 = s * q1, s2 = s * q2;
    S[0] += s1 * q1 + s2 * q2;
    S[1] += -(s0 * q1);
    S[2] += -(s0 * q2);
    S[3] += -s2;
    S[4] += s1;
    S[5] += s0 * q0 + s2 * q2;
    S[6] += -(s1 * q2);
    S[7] += s2;
    S[8] += -s0;
    S[9] += s0 * q0 + s1 * q1;
    S[10] += -s1;
    S[11] += s0;
    S[12] += s;
    S[13] += s2 * r1 - s1 * r2;
    S[14] += s0 * r2 - s2 * r0;
    S[15] += s1 * r0 - s0 * r1;
    S[16] += -(s * r0);
    S[17] += -(s * r1);
    S[18] += -(s * r2);
}

// x = -A^-1 b from the 19 sums: the Cholesky factor column by column, every inner sum subtracted in ascending k, then the
// forward and the backward substitution.  false: a pivot that is not finite and positive, a component of x that is not
// finite, or |x0..2| > pi.
USIP_HD bool solve6(const double S[NSUM], double x[6])
{
    double L[6][6] = {{S[0], 0, 0, 0, 0, 0},       {S[1], S[5], 0, 0, 0, 0},  {S[2], S[6], S[9], 0, 0, 0},
                      {0.0, S[7], S[10], S[12], 0, 0}, {S[3], 0.0, S[11], 0.0, S[12], 0}, {S[4], S[8], 0.0, 0.0, 0.0, S[12]}};
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        ok = ok && finite(d) && d > 0.0;
        const double piv = sqrt(d);
        L[j][j] = piv;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = L[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / piv;
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = S[13 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = 5; k > i; --k) v -= L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        x[i] = -x[i];
        ok = ok && finite(x[i]);
    }
    return ok && fabs(x[0]) <= PI && fabs(x[1]) <= PI && fabs(x[2]) <= PI;
}

// D = Rz(x2) Ry(x1) Rx(x0), row-major, |x| <= pi (csrc/posegraph_math.h takes its step's rotation from here too)
USIP_HD void rotation_zyx(const double x[3], double D[9])
{
    double sa, ca, sb, cb, sg, cg;
    fgr_sincos(x[0], &sa, &ca);
    fgr_sincos(x[1], &sb, &cb);
    fgr_sincos(x[2], &sg, &cg);
    D[0] = cg * cb; D[1] = (cg * sb) * sa - sg * ca; D[2] = (cg * sb) * ca + sg * sa;
    D[3] = sg * cb; D[4] = (sg * sb) * sa + cg * ca; D[5] = (sg * sb) * ca - cg * sa;
    D[6] = -sb;     D[7] = cb * sa;                  D[8] = cb * ca;
}

// Rd = Rz(x2) Ry(x1) Rx(x0); R <- Rd R, t <- Rd t + x3..5
USIP_HD void apply_step(Pose& p, const double x[6])
{
    double D[9];
    rotation_zyx(x, D);
    Pose n;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) n.R[3 * i + j] = (D[3 * i] * p.R[j] + D[3 * i + 1] * p.R[3 + j]) + D[3 * i + 2] * p.R[6 + j];
        n.t[i] = ((D[3 * i] * p.t[0] + D[3 * i + 1] * p.t[1]) + D[3 * i + 2] * p.t[2]) + x[3 + i];
    }
    p = n;
}

// Back to the fragments' own coordinates: t_out = -R mean2 + t scale + mean1.  norm: mean1[3], mean2[3], scale, 0.
USIP_HD void denormalise(const Pose& p, const double* norm, double Rt[12])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        Rt[4 * i] = p.R[3 * i];
        Rt[4 * i + 1] = p.R[3 * i + 1];
        Rt[4 * i + 2] = p.R[3 * i + 2];
        const double rm = (p.R[3 * i] * norm[3] + p.R[3 * i + 1] * norm[4]) + p.R[3 * i + 2] * norm[5];
        Rt[4 * i + 3] = (p.t[i] * norm[6] - rm) + norm[i];
    }
}
USIP_HD void identity_Rt(double Rt[12])
{
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = (k == 0 || k == 5 || k == 10) ? 1.0 : 0.0;
}

USIP_HD bool scale_ok(double scale) { return finite(scale) && scale > 0.0; }

// The three rows of one trial, from either source of draws; inside [0, nc), nc >= 1.  With nc < 3 rows repeat, and an edge
// between a row and itself has li = lj = 0, which the test refuses.
struct PhiloxTriples {
    uint64_t seed;
    const int64_t* ids;          // global pair ids (NULL: g = p)
    USIP_HD void get(int p, int t, int nc, int idx[3]) const
    {
        uint64_t b[4];
        usip_pairs::pairs_block(seed, 0, ids ? (uint64_t)ids[p] : (uint64_t)p, TAG_FGR, 0, (uint64_t)t, b);
        usip_pairs::PairsPerm perm;
        perm.init(b, (uint64_t)nc);
#pragma unroll
        for (int k = 0; k < 3; ++k) idx[k] = (int)perm((uint64_t)(k < nc ? k : nc - 1));
    }
    USIP_HD int trials(int nc) const { return TRIALS_PER_ROW * nc; }
};
struct ExplicitTriples {
    const int32_t* triples;      // i32 [P][T][3]
    int T;
    USIP_HD void get(int p, int t, int nc, int idx[3]) const
    {
        const int32_t* s = triples + ((long long)p * T + t) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) idx[k] = usip_reg::clamp_index(s[k], nc);
    }
    USIP_HD int trials(int nc) const { return TRIALS_PER_ROW * nc < T ? TRIALS_PER_ROW * nc : T; }
};

}  // namespace usip_fgr
