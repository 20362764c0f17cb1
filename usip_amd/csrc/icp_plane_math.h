// usip_amd/csrc/icp_plane_math.h -- the arithmetic of the point-to-plane fit of trimmed ICP, shared by
// icp_fit_plane_kernel of csrc/icp_plane.hip and the host twin of csrc/icp_cpu.cpp.  include/usip_hip.h (f-28) is the contract;
// the conventions are f-13's (csrc/icp_math.h): float32 inputs, float64 arithmetic, never contracted, sums in a fixed order.
// The loop around the fit -- the nearest pass, the trim, the stopping rule, the final pass -- is f-13's own and is not
// restated here.  The sine and cosine, the step's rotation (rotation_zyx) and its application (apply_step) are
// csrc/fgr_math.h's, so a step of this fit and a step of Fast Global Registration turn a pose by the same bits.
//
//   plane_terms   one kept row's 27 terms: with q the moved row of B, (a, n) the position and unit normal of its nearest
//                 row of A, J = (q x n, n) and r = (q - a) . n, the 21 upper entries of J'J row-major, then the six of J r
//   plane_solve   x = -H^-1 g by a Cholesky factorisation written as fgr_math.h's solve6 is, for a full upper triangle
//   plane_step    (R, t) <- (D R, D t + x3..5), D = rotation_zyx(x0..2), on the row-major [3][4] pose of f-13
#pragma once
#include "fgr_math.h"
#include "icp_math.h"

namespace usip_icp {

// entry (j, k), j <= k, of the upper triangle stored row by row in the first 21 of the PLANE_SUMS (csrc/icp_math.h) sums
USIP_HD constexpr int plane_at(int j, int k) { return j * 6 - (j * (j - 1)) / 2 + (k - j); }

// S += the terms of one row.  q: the moved row of B (f-9's xform, the bits the search used); a: the row of A the search
// named, x y z then its unit normal.  Negating n negates J and r together, so no term changes a bit.
USIP_HD void plane_terms(double S[PLANE_SUMS], double q0, double q1, double q2, const float* a)
{
    const double a0 = (double)a[0], a1 = (double)a[1], a2 = (double)a[2];
    const double n0 = (double)a[3], n1 = (double)a[4], n2 = (double)a[5];
    const double J[6] = {q1 * n2 - q2 * n1, q2 * n0 - q0 * n2, q0 * n1 - q1 * n0, n0, n1, n2};
    const double r = ((q0 - a0) * n0 + (q1 - a1) * n1) + (q2 - a2) * n2;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
#pragma unroll
        for (int k = j; k < 6; ++k) S[plane_at(j, k)] += J[j] * J[k];
        S[21 + j] += J[j] * r;
    }
}

// x = -H^-1 g from the 27 sums: the Cholesky factor column by column, every inner sum subtracted in ascending k, then the
// forward and the backward substitution.  false: a pivot that is not finite and positive, a component of x that is not
// finite, or |x0..2| > pi.
USIP_HD bool plane_solve(const double S[PLANE_SUMS], double x[6])
{
    double L[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) L[i][j] = j <= i ? S[plane_at(j, i)] : 0.0;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        ok = ok && usip_fgr::finite(d) && d > 0.0;
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
        double v = S[21 + i];
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
        ok = ok && usip_fgr::finite(x[i]);
    }
    return ok && fabs(x[0]) <= usip_fgr::PI && fabs(x[1]) <= usip_fgr::PI && fabs(x[2]) <= usip_fgr::PI;
}

// Rn = the pose Rt advanced by the step x, through usip_fgr::apply_step
USIP_HD void plane_step(const double* Rt, const double x[6], double Rn[12])
{
    usip_fgr::Pose p;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) p.R[3 * i + j] = Rt[4 * i + j];
        p.t[i] = Rt[4 * i + 3];
    }
    usip_fgr::apply_step(p, x);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Rn[4 * i + j] = p.R[3 * i + j];
        Rn[4 * i + 3] = p.t[i];
    }
}

}  // namespace usip_icp
