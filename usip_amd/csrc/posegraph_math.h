// usip_amd/csrc/posegraph_math.h -- the arithmetic of the dense information matrix over aligned points and of the robust
// pose-graph optimisation that prunes loop closures, shared by the kernels of csrc/posegraph.hip and the host
// twin of csrc/posegraph_cpu.cpp: both sides run the same float64 operations in the same order, so they agree bit for bit.
// include/usip_hip.h (f-14) is the contract.  The per-point terms of A'A are csrc/fragments_math.h's (info_terms, info_fill),
// the radius test is f-9's within, the bank's ranges are csrc/icp_math.h's, the step's rotation and max_nan csrc/fgr_math.h's.
//
// Reference semantics (evaluation/matlab/eval_indoor/split_txt_compute_G.m, computeInformation 'point'): A'A over every
// fragment-1 point a moved fragment-2 point reaches within 0.05 m, one term per reaching point.  The optimiser the reference
// feeds those matrices to (Choi, Zhou, Koltun, CVPR 2015) is not part of it: the definition here is this project's own,
// written from the paper -- switchable loop closures whose line process has the closed form l = (mu / (mu + f))^2.
#pragma once
#include "fgr_math.h"
#include "icp_math.h"

namespace usip_pg {

constexpr int LANES = 256;
constexpr int NMAX = 128;                       // fragments per scene
constexpr int MMAX = 6 * (NMAX - 1);            // unknowns per scene: fragment 0 is fixed
constexpr int CHUNKS = (MMAX + LANES - 1) / LANES;     // rows of the system a lane owns: l, l + 256, l + 512
constexpr int MSLOTS = CHUNKS * LANES;
constexpr int MAX_ITERATIONS = 256;
constexpr int SMAX = 65535;
// what the edge pass leaves per edge (i, j) for the assembly: the blocks (i, i), (j, j), (j, i) of l J'LJ and the two
// six-vectors of l J'Le
constexpr int B_II = 0, B_JJ = 36, B_JI = 72, G_I = 108, G_J = 114, EDGE_W = 120;
constexpr int ST_OK = 0, ST_PIVOT = 1, ST_NOT_FINITE = 2, ST_ANGLE = 3, ST_BAD_GRAPH = 4;

using usip_fgr::finite;
using usip_fgr::max_nan;
using usip_fgr::PI;
using usip_reg::clamp_index;

USIP_HD long long emax_of(int nmax) { return (long long)nmax * (nmax - 1) / 2; }

// [R | t] row-major 3 x 4.  The inverse R', -(R' t); the product A B.  Every sum from the left.
USIP_HD void rigid_inverse(const double* A, double* out)
{
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[4 * r + c] = A[4 * c + r];
        out[4 * r + 3] = -((A[r] * A[3] + A[4 + r] * A[7]) + A[8 + r] * A[11]);
    }
}
USIP_HD void rigid_compose(const double* A, const double* B, double* out)
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double v = (A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c];
            out[4 * r + c] = c == 3 ? v + A[4 * r + 3] : v;
        }
}

// The vector part of the quaternion of D's rotation, w >= 0.  Shepperd: the branch is the largest of (trace, R00, R11, R22),
// the lowest index on ties, so the square root's argument is at least 1 for a rotation and a half turn is finite.
USIP_HD void quat_vector(const double* D, double q[3])
{
    const double r00 = D[0], r11 = D[5], r22 = D[10], tr = (r00 + r11) + r22;
    int b = 0;
    double best = tr;
    if (r00 > best) { best = r00; b = 1; }
    if (r11 > best) { best = r11; b = 2; }
    if (r22 > best) { best = r22; b = 3; }
    double w, x, y, z;
    if (b == 0) {
        const double s = sqrt(1.0 + tr), f = 0.5 / s;
        w = 0.5 * s; x = (D[9] - D[6]) * f; y = (D[2] - D[8]) * f; z = (D[4] - D[1]) * f;
    } else if (b == 1) {
        const double s = sqrt(((1.0 + r00) - r11) - r22), f = 0.5 / s;
        x = 0.5 * s; w = (D[9] - D[6]) * f; y = (D[1] + D[4]) * f; z = (D[2] + D[8]) * f;
    } else if (b == 2) {
        const double s = sqrt(((1.0 + r11) - r00) - r22), f = 0.5 / s;
        y = 0.5 * s; w = (D[2] - D[8]) * f; x = (D[1] + D[4]) * f; z = (D[6] + D[9]) * f;
    } else {
        const double s = sqrt(((1.0 + r22) - r00) - r11), f = 0.5 / s;
        z = 0.5 * s; w = (D[4] - D[1]) * f; x = (D[2] + D[8]) * f; y = (D[6] + D[9]) * f;
    }
    const bool flip = w < 0.0;
    q[0] = flip ? -x : x;
    q[1] = flip ? -y : y;
    q[2] = flip ? -z : z;
}

// E = Ti^-1 Tj, D = E X^-1, e = [t(D); qv(D)]
USIP_HD void residual(const double* Ti, const double* Tj, const double* X, double E[12], double e[6])
{
    double inv[12], D[12];
    rigid_inverse(Ti, inv);
    rigid_compose(inv, Tj, E);
    rigid_inverse(X, inv);
    rigid_compose(E, inv, D);
    e[0] = D[3]; e[1] = D[7]; e[2] = D[11];
    quat_vector(D, e + 3);
}

// f = sum_r e_r (sum_c L_rc e_c), both ascending
USIP_HD double energy(const double* L, const double e[6])
{
    double f = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) s += L[6 * r + c] * e[c];
        f += e[r] * s;
    }
    return f;
}

// The line process in closed form: mu = L_00 tau2; an odometry edge is never switched off.
USIP_HD double weight(double f, double kappa, double tau2, bool odometry)
{
    if (odometry) return 1.0;
    const double mu = kappa * tau2, den = mu + f;
    if (!(finite(den) && den > 0.0)) return 0.0;
    const double q = mu / den;
    return q * q;
}

// What leaves the call for f: never a NaN.
USIP_HD double energy_out(double f) { return finite(f) ? f : -1.0; }

// Ad_E (rho, phi) = (R rho + t x (R phi), R phi), as a 6 x 6 matrix
USIP_HD void adjoint(const double E[12], double Ad[36])
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Ad[6 * r + c] = E[4 * r + c];
            Ad[6 * (r + 3) + c + 3] = E[4 * r + c];
            Ad[6 * (r + 3) + c] = 0.0;
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Ad[0 * 6 + 3 + c] = E[7] * E[8 + c] - E[11] * E[4 + c];
        Ad[1 * 6 + 3 + c] = E[11] * E[c] - E[3] * E[8 + c];
        Ad[2 * 6 + 3 + c] = E[3] * E[4 + c] - E[7] * E[c];
    }
}

// The edge's share of the normal equations under the weight l > 0, with J_i = -S, J_j = S Ad_E, S = diag(1, 1, 1, 1/2, 1/2,
// 1/2): M = S (l L) S, out[B_II] = M, out[B_JJ] = Ad' (M Ad), out[B_JI] = -(Ad' M), v = S ((l L) e), out[G_I] = -v, out[G_J]
// = Ad' v.  Every inner sum runs over k = 0 .. 5 from the left.
USIP_HD void edge_blocks(const double E[12], const double e[6], const double* L, double l, double* out)
{
    double Ad[36], M[36], v[6];
    adjoint(E, Ad);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const double sr = r < 3 ? 1.0 : 0.5;
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const double w = l * L[6 * r + c];
            M[6 * r + c] = (sr * w) * (c < 3 ? 1.0 : 0.5);
            s += w * e[c];
        }
        v[r] = sr * s;
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            out[B_II + 6 * r + c] = M[6 * r + c];
            double a = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) a += Ad[6 * k + r] * M[6 * k + c];
            out[B_JI + 6 * r + c] = -a;
        }
        out[G_I + r] = -v[r];
        double b = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) b += Ad[6 * k + r] * v[k];
        out[G_J + r] = b;
    }
    // (j, j) = Ad' (M Ad): a column of M Ad at a time
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double P[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double a = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) a += M[6 * r + k] * Ad[6 * k + c];
            P[r] = a;
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double a = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) a += Ad[6 * k + r] * P[k];
            out[B_JJ + 6 * r + c] = a;
        }
    }
}

// T <- T exp(d), d = (rho, phi): t <- R rho + t with the old R, then R <- R Rd, Rd = Rz(phi2) Ry(phi1) Rx(phi0)
USIP_HD void apply_update(double* T, const double d[6])
{
    double Rd[9], R[9];
    usip_fgr::rotation_zyx(d + 3, Rd);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = T[4 * r + c];
        T[4 * r + 3] = ((R[3 * r] * d[0] + R[3 * r + 1] * d[1]) + R[3 * r + 2] * d[2]) + T[4 * r + 3];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) T[4 * r + c] = (R[3 * r] * Rd[c] + R[3 * r + 1] * Rd[3 + c]) + R[3 * r + 2] * Rd[6 + c];
}

// Edge e of a scene is well formed: 0 <= i < j < n, and after its predecessor in the order (i, j).
USIP_HD bool edge_ok(const int32_t* ei, const int32_t* ej, int e, int n)
{
    const int i = ei[e], j = ej[e];
    if (!(0 <= i && i < j && j < n)) return false;
    if (e == 0) return true;
    const int pi = ei[e - 1], pj = ej[e - 1];
    return pi < i || (pi == i && pj < j);
}

// The workspace of one call: per scene the system (the factor's columns, their stride M rounded up to the lanes), the
// edges' blocks and weights, the incidence lists.
struct Layout {
    long long lt, blocks, wbuf, list, per_scene, bytes;
    USIP_HD Layout(int S, int Nmax, int Emax)
    {
        const long long M = 6LL * (Nmax - 1);
        long long at = 0;
        lt = at;     at += align(M * ((M + LANES - 1) / LANES * LANES) * 8);
        blocks = at; at += align((long long)Emax * EDGE_W * 8);
        wbuf = at;   at += align((long long)Emax * 8);
        list = at;   at += align(2LL * Emax * 4);
        per_scene = at;
        bytes = at * S;
    }
    USIP_HD static long long align(long long v) { return (v + 255) / 256 * 256; }
};

USIP_HD bool shape_ok(int S, int Nmax, int Emax)
{
    return S >= 0 && S <= SMAX && Nmax >= 2 && Nmax <= NMAX && Emax >= 1 && (long long)Emax <= emax_of(Nmax);
}

}  // namespace usip_pg
