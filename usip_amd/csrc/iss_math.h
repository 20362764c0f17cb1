// usip_amd/csrc/iss_math.h -- the arithmetic of the ISS baseline detector, shared by the kernels of
// csrc/iss.hip and the host twin of csrc/iss_cpu.cpp: both sides run the same float64 operations in the same order on the
// float32 points of a frame, so their results are equal bit for bit.
//
// Reference semantics: evaluation/save_keypoints.py:44-50 asks an external PCL binding (PCLKeypoint.keypointIss) for
// Intrinsic Shape Signatures keypoints with salient_radius 2, non_max_radius 2, gamma_21 = gamma_32 = 0.975, min_neighbors
// 5.  Neither the binding nor PCL is part of the reference: what follows is this project's own definition, written from
// PCL's ISSKeypoint3D (iss_3d.hpp) with border estimation off, which is what keypointIss uses:
//   membership     j in N_r(i) iff sqdist(i, j) < r * r (strict, as FLANN's radius result set; r * r once, in float64);
//                  the point itself is a member
//   scatter        C = sum over N_rs(i) of (p_j - p_i)(p_j - p_i)', NOT divided by the count (PCL does not divide); the
//                  six sums are taken in ascending position of the frame's stable order along x
//   eigenvalues    JACOBI_SWEEPS cyclic Jacobi sweeps of prepare_math.h, e1 >= e2 >= e3; saliency = e3 iff the three are
//                  finite, e3 >= 0, e2 / e1 < gamma_21 and e3 / e2 < gamma_32 (a NaN ratio fails), else 0; fewer than
//                  min_neighbors members: 0
//   suppression    i is a keypoint iff saliency[i] > 0, |N_rn(i)| >= min_neighbors and no member of N_rn(i) has a LARGER
//                  saliency (equal saliencies do not suppress each other)
#pragma once
#include "prepare_math.h"

namespace usip_iss {

using usip_prep::Cov;
using usip_prep::NMAX;
using usip_prep::TILE;

USIP_HD bool member(double d2, double r2) { return d2 < r2; }

// What every entry point of the baseline detectors (ISS, Harris3D, SIFT3D; device and host twin) refuses, and the live points
// of frame f: the first count[f] of N, clamped
USIP_HD bool bad_frames(int B, int N) { return B < 1 || B > 65535 || N < 1 || N > NMAX; }
USIP_HD bool bad_radius(double r) { return !(r > 0.0) || !(r < (double)INFINITY); }
USIP_HD int live_points(const int32_t* count, int f, int N)
{
    const int c = count ? count[f] : N;
    return c < 0 ? 0 : (c > N ? N : c);
}

// What one query gathers on its way through the frame at the salient radius: the members and the six sums, in the order
// the points are offered.
struct Scatter {
    Cov S;
    int32_t n = 0;
    USIP_HD void offer(double xi, double yi, double zi, float xj, float yj, float zj, double r2)
    {
        if (member(usip_prep::sqdist(xi, yi, zi, xj, yj, zj), r2)) {
            S.add((double)xj - xi, (double)yj - yi, (double)zj - zi);
            ++n;
        }
    }
};

// The saliency of a query from what it gathered.
USIP_HD double saliency_from(const Scatter& g, int min_neighbors, double gamma_21, double gamma_32)
{
    const Cov& S = g.S;
    double a[3][3] = {{S.s00, S.s01, S.s02}, {S.s01, S.s11, S.s12}, {S.s02, S.s12, S.s22}};
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};                // (the eigenvectors are not used)
    for (int sweep = 0; sweep < usip_prep::JACOBI_SWEEPS; ++sweep) {
        usip_prep::jacobi_rotate3<0, 1>(a, v);
        usip_prep::jacobi_rotate3<0, 2>(a, v);
        usip_prep::jacobi_rotate3<1, 2>(a, v);
    }
    double e1 = a[0][0], e2 = a[1][1], e3 = a[2][2], t;               // three compare-exchanges: e1 >= e2 >= e3
    if (e1 < e2) { t = e1; e1 = e2; e2 = t; }
    if (e2 < e3) { t = e2; e2 = e3; e3 = t; }
    if (e1 < e2) { t = e1; e1 = e2; e2 = t; }
    const double inf = (double)INFINITY;                               // (a NaN fails the comparison too)
    const bool finite = fabs(e1) < inf && fabs(e2) < inf && fabs(e3) < inf;
    const bool salient = g.n >= min_neighbors && finite && e3 >= 0.0 && e2 / e1 < gamma_21 && e3 / e2 < gamma_32;
    return salient ? e3 : 0.0;
}

// What one query gathers at the non-maximum radius: the members and whether one of them has a larger saliency.
struct Rivals {
    int32_t n = 0;
    bool larger = false;
    USIP_HD void offer(double xi, double yi, double zi, double si, float xj, float yj, float zj, double sj, double r2)
    {
        if (member(usip_prep::sqdist(xi, yi, zi, xj, yj, zj), r2)) {
            ++n;
            larger = larger || sj > si;
        }
    }
};

USIP_HD bool keypoint_from(const Rivals& g, double si, int min_neighbors)
{
    return si > 0.0 && g.n >= min_neighbors && !g.larger;
}

}  // namespace usip_iss
