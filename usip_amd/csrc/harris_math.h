// usip_amd/csrc/harris_math.h -- the arithmetic of the Harris3D baseline detector, shared by the kernels of
// csrc/harris.hip and the host twin of csrc/harris_cpu.cpp: both sides run the same float64 operations in the same order on
// the float32 points of a frame, so their results are equal bit for bit.  It sits over prepare_math.h (sqdist, the Jacobi,
// normal_from) and iss_math.h (member).
//
// Reference semantics: evaluation/save_keypoints.py:52-55, 303-313 asks an external PCL binding (PCLKeypoint.keypointHarris)
// for Harris3D keypoints of the xyz columns with radius 1, nms_threshold 0.001, threads 0.  Neither the binding nor PCL is
// part of the reference: what follows is this project's own definition, written from PCL's HarrisKeypoint3D with method
// HARRIS, its normals from NormalEstimation at the search radius and refineCorners off:
//   membership     usip_iss::member over usip_prep::sqdist: j in N_r(i) iff d2(i, j) < r * r (strict; r * r once, in
//                  float64); the point itself is a member
//   normal         over N_r(i), with d = p_j - p_i: the member count m, the three sums of d and the six sums of d d', taken
//                  in ascending position of the frame's stable order along x.  m < min_neighbors: NO NORMAL (zeros).  Else
//                  c_ab = s_ab - (s_a * s_b) / m and the normal is usip_prep::normal_from(Cov{c}, m, p_i, view = 0): its
//                  Jacobi sweeps, its first-of-equal rule, its (0, 0, 1) for a zero trace and its flip towards the origin
//   has a normal   a row of normals has one iff its three components are finite and not all zero -- which holds for every
//                  normal estimated here, fails for the zeros of a point without one, and is the rule for supplied normals
//                  (float32 cast to float64, used as given, not renormalised)
//   response       a point without a normal: response 0, members 0.  Else C = (sum of n_j n_j') / k over the members of
//                  N_r(i) that have a normal, in the same order; k is their count (>= 1: the point itself);
//                  trace = (c00 + c11) + c22; det as det3() spells it;
//                    HARRIS  (0.04 + det) - (0.04 * trace) * trace     (unit normals have trace 1: this is det)
//                    NOBLE   det / trace
//                    LOWE    det / (trace * trace)
//                    TOMASI  the smallest diagonal entry after JACOBI_SWEEPS sweeps over C
//                  a zero trace gives 0, a non-finite result gives 0
// Suppression and the keypoint count are iss_math.h's keypoint_from with min_neighbors = 1 on the thresholded response and
// usip_amd/baselines.py's selection rule.
#pragma once
#include "iss_math.h"

namespace usip_harris {

using usip_iss::member;
using usip_prep::Cov;
using usip_prep::NMAX;
using usip_prep::TILE;

enum Method : int { HARRIS = 0, NOBLE = 1, LOWE = 2, TOMASI = 3 };
USIP_HD bool known_method(int m) { return m >= HARRIS && m <= TOMASI; }

USIP_HD bool finite(double v) { return fabs(v) < (double)INFINITY; }   // (a NaN fails the comparison too)

// What one query gathers for its normal: the members, the three sums of d and the six of d d', in the order offered.
struct Moments {
    Cov S;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int32_t m = 0;
    USIP_HD void offer(double xi, double yi, double zi, float xj, float yj, float zj, double r2)
    {
        if (member(usip_prep::sqdist(xi, yi, zi, xj, yj, zj), r2)) {
            const double d0 = (double)xj - xi, d1 = (double)yj - yi, d2 = (double)zj - zi;
            s0 += d0;
            s1 += d1;
            s2 += d2;
            S.add(d0, d1, d2);
            ++m;
        }
    }
};

struct Normal3 { double x, y, z; };

USIP_HD bool has_normal(double n0, double n1, double n2)
{
    return finite(n0) && finite(n1) && finite(n2) && !(n0 == 0.0 && n1 == 0.0 && n2 == 0.0);
}

// The normal of the point p from what it gathered; zeros when it has none.
USIP_HD Normal3 normal_of(const Moments& g, int min_neighbors, double p0, double p1, double p2)
{
    if (g.m < min_neighbors) return Normal3{0.0, 0.0, 0.0};
    const double m = (double)g.m;
    Cov c;
    c.s00 = g.S.s00 - (g.s0 * g.s0) / m;
    c.s01 = g.S.s01 - (g.s0 * g.s1) / m;
    c.s02 = g.S.s02 - (g.s0 * g.s2) / m;
    c.s11 = g.S.s11 - (g.s1 * g.s1) / m;
    c.s12 = g.S.s12 - (g.s1 * g.s2) / m;
    c.s22 = g.S.s22 - (g.s2 * g.s2) / m;
    const usip_prep::Normal n = usip_prep::normal_from(c, g.m, p0, p1, p2, 0.0, 0.0, 0.0);
    const bool ok = has_normal(n.x, n.y, n.z);                         // (non-finite coordinates: no normal)
    return Normal3{ok ? n.x : 0.0, ok ? n.y : 0.0, ok ? n.z : 0.0};
}

// What one query gathers for its response: the members that have a normal and the six sums of n n', in the order offered.
struct Tensor {
    Cov S;
    int32_t k = 0;
    USIP_HD void offer(double xi, double yi, double zi, float xj, float yj, float zj, bool has, double n0, double n1, double n2,
                       double r2)
    {
        if (has && member(usip_prep::sqdist(xi, yi, zi, xj, yj, zj), r2)) {
            S.add(n0, n1, n2);
            ++k;
        }
    }
};

// the one evaluation order of the determinant of the symmetric 3x3
USIP_HD double det3(double c00, double c01, double c02, double c11, double c12, double c22)
{
    return (((((c00 * c11) * c22 + ((2.0 * c01) * c02) * c12) - (c02 * c02) * c11) - (c01 * c01) * c22) - (c12 * c12) * c00);
}

// The response of a query that has a normal, from what it gathered (k >= 1).
USIP_HD double response_from(const Tensor& g, int method)
{
    const double k = (double)g.k;
    const double c00 = g.S.s00 / k, c01 = g.S.s01 / k, c02 = g.S.s02 / k, c11 = g.S.s11 / k, c12 = g.S.s12 / k,
                 c22 = g.S.s22 / k;
    const double trace = (c00 + c11) + c22;
    const double det = det3(c00, c01, c02, c11, c12, c22);
    double r;
    if (method == TOMASI) {
        double a[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}};
        double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};            // (the eigenvectors are not used)
        for (int sweep = 0; sweep < usip_prep::JACOBI_SWEEPS; ++sweep) {
            usip_prep::jacobi_rotate3<0, 1>(a, v);
            usip_prep::jacobi_rotate3<0, 2>(a, v);
            usip_prep::jacobi_rotate3<1, 2>(a, v);
        }
        r = a[1][1] < a[0][0] ? a[1][1] : a[0][0];
        r = a[2][2] < r ? a[2][2] : r;
    } else if (method == NOBLE) {
        r = det / trace;
    } else if (method == LOWE) {
        r = det / (trace * trace);
    } else {
        r = (0.04 + det) - (0.04 * trace) * trace;
    }
    return (g.k < 1 || trace == 0.0 || !finite(r)) ? 0.0 : r;
}

}  // namespace usip_harris
