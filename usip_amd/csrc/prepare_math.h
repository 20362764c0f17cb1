// usip_amd/csrc/prepare_math.h -- the arithmetic of raw-scan preparation, shared by the kernels of
// csrc/prepare.hip and the host twin of csrc/prepare_cpu.cpp: both sides run the same float64 operations in the same order
// on the float32 rows of a scan (x y z reflectance), so their results are equal bit for bit.
//
// Reference semantics (evaluation/matlab/kitti_data_prepare/kitti_test_prepare.m:95-108, external findPointNormals.m):
//   knnsearch(k + 1), "remove self"   the K nearest other points, ascending (d2, index); here the point is left out by INDEX
//   C = sum d d' / K, eig, min         3x3 covariance about the point, eigenvector of the smallest eigenvalue, curvature
//                                      lambda_min / (l0 + l1 + l2); a fixed-sweep cyclic Jacobi instead of MATLAB's eig
//   dirLargest flip                    c = first arg max |normal|; negate when normal[c] * (p[c] - viewpoint[c]) > 0
//   pcdownsample 'gridAverage'         a MATLAB builtin without source: the cell, the key and the order of the sums below are
//                                      this project's own definition
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef USIP_HD
#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define USIP_HD __host__ __device__ __forceinline__
#else
#define USIP_HD inline
#endif
#endif

namespace usip_prep {

constexpr int KMAX = 16;                // neighbours per point
constexpr int NMAX = 1 << 20;           // points per scan
constexpr int TILE = 256;               // queries of a workgroup = database points of one LDS tile
constexpr int CELLS_MAX = 1 << 20;      // cells per axis: three of them fit an int64 key
// 3x3, float64: cyclic Jacobi converges quadratically once the off-diagonal mass is small; three sweeps bring it below
// 1e-3 of the norm for any symmetric 3x3, every further sweep squares it (1e-6, 1e-12, 1e-24, ...), so after 8 sweeps it
// is far below 1e-300 of the norm -- the constant registration_math.h uses for 4x4, for the same reason.
constexpr int JACOBI_SWEEPS = 8;

// squared distance of two float32 points in float64: (dx*dx + dy*dy) + dz*dz, never contracted
USIP_HD double sqdist(double xi, double yi, double zi, float xj, float yj, float zj)
{
    const double dx = xi - (double)xj, dy = yi - (double)yj, dz = zi - (double)zj;
    return (dx * dx + dy * dy) + dz * dz;
}

// the order of the neighbour list: ascending distance, ties towards the lower index
USIP_HD bool before(double d, int32_t j, double dk, int32_t jk) { return d < dk || (d == dk && j < jk); }

// The K best (d2, index) of everything offered so far, ascending.  Compile-time indices only: the list stays in registers.
template <int K>
struct KList {
    double d[K];
    int32_t j[K];
    USIP_HD void clear()
    {
#pragma unroll
        for (int k = 0; k < K; ++k) { d[k] = (double)INFINITY; j[k] = 0x7fffffff; }
    }
    USIP_HD double worst() const { return d[K - 1]; }
    USIP_HD bool admits(double dc, int32_t jc) const { return before(dc, jc, d[K - 1], j[K - 1]); }
    // insert a candidate that admits() accepted: one pass from the front; where the candidate goes before a slot it takes
    // the slot and the slot's entry travels on (it goes before everything behind it); the last one falls off the end
    USIP_HD void insert(double dc, int32_t jc)
    {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool b = before(dc, jc, d[k], j[k]);
            const double td = d[k];
            const int32_t tj = j[k];
            d[k] = b ? dc : td;
            j[k] = b ? jc : tj;
            dc = b ? td : dc;
            jc = b ? tj : jc;
        }
    }
};

// One Jacobi rotation in the (P, Q) plane of the symmetric 3x3 a (full storage), accumulated into the columns of v:
// the rotation of registration_math.h at 3x3.
template <int P, int Q>
USIP_HD void jacobi_rotate3(double a[3][3], double v[3][3])
{
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double root = sqrt(theta * theta + 1.0);                     // inf for a vanishing apq: t = 0, no NaN
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + root);
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {                                      // columns P, Q
        const double akp = a[k][P], akq = a[k][Q];
        a[k][P] = c * akp - s * akq;
        a[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {                                      // rows P, Q
        const double apk = a[P][k], aqk = a[Q][k];
        a[P][k] = c * apk - s * aqk;
        a[Q][k] = s * apk + c * aqk;
    }
    a[P][Q] = 0.0;
    a[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vkp = v[k][P], vkq = v[k][Q];
        v[k][P] = c * vkp - s * vkq;
        v[k][Q] = s * vkp + c * vkq;
    }
}

// The six sums of d d' over the neighbours, in the order they are offered (named fields, not an array: a kernel's loop
// over a run-time K must not index them)
struct Cov {
    double s00 = 0.0, s01 = 0.0, s02 = 0.0, s11 = 0.0, s12 = 0.0, s22 = 0.0;
    USIP_HD void add(double d0, double d1, double d2)
    {
        s00 += d0 * d0;
        s01 += d0 * d1;
        s02 += d0 * d2;
        s11 += d1 * d1;
        s12 += d1 * d2;
        s22 += d2 * d2;
    }
};
struct Normal { double x, y, z, curvature; };

// out = (nx, ny, nz, curvature) of the point p from the sums S over its K neighbours.  C = S / K; the eigenvector of the
// smallest eigenvalue (the first of equal ones) by a fixed number of Jacobi sweeps in a fixed order; curvature = lambda_min
// / (l0 + l1 + l2); the flip towards the view point.  A zero trace (every neighbour coincides with the point) gives
// (0, 0, 1, 0) before the flip -- MATLAB gives 0 / 0.
USIP_HD Normal normal_from(const Cov& S, int K, double p0, double p1, double p2, double view0, double view1, double view2)
{
    const double k = (double)K;
    const double c00 = S.s00 / k, c01 = S.s01 / k, c02 = S.s02 / k, c11 = S.s11 / k, c12 = S.s12 / k, c22 = S.s22 / k;
    double a[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}};
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        jacobi_rotate3<0, 1>(a, v);
        jacobi_rotate3<0, 2>(a, v);
        jacobi_rotate3<1, 2>(a, v);
    }
    const bool s1 = a[1][1] < a[0][0];
    double e = s1 ? a[1][1] : a[0][0];
    double n0 = s1 ? v[0][1] : v[0][0], n1 = s1 ? v[1][1] : v[1][0], n2 = s1 ? v[2][1] : v[2][0];
    const bool s2 = a[2][2] < e;
    e = s2 ? a[2][2] : e;
    n0 = s2 ? v[0][2] : n0;
    n1 = s2 ? v[1][2] : n1;
    n2 = s2 ? v[2][2] : n2;
    double curv = e / ((a[0][0] + a[1][1]) + a[2][2]);
    const bool flat = (c00 + c11) + c22 == 0.0;                        // every neighbour coincides with the point
    n0 = flat ? 0.0 : n0;
    n1 = flat ? 0.0 : n1;
    n2 = flat ? 1.0 : n2;
    curv = flat ? 0.0 : curv;
    const double a0 = fabs(n0), a1 = fabs(n1), a2 = fabs(n2);
    double nc = n0, pc = p0 - view0;                                   // the first of the largest |components|
    if (a1 > a0 && a1 >= a2) { nc = n1; pc = p1 - view1; }
    if (a2 > a0 && a2 > a1) { nc = n2; pc = p2 - view2; }
    const bool flip = nc * pc > 0.0;
    return Normal{flip ? -n0 : n0, flip ? -n1 : n1, flip ? -n2 : n2, curv};
}

// The grid of one scan: lohi = per-axis minimum and maximum of the scan (float32), leaf the cell size.
struct Grid {
    double lo[3], leaf;
    long long nx, ny;
    USIP_HD long long cell(double v, int axis) const
    {
        const double c = floor((v - lo[axis]) / leaf);
        return c < 0.0 ? 0 : (c > (double)(CELLS_MAX - 1) ? (long long)(CELLS_MAX - 1) : (long long)c);
    }
    USIP_HD void init(const float* lohi, double leaf_)
    {
        lo[0] = (double)lohi[0]; lo[1] = (double)lohi[1]; lo[2] = (double)lohi[2];
        leaf = leaf_;
        nx = cell((double)lohi[3], 0) + 1;
        ny = cell((double)lohi[4], 1) + 1;
    }
    USIP_HD long long key(float x, float y, float z) const
    {
        return (cell((double)z, 2) * ny + cell((double)y, 1)) * nx + cell((double)x, 0);
    }
};

// One cell's row: the members perm[first .. last) in that order (ascending original index), sums in float64, the mean
// normal divided by its norm (the first member's normal when the mean is exactly zero).
// An entry of perm outside [0, n) reads point 0: a wrong permutation gives wrong rows, never a wild read.
USIP_HD void cell_average(const float* xyzi, const double* nrm, const int32_t* perm, int n, long long first, long long last,
                          float row[8])
{
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long r = first; r < last; ++r) {
        const long long i = (unsigned)perm[r] < (unsigned)n ? perm[r] : 0;
        s[0] += (double)xyzi[4 * i];
        s[1] += (double)xyzi[4 * i + 1];
        s[2] += (double)xyzi[4 * i + 2];
        s[3] += nrm[4 * i];
        s[4] += nrm[4 * i + 1];
        s[5] += nrm[4 * i + 2];
        s[6] += nrm[4 * i + 3];
        s[7] += (double)xyzi[4 * i + 3];
    }
    const double c = (double)(last - first);
    double m0 = s[3] / c, m1 = s[4] / c, m2 = s[5] / c;
    const double len = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
    if (len == 0.0) {
        const long long i = (unsigned)perm[first] < (unsigned)n ? perm[first] : 0;
        m0 = nrm[4 * i]; m1 = nrm[4 * i + 1]; m2 = nrm[4 * i + 2];
    } else {
        m0 /= len; m1 /= len; m2 /= len;
    }
    row[0] = (float)(s[0] / c);
    row[1] = (float)(s[1] / c);
    row[2] = (float)(s[2] / c);
    row[3] = (float)m0;
    row[4] = (float)m1;
    row[5] = (float)m2;
    row[6] = (float)(s[6] / c);
    row[7] = (float)(s[7] / c);
}

}  // namespace usip_prep
