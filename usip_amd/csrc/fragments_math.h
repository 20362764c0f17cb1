// usip_amd/csrc/fragments_math.h -- the arithmetic of indoor fragment registration, shared by the kernels of
// csrc/fragments.hip and the host twin of csrc/fragments_cpu.cpp.  The convention is f-6's: float32 inputs, float64
// arithmetic, sums in a fixed order.  RANSAC (the rigid fit, the residual, the draws, the stopping rule and the refit), the
// clamps and the tree sum are csrc/registration_math.h's own; this header adds what register2Fragments.m does around them.
//
// Reference semantics (evaluation/matlab/eval_indoor/3dmatch/register2Fragments.m):
//   pdist2(b, a, 'euclidean', 'smallest', k)   per row of a the k nearest rows of b, ascending, the lower index on ties
//   union(m12, m21, 'rows')                    unique rows (i, q), sorted by i, then q
//   information matrix                         sum over inliers of A'A, A = [I3 | M], M = [0 2sz -2sy; -2sz 0 2sx; 2sy -2sx 0]
//                                              with s the inlier's fragment-1 keypoint
//   ratioAligned                               the share of a fragment's points with a point of the other fragment, moved
//                                              by the estimate, at sqrt(d2) < 0.2
#pragma once
#include "registration_math.h"

namespace usip_frag {

constexpr int KMAX = 8;                 // neighbours per descriptor
constexpr int UNION_MAX = 10240;        // k (Ma + Mp): every row of the union is a correspondence of the pair's RANSAC
static_assert(UNION_MAX <= usip_reg::NMAX, "the union of a pair must fit the RANSAC entry points");
constexpr int OTILE = 256;              // database points per LDS tile of the overlap walk
constexpr int INFO_W = 10;              // partial sums per lane of the information matrix (9 used)

// The K best (distance, index) a lane has seen, ascending; candidates arrive in ascending index, so a strict comparison
// keeps the lower index first among equal distances.  Compile-time indices only: the list stays in registers.
template <int K>
struct TopK {
    float d[K];
    int j[K];
    USIP_HD void clear()
    {
#pragma unroll
        for (int s = 0; s < K; ++s) { d[s] = __builtin_inff(); j[s] = 0x7fffffff; }
    }
    USIP_HD void offer(float dist, int idx)
    {
        if (!(dist < d[K - 1])) return;
        d[K - 1] = dist;
        j[K - 1] = idx;
#pragma unroll
        for (int s = K - 1; s > 0; --s)
            if (d[s] < d[s - 1]) {
                const float td = d[s]; d[s] = d[s - 1]; d[s - 1] = td;
                const int tj = j[s]; j[s] = j[s - 1]; j[s - 1] = tj;
            }
    }
    USIP_HD void pop()
    {
#pragma unroll
        for (int s = 0; s + 1 < K; ++s) { d[s] = d[s + 1]; j[s] = j[s + 1]; }
        d[K - 1] = __builtin_inff();
        j[K - 1] = 0x7fffffff;
    }
};

// One inlier's nine distinct terms of A'A: the three entries of M (2sx, 2sy, 2sz) and the six of M'M.
USIP_HD void info_terms(double sx, double sy, double sz, double t[9])
{
    const double ax = 2.0 * sx, ay = 2.0 * sy, az = 2.0 * sz;
    t[0] = ax;
    t[1] = ay;
    t[2] = az;
    t[3] = az * az + ay * ay;           // (4, 4)
    t[4] = az * az + ax * ax;           // (5, 5)
    t[5] = ay * ay + ax * ax;           // (6, 6)
    t[6] = ax * ay;                     // -(4, 5)
    t[7] = ax * az;                     // -(4, 6)
    t[8] = ay * az;                     // -(5, 6)
}

// The 6 x 6 matrix from the summed terms and the number of inliers: assigned entry by entry, so exactly symmetric.
USIP_HD void info_fill(const double s[9], int n, double out[36])
{
#pragma unroll
    for (int k = 0; k < 36; ++k) out[k] = 0.0;
    out[0] = out[7] = out[14] = (double)n;
    out[0 * 6 + 4] = out[4 * 6 + 0] = s[2];
    out[0 * 6 + 5] = out[5 * 6 + 0] = -s[1];
    out[1 * 6 + 3] = out[3 * 6 + 1] = -s[2];
    out[1 * 6 + 5] = out[5 * 6 + 1] = s[0];
    out[2 * 6 + 3] = out[3 * 6 + 2] = s[1];
    out[2 * 6 + 4] = out[4 * 6 + 2] = -s[0];
    out[3 * 6 + 3] = s[3];
    out[4 * 6 + 4] = s[4];
    out[5 * 6 + 5] = s[5];
    out[3 * 6 + 4] = out[4 * 6 + 3] = -s[6];
    out[3 * 6 + 5] = out[5 * 6 + 3] = -s[7];
    out[4 * 6 + 5] = out[5 * 6 + 4] = -s[8];
}

// b' = R b + t, one coordinate (Utils.apply_transform's order, as csrc/registration.hip's repeatability)
USIP_HD double xform(const double* Rt, int c, double b0, double b1, double b2)
{
    return ((Rt[4 * c] * b0 + Rt[4 * c + 1] * b1) + Rt[4 * c + 2] * b2) + Rt[4 * c + 3];
}

USIP_HD double sqdist3(double ax, double ay, double az, double bx, double by, double bz)
{
    const double d0 = ax - bx, d1 = ay - by, d2 = az - bz;
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

// sqrt(d2) < radius, the comparison register2Fragments.m makes; the square root is taken only near the radius
USIP_HD bool within(double d2, double radius, double r2hi) { return d2 <= r2hi && sqrt(d2) < radius; }
USIP_HD double radius_sq_hi(double radius) { return (radius * radius) * (1.0 + 8.0 * 2.220446049250313e-16); }

// A tile whose every point is at least gap > 0 away along x holds no point within the radius: d2 = (dx dx + ..) + ..
// >= fl(dx dx) >= fl(gap gap) and the square root is monotone, so sqrt(d2) >= sqrt(fl(gap gap)) >= radius.
USIP_HD bool beyond(double gap, double radius) { return gap > 0.0 && sqrt(gap * gap) >= radius; }

}  // namespace usip_frag
