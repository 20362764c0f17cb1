// usip_amd/csrc/sift_math.h -- the arithmetic of the SIFT3D baseline detector, shared by the kernels of
// csrc/sift.hip and the host twin of csrc/sift_cpu.cpp: both sides run the same float64 operations in the same order on the
// float32 points of a frame, so their results are equal bit for bit.  It sits over prepare_math.h (sqdist, KList) and
// iss_math.h (bad_frames, live_points).
//
// Reference semantics: evaluation/save_keypoints.py:57-61, 314-325 asks an external PCL binding (PCLKeypoint.keypointSift)
// for SIFT keypoints of the xyz columns with min_scale 0.5, n_octaves 4, n_scales_per_octave 8, min_contrast 0.1.  Neither
// the binding nor PCL is part of the reference, and the binding receives nothing but xyz: the field of the scale space can
// only be a function of a coordinate (PCL's field selector for xyz-only clouds is z).  What follows is this project's own
// definition, written from PCL's SIFTKeypoint; the field is an axis of the cloud or a scalar per point.
//   octaves        base_o = min_scale * 2^o.  Octave 0's cloud is the voxel average of the input at leaf base_0, octave o's
//                  the voxel average of octave o-1's cloud at leaf base_o.  cell = floor(v / leaf) per axis in float64 (the
//                  grid is anchored at the origin); each cell index + 2^20 takes 21 bits of an int64 key, x the highest;
//                  a cell index outside [-2^20, 2^20) or a non-finite coordinate drops the row (key DEAD_KEY).  A cell's
//                  centroid is the float64 sum of its members in ascending input index, divided by the count, cast to
//                  float32; its field is its own float32 coordinate (axis field) or the members' float64 mean cast to
//                  float32 (supplied field).  Rows in ascending key.  A cloud with fewer than MIN_POINTS = 25 points is
//                  treated as EMPTY by the three stages below (no keypoint; counts only shrink, so no later octave has one)
//   scales         S = n_scales_per_octave + 3, sigma_s = base_o * 2^((s - 1) / n_scales_per_octave); the caller computes the
//                  S values sigma_s^2 once on the host and hands the same array to either side
//   scale space    members of (i, s): d2(i, j) < 9 * sigma_s^2 (strict; 9.0 * sigma2 once, in float64); the point itself is
//                  one.  w = sift_exp(-((0.5 * d2) / sigma_s^2)); num_s += f_j * w, den_s += w in ascending position of the
//                  frame's stable order along x; G_s = num_s / den_s; DoG_s = G_{s+1} - G_s, s = 0 .. S-2
//   extrema        the neighbourhood of i: its 25 nearest rows, itself included, ascending (d2, row).  For s = 1 .. S-3, v =
//                  DoG_s[i] is extremal iff |v| >= min_contrast and (v == min_s and v < min_{s-1} and v < min_{s+1}) or the
//                  same with maxima and >.  A keypoint iff extremal at some s; scale_index = the lowest such s (0: none)
#pragma once
#include "iss_math.h"

namespace usip_sift {

using usip_iss::bad_frames;
using usip_prep::NMAX;
using usip_prep::TILE;

constexpr int NEAREST = 25;             // rows of a neighbourhood = the fewest points of an octave that yields keypoints
constexpr int MIN_POINTS = NEAREST;
constexpr int SCALES_MAX = 8 + 3;       // S at n_scales_per_octave = 8
constexpr int SCALES_MIN = 1 + 3;
constexpr long long CELL_OFFSET = 1LL << 20;
constexpr int64_t DEAD_KEY = 0x7fffffffffffffffLL;   // behind every cell's key

USIP_HD bool is_finite(double v) { return fabs(v) < (double)INFINITY; }   // (a NaN fails the comparison too)

// one axis' cell index + 2^20, or -1 for a row to drop
USIP_HD long long cell_of(float v, double leaf)
{
    const double c = floor((double)v / leaf);
    return (is_finite(c) && c >= -(double)CELL_OFFSET && c < (double)CELL_OFFSET) ? (long long)c + CELL_OFFSET : -1;
}

USIP_HD int64_t cell_key(float x, float y, float z, double leaf)
{
    const long long cx = cell_of(x, leaf), cy = cell_of(y, leaf), cz = cell_of(z, leaf);
    return (cx < 0 || cy < 0 || cz < 0) ? DEAD_KEY : (int64_t)((cx << 42) | (cy << 21) | cz);
}

// One cell's sums, in the order its members are added.  field == nullptr: the field is the centroid's coordinate `axis`.
struct CellSum {
    double sx = 0.0, sy = 0.0, sz = 0.0, sf = 0.0;
    int32_t c = 0;
    USIP_HD void add(float x, float y, float z, float f)
    {
        sx += (double)x;
        sy += (double)y;
        sz += (double)z;
        sf += (double)f;
        ++c;
    }
    USIP_HD void centroid(bool supplied, int axis, float* x, float* y, float* z, float* f) const
    {
        const double k = (double)c;
        *x = (float)(sx / k);
        *y = (float)(sy / k);
        *z = (float)(sz / k);
        *f = supplied ? (float)(sf / k) : (axis == 0 ? *x : (axis == 1 ? *y : *z));
    }
};

// The scales of one octave as either side sees them: sigma_s^2 as handed in.  The membership bound is bound(s) = 9.0 *
// sigma_s^2, one float64 product wherever it is taken (a kernel argument of its own per scale would cost the scale-space
// kernel 22 more scalar registers, which it does not have at S >= 8).
struct Scales {
    double s2[SCALES_MAX];
    USIP_HD double bound(int s) const { return 9.0 * s2[s]; }
};
inline Scales make_scales(const double* sigma2, int S)
{
    Scales sc;
    for (int s = 0; s < SCALES_MAX; ++s) sc.s2[s] = s < S ? sigma2[s] : 1.0;
    return sc;
}
// every sigma_s^2 finite and positive, and none smaller than the one before (the last bound is the walk's)
inline bool good_scales(const double* sigma2, int S)
{
    if (!sigma2 || S < SCALES_MIN || S > SCALES_MAX) return false;
    for (int s = 0; s < S; ++s)
        if (!(sigma2[s] > 0.0) || !is_finite(9.0 * sigma2[s]) || (s > 0 && sigma2[s] < sigma2[s - 1])) return false;
    return true;
}
// the walk's radius: the smallest float64 at or above sqrt(t) whose float64 square is at least t
inline double walk_radius(double t)
{
    double r = sqrt(t);
    while (r * r < t) r = nextafter(r, (double)INFINITY);
    return r;
}

// e^x for x in [-4.5, 0] (used to -745 without harm: the result is then 0 or tiny), this project's own: x = k ln 2 + r with
// k = rint(x / ln 2) and ln 2 split in two so that k * LN2_HI is exact for |k| < 2^20, |r| <= 0.347; the Taylor polynomial
// of degree 13 in Horner's order (the first term left out is r^14 / 14! < 5e-18); the power of two by ldexp, which is exact.
// Every operation is a single IEEE float64 operation in the order written: device and host agree bit for bit.
USIP_HD double sift_exp(double x)
{
    const double k = rint(x * 1.44269504088896338700e+00);
    const double r = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return ldexp(p, (int)k);
}

// What one query gathers on its way through the octave cloud: num_s and den_s of every scale, in the order the points are
// offered.  S is a compile-time bound: the sums stay in registers.
template <int S>
struct ScaleSums {
    double num[S], den[S];
    USIP_HD void clear()
    {
#pragma unroll
        for (int s = 0; s < S; ++s) { num[s] = 0.0; den[s] = 0.0; }
    }
    USIP_HD void offer(double xi, double yi, double zi, float xj, float yj, float zj, float fj, const Scales& sc)
    {
        const double d2 = usip_prep::sqdist(xi, yi, zi, xj, yj, zj);
        if (!(d2 < sc.bound(S - 1))) return;                              // (the bounds ascend: a member of no scale)
        const double h = 0.5 * d2, f = (double)fj;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (d2 < sc.bound(s)) {
                const double w = sift_exp(-(h / sc.s2[s]));
                num[s] += f * w;
                den[s] += w;
            }
        }
    }
    // DoG_s = G_{s+1} - G_s into out[s * stride], s = 0 .. S-2
    USIP_HD void dog(double* out, long long stride) const
    {
        double g = num[0] / den[0];
#pragma unroll
        for (int s = 0; s + 1 < S; ++s) {
            const double g1 = num[s + 1] / den[s + 1];
            out[s * stride] = g1 - g;
            g = g1;
        }
    }
};

// The minima and maxima of DoG over a neighbourhood, per scale, and the decision.
template <int S>
struct Extrema {
    double mn[S - 1], mx[S - 1];
    USIP_HD void clear()
    {
#pragma unroll
        for (int s = 0; s + 1 < S; ++s) { mn[s] = (double)INFINITY; mx[s] = -(double)INFINITY; }
    }
    // one row of the neighbourhood: col[s * stride] = DoG_s of that row
    USIP_HD void offer(const double* col, long long stride)
    {
#pragma unroll
        for (int s = 0; s + 1 < S; ++s) {
            const double v = col[s * stride];
            mn[s] = v < mn[s] ? v : mn[s];
            mx[s] = v > mx[s] ? v : mx[s];
        }
    }
    // the lowest s in 1 .. S-3 at which the point with DoG column `own` is extremal, 0 when there is none
    USIP_HD int decide(const double* own, long long stride, double min_contrast) const
    {
        int found = 0;
#pragma unroll
        for (int s = S - 3; s >= 1; --s) {
            const double v = own[s * stride];
            const bool low = v == mn[s] && v < mn[s - 1] && v < mn[s + 1];
            const bool high = v == mx[s] && v > mx[s - 1] && v > mx[s + 1];
            found = (fabs(v) >= min_contrast && (low || high)) ? s : found;
        }
        return found;
    }
};

// the live points of frame f as the three stages behind the voxel average see them
USIP_HD int octave_points(const int32_t* count, int f, int N)
{
    const int n = usip_iss::live_points(count, f, N);
    return n < MIN_POINTS ? 0 : n;
}

// S -> the instantiation for it
#define USIP_SIFT_DISPATCH(S, CALL)                                                      \
    switch (S) {                                                                         \
        case 4: CALL(4); break;   case 5: CALL(5); break;   case 6: CALL(6); break;      \
        case 7: CALL(7); break;   case 8: CALL(8); break;   case 9: CALL(9); break;      \
        case 10: CALL(10); break; case 11: CALL(11); break;                              \
        default: return USIP_EINVAL;                                                     \
    }

}  // namespace usip_sift
