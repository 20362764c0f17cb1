// usip_amd/csrc/spin.hip -- the spin-image baseline descriptor on the device: the hand-crafted descriptor the
// reference's indoor scoring scripts name (eval_indoor/3dmatch/evaluate.m: descriptorName = 'my'; % 3dmatch, spin, fpfh) and the
// reference does not contain.  csrc/spin_math.h has the semantics and the arithmetic, which the host twin (csrc/spin_cpu.cpp)
// shares.  pc f32 [B][3][N], count i32 [B] live points per frame, perm i32 [B][N] the frame SORTED ALONG X (the caller's
// permutation), keypoints f32 [B][3][M] at any positions, axes f64 [B][M][3], normals f64 [B][3][N] only with a support angle.
// The launch does not synchronise; no global atomics, no float atomics; no per-lane array with a run-time index.
//
// spin_image_kernel<STRUCTURE> is a sibling of shot_hist_kernel (csrc/shot.hip): grid = (ceil(M / 4), B), 256 lanes, one wave
// per keypoint.  The wave finds [lo, hi), the sorted positions with |x - q_x| < r, by two binary searches (wave-uniform); a row
// outside [lo, hi) has d2 >= r2, so the result is the all-pairs answer.  Lane l tests the rows lo + l + 64 k.  Each wave owns
// u64 hist[153] in LDS (4 * 153 * 8 = 4896 bytes per workgroup), zeroed first; a lane adds the at most four cells of each of its
// members with LDS 64-bit integer atomic adds (integer sums: the order is free); then lane l reads the columns l + 64 k and
// writes them to hist i64 [B][M][153] and, divided by the exact kp_members * 2^40, to spin f64 [B][M][153] (a wave's 64 lanes
// write 64 consecutive columns at a time); lane 0 writes kp_members i32 [B][M].  The support-angle test is a wave-uniform
// branch: without one no normal is read.  The waves of a workgroup are independent; the two workgroup barriers around the
// adds are shot_hist_kernel's, and every wave reaches them (an idle wave of the last workgroup walks nothing).
// Slots beyond kp_count[b] and keypoints without an axis get zeros.
#include "ascending_walk.h"
#include "spin_math.h"

using namespace usip_spin;
using usip_ascend::Frame;
using usip_iss::bad_frames;
using usip_iss::bad_radius;
using usip_iss::live_points;

namespace {

// [lo, hi) of the sorted positions that can hold a member of the keypoint at q_x; wave-uniform
struct Window {
    int lo, hi;
    USIP_DEV Window(const Frame& F, double qx, double r)
    {
        const auto xs = [&](int s) { return F.xs(s); };
        lo = first_within(F.n, qx, r, xs);
        hi = lo;
        int end = F.n;                                                 // the first position from lo on with x - q_x >= r
        while (hi < end) {
            const int mid = (hi + end) >> 1;
            if (xs(mid) - qx >= r) end = mid; else hi = mid + 1;
        }
    }
};

USIP_DEV int32_t fold(int32_t v)
{
#pragma unroll
    for (int off = LANES / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, LANES);
    return v;
}

template <int STRUCTURE>
__global__ __launch_bounds__(TILE) void spin_image_kernel(const float* __restrict__ pc, const int32_t* __restrict__ count,
                                                          const int32_t* __restrict__ perm, const double* __restrict__ normals,
                                                          const float* __restrict__ keypoints,
                                                          const int32_t* __restrict__ kp_count, const double* __restrict__ axes,
                                                          int N, int M, double r, double r2, double support,
                                                          long long* __restrict__ hist, double* __restrict__ spin,
                                                          int32_t* __restrict__ kp_members)
{
    __shared__ unsigned long long bins[TILE / LANES][WIDTH];
    const int f = blockIdx.y, lane = threadIdx.x & (LANES - 1), wave = threadIdx.x >> 6;
    const int q = blockIdx.x * (TILE / LANES) + wave;                  // the wave's keypoint
    const bool there = q < M;                                          // wave-uniform
    unsigned long long* mine = bins[wave];
    for (int c = lane; c < WIDTH; c += LANES) mine[c] = 0ULL;
    __syncthreads();
    const Frame F(pc, count, perm, N, f);
    int32_t k = 0;
    if (there && q < live_points(kp_count, f, M) && F.n > 0) {         // wave-uniform
        const float* kp = keypoints + 3LL * f * M;
        const double qx = (double)kp[q], qy = (double)kp[M + q], qz = (double)kp[2LL * M + q];
        const double* v = axes + 3 * ((long long)f * M + q);
        const Axis A(v[0], v[1], v[2]);
        if (A.ok) {                                                    // wave-uniform
            const bool angled = support > 0.0;                         // wave-uniform: normals may be NULL otherwise
            const double *nx = angled ? normals + 3LL * f * N : nullptr, *ny = angled ? nx + N : nullptr,
                         *nz = angled ? ny + N : nullptr;
            const Window win(F, qx, r);
            for (int s = win.lo + lane; s < win.hi; s += LANES) {
                const int j = F.at(s);
                const float xj = F.x[j], yj = F.y[j], zj = F.z[j];
                const double d2 = usip_prep::sqdist(qx, qy, qz, xj, yj, zj);
                if (!(d2 > 0.0 && member(d2, r2))) continue;
                if (angled && !supported(A, support, nx[j], ny[j], nz[j])) continue;
                Adds a;
                if (!member_adds<STRUCTURE>(A, r, d2, (double)xj - qx, (double)yj - qy, (double)zj - qz, a)) continue;
                ++k;
#pragma unroll
                for (int i = 0; i < ADDS; ++i)
                    if (a.q[i] > 0) atomicAdd(&mine[a.col[i]], (unsigned long long)a.q[i]);
            }
        }
    }
    __syncthreads();
    if (!there) return;
    k = fold(k);
    long long* hrow = hist + (long long)WIDTH * ((long long)f * M + q);
    double* srow = spin + (long long)WIDTH * ((long long)f * M + q);
#pragma unroll
    for (int i = 0; i < PER_LANE; ++i) {
        const int c = lane + LANES * i;
        if (c < WIDTH) {
            const long long h = (long long)mine[c];
            hrow[c] = h;
            srow[c] = column(h, k);
        }
    }
    if (lane == 0) kp_members[(long long)f * M + q] = k;
}

}  // namespace

extern "C" int usip_spin_image_f32(const float* pc, const int32_t* count, const int32_t* perm, const double* normals,
                                   const float* keypoints, const int32_t* kp_count, const double* axes, int B, int N, int M,
                                   double radius, double support_angle_cos, int structure, int64_t* hist, double* spin,
                                   int32_t* kp_members, void* stream)
{
    if (bad_frames(B, N) || bad_keypoints(M) || bad_radius(radius) || bad_support(support_angle_cos) ||
        bad_structure(structure) || !pc || !perm || !keypoints || !axes || !hist || !spin || !kp_members ||
        (support_angle_cos > 0.0 && !normals))
        return USIP_EINVAL;
    const dim3 grid(usip_ceil_div(M, TILE / LANES), B), block(TILE);
    if (structure == RADIAL)
        USIP_LAUNCH(spin_image_kernel<RADIAL>, grid, block, 0, (hipStream_t)stream, pc, count, perm, normals, keypoints,
                    kp_count, axes, N, M, radius, radius * radius, support_angle_cos, (long long*)hist, spin, kp_members);
    else
        USIP_LAUNCH(spin_image_kernel<RECTANGULAR>, grid, block, 0, (hipStream_t)stream, pc, count, perm, normals, keypoints,
                    kp_count, axes, N, M, radius, radius * radius, support_angle_cos, (long long*)hist, spin, kp_members);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
