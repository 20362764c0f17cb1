// usip_amd/csrc/spin.hip -- the spin-image baseline descriptor on the device: the hand-crafted descriptor the
// reference's indoor scoring scripts name (eval_indoor/3dmatch/evaluate.m: descriptorName = 'my'; % 3dmatch, spin, fpfh) and the
// reference does not contain.  csrc/spin_math.h has the semantics and the arithmetic, which the host twin (csrc/spin_cpu.cpp)
// shares.  pc f32 [B][3][N], count i32 [B] live points per frame, perm i32 [B][N] the frame SORTED ALONG X (the caller's
// permutation), keypoints f32 [B][3][M] at any positions, axes f64 [B][M][3], normals f64 [B][3][N] only with a support angle.
// The launch does not synchronise; no global atomics, no float atomics; no per-lane array with a run-time index.
//
// spin_image_kernel<STRUCTURE> is a pass of csrc/keypoint_walk.h's histogram() (one wave per keypoint; its window, its walk,
// its exactness argument and its two barriers): u64 hist[153] per wave in LDS (4 * 153 * 8 = 4896 bytes per workgroup), the at
// most four cells of a member added; hist i64 [B][M][153] and, divided by the exact kp_members * 2^40, spin f64 [B][M][153].
// The support-angle test is a wave-uniform branch: without one no normal is read.
// Slots beyond kp_count[b] and keypoints without an axis get zeros.
#include "keypoint_walk.h"
#include "spin_math.h"

using namespace usip_spin;
using usip_ascend::Frame;
using usip_iss::bad_frames;
using usip_iss::bad_radius;
using usip_keypoint::Keypoint;

namespace {

template <int STRUCTURE>
struct ImagePass {
    static constexpr int WIDTH = usip_spin::WIDTH;
    using Key = Axis;
    double r, r2, support;
    const double *nx, *ny, *nz, *axes;                                 // the frame's; no normals without a support angle
    USIP_DEV Key load(int q) const
    {
        const double* v = axes + 3LL * q;
        return Axis(v[0], v[1], v[2]);
    }
    USIP_DEV bool walks(const Key& A) const { return A.ok; }
    template <class Add>
    USIP_DEV void offer(const Key& A, const Keypoint& K, int j, float xj, float yj, float zj, double d2, int32_t& k, Add add) const
    {
        if (!(d2 > 0.0 && member(d2, r2))) return;
        if (support > 0.0 && !supported(A, support, nx[j], ny[j], nz[j])) return;   // wave-uniform: normals may be NULL otherwise
        Adds a;
        if (!member_adds<STRUCTURE>(A, r, d2, (double)xj - K.x, (double)yj - K.y, (double)zj - K.z, a)) return;
        ++k;
#pragma unroll
        for (int i = 0; i < ADDS; ++i)
            if (a.q[i] > 0) add(a.col[i], a.q[i]);
    }
    USIP_DEV void finish(const long long (&)[PER_LANE], int) const {}
    USIP_DEV double column(long long h, int32_t k) const { return usip_spin::column(h, k); }
};

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
    const int f = blockIdx.y;
    const Frame F(pc, count, perm, N, f);
    const bool angled = support > 0.0;
    const double *nx = angled ? normals + 3LL * f * N : nullptr, *ny = angled ? nx + N : nullptr, *nz = angled ? ny + N : nullptr;
    ImagePass<STRUCTURE> pass{r, r2, support, nx, ny, nz, axes + 3LL * f * M};
    usip_keypoint::histogram(F, keypoints, kp_count, M, r, bins, hist, spin, kp_members, pass);
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
