// usip_amd/csrc/shot.hip -- the SHOT-352 baseline descriptor on the device: the hand-crafted descriptor the
// reference's outdoor scoring script is set to (eval_outdoor/kitti/evaluate_kitti.m: .../kitti/shot/iss_256, FEATURE_DIM = 352)
// and the reference does not contain.  csrc/shot_math.h has the semantics and the arithmetic, which the host twin
// (csrc/shot_cpu.cpp) shares.  pc f32 [B][3][N], count i32 [B] live points per frame, perm i32 [B][N] the frame SORTED ALONG X
// (the caller's permutation), keypoints f32 [B][3][M] at any positions.  No launch synchronises; no global atomics, no float
// atomics; no per-lane array with a run-time index.
//
// Both kernels run one wave per keypoint over csrc/keypoint_walk.h (its window, its walk and its exactness argument).
//
//   shot_lrf_kernel    seven float64 sums per lane (named fields), folded by the xor-butterfly 32 .. 1, after which EVERY lane
//                      holds the same seven numbers and runs the same Jacobi on them (no broadcast); a second walk over the
//                      same rows takes the four integer sign counts, folded likewise; lane 0 writes lrf f64 [B][M][9] and
//                      lrf_members i32 [B][M].  No LDS.
//   shot_hist_kernel   a pass of that header's histogram(): u64 hist[352] per wave in LDS (4 * 352 * 8 = 11 264 bytes per
//                      workgroup), the at most five columns of a member added; the pass takes the descriptor's sum of squares
//                      in the contract's order (partial l over the columns l + 64 k, then the fold) before hist i64 [B][M][352]
//                      and shot f64 [B][M][352] are written.
// Slots beyond kp_count[b] get zeros.
#include "keypoint_walk.h"
#include "shot_math.h"

using namespace usip_shot;
using usip_ascend::Frame;
using usip_iss::bad_frames;
using usip_iss::bad_radius;
using usip_keypoint::fold;
using usip_keypoint::Keypoint;
using usip_keypoint::Window;

namespace {

// amdgpu_waves_per_eu(4): the allocator is told to stay within the 128 registers that four waves per SIMD allow
// (tests/test_shot_isa.py: no scratch, no spill)
__global__ __launch_bounds__(TILE) __attribute__((amdgpu_waves_per_eu(4))) void shot_lrf_kernel(
    const float* __restrict__ pc, const int32_t* __restrict__ count, const int32_t* __restrict__ perm,
    const float* __restrict__ keypoints, const int32_t* __restrict__ kp_count, int N, int M, double r, double r2,
    double* __restrict__ lrf, int32_t* __restrict__ lrf_members)
{
    const Frame F(pc, count, perm, N, blockIdx.y);
    const Keypoint K(F, keypoints, kp_count, M);
    if (!K.there) return;                                              // wave-uniform
    const Window W(F, K, r);                                           // wave-uniform
    Sums S;
    int32_t k = 0;
    usip_keypoint::walk(F, W, K, [&](int, float xj, float yj, float zj, double d2) {
        if (member(d2, r2)) {
            S.add(r, d2, (double)xj - K.x, (double)yj - K.y, (double)zj - K.z);
            ++k;
        }
    });
    S.w = fold(S.w);                                                   // every lane: the same seven numbers
    S.s00 = fold(S.s00);
    S.s01 = fold(S.s01);
    S.s02 = fold(S.s02);
    S.s11 = fold(S.s11);
    S.s12 = fold(S.s12);
    S.s22 = fold(S.s22);
    k = fold(k);
    const Axes A = axes_from(S, k);
    Votes V;
    if (A.ok)
#pragma unroll 1                                                       // (unrolled, the walk's rows in flight beside the axes spill)
        for (int s = W.lo + K.lane; s < W.hi; s += LANES) {
            const int j = F.at(s);
            const float xj = F.x[j], yj = F.y[j], zj = F.z[j];
            if (member(usip_prep::sqdist(K.x, K.y, K.z, xj, yj, zj), r2))
                V.add(A, (double)xj - K.x, (double)yj - K.y, (double)zj - K.z);
        }
    V.xp = fold(V.xp);
    V.xn = fold(V.xn);
    V.zp = fold(V.zp);
    V.zn = fold(V.zn);
    if (K.lane != 0) return;
    double out[9];
    frame_from(A, V, out);
    double* row = lrf + 9 * K.slot(M);
#pragma unroll
    for (int c = 0; c < 9; ++c) row[c] = out[c];
    lrf_members[K.slot(M)] = k;
}

struct HistPass {
    static constexpr int WIDTH = usip_shot::WIDTH;
    struct Key {
        Lrf L;
        bool framed;
    };
    double r, r2;
    const double *nx, *ny, *nz, *lrf;                                  // the frame's
    double ss = 0.0, root = 0.0;
    USIP_DEV Key load(int q) const
    {
        const double* l = lrf + 9LL * q;
        const Lrf L{l[0], l[1], l[2], l[3], l[4], l[5], l[6], l[7], l[8]};
        return {L, L.exists()};
    }
    USIP_DEV bool walks(const Key&) const { return true; }             // (a member counts even without a frame)
    template <class Add>
    USIP_DEV void offer(const Key& key, const Keypoint& K, int j, float xj, float yj, float zj, double d2, int32_t& k, Add add) const
    {
        if (!(d2 > 0.0 && member(d2, r2))) return;
        const double n0 = nx[j], n1 = ny[j], n2 = nz[j];
        if (!describes(d2, r2, n0, n1, n2)) return;
        ++k;
        if (!key.framed) return;
        Adds a;
        member_adds(key.L, r, d2, (double)xj - K.x, (double)yj - K.y, (double)zj - K.z, n0, n1, n2, a);
#pragma unroll
        for (int i = 0; i < ADDS; ++i)
            if (a.col[i] >= 0) add(a.col[i], a.q[i]);
    }
    USIP_DEV void finish(const long long (&h)[PER_LANE], int lane)     // the sum of squares: partial l over the columns l + 64 k
    {
#pragma unroll
        for (int i = 0; i < PER_LANE; ++i)
            if (lane + LANES * i < WIDTH) ss += (double)h[i] * (double)h[i];
        ss = fold(ss);
        root = sqrt(ss);
    }
    USIP_DEV double column(long long h, int32_t) const { return ss > 0.0 ? (double)h / root : 0.0; }
};

__global__ __launch_bounds__(TILE) void shot_hist_kernel(const float* __restrict__ pc, const int32_t* __restrict__ count,
                                                         const int32_t* __restrict__ perm, const double* __restrict__ normals,
                                                         const float* __restrict__ keypoints,
                                                         const int32_t* __restrict__ kp_count, const double* __restrict__ lrf,
                                                         int N, int M, double r, double r2, long long* __restrict__ hist,
                                                         double* __restrict__ shot, int32_t* __restrict__ kp_members)
{
    __shared__ unsigned long long bins[TILE / LANES][WIDTH];
    const int f = blockIdx.y;
    const Frame F(pc, count, perm, N, f);
    const double* nx = normals + 3LL * f * N;
    HistPass pass{r, r2, nx, nx + N, nx + 2LL * N, lrf + 9LL * f * M};
    usip_keypoint::histogram(F, keypoints, kp_count, M, r, bins, hist, shot, kp_members, pass);
}

}  // namespace

extern "C" int usip_shot_lrf_f32(const float* pc, const int32_t* count, const int32_t* perm, const float* keypoints,
                                 const int32_t* kp_count, int B, int N, int M, double radius, double* lrf,
                                 int32_t* lrf_members, void* stream)
{
    if (bad_frames(B, N) || bad_keypoints(M) || bad_radius(radius) || !pc || !perm || !keypoints || !lrf || !lrf_members)
        return USIP_EINVAL;
    USIP_LAUNCH(shot_lrf_kernel, dim3(usip_ceil_div(M, TILE / LANES), B), dim3(TILE), 0, (hipStream_t)stream, pc, count, perm,
                keypoints, kp_count, N, M, radius, radius * radius, lrf, lrf_members);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_shot_hist_f32(const float* pc, const int32_t* count, const int32_t* perm, const double* normals,
                                  const float* keypoints, const int32_t* kp_count, const double* lrf, int B, int N, int M,
                                  double radius, int64_t* hist, double* shot, int32_t* kp_members, void* stream)
{
    if (bad_frames(B, N) || bad_keypoints(M) || bad_radius(radius) || !pc || !perm || !normals || !keypoints || !lrf || !hist ||
        !shot || !kp_members)
        return USIP_EINVAL;
    USIP_LAUNCH(shot_hist_kernel, dim3(usip_ceil_div(M, TILE / LANES), B), dim3(TILE), 0, (hipStream_t)stream, pc, count, perm,
                normals, keypoints, kp_count, lrf, N, M, radius, radius * radius, (long long*)hist, shot, kp_members);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
