// usip_amd/csrc/shot.hip -- the SHOT-352 baseline descriptor on the device: the hand-crafted descriptor the
// reference's outdoor scoring script is set to (eval_outdoor/kitti/evaluate_kitti.m: .../kitti/shot/iss_256, FEATURE_DIM = 352)
// and the reference does not contain.  csrc/shot_math.h has the semantics and the arithmetic, which the host twin
// (csrc/shot_cpu.cpp) shares.  pc f32 [B][3][N], count i32 [B] live points per frame, perm i32 [B][N] the frame SORTED ALONG X
// (the caller's permutation), keypoints f32 [B][3][M] at any positions.  No launch synchronises; no global atomics, no float
// atomics; no per-lane array with a run-time index.
//
// Both kernels are siblings of fpfh_gather_kernel (csrc/fpfh.hip): grid = (ceil(M / 4), B), 256 lanes, one wave per keypoint.
// The wave finds [lo, hi), the sorted positions with |x - q_x| < r, by two binary searches (wave-uniform); that kernel's
// exactness argument applies unchanged: a row outside [lo, hi) has d2 >= r2, so the result is the all-pairs answer.  Lane l
// tests the rows lo + l + 64 k, ascending.
//
//   shot_lrf_kernel    seven float64 sums per lane (named fields), folded by the xor-butterfly 32 .. 1, after which EVERY lane
//                      holds the same seven numbers and runs the same Jacobi on them (no broadcast); a second walk over the
//                      same rows takes the four integer sign counts, folded likewise; lane 0 writes lrf f64 [B][M][9] and
//                      lrf_members i32 [B][M].  No LDS.
//   shot_hist_kernel   each wave owns u64 hist[352] in LDS (4 * 352 * 8 = 11 264 bytes per workgroup), zeroed first; a lane
//                      adds the at most five columns of each of its members with LDS 64-bit integer atomic adds (integer sums:
//                      the order is free); then lane l reads the columns l + 64 k, takes the descriptor's sum of squares in
//                      the contract's order and writes them to hist i64 [B][M][352] and shot f64 [B][M][352] (a wave's 64
//                      lanes write 64 consecutive columns at a time); lane 0 writes kp_members i32 [B][M].  The waves of a
//                      workgroup are independent; the two workgroup barriers around the adds are more than the wave-level
//                      ordering this needs and cost nothing measurable, and every wave reaches them (an idle wave of the last
//                      workgroup walks nothing).
// Slots beyond kp_count[b] get zeros.
#include "ascending_walk.h"
#include "shot_math.h"

using namespace usip_shot;
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

USIP_DEV double fold(double v)
{
#pragma unroll
    for (int off = LANES / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, LANES);
    return v;
}

USIP_DEV int32_t fold(int32_t v)
{
#pragma unroll
    for (int off = LANES / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, LANES);
    return v;
}

// amdgpu_waves_per_eu(4): the allocator is told to stay within the 128 registers that four waves per SIMD allow
// (tests/test_shot_isa.py: no scratch, no spill)
__global__ __launch_bounds__(TILE) __attribute__((amdgpu_waves_per_eu(4))) void shot_lrf_kernel(
    const float* __restrict__ pc, const int32_t* __restrict__ count, const int32_t* __restrict__ perm,
    const float* __restrict__ keypoints, const int32_t* __restrict__ kp_count, int N, int M, double r, double r2,
    double* __restrict__ lrf, int32_t* __restrict__ lrf_members)
{
    const int f = blockIdx.y, lane = threadIdx.x & (LANES - 1);
    const int q = blockIdx.x * (TILE / LANES) + (threadIdx.x >> 6);    // the wave's keypoint
    if (q >= M) return;                                                // wave-uniform
    const Frame F(pc, count, perm, N, f);
    const bool live = q < live_points(kp_count, f, M) && F.n > 0;      // wave-uniform (an empty frame has no row to read)
    const float* kp = keypoints + 3LL * f * M;
    const double qx = (double)kp[q], qy = (double)kp[M + q], qz = (double)kp[2LL * M + q];
    int lo = 0, hi = 0;
    if (live) {
        const Window W(F, qx, r);
        lo = W.lo;
        hi = W.hi;
    }
    Sums S;
    int32_t k = 0;
    for (int s = lo + lane; s < hi; s += LANES) {
        const int j = F.at(s);
        const float xj = F.x[j], yj = F.y[j], zj = F.z[j];
        const double d2 = usip_prep::sqdist(qx, qy, qz, xj, yj, zj);
        if (member(d2, r2)) {
            S.add(r, d2, (double)xj - qx, (double)yj - qy, (double)zj - qz);
            ++k;
        }
    }
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
        for (int s = lo + lane; s < hi; s += LANES) {
            const int j = F.at(s);
            const float xj = F.x[j], yj = F.y[j], zj = F.z[j];
            if (member(usip_prep::sqdist(qx, qy, qz, xj, yj, zj), r2)) V.add(A, (double)xj - qx, (double)yj - qy, (double)zj - qz);
        }
    V.xp = fold(V.xp);
    V.xn = fold(V.xn);
    V.zp = fold(V.zp);
    V.zn = fold(V.zn);
    if (lane != 0) return;
    double out[9];
    frame_from(A, V, out);
    double* row = lrf + 9 * ((long long)f * M + q);
#pragma unroll
    for (int c = 0; c < 9; ++c) row[c] = out[c];
    lrf_members[(long long)f * M + q] = k;
}

__global__ __launch_bounds__(TILE) void shot_hist_kernel(const float* __restrict__ pc, const int32_t* __restrict__ count,
                                                         const int32_t* __restrict__ perm, const double* __restrict__ normals,
                                                         const float* __restrict__ keypoints,
                                                         const int32_t* __restrict__ kp_count, const double* __restrict__ lrf,
                                                         int N, int M, double r, double r2, long long* __restrict__ hist,
                                                         double* __restrict__ shot, int32_t* __restrict__ kp_members)
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
        const double* l = lrf + 9 * ((long long)f * M + q);
        const Lrf L{l[0], l[1], l[2], l[3], l[4], l[5], l[6], l[7], l[8]};
        const bool framed = L.exists();
        const double *nx = normals + 3LL * f * N, *ny = nx + N, *nz = ny + N;
        const Window W(F, qx, r);
        for (int s = W.lo + lane; s < W.hi; s += LANES) {
            const int j = F.at(s);
            const float xj = F.x[j], yj = F.y[j], zj = F.z[j];
            const double d2 = usip_prep::sqdist(qx, qy, qz, xj, yj, zj);
            if (!(d2 > 0.0 && member(d2, r2))) continue;
            const double n0 = nx[j], n1 = ny[j], n2 = nz[j];
            if (!describes(d2, r2, n0, n1, n2)) continue;
            ++k;
            if (!framed) continue;
            Adds a;
            member_adds(L, r, d2, (double)xj - qx, (double)yj - qy, (double)zj - qz, n0, n1, n2, a);
#pragma unroll
            for (int i = 0; i < ADDS; ++i)
                if (a.col[i] >= 0) atomicAdd(&mine[a.col[i]], (unsigned long long)a.q[i]);
        }
    }
    __syncthreads();
    if (!there) return;
    k = fold(k);
    double h[PER_LANE], ss = 0.0;
#pragma unroll
    for (int i = 0; i < PER_LANE; ++i) {
        const int c = lane + LANES * i;
        h[i] = c < WIDTH ? (double)(long long)mine[c] : 0.0;
        if (c < WIDTH) ss += h[i] * h[i];
    }
    ss = fold(ss);
    const double root = sqrt(ss);
    long long* hrow = hist + (long long)WIDTH * ((long long)f * M + q);
    double* srow = shot + (long long)WIDTH * ((long long)f * M + q);
#pragma unroll
    for (int i = 0; i < PER_LANE; ++i) {
        const int c = lane + LANES * i;
        if (c < WIDTH) {
            hrow[c] = (long long)mine[c];
            srow[c] = ss > 0.0 ? h[i] / root : 0.0;
        }
    }
    if (lane == 0) kp_members[(long long)f * M + q] = k;
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
