// usip_amd/csrc/fpfh.hip -- the FPFH baseline descriptor on the device: the hand-crafted descriptor the
// reference's scoring scripts name beside its learned one (eval_indoor/3dmatch/evaluate.m: descriptorName = 'my'; % 3dmatch,
// spin, fpfh) and do not contain.  csrc/fpfh_math.h has the semantics and the arithmetic, which the host twin
// (csrc/fpfh_cpu.cpp) shares.  pc f32 [B][3][N], count i32 [B] live points per frame, perm i32 [B][N] the frame SORTED ALONG X
// (the caller's permutation).  No launch synchronises; no atomics; no per-lane array with a run-time index.
//
//   fpfh_spfh_kernel     a pass of csrc/ascending_walk.h (its geometry, its walk and its exactness argument at the radius r):
//                        grid = (tiles of a frame, B), one lane per query; the tile's float64 normals are staged beside its
//                        points (three planes; whether a row has a normal rides in the float4 row's fourth component).  The 33
//                        counters of a lane live in LDS as hist[33][256] i32, bin-major with the lane as the fast index: a
//                        lane touches only its own column (no synchronisation), and a wave's updates of any bins fall on
//                        the banks lane % 32, distinct within each half-wave.  LDS: 2 * 256 * 16 (tiles) + 2 * 3 * 256 * 8
//                        (normals) + 33 * 256 * 4 (histograms) = 54 272 bytes.  Counts are integers: the walk's order cannot
//                        move them.  spfh i32 [B][N][33] and members i32 [B][N] at ORIGINAL indices, every row written whole
//                        by its lane.  A query without a normal walks nothing and gets zeros.
//   fpfh_gather_kernel   one wave per keypoint over csrc/keypoint_walk.h (its window, its walk and its exactness argument): a
//                        member's 33-int row and count are read and added to 33 float64 sums in registers (static indices);
//                        the lanes fold by the xor-butterfly 32 .. 1, lane 0 normalises and writes fpfh f64 [B][M][33] and
//                        kp_members i32 [B][M].
// Slots beyond count[b] / kp_count[b] get zeros.
#include "keypoint_walk.h"

using namespace usip_fpfh;
using usip_ascend::ascend;
using usip_ascend::Frame;
using usip_iss::bad_frames;
using usip_iss::bad_radius;
using usip_keypoint::Keypoint;
using usip_keypoint::Window;

namespace {

struct SpfhPass {
    static constexpr int ROWS = 2;
    struct Side { double n0, n1, n2; };                                // the row's normal
    double r2;
    const double *nx, *ny, *nz;
    int32_t *spfh, *mem;                                               // the frame's
    double (*tn)[3][TILE];
    int32_t (*hist)[TILE];
    bool mine = false;
    double m0 = 0.0, m1 = 0.0, m2 = 0.0;                               // the query's normal
    int32_t k = 0;
    USIP_DEV bool walks(bool live, int me)
    {
#pragma unroll
        for (int b = 0; b < WIDTH; ++b) hist[b][threadIdx.x] = 0;
        m0 = nx[me];
        m1 = ny[me];
        m2 = nz[me];
        return mine = live && has_normal(m0, m1, m2);
    }
    USIP_DEV float stage(int slot, int l, int j) const
    {
        const double n0 = nx[j], n1 = ny[j], n2 = nz[j];
        tn[slot][0][l] = n0;
        tn[slot][1][l] = n1;
        tn[slot][2][l] = n2;
        return has_normal(n0, n1, n2) ? 1.0f : 0.0f;
    }
    USIP_DEV Side side(int slot, int c) const { return {tn[slot][0][c], tn[slot][1][c], tn[slot][2][c]}; }
    USIP_DEV void offer(double xi, double yi, double zi, float4 o, Side s)
    {
        const double d2 = usip_prep::sqdist(xi, yi, zi, o.x, o.y, o.z);
        if (o.w != 0.0f && member(d2, r2)) {
            ++k;
            Bins h;
            if (pair_bins(xi, yi, zi, o.x, o.y, o.z, d2, m0, m1, m2, s.n0, s.n1, s.n2, h)) {
                ++hist[h.h1][threadIdx.x];
                ++hist[BINS + h.h2][threadIdx.x];
                ++hist[2 * BINS + h.h3][threadIdx.x];
            }
        }
    }
    USIP_DEV void dead(int q) const
    {
        int32_t* row = spfh + (long long)WIDTH * q;
#pragma unroll
        for (int b = 0; b < WIDTH; ++b) row[b] = 0;
        mem[q] = 0;
    }
    USIP_DEV void write(int me, double xi, double yi, double zi) const
    {
        int32_t* row = spfh + (long long)WIDTH * me;
#pragma unroll
        for (int b = 0; b < WIDTH; ++b) row[b] = hist[b][threadIdx.x];
        mem[me] = mine ? k - own(xi, yi, zi, r2) : 0;
    }
};

__global__ __launch_bounds__(TILE) void fpfh_spfh_kernel(const float* __restrict__ pc, const int32_t* __restrict__ count,
                                                         const int32_t* __restrict__ perm, const double* __restrict__ normals,
                                                         int N, double r, double r2, int32_t* __restrict__ spfh,
                                                         int32_t* __restrict__ members, int32_t* __restrict__ visited)
{
    __shared__ float4 tile[2][TILE];
    __shared__ double tn[2][3][TILE];
    __shared__ int32_t hist[WIDTH][TILE];
    const int f = blockIdx.y;
    const Frame F(pc, count, perm, N, f);
    const double* nx = normals + 3LL * f * N;
    SpfhPass pass{r2, nx, nx + N, nx + 2LL * N, spfh + (long long)WIDTH * f * N, members + (long long)f * N, tn, hist};
    ascend(F, N, r, tile, visited, pass);
}

// amdgpu_waves_per_eu(4): the 33 float64 sums are 66 registers and a member's row another 33 in flight; the allocator is told
// to stay within the 128 that four waves per SIMD allow (tests/test_fpfh_isa.py: no scratch, no spill)
__global__ __launch_bounds__(TILE) __attribute__((amdgpu_waves_per_eu(4))) void fpfh_gather_kernel(
    const float* __restrict__ pc, const int32_t* __restrict__ count, const int32_t* __restrict__ perm,
    const int32_t* __restrict__ spfh, const int32_t* __restrict__ members, const float* __restrict__ keypoints,
    const int32_t* __restrict__ kp_count, int N, int M, double r, double r2, double* __restrict__ fpfh,
    int32_t* __restrict__ kp_members)
{
    const Frame F(pc, count, perm, N, blockIdx.y);
    const Keypoint K(F, keypoints, kp_count, M);
    if (!K.there) return;                                              // wave-uniform
    const int32_t* rows = spfh + (long long)WIDTH * K.f * N;
    const int32_t* mem = members + (long long)K.f * N;
    double acc[WIDTH];
#pragma unroll
    for (int b = 0; b < WIDTH; ++b) acc[b] = 0.0;
    int32_t k = 0;
    usip_keypoint::walk(F, Window(F, K, r), K, [&](int j, float, float, float, double d2) {
        const int32_t mj = mem[j];
        if (gathers(d2, r2, mj)) {
            add_row(acc, rows + (long long)WIDTH * j, mj, d2);
            ++k;
        }
    });
#pragma unroll 1                                                       // (unrolled, six steps' exchanges in flight spill)
    for (int off = LANES / 2; off >= 1; off >>= 1) {
#pragma unroll
        for (int h = 0; h < WIDTH; h += BINS) {                        // (eleven exchanges in flight, not all 33)
#pragma unroll
            for (int b = h; b < h + BINS; ++b) acc[b] += __shfl_xor(acc[b], off, LANES);
            __builtin_amdgcn_sched_barrier(0);
        }
        k += __shfl_xor(k, off, LANES);
    }
    if (K.lane != 0) return;
    double* out = fpfh + WIDTH * K.slot(M);
    const auto put = [&](int h) {                                      // (a block leaves before the next is scaled)
#pragma unroll
        for (int b = h * BINS; b < h * BINS + BINS; ++b) out[b] = acc[b];
        __builtin_amdgcn_sched_barrier(0);
    };
    normalise<0>(acc);
    put(0);
    normalise<1>(acc);
    put(1);
    normalise<2>(acc);
    put(2);
    kp_members[K.slot(M)] = k;
}

}  // namespace

extern "C" int usip_fpfh_spfh_f32(const float* pc, const int32_t* count, const int32_t* perm, const double* normals, int B,
                                  int N, double radius, int32_t* spfh, int32_t* members, int32_t* tiles_visited, void* stream)
{
    if (bad_frames(B, N) || bad_radius(radius) || !pc || !perm || !normals || !spfh || !members) return USIP_EINVAL;
    USIP_LAUNCH(fpfh_spfh_kernel, dim3(usip_ceil_div(N, TILE), B), dim3(TILE), 0, (hipStream_t)stream, pc, count, perm, normals,
                N, radius, radius * radius, spfh, members, tiles_visited);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_fpfh_gather_f32(const float* pc, const int32_t* count, const int32_t* perm, const int32_t* spfh,
                                    const int32_t* members, const float* keypoints, const int32_t* kp_count, int B, int N,
                                    int M, double radius, double* fpfh, int32_t* kp_members, void* stream)
{
    if (bad_frames(B, N) || bad_keypoints(M) || bad_radius(radius) || !pc || !perm || !spfh || !members || !keypoints ||
        !fpfh || !kp_members)
        return USIP_EINVAL;
    USIP_LAUNCH(fpfh_gather_kernel, dim3(usip_ceil_div(M, TILE / LANES), B), dim3(TILE), 0, (hipStream_t)stream, pc, count,
                perm, spfh, members, keypoints, kp_count, N, M, radius, radius * radius, fpfh, kp_members);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
