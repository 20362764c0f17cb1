// usip_amd/csrc/iss.hip -- the ISS baseline detector on the device: the hand-crafted keypoints the
// reference compares its learned detector with (evaluation/save_keypoints.py:44-50, method = 'iss', through an external
// PCL binding).  csrc/iss_math.h has the semantics and the arithmetic, which the host twin (csrc/iss_cpu.cpp) shares.
// Batched over frames: pc f32 [B][3][N], count i32 [B] live points per frame (the first count[b] of N), grid = (tiles of
// a frame, B).  No launch synchronises; no atomics, no float reduction across lanes.
//
//   iss_saliency_kernel   csrc/ascending_walk.h's kernel at rs: the member count and the six scatter sums stay in registers.
//                         Then per lane: 3x3 Jacobi, the gates; saliency f64 and neighbours i32 at ORIGINAL indices.
//   iss_nms_kernel        the same walk at rn, written out over walk_tiles, with the tile's saliencies staged beside its
//                         points: the members and whether one of them has a larger saliency; keypoint u8 at original
//                         indices.  A workgroup none of whose queries is salient writes zeros and leaves.
// Slots beyond count[b] get saliency 0, neighbours 0, keypoint 0.
#include "ascending_walk.h"

using namespace usip_iss;
using usip_ascend::ascend;
using usip_ascend::Frame;
using usip_ascend::walk_tiles;

namespace {

struct SaliencyPass : usip_ascend::Plain {
    static constexpr int ROWS = 4;
    double r2, gamma_21, gamma_32;
    int min_neighbors;
    double* sal;
    int32_t* nb;
    Scatter g;
    USIP_DEV void offer(double xi, double yi, double zi, float4 o, Side) { g.offer(xi, yi, zi, o.x, o.y, o.z, r2); }
    USIP_DEV void dead(int q) const { sal[q] = 0.0; nb[q] = 0; }
    USIP_DEV void write(int me, double, double, double) const
    {
        sal[me] = saliency_from(g, min_neighbors, gamma_21, gamma_32);
        nb[me] = g.n;
    }
};

__global__ __launch_bounds__(TILE) void iss_saliency_kernel(const float* __restrict__ pc, const int32_t* __restrict__ count,
                                                            const int32_t* __restrict__ perm, int N, double rs, double r2,
                                                            double gamma_21, double gamma_32, int min_neighbors,
                                                            double* __restrict__ saliency, int32_t* __restrict__ neighbours,
                                                            int32_t* __restrict__ visited)
{
    __shared__ float4 tile[2][TILE];
    const int f = blockIdx.y;
    const Frame F(pc, count, perm, N, f);
    SaliencyPass pass{{}, r2, gamma_21, gamma_32, min_neighbors, saliency + (long long)f * N, neighbours + (long long)f * N};
    ascend(F, N, rs, tile, visited, pass);
}

// This kernel keeps the body in place.  As a pass of ascend() -- the vote in front of it, the query's index, saliency and
// coordinates loaded again behind the vote's barrier -- it took 541 instructions for 469 and 130.7 / 129.3 us for the 123.4 /
// 123.6 us of tools/iss_bench.py's suppression stage on one MI355X, with parent-against-parent runs within 0.7 %
// (profiles/f18_baseline_walk_ab.json): what the vote needs is what the walk needs, and it is loaded once here.
__global__ __launch_bounds__(TILE) void iss_nms_kernel(const float* __restrict__ pc, const int32_t* __restrict__ count,
                                                       const int32_t* __restrict__ perm, const double* __restrict__ saliency,
                                                       int N, double rn, double r2, int min_neighbors,
                                                       uint8_t* __restrict__ keypoint)
{
    __shared__ float4 tile[2][TILE];
    __shared__ double tsal[2][TILE];
    __shared__ int vote[TILE / 64];
    const int l = threadIdx.x, w = blockIdx.x, f = blockIdx.y;
    const Frame F(pc, count, perm, N, f);
    const int q = w * TILE + l;
    const double* sal = saliency + (long long)f * N;
    uint8_t* kp = keypoint + (long long)f * N;
    if (q >= F.n && q < N) kp[q] = 0;
    if (w * TILE >= F.n) return;
    const bool live = q < F.n;
    const int me = F.at(q);
    const double xi = (double)F.x[me], yi = (double)F.y[me], zi = (double)F.z[me], si = sal[me];
    const bool wave_salient = __ballot(live && si > 0.0) != 0;
    if ((l & 63) == 0) vote[l >> 6] = wave_salient;
    __syncthreads();
    if (!(vote[0] | vote[1] | vote[2] | vote[3])) {                    // workgroup-uniform: nobody here can be a keypoint
        if (live) kp[me] = 0;
        return;
    }
    Rivals g;
    walk_tiles(
        F, w, rn, live,
        [&](int slot, int t) {
            const int j = F.at(t * TILE + l);
            tile[slot][l] = make_float4(F.x[j], F.y[j], F.z[j], 0.0f);
            tsal[slot][l] = sal[j];
        },
        [&](int slot) { return (double)tile[slot][0].x; },
        [&](int slot, int rows) {
            int c = 0;
            for (; c + 4 <= rows; c += 4) {
                const float4 o0 = tile[slot][c], o1 = tile[slot][c + 1], o2 = tile[slot][c + 2], o3 = tile[slot][c + 3];
                const double s0 = tsal[slot][c], s1 = tsal[slot][c + 1], s2 = tsal[slot][c + 2], s3 = tsal[slot][c + 3];
                g.offer(xi, yi, zi, si, o0.x, o0.y, o0.z, s0, r2);
                g.offer(xi, yi, zi, si, o1.x, o1.y, o1.z, s1, r2);
                g.offer(xi, yi, zi, si, o2.x, o2.y, o2.z, s2, r2);
                g.offer(xi, yi, zi, si, o3.x, o3.y, o3.z, s3, r2);
            }
            for (; c < rows; ++c) {
                const float4 o = tile[slot][c];
                g.offer(xi, yi, zi, si, o.x, o.y, o.z, tsal[slot][c], r2);
            }
        });
    if (live) kp[me] = keypoint_from(g, si, min_neighbors) ? 1 : 0;
}

}  // namespace

extern "C" int usip_iss_saliency_f32(const float* pc, const int32_t* count, const int32_t* perm, int B, int N,
                                     double salient_radius, double gamma_21, double gamma_32, int min_neighbors,
                                     double* saliency, int32_t* neighbours, int32_t* tiles_visited, void* stream)
{
    if (bad_frames(B, N) || bad_radius(salient_radius) || min_neighbors < 1 || !pc || !perm || !saliency || !neighbours)
        return USIP_EINVAL;
    USIP_LAUNCH(iss_saliency_kernel, dim3(usip_ceil_div(N, TILE), B), dim3(TILE), 0, (hipStream_t)stream, pc, count, perm,
                N, salient_radius, salient_radius * salient_radius, gamma_21, gamma_32, min_neighbors, saliency, neighbours,
                tiles_visited);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_iss_nms_f32(const float* pc, const int32_t* count, const int32_t* perm, const double* saliency, int B,
                                int N, double non_max_radius, int min_neighbors, uint8_t* keypoint, void* stream)
{
    if (bad_frames(B, N) || bad_radius(non_max_radius) || min_neighbors < 1 || !pc || !perm || !saliency || !keypoint)
        return USIP_EINVAL;
    USIP_LAUNCH(iss_nms_kernel, dim3(usip_ceil_div(N, TILE), B), dim3(TILE), 0, (hipStream_t)stream, pc, count, perm,
                saliency, N, non_max_radius, non_max_radius * non_max_radius, min_neighbors, keypoint);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
