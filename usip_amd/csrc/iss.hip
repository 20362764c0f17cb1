// usip_amd/csrc/iss.hip -- the ISS baseline detector on the device: the hand-crafted keypoints the
// reference compares its learned detector with (evaluation/save_keypoints.py:44-50, method = 'iss', through an external
// PCL binding).  csrc/iss_math.h has the semantics and the arithmetic, which the host twin (csrc/iss_cpu.cpp) shares.
// Batched over frames: pc f32 [B][3][N], count i32 [B] live points per frame (the first count[b] of N), grid = (tiles of
// a frame, B).  No launch synchronises; no atomics, no float reduction across lanes.
//
//   iss_saliency_kernel   a workgroup owns TILE = 256 consecutive queries of a frame SORTED ALONG X (the caller's
//                         permutation), one lane per query; the member count and the six scatter sums stay in registers.
//                         Database tiles of 256 points are staged in LDS as 16-byte rows and read by every lane at the same
//                         address (broadcast reads).  The walk goes over the tiles in ASCENDING order -- the order of the
//                         sums is part of the contract -- from the first tile whose largest x is within rs of the
//                         workgroup's smallest query x to the last tile whose smallest x is within rs of its largest.
//                         A tile left out on the low side has gap = fl(xlo - xmax) >= rs, so for every query x_i >= xlo
//                         and every point x_j <= xmax of it dx = fl(x_i - x_j) >= gap >= rs (float64 rounding is monotone),
//                         hence d2 = fl(fl(dx dx + dy dy) + dz dz) >= fl(dx dx) >= fl(rs rs) = r2: no member.  The high
//                         side likewise.  The result is the all-pairs answer, sums in the all-pairs order.
//                         Then per lane: 3x3 Jacobi, the gates; saliency f64 and neighbours i32 at ORIGINAL indices.
//   iss_nms_kernel        the same walk at rn with the tile's saliencies staged beside its points: the members and whether
//                         one of them has a larger saliency; keypoint u8 at original indices.  A workgroup none of whose
//                         queries is salient writes zeros and leaves.
// Slots beyond count[b] get saliency 0, neighbours 0, keypoint 0.  An entry of perm outside [0, count) reads point 0: a
// wrong permutation gives wrong values, never a wild read.
#include "iss_walk.h"                                                  // Frame and walk_tiles, shared with csrc/harris.hip

using namespace usip_iss;

namespace {

__global__ __launch_bounds__(TILE) void iss_saliency_kernel(const float* __restrict__ pc, const int32_t* __restrict__ count,
                                                            const int32_t* __restrict__ perm, int N, double rs, double r2,
                                                            double gamma_21, double gamma_32, int min_neighbors,
                                                            double* __restrict__ saliency, int32_t* __restrict__ neighbours,
                                                            int32_t* __restrict__ visited)
{
    __shared__ float4 tile[2][TILE];
    const int l = threadIdx.x, w = blockIdx.x, f = blockIdx.y;
    const Frame F(pc, count, perm, N, f);
    const int q = w * TILE + l;                                        // position in the sorted order
    double* sal = saliency + (long long)f * N;
    int32_t* nb = neighbours + (long long)f * N;
    if (q >= F.n && q < N) {                                           // a dead slot: q itself (the live ones are 0 .. n-1)
        sal[q] = 0.0;
        nb[q] = 0;
    }
    if (w * TILE >= F.n) {                                             // workgroup-uniform: no query here
        if (visited && l == 0) visited[(long long)f * gridDim.x + w] = 0;
        return;
    }
    const bool live = q < F.n;
    const int me = F.at(q);
    const double xi = (double)F.x[me], yi = (double)F.y[me], zi = (double)F.z[me];
    Scatter g;
    const int seen = walk_tiles(
        F, w, rs, live,
        [&](int slot, int t) {
            const int j = F.at(t * TILE + l);
            tile[slot][l] = make_float4(F.x[j], F.y[j], F.z[j], 0.0f);
        },
        [&](int slot) { return (double)tile[slot][0].x; },
        [&](int slot, int rows) {
            int c = 0;
            for (; c + 4 <= rows; c += 4) {                            // four rows in flight: the LDS latency overlaps
                const float4 o0 = tile[slot][c], o1 = tile[slot][c + 1], o2 = tile[slot][c + 2], o3 = tile[slot][c + 3];
                g.offer(xi, yi, zi, o0.x, o0.y, o0.z, r2);
                g.offer(xi, yi, zi, o1.x, o1.y, o1.z, r2);
                g.offer(xi, yi, zi, o2.x, o2.y, o2.z, r2);
                g.offer(xi, yi, zi, o3.x, o3.y, o3.z, r2);
            }
            for (; c < rows; ++c) {
                const float4 o = tile[slot][c];
                g.offer(xi, yi, zi, o.x, o.y, o.z, r2);
            }
        });
    if (live) {
        sal[me] = saliency_from(g, min_neighbors, gamma_21, gamma_32);
        nb[me] = g.n;
    }
    if (visited && l == 0) visited[(long long)f * gridDim.x + w] = seen;
}

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

bool bad_shape(int B, int N, double r, int min_neighbors)
{
    return B < 1 || B > 65535 || N < 1 || N > NMAX || min_neighbors < 1 || !(r > 0.0) || !(r < (double)INFINITY);
}

}  // namespace

extern "C" int usip_iss_saliency_f32(const float* pc, const int32_t* count, const int32_t* perm, int B, int N,
                                     double salient_radius, double gamma_21, double gamma_32, int min_neighbors,
                                     double* saliency, int32_t* neighbours, int32_t* tiles_visited, void* stream)
{
    if (bad_shape(B, N, salient_radius, min_neighbors) || !pc || !perm || !saliency || !neighbours) return USIP_EINVAL;
    USIP_LAUNCH(iss_saliency_kernel, dim3(usip_ceil_div(N, TILE), B), dim3(TILE), 0, (hipStream_t)stream, pc, count, perm,
                N, salient_radius, salient_radius * salient_radius, gamma_21, gamma_32, min_neighbors, saliency, neighbours,
                tiles_visited);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_iss_nms_f32(const float* pc, const int32_t* count, const int32_t* perm, const double* saliency, int B,
                                int N, double non_max_radius, int min_neighbors, uint8_t* keypoint, void* stream)
{
    if (bad_shape(B, N, non_max_radius, min_neighbors) || !pc || !perm || !saliency || !keypoint) return USIP_EINVAL;
    USIP_LAUNCH(iss_nms_kernel, dim3(usip_ceil_div(N, TILE), B), dim3(TILE), 0, (hipStream_t)stream, pc, count, perm,
                saliency, N, non_max_radius, non_max_radius * non_max_radius, min_neighbors, keypoint);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
