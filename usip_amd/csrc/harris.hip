// usip_amd/csrc/harris.hip -- the Harris3D baseline detector on the device: the second hand-crafted detector
// the reference compares its learned one with (evaluation/save_keypoints.py:52-55, 303-313, method = 'harris', through an
// external PCL binding).  csrc/harris_math.h has the semantics and the arithmetic, which the host twin
// (csrc/harris_cpu.cpp) shares.  The geometry is csrc/iss.hip's: pc f32 [B][3][N], count i32 [B] live points per frame,
// grid = (tiles of a frame, B), a workgroup owns TILE = 256 consecutive queries of a frame SORTED ALONG X (the caller's
// permutation), one lane per query; database tiles of 256 rows are double-buffered in LDS and read by every lane at the same
// address (broadcast reads); the tiles are walked in ASCENDING order by iss_walk.h's walk_tiles, whose exactness argument
// (csrc/iss.hip) holds at the radius r: the result is the all-pairs answer, sums in the all-pairs order.  No launch
// synchronises; no atomics, no float reduction across lanes, no per-lane array with a run-time index.
//
//   harris_normals_kernel    the member count, the three sums of d = p_j - p_i and the six of d d' stay in registers; then
//                            per lane the covariance about the mean, normal_from's Jacobi and flip; normals f64 [B][3][N]
//                            and neighbours i32 [B][N] at ORIGINAL indices.  Fewer than min_neighbors members: zeros, and
//                            neighbours still holds the count.
//   harris_response_kernel   the same walk with the tile's normals staged beside its points (three float64 planes; whether
//                            a row has a normal rides in the float4 row's fourth component); k and the six sums of n n' stay
//                            in registers; response f64 [B][N] and members i32 [B][N] at original indices.  A query
//                            without a normal walks nothing and gets response 0, members 0.
// Slots beyond count[b] get zeros.  An entry of perm outside [0, count) reads point 0: a wrong permutation gives wrong
// values, never a wild read.
#include "iss_walk.h"
#include "harris_math.h"

using namespace usip_harris;
using usip_iss::Frame;
using usip_iss::walk_tiles;

namespace {

__global__ __launch_bounds__(TILE) void harris_normals_kernel(const float* __restrict__ pc, const int32_t* __restrict__ count,
                                                              const int32_t* __restrict__ perm, int N, double r, double r2,
                                                              int min_neighbors, double* __restrict__ normals,
                                                              int32_t* __restrict__ neighbours)
{
    __shared__ float4 tile[2][TILE];
    const int l = threadIdx.x, w = blockIdx.x, f = blockIdx.y;
    const Frame F(pc, count, perm, N, f);
    const int q = w * TILE + l;                                        // position in the sorted order
    double* nx = normals + 3LL * f * N;
    double* ny = nx + N;
    double* nz = ny + N;
    int32_t* nb = neighbours + (long long)f * N;
    if (q >= F.n && q < N) {                                           // a dead slot: q itself (the live ones are 0 .. n-1)
        nx[q] = 0.0;
        ny[q] = 0.0;
        nz[q] = 0.0;
        nb[q] = 0;
    }
    if (w * TILE >= F.n) return;                                       // workgroup-uniform: no query here
    const bool live = q < F.n;
    const int me = F.at(q);
    const double xi = (double)F.x[me], yi = (double)F.y[me], zi = (double)F.z[me];
    Moments g;
    walk_tiles(
        F, w, r, live,
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
        const Normal3 n = normal_of(g, min_neighbors, xi, yi, zi);
        nx[me] = n.x;
        ny[me] = n.y;
        nz[me] = n.z;
        nb[me] = g.m;
    }
}

__global__ __launch_bounds__(TILE) void harris_response_kernel(const float* __restrict__ pc, const int32_t* __restrict__ count,
                                                               const int32_t* __restrict__ perm,
                                                               const double* __restrict__ normals, int N, double r, double r2,
                                                               int method, double* __restrict__ response,
                                                               int32_t* __restrict__ members, int32_t* __restrict__ visited)
{
    __shared__ float4 tile[2][TILE];
    __shared__ double tn[2][3][TILE];
    const int l = threadIdx.x, w = blockIdx.x, f = blockIdx.y;
    const Frame F(pc, count, perm, N, f);
    const int q = w * TILE + l;
    const double* nx = normals + 3LL * f * N;
    const double* ny = nx + N;
    const double* nz = ny + N;
    double* res = response + (long long)f * N;
    int32_t* mem = members + (long long)f * N;
    if (q >= F.n && q < N) {
        res[q] = 0.0;
        mem[q] = 0;
    }
    if (w * TILE >= F.n) {
        if (visited && l == 0) visited[(long long)f * gridDim.x + w] = 0;
        return;
    }
    const bool live = q < F.n;
    const int me = F.at(q);
    const double xi = (double)F.x[me], yi = (double)F.y[me], zi = (double)F.z[me];
    const bool mine = live && has_normal(nx[me], ny[me], nz[me]);
    Tensor g;
    const int seen = walk_tiles(
        F, w, r, mine,
        [&](int slot, int t) {
            const int j = F.at(t * TILE + l);
            const double n0 = nx[j], n1 = ny[j], n2 = nz[j];
            tile[slot][l] = make_float4(F.x[j], F.y[j], F.z[j], has_normal(n0, n1, n2) ? 1.0f : 0.0f);
            tn[slot][0][l] = n0;
            tn[slot][1][l] = n1;
            tn[slot][2][l] = n2;
        },
        [&](int slot) { return (double)tile[slot][0].x; },
        [&](int slot, int rows) {
            int c = 0;
            for (; c + 2 <= rows; c += 2) {                            // two rows in flight: the LDS latency overlaps
                const float4 o0 = tile[slot][c], o1 = tile[slot][c + 1];
                const double a0 = tn[slot][0][c], a1 = tn[slot][1][c], a2 = tn[slot][2][c];
                const double b0 = tn[slot][0][c + 1], b1 = tn[slot][1][c + 1], b2 = tn[slot][2][c + 1];
                g.offer(xi, yi, zi, o0.x, o0.y, o0.z, o0.w != 0.0f, a0, a1, a2, r2);
                g.offer(xi, yi, zi, o1.x, o1.y, o1.z, o1.w != 0.0f, b0, b1, b2, r2);
            }
            for (; c < rows; ++c) {
                const float4 o = tile[slot][c];
                g.offer(xi, yi, zi, o.x, o.y, o.z, o.w != 0.0f, tn[slot][0][c], tn[slot][1][c], tn[slot][2][c], r2);
            }
        });
    if (live) {
        res[me] = mine ? response_from(g, method) : 0.0;
        mem[me] = mine ? g.k : 0;
    }
    if (visited && l == 0) visited[(long long)f * gridDim.x + w] = seen;
}

bool bad_shape(int B, int N, double r)
{
    return B < 1 || B > 65535 || N < 1 || N > NMAX || !(r > 0.0) || !(r < (double)INFINITY);
}

}  // namespace

extern "C" int usip_harris_normals_f32(const float* pc, const int32_t* count, const int32_t* perm, int B, int N, double radius,
                                       int min_neighbors, double* normals, int32_t* neighbours, void* stream)
{
    if (bad_shape(B, N, radius) || min_neighbors < 1 || !pc || !perm || !normals || !neighbours) return USIP_EINVAL;
    USIP_LAUNCH(harris_normals_kernel, dim3(usip_ceil_div(N, TILE), B), dim3(TILE), 0, (hipStream_t)stream, pc, count, perm, N,
                radius, radius * radius, min_neighbors, normals, neighbours);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_harris_response_f32(const float* pc, const int32_t* count, const int32_t* perm, const double* normals,
                                        int B, int N, double radius, int method, double* response, int32_t* members,
                                        int32_t* tiles_visited, void* stream)
{
    if (bad_shape(B, N, radius) || !known_method(method) || !pc || !perm || !normals || !response || !members)
        return USIP_EINVAL;
    USIP_LAUNCH(harris_response_kernel, dim3(usip_ceil_div(N, TILE), B), dim3(TILE), 0, (hipStream_t)stream, pc, count, perm,
                normals, N, radius, radius * radius, method, response, members, tiles_visited);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
