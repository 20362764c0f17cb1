// usip_amd/csrc/harris.hip -- the Harris3D baseline detector on the device: the second hand-crafted detector
// the reference compares its learned one with (evaluation/save_keypoints.py:52-55, 303-313, method = 'harris', through an
// external PCL binding).  csrc/harris_math.h has the semantics and the arithmetic, which the host twin
// (csrc/harris_cpu.cpp) shares.  The geometry, the walk and its exactness argument at the radius r are
// csrc/ascending_walk.h's: pc f32 [B][3][N], count i32 [B] live points per frame, grid = (tiles of a frame, B), one lane per
// query of a frame SORTED ALONG X (the caller's permutation); the result is the all-pairs answer, sums in the all-pairs order.
// No launch synchronises; no atomics, no float reduction across lanes, no per-lane array with a run-time index.
//
//   harris_normals_kernel    the member count, the three sums of d = p_j - p_i and the six of d d' stay in registers; then
//                            per lane the covariance about the mean, normal_from's Jacobi and flip; normals f64 [B][3][N]
//                            and neighbours i32 [B][N] at ORIGINAL indices.  Fewer than min_neighbors members: zeros, and
//                            neighbours still holds the count.
//   harris_response_kernel   the same walk with the tile's normals staged beside its points (three float64 planes; whether
//                            a row has a normal rides in the float4 row's fourth component); k and the six sums of n n' stay
//                            in registers; response f64 [B][N] and members i32 [B][N] at original indices.  A query
//                            without a normal walks nothing and gets response 0, members 0.
// Slots beyond count[b] get zeros.
#include "ascending_walk.h"
#include "harris_math.h"

using namespace usip_harris;
using usip_ascend::ascend;
using usip_ascend::Frame;
using usip_iss::bad_frames;
using usip_iss::bad_radius;

namespace {

struct NormalsPass : usip_ascend::Plain {
    static constexpr int ROWS = 4;
    double r2;
    int min_neighbors;
    double *nx, *ny, *nz;
    int32_t* nb;
    Moments g;
    USIP_DEV void offer(double xi, double yi, double zi, float4 o, Side) { g.offer(xi, yi, zi, o.x, o.y, o.z, r2); }
    USIP_DEV void dead(int q) const { nx[q] = 0.0; ny[q] = 0.0; nz[q] = 0.0; nb[q] = 0; }
    USIP_DEV void write(int me, double xi, double yi, double zi) const
    {
        const Normal3 n = normal_of(g, min_neighbors, xi, yi, zi);
        nx[me] = n.x;
        ny[me] = n.y;
        nz[me] = n.z;
        nb[me] = g.m;
    }
};

struct ResponsePass {
    static constexpr int ROWS = 2;
    struct Side { double n0, n1, n2; };                                // the row's normal
    double r2;
    int method;
    const double *nx, *ny, *nz;
    double* res;
    int32_t* mem;
    double (*tn)[3][TILE];
    bool mine = false;
    Tensor g;
    USIP_DEV bool walks(bool live, int me) { return mine = live && has_normal(nx[me], ny[me], nz[me]); }
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
        g.offer(xi, yi, zi, o.x, o.y, o.z, o.w != 0.0f, s.n0, s.n1, s.n2, r2);
    }
    USIP_DEV void dead(int q) const { res[q] = 0.0; mem[q] = 0; }
    USIP_DEV void write(int me, double, double, double) const
    {
        res[me] = mine ? response_from(g, method) : 0.0;
        mem[me] = mine ? g.k : 0;
    }
};

__global__ __launch_bounds__(TILE) void harris_normals_kernel(const float* __restrict__ pc, const int32_t* __restrict__ count,
                                                              const int32_t* __restrict__ perm, int N, double r, double r2,
                                                              int min_neighbors, double* __restrict__ normals,
                                                              int32_t* __restrict__ neighbours)
{
    __shared__ float4 tile[2][TILE];
    const int f = blockIdx.y;
    const Frame F(pc, count, perm, N, f);
    double* nx = normals + 3LL * f * N;
    NormalsPass pass{{}, r2, min_neighbors, nx, nx + N, nx + 2LL * N, neighbours + (long long)f * N};
    ascend(F, N, r, tile, nullptr, pass);
}

__global__ __launch_bounds__(TILE) void harris_response_kernel(const float* __restrict__ pc, const int32_t* __restrict__ count,
                                                               const int32_t* __restrict__ perm,
                                                               const double* __restrict__ normals, int N, double r, double r2,
                                                               int method, double* __restrict__ response,
                                                               int32_t* __restrict__ members, int32_t* __restrict__ visited)
{
    __shared__ float4 tile[2][TILE];
    __shared__ double tn[2][3][TILE];
    const int f = blockIdx.y;
    const Frame F(pc, count, perm, N, f);
    const double* nx = normals + 3LL * f * N;
    ResponsePass pass{r2, method, nx, nx + N, nx + 2LL * N, response + (long long)f * N, members + (long long)f * N, tn};
    ascend(F, N, r, tile, visited, pass);
}

}  // namespace

extern "C" int usip_harris_normals_f32(const float* pc, const int32_t* count, const int32_t* perm, int B, int N, double radius,
                                       int min_neighbors, double* normals, int32_t* neighbours, void* stream)
{
    if (bad_frames(B, N) || bad_radius(radius) || min_neighbors < 1 || !pc || !perm || !normals || !neighbours)
        return USIP_EINVAL;
    USIP_LAUNCH(harris_normals_kernel, dim3(usip_ceil_div(N, TILE), B), dim3(TILE), 0, (hipStream_t)stream, pc, count, perm, N,
                radius, radius * radius, min_neighbors, normals, neighbours);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_harris_response_f32(const float* pc, const int32_t* count, const int32_t* perm, const double* normals,
                                        int B, int N, double radius, int method, double* response, int32_t* members,
                                        int32_t* tiles_visited, void* stream)
{
    if (bad_frames(B, N) || bad_radius(radius) || !known_method(method) || !pc || !perm || !normals || !response || !members)
        return USIP_EINVAL;
    USIP_LAUNCH(harris_response_kernel, dim3(usip_ceil_div(N, TILE), B), dim3(TILE), 0, (hipStream_t)stream, pc, count, perm,
                normals, N, radius, radius * radius, method, response, members, tiles_visited);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
