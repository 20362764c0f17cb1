// usip_amd/csrc/prepare.hip -- raw LiDAR scans prepared on the device: K nearest neighbours of every
// point, surface normal and curvature, voxel-grid average.  Replaces the reference's MATLAB preparation
// (evaluation/matlab/kitti_data_prepare/kitti_test_prepare.m:95-108: findPointNormals + pcdownsample 'gridAverage');
// csrc/prepare_math.h has the semantics and the arithmetic, which the host twin (csrc/prepare_cpu.cpp) shares.
// No launch synchronises.
//
//   scan_knn_kernel<K>         a workgroup owns TILE = 256 consecutive queries of the scan SORTED ALONG X (the caller's
//                              permutation), one lane per query, its K-list (float64 d2, int32 index) in registers.  Database
//                              tiles of 256 points are staged in LDS as 16-byte rows and walked by every lane at the same
//                              address (broadcast reads).  The walk starts at the workgroup's own tile and goes outward in
//                              both directions; a direction ends once the squared x-gap between its next tile and the
//                              workgroup's query range exceeds the largest K-th distance any lane still holds (a
//                              workgroup-wide max through LDS).  Every point of a skipped tile has d2 >= fl(gap * gap) > that
//                              K-th distance for every lane (float64 rounding is monotone), so it could not have entered
//                              any list: the result is the all-pairs answer, ties on ORIGINAL indices included.
//   scan_normals_kernel        one lane per point: gathers its K neighbours, covariance, 3x3 Jacobi, flip -- in registers.
//   scan_voxel_keys_kernel     one lane per point: the int64 key of its cell.
//   scan_voxel_average_kernel  one lane per occupied cell: its members in ascending original index, float64 sums in that
//                              order (no atomics: bit-reproducible and the host twin's order).
#include "common.h"
#include "bank.h"
#include "prepare_math.h"
#include "tile_walk.h"

using namespace usip_prep;
using usip_bank::safe_index;
using usip_walk::block_minmax;
using usip_walk::Tiles;

static_assert(usip_prep::TILE == usip_walk::WALK_TILE, "scan_knn_kernel walks tile_walk.h's tiles");

namespace {

template <int K>
__global__ __launch_bounds__(TILE) void scan_knn_kernel(const float4* __restrict__ pts, const int32_t* __restrict__ perm,
                                                        int n, int32_t* __restrict__ idx, int32_t* __restrict__ visited)
{
    __shared__ float4 tile[2][TILE];
    __shared__ int32_t orig[2][TILE];
    __shared__ double slots[4];
    const int l = threadIdx.x, b = blockIdx.x;
    const int q = b * TILE + l;                                        // position in the sorted order
    const bool live = q < n;
    const int me = safe_index(perm[live ? q : n - 1], n);
    const float4 p = pts[me];
    const double xi = (double)p.x, yi = (double)p.y, zi = (double)p.z;
    const auto x_at = [&](int s) { return (double)pts[safe_index(perm[s], n)].x; };
    const Tiles<decltype(x_at)> tiles(n, x_at);
    const double xlo = tiles.near_x(1, b), xhi = tiles.near_x(0, b);   // the x range of this workgroup's queries

    KList<K> list;
    list.clear();

    auto stage = [&](int slot, int t) {                                // tile t of the sorted order -> LDS
        const int s = t * TILE + l;
        const int j = safe_index(perm[s < n ? s : n - 1], n);
        tile[slot][l] = pts[j];
        orig[slot][l] = j;
    };
    auto offer = [&](double d, int slot, int c) {
        if (d <= list.worst()) {                                       // rare after the first tiles
            const int32_t j = orig[slot][c];
            if (j != me && list.admits(d, j)) list.insert(d, j);
        }
    };
    auto walk = [&](int slot, int t, int count) {
        int c = 0;
        for (; c + 4 <= count; c += 4) {                               // four rows in flight: the LDS latency overlaps
            const float4 o0 = tile[slot][c], o1 = tile[slot][c + 1], o2 = tile[slot][c + 2], o3 = tile[slot][c + 3];
            const double d0 = sqdist(xi, yi, zi, o0.x, o0.y, o0.z), d1 = sqdist(xi, yi, zi, o1.x, o1.y, o1.z);
            const double d2 = sqdist(xi, yi, zi, o2.x, o2.y, o2.z), d3 = sqdist(xi, yi, zi, o3.x, o3.y, o3.z);
            const double lo01 = d0 < d1 ? d0 : d1, lo23 = d2 < d3 ? d2 : d3;
            if ((lo01 < lo23 ? lo01 : lo23) <= list.worst()) {
                offer(d0, slot, c);
                offer(d1, slot, c + 1);
                offer(d2, slot, c + 2);
                offer(d3, slot, c + 3);
            }
        }
        for (; c < count; ++c) {
            const float4 o = tile[slot][c];
            offer(sqdist(xi, yi, zi, o.x, o.y, o.z), slot, c);
        }
    };

    stage(0, b);
    __syncthreads();
    if (live) walk(0, b, tiles.rows(b));
    int left = b - 1, right = b + 1, seen = 1;
    while (true) {
        double unused = 0.0, bound = live ? list.worst() : -1.0;
        __syncthreads();                                               // the previous round's reads are done
        block_minmax<false, true>(unused, bound, slots);               // (also: every lane is done with the tiles)
        if (left >= 0) {
            const double gap = xlo - tiles.near_x(0, left);
            if (gap * gap > bound) left = -1;
        }
        if (right < tiles.tiles) {
            const double gap = tiles.near_x(1, right) - xhi;
            if (gap * gap > bound) right = tiles.tiles;
        }
        if (left < 0 && right >= tiles.tiles) break;                   // workgroup-uniform
        if (left >= 0) stage(0, left);
        if (right < tiles.tiles) stage(1, right);
        __syncthreads();
        if (left >= 0) {
            if (live) walk(0, left, tiles.rows(left));
            --left;
            ++seen;
        }
        if (right < tiles.tiles) {
            if (live) walk(1, right, tiles.rows(right));
            ++right;
            ++seen;
        }
    }
    if (live) {
#pragma unroll
        for (int k = 0; k < K; ++k) idx[(long long)me * K + k] = list.j[k];
    }
    if (visited && l == 0) visited[b] = seen;
}

__global__ __launch_bounds__(256) void scan_normals_kernel(const float4* __restrict__ pts, const int32_t* __restrict__ idx,
                                                           int n, int K, double v0, double v1, double v2,
                                                           double* __restrict__ nrm64, float4* __restrict__ nrm32)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    const double p0 = (double)p.x, p1 = (double)p.y, p2 = (double)p.z;
    Cov S;
    for (int k = 0; k < K; ++k) {
        const float4 o = pts[safe_index(idx[(long long)i * K + k], n)];
        S.add(p0 - (double)o.x, p1 - (double)o.y, p2 - (double)o.z);
    }
    const Normal out = normal_from(S, K, p0, p1, p2, v0, v1, v2);
    if (nrm64) {
        nrm64[4LL * i] = out.x;
        nrm64[4LL * i + 1] = out.y;
        nrm64[4LL * i + 2] = out.z;
        nrm64[4LL * i + 3] = out.curvature;
    }
    if (nrm32) nrm32[i] = make_float4((float)out.x, (float)out.y, (float)out.z, (float)out.curvature);
}

__global__ __launch_bounds__(256) void scan_voxel_keys_kernel(const float4* __restrict__ pts, int n,
                                                              const float* __restrict__ lohi, double leaf,
                                                              int64_t* __restrict__ keys)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Grid g;
    g.init(lohi, leaf);
    const float4 p = pts[i];
    keys[i] = g.key(p.x, p.y, p.z);
}

__global__ __launch_bounds__(256) void scan_voxel_average_kernel(const float* __restrict__ xyzi,
                                                                 const double* __restrict__ nrm,
                                                                 const int32_t* __restrict__ perm,
                                                                 const int32_t* __restrict__ start, int n, int m,
                                                                 float* __restrict__ rows)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= m) return;
    int first = start[c], last = start[c + 1];
    first = first < 0 ? 0 : (first > n ? n : first);                   // a segment never leaves perm
    last = last < first ? first : (last > n ? n : last);
    float row[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (last > first) cell_average(xyzi, nrm, perm, n, first, last, row);
    float4* o = reinterpret_cast<float4*>(rows + 8LL * c);
    o[0] = make_float4(row[0], row[1], row[2], row[3]);
    o[1] = make_float4(row[4], row[5], row[6], row[7]);
}

template <int K>
int launch_knn(const float* xyzi, const int32_t* perm, int n, int32_t* idx, int32_t* visited, hipStream_t stream)
{
    USIP_LAUNCH(scan_knn_kernel<K>, dim3(usip_ceil_div(n, TILE)), dim3(TILE), 0, stream,
                reinterpret_cast<const float4*>(xyzi), perm, n, idx, visited);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

}  // namespace

extern "C" int usip_scan_knn_f32(const float* xyzi, const int32_t* perm, int n, int K, int32_t* idx, int32_t* tiles_visited,
                                 void* stream)
{
    if (K < 1 || K > KMAX || n < K + 1 || n > NMAX) return USIP_EINVAL;
    if (!xyzi || !perm || !idx) return USIP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    switch (K) {
#define USIP_KNN_CASE(k) case k: return launch_knn<k>(xyzi, perm, n, idx, tiles_visited, st)
        USIP_KNN_CASE(1); USIP_KNN_CASE(2); USIP_KNN_CASE(3); USIP_KNN_CASE(4);
        USIP_KNN_CASE(5); USIP_KNN_CASE(6); USIP_KNN_CASE(7); USIP_KNN_CASE(8);
        USIP_KNN_CASE(9); USIP_KNN_CASE(10); USIP_KNN_CASE(11); USIP_KNN_CASE(12);
        USIP_KNN_CASE(13); USIP_KNN_CASE(14); USIP_KNN_CASE(15); USIP_KNN_CASE(16);
#undef USIP_KNN_CASE
    }
    return USIP_EINVAL;
}

extern "C" int usip_scan_normals_f32(const float* xyzi, const int32_t* idx, int n, int K, const double* viewpoint,
                                     double* normals_f64, float* normals_f32, void* stream)
{
    if (K < 1 || K > KMAX || n < K + 1 || n > NMAX) return USIP_EINVAL;
    if (!xyzi || !idx || !viewpoint || (!normals_f64 && !normals_f32)) return USIP_EINVAL;
    USIP_LAUNCH(scan_normals_kernel, dim3(usip_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream,
                reinterpret_cast<const float4*>(xyzi), idx, n, K, viewpoint[0], viewpoint[1], viewpoint[2], normals_f64,
                reinterpret_cast<float4*>(normals_f32));
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_scan_voxel_keys_f32(const float* xyzi, int n, const float* lohi, double leaf, int64_t* keys, void* stream)
{
    if (n < 1 || n > NMAX || !(leaf > 0.0)) return USIP_EINVAL;
    if (!xyzi || !lohi || !keys) return USIP_EINVAL;
    USIP_LAUNCH(scan_voxel_keys_kernel, dim3(usip_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream,
                reinterpret_cast<const float4*>(xyzi), n, lohi, leaf, keys);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

extern "C" int usip_scan_voxel_average_f32(const float* xyzi, const double* normals_f64, const int32_t* perm,
                                           const int32_t* start, int n, int m, float* rows, void* stream)
{
    if (n < 1 || n > NMAX || m < 0 || m > n) return USIP_EINVAL;
    if (m == 0) return USIP_OK;
    if (!xyzi || !normals_f64 || !perm || !start || !rows) return USIP_EINVAL;
    USIP_LAUNCH(scan_voxel_average_kernel, dim3(usip_ceil_div(m, 256)), dim3(256), 0, (hipStream_t)stream, xyzi,
                normals_f64, perm, start, n, m, rows);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
