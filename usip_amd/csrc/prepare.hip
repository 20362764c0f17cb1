// usip_amd/csrc/prepare.hip -- raw LiDAR scans prepared on the device: K nearest neighbours of every
// point, surface normal and curvature, voxel-grid average.  Replaces the reference's MATLAB preparation
// (evaluation/matlab/kitti_data_prepare/kitti_test_prepare.m:95-108: findPointNormals + pcdownsample 'gridAverage');
// csrc/prepare_math.h has the semantics and the arithmetic, which the host twin (csrc/prepare_cpu.cpp) shares.
// No launch synchronises.
//
//   scan_knn_kernel<K>         csrc/knn_walk.h's outward walk over the scan's float4 rows: a point is not its own
//                              neighbour, four rows in flight; idx i32 [n][K], tiles_visited i32 [tiles].
//   scan_normals_kernel        one lane per point: gathers its K neighbours, covariance, 3x3 Jacobi, flip -- in registers.
//   scan_voxel_keys_kernel     one lane per point: the int64 key of its cell.
//   scan_voxel_average_kernel  one lane per occupied cell: its members in ascending original index, float64 sums in that
//                              order (no atomics: bit-reproducible and the host twin's order).
#include "common.h"
#include "bank.h"
#include "prepare_math.h"
#include "knn_walk.h"

using namespace usip_prep;
using usip_bank::safe_index;
using usip_walk::nearest_rows;

namespace {

// the scan as knn_walk.h reads it
struct ScanRows {
    const float4* pts;
    const int32_t* perm;
    int n;
    __device__ __forceinline__ int at(int s) const { return safe_index(perm[s], n); }
    __device__ __forceinline__ float4 row(int j) const { return pts[j]; }
};

template <int K>
__global__ __launch_bounds__(TILE) void scan_knn_kernel(const float4* __restrict__ pts, const int32_t* __restrict__ perm,
                                                        int n, int32_t* __restrict__ idx, int32_t* __restrict__ visited)
{
    __shared__ float4 tile[2][TILE];
    __shared__ int32_t orig[2][TILE];
    __shared__ double slots[4];
    const int seen = nearest_rows<K, false, true>(ScanRows{pts, perm, n}, blockIdx.x, tile, orig, slots, idx);
    if (visited && threadIdx.x == 0) visited[blockIdx.x] = seen;
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
