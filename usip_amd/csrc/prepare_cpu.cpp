// usip_amd/csrc/prepare_cpu.cpp -- host twin of csrc/prepare.hip: the same arithmetic (csrc/prepare_math.h)
// on host pointers.  The neighbour search is the plain all-pairs walk in original index order -- the K best under the
// (d2, index) order do not depend on the order candidates are offered in, so it is what the device's pruned walk over the
// x-sorted scan must reproduce; threads split the queries, nothing else.  Never reached from the device entry points.
#include <cmath>
#include <vector>
#include "host_split.h"
#include "prepare_math.h"
#include "../../include/usip_hip.h"

using namespace usip_prep;

namespace {

template <int K>
void knn_range(const float* xyzi, int n, int32_t* idx, int lo, int hi)
{
    for (int i = lo; i < hi; ++i) {
        const double xi = (double)xyzi[4LL * i], yi = (double)xyzi[4LL * i + 1], zi = (double)xyzi[4LL * i + 2];
        KList<K> list;
        list.clear();
        for (int j = 0; j < n; ++j) {
            const double d = sqdist(xi, yi, zi, xyzi[4LL * j], xyzi[4LL * j + 1], xyzi[4LL * j + 2]);
            if (d <= list.worst() && j != i && list.admits(d, j)) list.insert(d, j);
        }
        for (int k = 0; k < K; ++k) idx[(long long)i * K + k] = list.j[k];
    }
}

template <int K>
int knn_host(const float* xyzi, int n, int32_t* idx, int num_threads)
{
    usip_host::split(n, num_threads, [=](int lo, int hi) { knn_range<K>(xyzi, n, idx, lo, hi); });
    return USIP_OK;
}

}  // namespace

extern "C" int usip_scan_knn_f32_cpu(const float* xyzi, int n, int K, int32_t* idx, int num_threads)
{
    if (K < 1 || K > KMAX || n < K + 1 || n > NMAX) return USIP_EINVAL;
    if (!xyzi || !idx) return USIP_EINVAL;
    switch (K) {
#define USIP_KNN_CASE(k) case k: return knn_host<k>(xyzi, n, idx, num_threads)
        USIP_KNN_CASE(1); USIP_KNN_CASE(2); USIP_KNN_CASE(3); USIP_KNN_CASE(4);
        USIP_KNN_CASE(5); USIP_KNN_CASE(6); USIP_KNN_CASE(7); USIP_KNN_CASE(8);
        USIP_KNN_CASE(9); USIP_KNN_CASE(10); USIP_KNN_CASE(11); USIP_KNN_CASE(12);
        USIP_KNN_CASE(13); USIP_KNN_CASE(14); USIP_KNN_CASE(15); USIP_KNN_CASE(16);
#undef USIP_KNN_CASE
    }
    return USIP_EINVAL;
}

extern "C" int usip_scan_normals_f32_cpu(const float* xyzi, const int32_t* idx, int n, int K, const double* viewpoint,
                                         double* normals_f64, float* normals_f32)
{
    if (K < 1 || K > KMAX || n < K + 1 || n > NMAX) return USIP_EINVAL;
    if (!xyzi || !idx || !viewpoint || (!normals_f64 && !normals_f32)) return USIP_EINVAL;
    for (int i = 0; i < n; ++i) {
        const double pd[3] = {(double)xyzi[4LL * i], (double)xyzi[4LL * i + 1], (double)xyzi[4LL * i + 2]};
        Cov S;
        for (int k = 0; k < K; ++k) {
            int j = idx[(long long)i * K + k];
            j = (unsigned)j < (unsigned)n ? j : 0;
            S.add(pd[0] - (double)xyzi[4LL * j], pd[1] - (double)xyzi[4LL * j + 1], pd[2] - (double)xyzi[4LL * j + 2]);
        }
        const Normal r = normal_from(S, K, pd[0], pd[1], pd[2], viewpoint[0], viewpoint[1], viewpoint[2]);
        const double out[4] = {r.x, r.y, r.z, r.curvature};
        for (int c = 0; c < 4; ++c) {
            if (normals_f64) normals_f64[4LL * i + c] = out[c];
            if (normals_f32) normals_f32[4LL * i + c] = (float)out[c];
        }
    }
    return USIP_OK;
}

extern "C" int usip_scan_voxel_keys_f32_cpu(const float* xyzi, int n, const float* lohi, double leaf, int64_t* keys)
{
    if (n < 1 || n > NMAX || !(leaf > 0.0)) return USIP_EINVAL;
    if (!xyzi || !lohi || !keys) return USIP_EINVAL;
    Grid g;
    g.init(lohi, leaf);
    for (int i = 0; i < n; ++i) keys[i] = g.key(xyzi[4LL * i], xyzi[4LL * i + 1], xyzi[4LL * i + 2]);
    return USIP_OK;
}

extern "C" int usip_scan_voxel_average_f32_cpu(const float* xyzi, const double* normals_f64, const int32_t* perm,
                                               const int32_t* start, int n, int m, float* rows)
{
    if (n < 1 || n > NMAX || m < 0 || m > n) return USIP_EINVAL;
    if (m == 0) return USIP_OK;
    if (!xyzi || !normals_f64 || !perm || !start || !rows) return USIP_EINVAL;
    for (int c = 0; c < m; ++c) {
        int first = start[c], last = start[c + 1];
        first = first < 0 ? 0 : (first > n ? n : first);
        last = last < first ? first : (last > n ? n : last);
        float row[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (last > first) cell_average(xyzi, normals_f64, perm, n, first, last, row);
        for (int k = 0; k < 8; ++k) rows[8LL * c + k] = row[k];
    }
    return USIP_OK;
}
