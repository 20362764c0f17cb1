// usip_amd/csrc/iss_cpu.cpp -- host twin of csrc/iss.hip: the same arithmetic (csrc/iss_math.h) on host
// pointers.  Every query tests ALL live points of its frame, in the frame's stable order along x (its own sort, no
// permutation is handed in) -- the order the contract fixes for the six sums, and what the device's pruned walk over the
// caller's permutation must reproduce bit for bit.  The suppression pass does not depend on an order and walks the
// original one.  Threads split the queries, nothing else.  Never reached from the device entry points.
#include <cmath>
#include "frames_host.h"
#include "../../include/usip_hip.h"

using namespace usip_iss;
using usip_host::for_each_query;
using usip_host::split;

extern "C" int usip_iss_saliency_f32_cpu(const float* pc, const int32_t* count, int B, int N, double salient_radius,
                                         double gamma_21, double gamma_32, int min_neighbors, double* saliency,
                                         int32_t* neighbours, int num_threads)
{
    if (bad_frames(B, N) || bad_radius(salient_radius) || min_neighbors < 1 || !pc || !saliency || !neighbours)
        return USIP_EINVAL;
    const double r2 = salient_radius * salient_radius;
    usip_host::SortedFrame S(N);
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        double* sal = saliency + (long long)f * N;
        int32_t* nb = neighbours + (long long)f * N;
        const int n = live_points(count, f, N);
        for (int i = n; i < N; ++i) { sal[i] = 0.0; nb[i] = 0; }
        S.sort(x, y, z, n);
        for_each_query(n, num_threads, [=, &S](int i) {
            const double xi = (double)x[i], yi = (double)y[i], zi = (double)z[i];
            Scatter g;
            for (int s = 0; s < n; ++s) g.offer(xi, yi, zi, S.x[s], S.y[s], S.z[s], r2);
            sal[i] = saliency_from(g, min_neighbors, gamma_21, gamma_32);
            nb[i] = g.n;
        });
    }
    return USIP_OK;
}

extern "C" int usip_iss_nms_f32_cpu(const float* pc, const int32_t* count, const double* saliency, int B, int N,
                                    double non_max_radius, int min_neighbors, uint8_t* keypoint, int num_threads)
{
    if (bad_frames(B, N) || bad_radius(non_max_radius) || min_neighbors < 1 || !pc || !saliency || !keypoint)
        return USIP_EINVAL;
    const double r2 = non_max_radius * non_max_radius;
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        const double* sal = saliency + (long long)f * N;
        uint8_t* kp = keypoint + (long long)f * N;
        const int n = live_points(count, f, N);
        for (int i = n; i < N; ++i) kp[i] = 0;
        split(n, num_threads, [=](long long lo, long long hi) {
            for (long long i = lo; i < hi; ++i) {
                const double xi = (double)x[i], yi = (double)y[i], zi = (double)z[i], si = sal[i];
                Rivals g;
                if (si > 0.0)                                          // (nothing else can be a keypoint)
                    for (int j = 0; j < n; ++j) g.offer(xi, yi, zi, si, x[j], y[j], z[j], sal[j], r2);
                kp[i] = keypoint_from(g, si, min_neighbors) ? 1 : 0;
            }
        });
    }
    return USIP_OK;
}
