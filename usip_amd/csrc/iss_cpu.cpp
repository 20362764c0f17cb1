// usip_amd/csrc/iss_cpu.cpp -- host twin of csrc/iss.hip: the same arithmetic (csrc/iss_math.h) on host
// pointers.  Every query tests ALL live points of its frame, in the frame's stable order along x (its own sort, no
// permutation is handed in) -- the order the contract fixes for the six sums, and what the device's pruned walk over the
// caller's permutation must reproduce bit for bit.  The suppression pass does not depend on an order and walks the
// original one.  Threads split the queries, nothing else.  Never reached from the device entry points.
#include <algorithm>
#include <cmath>
#include <vector>
#include "host_split.h"
#include "iss_math.h"
#include "../../include/usip_hip.h"

using namespace usip_iss;
using usip_host::split;

namespace {

int live_points(const int32_t* count, int f, int N)
{
    const int c = count ? count[f] : N;
    return c < 0 ? 0 : (c > N ? N : c);
}

bool bad_shape(int B, int N, double r, int min_neighbors)
{
    return B < 1 || B > 65535 || N < 1 || N > NMAX || min_neighbors < 1 || !(r > 0.0) || !(r < (double)INFINITY);
}

}  // namespace

extern "C" int usip_iss_saliency_f32_cpu(const float* pc, const int32_t* count, int B, int N, double salient_radius,
                                         double gamma_21, double gamma_32, int min_neighbors, double* saliency,
                                         int32_t* neighbours, int num_threads)
{
    if (bad_shape(B, N, salient_radius, min_neighbors) || !pc || !saliency || !neighbours) return USIP_EINVAL;
    const double r2 = salient_radius * salient_radius;
    std::vector<float> sorted(3 * (size_t)N);
    std::vector<int32_t> order(N);
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        double* sal = saliency + (long long)f * N;
        int32_t* nb = neighbours + (long long)f * N;
        const int n = live_points(count, f, N);
        for (int i = n; i < N; ++i) { sal[i] = 0.0; nb[i] = 0; }
        for (int i = 0; i < n; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.begin() + n, [&](int32_t a, int32_t b) { return x[a] < x[b]; });
        float *sx = sorted.data(), *sy = sx + N, *sz = sy + N;
        for (int s = 0; s < n; ++s) { sx[s] = x[order[s]]; sy[s] = y[order[s]]; sz[s] = z[order[s]]; }
        split(n, num_threads, [=](long long lo, long long hi) {
            for (long long i = lo; i < hi; ++i) {
                const double xi = (double)x[i], yi = (double)y[i], zi = (double)z[i];
                Scatter g;
                for (int s = 0; s < n; ++s) g.offer(xi, yi, zi, sx[s], sy[s], sz[s], r2);
                sal[i] = saliency_from(g, min_neighbors, gamma_21, gamma_32);
                nb[i] = g.n;
            }
        });
    }
    return USIP_OK;
}

extern "C" int usip_iss_nms_f32_cpu(const float* pc, const int32_t* count, const double* saliency, int B, int N,
                                    double non_max_radius, int min_neighbors, uint8_t* keypoint, int num_threads)
{
    if (bad_shape(B, N, non_max_radius, min_neighbors) || !pc || !saliency || !keypoint) return USIP_EINVAL;
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
