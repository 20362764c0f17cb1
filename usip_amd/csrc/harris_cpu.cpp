// usip_amd/csrc/harris_cpu.cpp -- host twin of csrc/harris.hip: the same arithmetic (csrc/harris_math.h) on
// host pointers.  Every query tests ALL live points of its frame, in the frame's stable order along x (its own sort, no
// permutation is handed in) -- the order the contract fixes for the sums, and what the device's pruned walk over the
// caller's permutation must reproduce bit for bit.  Threads split the queries, nothing else.  Never reached from the device
// entry points.
#include <algorithm>
#include <cmath>
#include <vector>
#include "host_split.h"
#include "harris_math.h"
#include "../../include/usip_hip.h"

using namespace usip_harris;
using usip_host::split;

namespace {

int live_points(const int32_t* count, int f, int N)
{
    const int c = count ? count[f] : N;
    return c < 0 ? 0 : (c > N ? N : c);
}

bool bad_shape(int B, int N, double r)
{
    return B < 1 || B > 65535 || N < 1 || N > NMAX || !(r > 0.0) || !(r < (double)INFINITY);
}

// order[0 .. n): the frame's live points ascending along x, ties towards the lower index
void sort_along_x(const float* x, int n, std::vector<int32_t>& order)
{
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.begin() + n, [&](int32_t a, int32_t b) { return x[a] < x[b]; });
}

}  // namespace

extern "C" int usip_harris_normals_f32_cpu(const float* pc, const int32_t* count, int B, int N, double radius,
                                           int min_neighbors, double* normals, int32_t* neighbours, int num_threads)
{
    if (bad_shape(B, N, radius) || min_neighbors < 1 || !pc || !normals || !neighbours) return USIP_EINVAL;
    const double r2 = radius * radius;
    std::vector<float> sorted(3 * (size_t)N);
    std::vector<int32_t> order(N);
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        double *nx = normals + 3LL * f * N, *ny = nx + N, *nz = ny + N;
        int32_t* nb = neighbours + (long long)f * N;
        const int n = live_points(count, f, N);
        for (int i = n; i < N; ++i) { nx[i] = 0.0; ny[i] = 0.0; nz[i] = 0.0; nb[i] = 0; }
        sort_along_x(x, n, order);
        float *sx = sorted.data(), *sy = sx + N, *sz = sy + N;
        for (int s = 0; s < n; ++s) { sx[s] = x[order[s]]; sy[s] = y[order[s]]; sz[s] = z[order[s]]; }
        split(n, num_threads, [=](long long lo, long long hi) {
            for (long long i = lo; i < hi; ++i) {
                const double xi = (double)x[i], yi = (double)y[i], zi = (double)z[i];
                Moments g;
                for (int s = 0; s < n; ++s) g.offer(xi, yi, zi, sx[s], sy[s], sz[s], r2);
                const Normal3 nrm = normal_of(g, min_neighbors, xi, yi, zi);
                nx[i] = nrm.x;
                ny[i] = nrm.y;
                nz[i] = nrm.z;
                nb[i] = g.m;
            }
        });
    }
    return USIP_OK;
}

extern "C" int usip_harris_response_f32_cpu(const float* pc, const int32_t* count, const double* normals, int B, int N,
                                            double radius, int method, double* response, int32_t* members, int num_threads)
{
    if (bad_shape(B, N, radius) || !known_method(method) || !pc || !normals || !response || !members) return USIP_EINVAL;
    const double r2 = radius * radius;
    std::vector<float> sorted(3 * (size_t)N);
    std::vector<double> snormal(3 * (size_t)N);
    std::vector<uint8_t> shas(N);
    std::vector<int32_t> order(N);
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        const double *nx = normals + 3LL * f * N, *ny = nx + N, *nz = ny + N;
        double* res = response + (long long)f * N;
        int32_t* mem = members + (long long)f * N;
        const int n = live_points(count, f, N);
        for (int i = n; i < N; ++i) { res[i] = 0.0; mem[i] = 0; }
        sort_along_x(x, n, order);
        float *sx = sorted.data(), *sy = sx + N, *sz = sy + N;
        double *s0 = snormal.data(), *s1 = s0 + N, *s2 = s1 + N;
        uint8_t* sh = shas.data();
        for (int s = 0; s < n; ++s) {
            const int j = order[s];
            sx[s] = x[j]; sy[s] = y[j]; sz[s] = z[j];
            s0[s] = nx[j]; s1[s] = ny[j]; s2[s] = nz[j];
            sh[s] = has_normal(nx[j], ny[j], nz[j]) ? 1 : 0;
        }
        split(n, num_threads, [=](long long lo, long long hi) {
            for (long long i = lo; i < hi; ++i) {
                const double xi = (double)x[i], yi = (double)y[i], zi = (double)z[i];
                const bool mine = has_normal(nx[i], ny[i], nz[i]);
                Tensor g;
                if (mine)
                    for (int s = 0; s < n; ++s) g.offer(xi, yi, zi, sx[s], sy[s], sz[s], sh[s] != 0, s0[s], s1[s], s2[s], r2);
                res[i] = mine ? response_from(g, method) : 0.0;
                mem[i] = mine ? g.k : 0;
            }
        });
    }
    return USIP_OK;
}
