// usip_amd/csrc/harris_cpu.cpp -- host twin of csrc/harris.hip: the same arithmetic (csrc/harris_math.h) on
// host pointers.  Every query tests ALL live points of its frame, in the frame's stable order along x (its own sort, no
// permutation is handed in) -- the order the contract fixes for the sums, and what the device's pruned walk over the
// caller's permutation must reproduce bit for bit.  Threads split the queries, nothing else.  Never reached from the device
// entry points.
#include <cmath>
#include <vector>
#include "frames_host.h"
#include "harris_math.h"
#include "../../include/usip_hip.h"

using namespace usip_harris;
using usip_host::for_each_query;
using usip_iss::bad_frames;
using usip_iss::bad_radius;
using usip_iss::live_points;

extern "C" int usip_harris_normals_f32_cpu(const float* pc, const int32_t* count, int B, int N, double radius,
                                           int min_neighbors, double* normals, int32_t* neighbours, int num_threads)
{
    if (bad_frames(B, N) || bad_radius(radius) || min_neighbors < 1 || !pc || !normals || !neighbours) return USIP_EINVAL;
    const double r2 = radius * radius;
    usip_host::SortedFrame S(N);
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        double *nx = normals + 3LL * f * N, *ny = nx + N, *nz = ny + N;
        int32_t* nb = neighbours + (long long)f * N;
        const int n = live_points(count, f, N);
        for (int i = n; i < N; ++i) { nx[i] = 0.0; ny[i] = 0.0; nz[i] = 0.0; nb[i] = 0; }
        S.sort(x, y, z, n);
        for_each_query(n, num_threads, [=, &S](int i) {
            const double xi = (double)x[i], yi = (double)y[i], zi = (double)z[i];
            Moments g;
            for (int s = 0; s < n; ++s) g.offer(xi, yi, zi, S.x[s], S.y[s], S.z[s], r2);
            const Normal3 nrm = normal_of(g, min_neighbors, xi, yi, zi);
            nx[i] = nrm.x;
            ny[i] = nrm.y;
            nz[i] = nrm.z;
            nb[i] = g.m;
        });
    }
    return USIP_OK;
}

extern "C" int usip_harris_response_f32_cpu(const float* pc, const int32_t* count, const double* normals, int B, int N,
                                            double radius, int method, double* response, int32_t* members, int num_threads)
{
    if (bad_frames(B, N) || bad_radius(radius) || !known_method(method) || !pc || !normals || !response || !members)
        return USIP_EINVAL;
    const double r2 = radius * radius;
    usip_host::SortedFrame S(N);
    std::vector<double> snormal(3 * (size_t)N);                        // the normals in the sorted order
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        const double *nx = normals + 3LL * f * N, *ny = nx + N, *nz = ny + N;
        double* res = response + (long long)f * N;
        int32_t* mem = members + (long long)f * N;
        const int n = live_points(count, f, N);
        for (int i = n; i < N; ++i) { res[i] = 0.0; mem[i] = 0; }
        S.sort(x, y, z, n);
        double *s0 = snormal.data(), *s1 = s0 + N, *s2 = s1 + N;
        S.gather(nx, s0);
        S.gather(ny, s1);
        S.gather(nz, s2);
        for_each_query(n, num_threads, [=, &S](int i) {
            const double xi = (double)x[i], yi = (double)y[i], zi = (double)z[i];
            const bool mine = has_normal(nx[i], ny[i], nz[i]);
            Tensor g;
            if (mine)
                for (int s = 0; s < n; ++s)
                    g.offer(xi, yi, zi, S.x[s], S.y[s], S.z[s], has_normal(s0[s], s1[s], s2[s]), s0[s], s1[s], s2[s], r2);
            res[i] = mine ? response_from(g, method) : 0.0;
            mem[i] = mine ? g.k : 0;
        });
    }
    return USIP_OK;
}
