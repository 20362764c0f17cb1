// usip_amd/csrc/fpfh_cpu.cpp -- host twin of csrc/fpfh.hip: the same arithmetic (csrc/fpfh_math.h) on host
// pointers.  Every query and every keypoint tests ALL live points of its frame, in the frame's stable order along x (its own
// sort, no permutation is handed in).  The SPFH counts are integers, so their order is free; the gather's 33 float64 sums take
// the contract's order: 64 partial sums, the one of lane l over the sorted positions lo + l + 64 k ascending (lo =
// first_within()), folded by the xor-butterfly 32 .. 1 -- what the device's wave per keypoint does over its pruned range.
// Threads split the queries / keypoints, nothing else.  Never reached from the device entry points.
#include <cmath>
#include <vector>
#include "frames_host.h"
#include "fpfh_math.h"
#include "../../include/usip_hip.h"

using namespace usip_fpfh;
using usip_host::for_each_query;
using usip_iss::bad_frames;
using usip_iss::bad_radius;
using usip_iss::live_points;

extern "C" int usip_fpfh_spfh_f32_cpu(const float* pc, const int32_t* count, const double* normals, int B, int N,
                                      double radius, int32_t* spfh, int32_t* members, int num_threads)
{
    if (bad_frames(B, N) || bad_radius(radius) || !pc || !normals || !spfh || !members) return USIP_EINVAL;
    const double r2 = radius * radius;
    usip_host::SortedFrame S(N);
    std::vector<double> snormal(3 * (size_t)N);                        // the normals in the sorted order
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        const double *nx = normals + 3LL * f * N, *ny = nx + N, *nz = ny + N;
        int32_t* rows = spfh + (long long)WIDTH * f * N;
        int32_t* mem = members + (long long)f * N;
        const int n = live_points(count, f, N);
        for (int i = n; i < N; ++i) {
            for (int b = 0; b < WIDTH; ++b) rows[(long long)WIDTH * i + b] = 0;
            mem[i] = 0;
        }
        S.sort(x, y, z, n);
        double *s0 = snormal.data(), *s1 = s0 + N, *s2 = s1 + N;
        S.gather(nx, s0);
        S.gather(ny, s1);
        S.gather(nz, s2);
        for_each_query(n, num_threads, [=, &S](int i) {
            const double xi = (double)x[i], yi = (double)y[i], zi = (double)z[i];
            const bool mine = has_normal(nx[i], ny[i], nz[i]);
            int32_t hist[WIDTH] = {0};
            int32_t k = 0;
            if (mine)
                for (int s = 0; s < n; ++s) {
                    const double d2 = usip_prep::sqdist(xi, yi, zi, S.x[s], S.y[s], S.z[s]);
                    if (!has_normal(s0[s], s1[s], s2[s]) || !member(d2, r2)) continue;
                    ++k;
                    Bins h;
                    if (pair_bins(xi, yi, zi, S.x[s], S.y[s], S.z[s], d2, nx[i], ny[i], nz[i], s0[s], s1[s], s2[s], h)) {
                        ++hist[h.h1];
                        ++hist[BINS + h.h2];
                        ++hist[2 * BINS + h.h3];
                    }
                }
            for (int b = 0; b < WIDTH; ++b) rows[(long long)WIDTH * i + b] = hist[b];
            mem[i] = mine ? k - own(xi, yi, zi, r2) : 0;
        });
    }
    return USIP_OK;
}

extern "C" int usip_fpfh_gather_f32_cpu(const float* pc, const int32_t* count, const int32_t* spfh, const int32_t* members,
                                        const float* keypoints, const int32_t* kp_count, int B, int N, int M, double radius,
                                        double* fpfh, int32_t* kp_members, int num_threads)
{
    if (bad_frames(B, N) || bad_keypoints(M) || bad_radius(radius) || !pc || !spfh || !members || !keypoints || !fpfh ||
        !kp_members)
        return USIP_EINVAL;
    const double r2 = radius * radius;
    usip_host::SortedFrame S(N);
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        const float* kp = keypoints + 3LL * f * M;
        const int32_t* rows = spfh + (long long)WIDTH * f * N;
        const int32_t* mem = members + (long long)f * N;
        double* out = fpfh + (long long)WIDTH * f * M;
        int32_t* km = kp_members + (long long)f * M;
        const int n = live_points(count, f, N), m = live_points(kp_count, f, M);
        for (int q = m; q < M; ++q) {
            for (int b = 0; b < WIDTH; ++b) out[(long long)WIDTH * q + b] = 0.0;
            km[q] = 0;
        }
        S.sort(x, y, z, n);
        for_each_query(m, num_threads, [=, &S](int q) {
            const double qx = (double)kp[q], qy = (double)kp[M + q], qz = (double)kp[2LL * M + q];
            std::vector<double> lanes((size_t)LANES * WIDTH, 0.0);     // lane l's 33 sums at lanes[l * 33]
            int32_t k = 0;
            const int lo = first_within(n, qx, radius, [&S](int s) { return (double)S.x[s]; });
            for (int s = lo; s < n; ++s) {
                const int j = S.order[s];
                const double d2 = usip_prep::sqdist(qx, qy, qz, S.x[s], S.y[s], S.z[s]);
                if (!gathers(d2, r2, mem[j])) continue;
                add_row(&lanes[(size_t)((s - lo) % LANES) * WIDTH], rows + (long long)WIDTH * j, mem[j], d2);
                ++k;
            }
            for (int off = LANES / 2; off >= 1; off >>= 1)
                for (int l = 0; l < off; ++l)
                    for (int b = 0; b < WIDTH; ++b) lanes[(size_t)l * WIDTH + b] += lanes[(size_t)(l + off) * WIDTH + b];
            normalise<0>(lanes.data());
            normalise<1>(lanes.data());
            normalise<2>(lanes.data());
            for (int b = 0; b < WIDTH; ++b) out[(long long)WIDTH * q + b] = lanes[b];
            km[q] = k;
        });
    }
    return USIP_OK;
}
