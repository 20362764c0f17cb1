// usip_amd/csrc/shot_cpu.cpp -- host twin of csrc/shot.hip: the same arithmetic (csrc/shot_math.h) on host
// pointers.  Every keypoint tests ALL live points of its frame from first_within() on, in the frame's stable order along x (its
// own sort, no permutation is handed in).  The frame's seven float64 sums take the contract's order: 64 partial sums, the one
// of lane l over the sorted positions lo + l + 64 k ascending, folded by the xor-butterfly 32 .. 1 -- what the device's wave per
// keypoint does over its pruned range; the sign counts and the histogram are integers, so their order is free; the descriptor's
// sum of squares takes its 64 partial sums over the columns l + 64 k.  Threads split the keypoints, nothing else.  Never reached
// from the device entry points.
#include <cmath>
#include <vector>
#include "frames_host.h"
#include "shot_math.h"
#include "../../include/usip_hip.h"

using namespace usip_shot;
using usip_host::for_each_query;
using usip_iss::bad_frames;
using usip_iss::bad_radius;
using usip_iss::live_points;

extern "C" int usip_shot_lrf_f32_cpu(const float* pc, const int32_t* count, const float* keypoints, const int32_t* kp_count,
                                     int B, int N, int M, double radius, double* lrf, int32_t* lrf_members, int num_threads)
{
    if (bad_frames(B, N) || bad_keypoints(M) || bad_radius(radius) || !pc || !keypoints || !lrf || !lrf_members)
        return USIP_EINVAL;
    const double r2 = radius * radius;
    usip_host::SortedFrame S(N);
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        const float* kp = keypoints + 3LL * f * M;
        double* out = lrf + 9LL * f * M;
        int32_t* lm = lrf_members + (long long)f * M;
        const int n = live_points(count, f, N), m = live_points(kp_count, f, M);
        for (int q = m; q < M; ++q) {
            for (int c = 0; c < 9; ++c) out[9LL * q + c] = 0.0;
            lm[q] = 0;
        }
        S.sort(x, y, z, n);
        for_each_query(m, num_threads, [=, &S](int q) {
            const double qx = (double)kp[q], qy = (double)kp[M + q], qz = (double)kp[2LL * M + q];
            Sums lanes[LANES];
            int32_t k = 0;
            const int lo = first_within(n, qx, radius, [&S](int s) { return (double)S.x[s]; });
            for (int s = lo; s < n; ++s) {
                const double d2 = usip_prep::sqdist(qx, qy, qz, S.x[s], S.y[s], S.z[s]);
                if (!member(d2, r2)) continue;
                lanes[(s - lo) % LANES].add(radius, d2, (double)S.x[s] - qx, (double)S.y[s] - qy, (double)S.z[s] - qz);
                ++k;
            }
            for (int off = LANES / 2; off >= 1; off >>= 1)
                for (int l = 0; l < off; ++l) lanes[l].fold(lanes[l + off]);
            const Axes A = axes_from(lanes[0], k);
            Votes V;
            if (A.ok)
                for (int s = lo; s < n; ++s)
                    if (member(usip_prep::sqdist(qx, qy, qz, S.x[s], S.y[s], S.z[s]), r2))
                        V.add(A, (double)S.x[s] - qx, (double)S.y[s] - qy, (double)S.z[s] - qz);
            frame_from(A, V, out + 9LL * q);
            lm[q] = k;
        });
    }
    return USIP_OK;
}

extern "C" int usip_shot_hist_f32_cpu(const float* pc, const int32_t* count, const double* normals, const float* keypoints,
                                      const int32_t* kp_count, const double* lrf, int B, int N, int M, double radius,
                                      int64_t* hist, double* shot, int32_t* kp_members, int num_threads)
{
    if (bad_frames(B, N) || bad_keypoints(M) || bad_radius(radius) || !pc || !normals || !keypoints || !lrf || !hist || !shot ||
        !kp_members)
        return USIP_EINVAL;
    const double r2 = radius * radius;
    usip_host::SortedFrame S(N);
    std::vector<double> snormal(3 * (size_t)N);                        // the normals in the sorted order
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        const double *nx = normals + 3LL * f * N, *ny = nx + N, *nz = ny + N;
        const float* kp = keypoints + 3LL * f * M;
        const double* frames = lrf + 9LL * f * M;
        int64_t* hrows = hist + (long long)WIDTH * f * M;
        double* srows = shot + (long long)WIDTH * f * M;
        int32_t* km = kp_members + (long long)f * M;
        const int n = live_points(count, f, N), m = live_points(kp_count, f, M);
        for (int q = m; q < M; ++q) {
            for (int b = 0; b < WIDTH; ++b) {
                hrows[(long long)WIDTH * q + b] = 0;
                srows[(long long)WIDTH * q + b] = 0.0;
            }
            km[q] = 0;
        }
        S.sort(x, y, z, n);
        double *s0 = snormal.data(), *s1 = s0 + N, *s2 = s1 + N;
        S.gather(nx, s0);
        S.gather(ny, s1);
        S.gather(nz, s2);
        for_each_query(m, num_threads, [=, &S](int q) {
            const double qx = (double)kp[q], qy = (double)kp[M + q], qz = (double)kp[2LL * M + q];
            const double* l = frames + 9LL * q;
            const Lrf L{l[0], l[1], l[2], l[3], l[4], l[5], l[6], l[7], l[8]};
            const bool framed = L.exists();
            long long bins[WIDTH] = {0};
            int32_t k = 0;
            for (int s = 0; s < n; ++s) {
                const double d2 = usip_prep::sqdist(qx, qy, qz, S.x[s], S.y[s], S.z[s]);
                if (!describes(d2, r2, s0[s], s1[s], s2[s])) continue;
                ++k;
                if (!framed) continue;
                Adds a;
                member_adds(L, radius, d2, (double)S.x[s] - qx, (double)S.y[s] - qy, (double)S.z[s] - qz, s0[s], s1[s], s2[s], a);
                for (int i = 0; i < ADDS; ++i)
                    if (a.col[i] >= 0) bins[a.col[i]] += a.q[i];
            }
            double part[LANES] = {0.0};
            for (int b = 0; b < WIDTH; ++b) {                          // ascending b: partial b % 64 takes its columns ascending
                const double h = (double)bins[b];
                part[b % LANES] += h * h;
            }
            for (int off = LANES / 2; off >= 1; off >>= 1)
                for (int p = 0; p < off; ++p) part[p] += part[p + off];
            const double ss = part[0], root = sqrt(ss);
            for (int b = 0; b < WIDTH; ++b) {
                hrows[(long long)WIDTH * q + b] = bins[b];
                srows[(long long)WIDTH * q + b] = ss > 0.0 ? (double)bins[b] / root : 0.0;
            }
            km[q] = k;
        });
    }
    return USIP_OK;
}

extern "C" int usip_shot_angle_f64_cpu(const double* y, const double* x, long long n, double* out)
{
    if (!y || !x || !out || n < 0) return USIP_EINVAL;
    for (long long i = 0; i < n; ++i) out[i] = angle(y[i], x[i]);
    return USIP_OK;
}
