// usip_amd/csrc/spin_cpu.cpp -- host twin of csrc/spin.hip: the same arithmetic (csrc/spin_math.h) on host
// pointers.  Every keypoint tests ALL live points of its frame, in the frame's stable order along x (its own sort, no
// permutation is handed in); the image is a sum of integers, so the order is free and the device's pruned walk over its window
// gives the same numbers.  Threads split the keypoints, nothing else.  Never reached from the device entry point.
#include <cmath>
#include <vector>
#include "frames_host.h"
#include "spin_math.h"
#include "../../include/usip_hip.h"

using namespace usip_spin;
using usip_host::for_each_query;
using usip_iss::bad_frames;
using usip_iss::bad_radius;
using usip_iss::live_points;

namespace {

template <int STRUCTURE>
void describe(const usip_host::SortedFrame& S, int n, const double* s0, const double* s1, const double* s2, double qx, double qy,
              double qz, const Axis& A, double radius, double r2, double support, long long bins[WIDTH], int32_t& k)
{
    for (int s = 0; s < n; ++s) {
        const double d2 = usip_prep::sqdist(qx, qy, qz, S.x[s], S.y[s], S.z[s]);
        if (!(d2 > 0.0 && member(d2, r2))) continue;
        if (support > 0.0 && !supported(A, support, s0[s], s1[s], s2[s])) continue;
        Adds a;
        if (!member_adds<STRUCTURE>(A, radius, d2, (double)S.x[s] - qx, (double)S.y[s] - qy, (double)S.z[s] - qz, a)) continue;
        ++k;
        for (int i = 0; i < ADDS; ++i)
            if (a.q[i] > 0) bins[a.col[i]] += a.q[i];
    }
}

}  // namespace

extern "C" int usip_spin_image_f32_cpu(const float* pc, const int32_t* count, const double* normals, const float* keypoints,
                                       const int32_t* kp_count, const double* axes, int B, int N, int M, double radius,
                                       double support_angle_cos, int structure, int64_t* hist, double* spin,
                                       int32_t* kp_members, int num_threads)
{
    if (bad_frames(B, N) || bad_keypoints(M) || bad_radius(radius) || bad_support(support_angle_cos) ||
        bad_structure(structure) || !pc || !keypoints || !axes || !hist || !spin || !kp_members ||
        (support_angle_cos > 0.0 && !normals))
        return USIP_EINVAL;
    const double r2 = radius * radius;
    const bool angled = support_angle_cos > 0.0;
    usip_host::SortedFrame S(N);
    std::vector<double> snormal(angled ? 3 * (size_t)N : 0);           // the normals in the sorted order
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        const float* kp = keypoints + 3LL * f * M;
        const double* rows = axes + 3LL * f * M;
        int64_t* hrows = hist + (long long)WIDTH * f * M;
        double* srows = spin + (long long)WIDTH * f * M;
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
        double *s0 = nullptr, *s1 = nullptr, *s2 = nullptr;
        if (angled) {
            const double *nx = normals + 3LL * f * N, *ny = nx + N, *nz = ny + N;
            s0 = snormal.data();
            s1 = s0 + N;
            s2 = s1 + N;
            S.gather(nx, s0);
            S.gather(ny, s1);
            S.gather(nz, s2);
        }
        for_each_query(m, num_threads, [=, &S](int q) {
            const double qx = (double)kp[q], qy = (double)kp[M + q], qz = (double)kp[2LL * M + q];
            const Axis A(rows[3LL * q], rows[3LL * q + 1], rows[3LL * q + 2]);
            long long bins[WIDTH] = {0};
            int32_t k = 0;
            if (A.ok) {
                if (structure == RADIAL)
                    describe<RADIAL>(S, n, s0, s1, s2, qx, qy, qz, A, radius, r2, support_angle_cos, bins, k);
                else
                    describe<RECTANGULAR>(S, n, s0, s1, s2, qx, qy, qz, A, radius, r2, support_angle_cos, bins, k);
            }
            for (int b = 0; b < WIDTH; ++b) {
                hrows[(long long)WIDTH * q + b] = bins[b];
                srows[(long long)WIDTH * q + b] = column(bins[b], k);
            }
            km[q] = k;
        });
    }
    return USIP_OK;
}
