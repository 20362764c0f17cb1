// usip_amd/csrc/fpfh_cpu.cpp -- host twin of csrc/fpfh.hip: the same arithmetic (csrc/fpfh_math.h) on host
// pointers, over the frame loop of csrc/frames_host.h and the keypoint loop and the contract's order of sums of
// csrc/keypoints_host.h.  The SPFH counts are integers, so their order is free; the gather's 33 float64 sums take the
// contract's order.  Threads split the queries / keypoints, nothing else.  Never reached from the device entry points.
#include <array>
#include <cmath>
#include <vector>
#include "keypoints_host.h"
#include "../../include/usip_hip.h"

using namespace usip_fpfh;
using usip_host::for_each_keypoint;
using usip_host::for_each_query;
using usip_host::Rows;
using usip_iss::bad_frames;
using usip_iss::bad_radius;

extern "C" int usip_fpfh_spfh_f32_cpu(const float* pc, const int32_t* count, const double* normals, int B, int N,
                                      double radius, int32_t* spfh, int32_t* members, int num_threads)
{
    if (bad_frames(B, N) || bad_radius(radius) || !pc || !normals || !spfh || !members) return USIP_EINVAL;
    const double r2 = radius * radius;
    usip_host::DescribedFrame S(N, true);
    for (int f = 0; f < B; ++f) {
        const float *x = pc + 3LL * f * N, *y = x + N, *z = y + N;
        const double *nx = normals + 3LL * f * N, *ny = nx + N, *nz = ny + N;
        int32_t* rows = spfh + (long long)WIDTH * f * N;
        int32_t* mem = members + (long long)f * N;
        S.sort(pc, count, normals, f);
        const int n = S.n;
        std::fill(rows + (long long)WIDTH * n, rows + (long long)WIDTH * N, 0);
        std::fill(mem + n, mem + N, 0);
        for_each_query(n, num_threads, [=, &S](int i) {
            const double xi = (double)x[i], yi = (double)y[i], zi = (double)z[i];
            const bool mine = has_normal(nx[i], ny[i], nz[i]);
            int32_t hist[WIDTH] = {0};
            int32_t k = 0;
            if (mine)
                for (int s = 0; s < n; ++s) {
                    const double d2 = usip_prep::sqdist(xi, yi, zi, S.x[s], S.y[s], S.z[s]);
                    if (!has_normal(S.n0[s], S.n1[s], S.n2[s]) || !member(d2, r2)) continue;
                    ++k;
                    Bins h;
                    if (pair_bins(xi, yi, zi, S.x[s], S.y[s], S.z[s], d2, nx[i], ny[i], nz[i], S.n0[s], S.n1[s], S.n2[s], h)) {
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
    const Rows out(fpfh, WIDTH);
    const Rows km(kp_members, 1);
    for_each_keypoint(pc, count, nullptr, keypoints, kp_count, B, N, M, num_threads,
                      [=](const usip_host::DescribedFrame& S, long long slot, double qx, double qy, double qz) {
        const int32_t* rows = spfh + (long long)WIDTH * S.f * N;
        const int32_t* mem = members + (long long)S.f * N;
        std::vector<std::array<double, WIDTH>> lanes(LANES);           // lane l's 33 sums, zeros
        int32_t k = 0;
        const int lo = first_within(S.n, qx, radius, [&S](int s) { return (double)S.x[s]; });
        for (int s = lo; s < S.n; ++s) {
            const int j = S.order[s];
            const double d2 = usip_prep::sqdist(qx, qy, qz, S.x[s], S.y[s], S.z[s]);
            if (!gathers(d2, r2, mem[j])) continue;
            add_row(lanes[(s - lo) % LANES].data(), rows + (long long)WIDTH * j, mem[j], d2);
            ++k;
        }
        usip_host::fold_lanes(lanes.data(), [](std::array<double, WIDTH>& a, const std::array<double, WIDTH>& b) {
            for (int c = 0; c < WIDTH; ++c) a[c] += b[c];
        });
        double* acc = lanes[0].data();
        normalise<0>(acc);
        normalise<1>(acc);
        normalise<2>(acc);
        for (int b = 0; b < WIDTH; ++b) out[slot][b] = acc[b];
        km[slot][0] = k;
    }, out, km);
    return USIP_OK;
}
