// usip_amd/csrc/spin_cpu.cpp -- host twin of csrc/spin.hip: the same arithmetic (csrc/spin_math.h) on host
// pointers, over the keypoint loop of csrc/keypoints_host.h; the image is a sum of integers, so the order is free and the
// device's pruned walk over its window gives the same numbers.  Never reached from the device entry point.
#include <cmath>
#include <vector>
#include "keypoints_host.h"
#include "spin_math.h"
#include "../../include/usip_hip.h"

using namespace usip_spin;
using usip_host::DescribedFrame;
using usip_host::for_each_keypoint;
using usip_host::Rows;
using usip_iss::bad_frames;
using usip_iss::bad_radius;

namespace {

template <int STRUCTURE>
void describe(const DescribedFrame& S, double qx, double qy, double qz, const Axis& A, double radius, double r2, double support,
              long long bins[WIDTH], int32_t& k)
{
    for (int s = 0; s < S.n; ++s) {
        const double d2 = usip_prep::sqdist(qx, qy, qz, S.x[s], S.y[s], S.z[s]);
        if (!(d2 > 0.0 && member(d2, r2))) continue;
        if (support > 0.0 && !supported(A, support, S.n0[s], S.n1[s], S.n2[s])) continue;
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
    const Rows hrows(hist, WIDTH);
    const Rows srows(spin, WIDTH);
    const Rows km(kp_members, 1);
    for_each_keypoint(pc, count, support_angle_cos > 0.0 ? normals : nullptr, keypoints, kp_count, B, N, M, num_threads,
                      [=](const DescribedFrame& S, long long slot, double qx, double qy, double qz) {
        const double* v = axes + 3 * slot;
        const Axis A(v[0], v[1], v[2]);
        long long bins[WIDTH] = {0};
        int32_t k = 0;
        if (A.ok) {
            if (structure == RADIAL)
                describe<RADIAL>(S, qx, qy, qz, A, radius, r2, support_angle_cos, bins, k);
            else
                describe<RECTANGULAR>(S, qx, qy, qz, A, radius, r2, support_angle_cos, bins, k);
        }
        for (int b = 0; b < WIDTH; ++b) {
            hrows[slot][b] = bins[b];
            srows[slot][b] = column(bins[b], k);
        }
        km[slot][0] = k;
    }, hrows, srows, km);
    return USIP_OK;
}
