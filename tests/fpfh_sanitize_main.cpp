// tests/fpfh_sanitize_main.cpp -- a stand-alone driver of the f-19 host twin (usip_amd/csrc/fpfh_cpu.cpp) for a build under
// -fsanitize=address,undefined (tests/test_fpfh_cpu.py compiles and runs it): random frames with counts in and out of range,
// ties along x, non-finite coordinates and normals, rows without a normal, keypoints on cloud points, outside the cloud and
// non-finite.  Every array is sized exactly, so a read or write one element outside is reported.  Exit status 0: every call
// returned USIP_OK or, where the arguments are outside the limits, USIP_EINVAL.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "../include/usip_hip.h"

int main()
{
    std::mt19937_64 rng(19);
    std::uniform_real_distribution<float> coord(-2.f, 2.f);
    int calls = 0, refused = 0;
    for (int round = 0; round < 60; ++round) {
        const int sizes[] = {1, 2, 3, 40, 255, 256, 257, 515};
        const int counts[] = {1, 2, 63, 64, 65, 130};
        const int B = 1 + (int)(rng() % 3), N = sizes[rng() % 8], M = counts[rng() % 6];
        std::vector<float> pc((size_t)B * 3 * N), kp((size_t)B * 3 * M);
        for (auto& v : pc) v = round % 5 == 4 ? (float)(int)(coord(rng) * 4.f) / 4.f : coord(rng);       // ties
        if (round % 9 == 8) pc[rng() % pc.size()] = NAN;
        if (round % 9 == 7) pc[rng() % pc.size()] = INFINITY;
        for (auto& v : kp) v = 1.5f * coord(rng);                         // some outside the cloud
        for (int f = 0; f < B; ++f)                                       // the first keypoint of a frame ON its first point
            for (int c = 0; c < 3; ++c) kp[((size_t)f * 3 + c) * M] = pc[((size_t)f * 3 + c) * N];
        if (round % 6 == 5) kp[rng() % kp.size()] = NAN;
        if (round % 6 == 4) kp[rng() % kp.size()] = -INFINITY;
        std::vector<int32_t> count((size_t)B), kp_count((size_t)B);
        for (auto& c : count) c = (int32_t)(rng() % (N + 6)) - 3;         // below 0 and above N: clamped
        for (auto& c : kp_count) c = (int32_t)(rng() % (M + 6)) - 3;
        const bool with_count = round % 3 != 0, with_kp_count = round % 4 != 0;
        const int threads = 1 + (int)(rng() % 3);
        const double radius = round % 7 == 6 ? 100.0 : 0.5 + 0.25 * (double)(rng() % 4);
        std::vector<double> normals((size_t)B * 3 * N), fpfh((size_t)B * M * 33);
        for (auto& v : normals) v = (double)coord(rng);
        if (round % 4 == 1) {
            normals[rng() % normals.size()] = NAN;
            normals[rng() % normals.size()] = -INFINITY;
        }
        for (int z = 0; z < 1 + N / 8; ++z) {                             // rows without a normal
            const size_t i = rng() % ((size_t)B * N), f = i / N, s = i % N;
            for (int c = 0; c < 3; ++c) normals[(f * 3 + c) * N + s] = 0.0;
        }
        std::vector<int32_t> spfh((size_t)B * N * 33), members((size_t)B * N), kp_members((size_t)B * M);
        int rc = usip_fpfh_spfh_f32_cpu(pc.data(), with_count ? count.data() : nullptr, normals.data(), B, N, radius,
                                        spfh.data(), members.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: spfh returned %d\n", round, rc); return 1; }
        for (size_t i = 0; i < members.size(); ++i) {
            if (members[i] < 0 || members[i] > N - 1) { std::printf("round %d: members %d\n", round, members[i]); return 1; }
            for (int h = 0; h < 3; ++h) {
                int32_t sum = 0;
                for (int b = 0; b < 11; ++b) sum += spfh[i * 33 + h * 11 + b];
                if (sum < 0 || sum > members[i]) { std::printf("round %d: a histogram of %d over %d\n", round, sum, members[i]); return 1; }
            }
        }
        rc = usip_fpfh_gather_f32_cpu(pc.data(), with_count ? count.data() : nullptr, spfh.data(), members.data(), kp.data(),
                                      with_kp_count ? kp_count.data() : nullptr, B, N, M, radius, fpfh.data(),
                                      kp_members.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: gather returned %d\n", round, rc); return 1; }
        for (size_t i = 0; i < fpfh.size(); ++i)
            if (!(fpfh[i] >= 0.0 && fpfh[i] <= 100.0 * (1.0 + 1e-12)) || kp_members[i / 33] < 0 || kp_members[i / 33] > N) {
                std::printf("round %d: fpfh %g, kp_members %d at %zu\n", round, fpfh[i], kp_members[i / 33], i);
                return 1;
            }
        // outside the limits: refused before anything is read
        const int bad[] = {
            usip_fpfh_spfh_f32_cpu(pc.data(), nullptr, normals.data(), B, N, 0.0, spfh.data(), members.data(), 1),
            usip_fpfh_spfh_f32_cpu(pc.data(), nullptr, normals.data(), B, N, (double)NAN, spfh.data(), members.data(), 1),
            usip_fpfh_spfh_f32_cpu(pc.data(), nullptr, normals.data(), 65536, N, 1.0, spfh.data(), members.data(), 1),
            usip_fpfh_spfh_f32_cpu(pc.data(), nullptr, normals.data(), B, (1 << 20) + 1, 1.0, spfh.data(), members.data(), 1),
            usip_fpfh_spfh_f32_cpu(pc.data(), nullptr, nullptr, B, N, 1.0, spfh.data(), members.data(), 1),
            usip_fpfh_spfh_f32_cpu(pc.data(), nullptr, normals.data(), B, N, 1.0, nullptr, members.data(), 1),
            usip_fpfh_gather_f32_cpu(pc.data(), nullptr, spfh.data(), members.data(), kp.data(), nullptr, B, N, 0, 1.0,
                                     fpfh.data(), kp_members.data(), 1),
            usip_fpfh_gather_f32_cpu(pc.data(), nullptr, spfh.data(), members.data(), kp.data(), nullptr, B, N, 65536, 1.0,
                                     fpfh.data(), kp_members.data(), 1),
            usip_fpfh_gather_f32_cpu(pc.data(), nullptr, spfh.data(), members.data(), kp.data(), nullptr, B, N, M,
                                     (double)INFINITY, fpfh.data(), kp_members.data(), 1),
            usip_fpfh_gather_f32_cpu(pc.data(), nullptr, spfh.data(), members.data(), nullptr, nullptr, B, N, M, 1.0,
                                     fpfh.data(), kp_members.data(), 1),
            usip_fpfh_gather_f32_cpu(pc.data(), nullptr, nullptr, members.data(), kp.data(), nullptr, B, N, M, 1.0,
                                     fpfh.data(), kp_members.data(), 1),
            usip_fpfh_gather_f32_cpu(pc.data(), nullptr, spfh.data(), members.data(), kp.data(), nullptr, 0, N, M, 1.0,
                                     fpfh.data(), kp_members.data(), 1)};
        for (int rcb : bad) {
            ++calls;
            if (rcb != USIP_EINVAL) { std::printf("round %d: a call outside the limits returned %d\n", round, rcb); return 1; }
            ++refused;
        }
    }
    std::printf("%d calls, %d refused as they must be, no finding\n", calls, refused);
    return 0;
}
