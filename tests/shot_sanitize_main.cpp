// tests/shot_sanitize_main.cpp -- a stand-alone driver of the f-20 host twin (usip_amd/csrc/shot_cpu.cpp) for a build under
// -fsanitize=address,undefined (tests/test_shot_cpu.py compiles and runs it): random frames with counts in and out of range,
// ties along x, non-finite coordinates and normals, rows without a normal, keypoints on cloud points, outside the cloud and
// non-finite, computed frames and supplied ones that are no frame.  Every array is sized exactly, so a read or write one
// element outside is reported.  Exit status 0: every call returned USIP_OK or, where the arguments are outside the limits,
// USIP_EINVAL.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "../include/usip_hip.h"

int main()
{
    std::mt19937_64 rng(20);
    std::uniform_real_distribution<float> coord(-2.f, 2.f);
    int calls = 0, refused = 0;
    for (int round = 0; round < 60; ++round) {
        const int sizes[] = {1, 2, 5, 40, 63, 64, 65, 515};
        const int counts[] = {1, 2, 3, 4, 5, 70};
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
        const double radius = round % 7 == 6 ? 100.0 : 0.5 + 0.5 * (double)(rng() % 4);
        std::vector<double> normals((size_t)B * 3 * N), lrf((size_t)B * M * 9), shot((size_t)B * M * 352);
        for (auto& v : normals) v = (double)coord(rng);
        if (round % 4 == 1) {
            normals[rng() % normals.size()] = NAN;
            normals[rng() % normals.size()] = -INFINITY;
        }
        for (int z = 0; z < 1 + N / 8; ++z) {                             // rows without a normal
            const size_t i = rng() % ((size_t)B * N), f = i / N, s = i % N;
            for (int c = 0; c < 3; ++c) normals[(f * 3 + c) * N + s] = 0.0;
        }
        std::vector<int32_t> lrf_members((size_t)B * M), kp_members((size_t)B * M);
        std::vector<int64_t> hist((size_t)B * M * 352);
        int rc = usip_shot_lrf_f32_cpu(pc.data(), with_count ? count.data() : nullptr, kp.data(),
                                       with_kp_count ? kp_count.data() : nullptr, B, N, M, radius, lrf.data(),
                                       lrf_members.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: lrf returned %d\n", round, rc); return 1; }
        for (size_t i = 0; i < lrf.size(); ++i)
            if (!(std::fabs(lrf[i]) <= 1.0 + 1e-12) || lrf_members[i / 9] < 0 || lrf_members[i / 9] > N) {
                std::printf("round %d: lrf %g, members %d at %zu\n", round, lrf[i], lrf_members[i / 9], i);
                return 1;
            }
        if (round % 5 == 3) {                                             // supplied rows that are frames, and some that are not
            for (auto& v : lrf) v = (double)coord(rng);
            lrf[rng() % lrf.size()] = NAN;
            lrf[rng() % lrf.size()] = INFINITY;
            for (int c = 0; c < 9; ++c) lrf[c] = 0.0;
        }
        rc = usip_shot_hist_f32_cpu(pc.data(), with_count ? count.data() : nullptr, normals.data(), kp.data(),
                                    with_kp_count ? kp_count.data() : nullptr, lrf.data(), B, N, M, radius, hist.data(),
                                    shot.data(), kp_members.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: hist returned %d\n", round, rc); return 1; }
        for (size_t q = 0; q < kp_members.size(); ++q) {
            int64_t sum = 0;
            for (int b = 0; b < 352; ++b) {
                const int64_t h = hist[q * 352 + b];
                const double s = shot[q * 352 + b];
                if (h < 0 || !(s >= 0.0 && s <= 1.0 + 1e-12)) { std::printf("round %d: hist %lld, shot %g\n", round, (long long)h, s); return 1; }
                sum += h;
            }
            if (kp_members[q] < 0 || kp_members[q] > N || sum > (int64_t)kp_members[q] * 4 * (1LL << 32)) {
                std::printf("round %d: a histogram of %lld over %d members\n", round, (long long)sum, kp_members[q]);
                return 1;
            }
        }
        // outside the limits: refused before anything is read
        const int bad[] = {
            usip_shot_lrf_f32_cpu(pc.data(), nullptr, kp.data(), nullptr, B, N, M, 0.0, lrf.data(), lrf_members.data(), 1),
            usip_shot_lrf_f32_cpu(pc.data(), nullptr, kp.data(), nullptr, B, N, M, (double)NAN, lrf.data(), lrf_members.data(), 1),
            usip_shot_lrf_f32_cpu(pc.data(), nullptr, kp.data(), nullptr, 65536, N, M, 1.0, lrf.data(), lrf_members.data(), 1),
            usip_shot_lrf_f32_cpu(pc.data(), nullptr, kp.data(), nullptr, B, (1 << 20) + 1, M, 1.0, lrf.data(), lrf_members.data(), 1),
            usip_shot_lrf_f32_cpu(pc.data(), nullptr, kp.data(), nullptr, B, N, 0, 1.0, lrf.data(), lrf_members.data(), 1),
            usip_shot_lrf_f32_cpu(pc.data(), nullptr, kp.data(), nullptr, B, N, 65536, 1.0, lrf.data(), lrf_members.data(), 1),
            usip_shot_lrf_f32_cpu(pc.data(), nullptr, nullptr, nullptr, B, N, M, 1.0, lrf.data(), lrf_members.data(), 1),
            usip_shot_lrf_f32_cpu(pc.data(), nullptr, kp.data(), nullptr, B, N, M, 1.0, nullptr, lrf_members.data(), 1),
            usip_shot_hist_f32_cpu(pc.data(), nullptr, normals.data(), kp.data(), nullptr, lrf.data(), B, N, M, (double)INFINITY,
                                   hist.data(), shot.data(), kp_members.data(), 1),
            usip_shot_hist_f32_cpu(pc.data(), nullptr, nullptr, kp.data(), nullptr, lrf.data(), B, N, M, 1.0, hist.data(),
                                   shot.data(), kp_members.data(), 1),
            usip_shot_hist_f32_cpu(pc.data(), nullptr, normals.data(), kp.data(), nullptr, nullptr, B, N, M, 1.0, hist.data(),
                                   shot.data(), kp_members.data(), 1),
            usip_shot_hist_f32_cpu(pc.data(), nullptr, normals.data(), kp.data(), nullptr, lrf.data(), B, N, M, 1.0, nullptr,
                                   shot.data(), kp_members.data(), 1),
            usip_shot_hist_f32_cpu(pc.data(), nullptr, normals.data(), kp.data(), nullptr, lrf.data(), 0, N, M, 1.0, hist.data(),
                                   shot.data(), kp_members.data(), 1),
            usip_shot_hist_f32_cpu(pc.data(), nullptr, normals.data(), kp.data(), nullptr, lrf.data(), B, N, 65536, 1.0,
                                   hist.data(), shot.data(), kp_members.data(), 1)};
        for (int rcb : bad) {
            ++calls;
            if (rcb != USIP_EINVAL) { std::printf("round %d: a call outside the limits returned %d\n", round, rcb); return 1; }
            ++refused;
        }
    }
    std::printf("%d calls, %d refused as they must be, no finding\n", calls, refused);
    return 0;
}
