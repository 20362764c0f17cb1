// tests/spin_sanitize_main.cpp -- a stand-alone driver of the f-21 host twin (usip_amd/csrc/spin_cpu.cpp) for a build under
// -fsanitize=address,undefined (tests/test_spin_cpu.py compiles and runs it): random frames with counts in and out of range,
// ties along x, non-finite coordinates and normals, rows without a normal, keypoints on cloud points, outside the cloud and
// non-finite, axes of any length and rows that are no axis, both structures, with and without a support angle (without one
// the normals pointer is NULL).  Every array is sized exactly, so a read or write one element outside is reported.  Exit
// status 0: every call returned USIP_OK or, where the arguments are outside the limits, USIP_EINVAL, and every row of the
// integer image holds exactly 2^40 per member.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "../include/usip_hip.h"

int main()
{
    std::mt19937_64 rng(21);
    std::uniform_real_distribution<float> coord(-2.f, 2.f);
    int calls = 0, refused = 0;
    for (int round = 0; round < 80; ++round) {
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
        const int threads = 1 + (int)(rng() % 3), structure = round % 2;
        const double radius = round % 7 == 6 ? 100.0 : 0.5 + 0.5 * (double)(rng() % 4);
        const double support = round % 3 == 2 ? 0.0 : 0.25 * (double)(rng() % 5);             // 0, 1/4 .. 1
        std::vector<double> normals((size_t)B * 3 * N), axes((size_t)B * M * 3), spin((size_t)B * M * 153);
        for (auto& v : normals) v = (double)coord(rng);
        if (round % 4 == 1) {
            normals[rng() % normals.size()] = NAN;
            normals[rng() % normals.size()] = -INFINITY;
        }
        for (int z = 0; z < 1 + N / 8; ++z) {                             // rows without a normal
            const size_t i = rng() % ((size_t)B * N), f = i / N, s = i % N;
            for (int c = 0; c < 3; ++c) normals[(f * 3 + c) * N + s] = 0.0;
        }
        for (auto& v : axes) v = (double)coord(rng) * (round % 8 == 3 ? 1e160 : 1.0);         // (v . v overflows: no axis)
        if (round % 5 == 3) {                                             // rows that are no axis
            axes[rng() % axes.size()] = NAN;
            axes[rng() % axes.size()] = INFINITY;
            for (int c = 0; c < 3; ++c) axes[c] = 0.0;
        }
        std::vector<int32_t> kp_members((size_t)B * M);
        std::vector<int64_t> hist((size_t)B * M * 153);
        const int rc = usip_spin_image_f32_cpu(pc.data(), with_count ? count.data() : nullptr,
                                               support > 0.0 ? normals.data() : nullptr, kp.data(),
                                               with_kp_count ? kp_count.data() : nullptr, axes.data(), B, N, M, radius, support,
                                               structure, hist.data(), spin.data(), kp_members.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: returned %d\n", round, rc); return 1; }
        for (size_t q = 0; q < kp_members.size(); ++q) {
            int64_t sum = 0;
            for (int b = 0; b < 153; ++b) {
                const int64_t h = hist[q * 153 + b];
                const double s = spin[q * 153 + b];
                if (h < 0 || !(s >= 0.0 && s <= 1.0)) { std::printf("round %d: hist %lld, spin %g\n", round, (long long)h, s); return 1; }
                sum += h;
            }
            if (kp_members[q] < 0 || kp_members[q] > N || sum != (int64_t)kp_members[q] * (1LL << 40)) {
                std::printf("round %d: an image of %lld over %d members\n", round, (long long)sum, kp_members[q]);
                return 1;
            }
        }
        // outside the limits: refused before anything is read
#define SPIN(pc_, nrm_, kp_, ax_, B_, N_, M_, r_, s_, st_, h_, sp_, km_)                                                      \
    usip_spin_image_f32_cpu(pc_, nullptr, nrm_, kp_, nullptr, ax_, B_, N_, M_, r_, s_, st_, h_, sp_, km_, 1)
        const float* P = pc.data();
        const float* K = kp.data();
        const double *NR = normals.data(), *AX = axes.data();
        int64_t* H = hist.data();
        double* S = spin.data();
        int32_t* KM = kp_members.data();
        const int bad[] = {SPIN(P, NR, K, AX, B, N, M, 0.0, 0.0, 0, H, S, KM),
                           SPIN(P, NR, K, AX, B, N, M, (double)NAN, 0.0, 0, H, S, KM),
                           SPIN(P, NR, K, AX, B, N, M, (double)INFINITY, 0.0, 1, H, S, KM),
                           SPIN(P, NR, K, AX, 65536, N, M, 1.0, 0.0, 0, H, S, KM),
                           SPIN(P, NR, K, AX, 0, N, M, 1.0, 0.0, 0, H, S, KM),
                           SPIN(P, NR, K, AX, B, (1 << 20) + 1, M, 1.0, 0.0, 0, H, S, KM),
                           SPIN(P, NR, K, AX, B, N, 0, 1.0, 0.0, 0, H, S, KM),
                           SPIN(P, NR, K, AX, B, N, 65536, 1.0, 0.0, 0, H, S, KM),
                           SPIN(P, NR, K, AX, B, N, M, 1.0, -0.25, 0, H, S, KM),
                           SPIN(P, NR, K, AX, B, N, M, 1.0, 1.25, 0, H, S, KM),
                           SPIN(P, NR, K, AX, B, N, M, 1.0, (double)NAN, 0, H, S, KM),
                           SPIN(P, nullptr, K, AX, B, N, M, 1.0, 0.5, 0, H, S, KM),
                           SPIN(P, NR, K, AX, B, N, M, 1.0, 0.0, 2, H, S, KM),
                           SPIN(P, NR, K, AX, B, N, M, 1.0, 0.0, -1, H, S, KM),
                           SPIN(nullptr, NR, K, AX, B, N, M, 1.0, 0.0, 0, H, S, KM),
                           SPIN(P, NR, nullptr, AX, B, N, M, 1.0, 0.0, 0, H, S, KM),
                           SPIN(P, NR, K, nullptr, B, N, M, 1.0, 0.0, 0, H, S, KM),
                           SPIN(P, NR, K, AX, B, N, M, 1.0, 0.0, 0, nullptr, S, KM),
                           SPIN(P, NR, K, AX, B, N, M, 1.0, 0.0, 0, H, nullptr, KM),
                           SPIN(P, NR, K, AX, B, N, M, 1.0, 0.0, 0, H, S, nullptr)};
#undef SPIN
        for (int rcb : bad) {
            ++calls;
            if (rcb != USIP_EINVAL) { std::printf("round %d: a call outside the limits returned %d\n", round, rcb); return 1; }
            ++refused;
        }
    }
    std::printf("%d calls, %d refused as they must be, no finding\n", calls, refused);
    return 0;
}
