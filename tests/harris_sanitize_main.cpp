// tests/harris_sanitize_main.cpp -- a stand-alone driver of the f-16 host twin (usip_amd/csrc/harris_cpu.cpp) for a build
// under -fsanitize=address,undefined (tests/test_harris_cpu.py compiles and runs it): random frames with counts in and out of
// range, ties along x, non-finite coordinates and normals, every response.  Every array is sized exactly, so a read or write
// one element outside is reported.  Exit status 0: every call returned USIP_OK or, where the arguments are outside the limits,
// USIP_EINVAL.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "../include/usip_hip.h"

int main()
{
    std::mt19937_64 rng(16);
    std::uniform_real_distribution<float> coord(-2.f, 2.f);
    int calls = 0, refused = 0;
    for (int round = 0; round < 60; ++round) {
        const int sizes[] = {1, 2, 3, 40, 255, 256, 257, 515};
        const int B = 1 + (int)(rng() % 3), N = sizes[rng() % 8];
        std::vector<float> pc((size_t)B * 3 * N);
        for (auto& v : pc) v = round % 5 == 4 ? (float)(int)(coord(rng) * 4.f) / 4.f : coord(rng);       // ties
        if (round % 9 == 8) pc[rng() % pc.size()] = NAN;
        if (round % 9 == 7) pc[rng() % pc.size()] = INFINITY;
        std::vector<int32_t> count((size_t)B);
        for (auto& c : count) c = (int32_t)(rng() % (N + 6)) - 3;         // below 0 and above N: clamped
        const bool with_count = round % 3 != 0;
        const int threads = 1 + (int)(rng() % 3), min_neighbors = 1 + (int)(rng() % 5), method = (int)(rng() % 4);
        const double radius = round % 7 == 6 ? 100.0 : 0.5 + 0.25 * (double)(rng() % 4);
        std::vector<double> normals((size_t)B * 3 * N), response((size_t)B * N);
        std::vector<int32_t> neighbours((size_t)B * N), members((size_t)B * N);
        int rc = usip_harris_normals_f32_cpu(pc.data(), with_count ? count.data() : nullptr, B, N, radius, min_neighbors,
                                             normals.data(), neighbours.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: normals returned %d\n", round, rc); return 1; }
        if (round % 4 == 1) {                                          // supplied normals: anything, non-finite and zero rows too
            for (auto& v : normals) v = (double)coord(rng);
            normals[rng() % normals.size()] = NAN;
            normals[rng() % normals.size()] = -INFINITY;
            const size_t i = rng() % ((size_t)B * N), f = i / N, s = i % N;
            for (int c = 0; c < 3; ++c) normals[(f * 3 + c) * N + s] = 0.0;
        }
        rc = usip_harris_response_f32_cpu(pc.data(), with_count ? count.data() : nullptr, normals.data(), B, N, radius, method,
                                          response.data(), members.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: response returned %d\n", round, rc); return 1; }
        for (size_t i = 0; i < response.size(); ++i)
            if (!(std::fabs(response[i]) < INFINITY) || members[i] < 0 || members[i] > N) {
                std::printf("round %d: response %g, members %d at %zu\n", round, response[i], members[i], i);
                return 1;
            }
        // outside the limits: refused before anything is read
        const int bad[] = {
            usip_harris_normals_f32_cpu(pc.data(), nullptr, B, N, 0.0, 3, normals.data(), neighbours.data(), 1),
            usip_harris_normals_f32_cpu(pc.data(), nullptr, B, N, 1.0, 0, normals.data(), neighbours.data(), 1),
            usip_harris_normals_f32_cpu(pc.data(), nullptr, 65536, N, 1.0, 3, normals.data(), neighbours.data(), 1),
            usip_harris_normals_f32_cpu(pc.data(), nullptr, B, (1 << 20) + 1, 1.0, 3, normals.data(), neighbours.data(), 1),
            usip_harris_normals_f32_cpu(pc.data(), nullptr, B, N, (double)NAN, 3, normals.data(), neighbours.data(), 1),
            usip_harris_response_f32_cpu(pc.data(), nullptr, normals.data(), B, N, (double)INFINITY, 0, response.data(),
                                         members.data(), 1),
            usip_harris_response_f32_cpu(pc.data(), nullptr, normals.data(), B, N, 1.0, 4, response.data(), members.data(), 1),
            usip_harris_response_f32_cpu(pc.data(), nullptr, normals.data(), B, N, 1.0, -1, response.data(), members.data(), 1),
            usip_harris_response_f32_cpu(pc.data(), nullptr, nullptr, B, N, 1.0, 0, response.data(), members.data(), 1),
            usip_harris_response_f32_cpu(pc.data(), nullptr, normals.data(), 0, N, 1.0, 0, response.data(), members.data(), 1)};
        for (int rcb : bad) {
            ++calls;
            if (rcb != USIP_EINVAL) { std::printf("round %d: a call outside the limits returned %d\n", round, rcb); return 1; }
            ++refused;
        }
    }
    std::printf("%d calls, %d refused as they must be, no finding\n", calls, refused);
    return 0;
}
