// tests/icp_plane_sanitize_main.cpp -- a stand-alone driver of the f-28 host twin (usip_icp_refine_plane_f32_cpu of
// usip_amd/csrc/icp_cpu.cpp) for a build under -fsanitize=address,undefined (tests/test_icp_plane_cpu.py compiles and runs
// it): random banks of 6 to 8 columns whose normals are unit vectors, zeros, all alike or junk, pairs with fragment ids,
// offsets, orders and masks in and out of range, every optional output given and withheld.  Every array is sized exactly, so
// a read or write one element outside is reported.  Exit status 0: every call returned USIP_OK or, where the arguments are
// outside the limits (a bank without room for normals among them), USIP_EINVAL.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "../include/usip_hip.h"

int main()
{
    std::mt19937_64 rng(28);
    std::uniform_real_distribution<float> coord(-2.f, 2.f);
    int calls = 0, refused = 0, steps = 0;
    for (int round = 0; round < 60; ++round) {
        const int F = 1 + (int)(rng() % 5), row_len = 6 + (int)(rng() % 3), P = 1 + (int)(rng() % 6);
        std::vector<int64_t> offsets((size_t)F + 1, 0);
        for (int f = 0; f < F; ++f) {
            const int choices[] = {0, 1, 3, 255, 256, 257, 40, 515};
            offsets[(size_t)f + 1] = offsets[(size_t)f] + choices[rng() % 8];
        }
        const long long total = offsets[(size_t)F];
        int Lmax = 1;
        for (int f = 0; f < F; ++f) Lmax = std::max<long long>(Lmax, offsets[(size_t)f + 1] - offsets[(size_t)f]);
        if (round % 7 == 3) Lmax = std::max(1, Lmax / 2);              // fragments longer than Lmax are cut
        std::vector<float> rows((size_t)total * row_len + 1);          // (+ 1: an empty bank still has an address)
        for (auto& v : rows) v = coord(rng);
        for (long long r = 0; r < total; ++r) {                         // the normals: unit, zero, one wall, or left as junk
            float* n = rows.data() + (size_t)r * row_len + 3;
            const int kind = round % 4;
            if (kind == 0) {
                const float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
                if (len > 0.f) { n[0] /= len; n[1] /= len; n[2] /= len; }
            } else if (kind == 1) {
                n[0] = n[1] = n[2] = 0.f;
            } else if (kind == 2) {
                n[0] = 1.f; n[1] = n[2] = 0.f;
            }
        }
        std::vector<int32_t> perm1((size_t)total + 1);
        for (auto& v : perm1) v = (int32_t)(rng() % 700) - 50;          // any value: the twin clamps what it reads
        if (round % 11 == 5) { offsets[1] = -4; offsets[(size_t)F] = total + 9; }
        std::vector<int32_t> frag1((size_t)P), frag2((size_t)P), order2((size_t)P * Lmax);
        std::vector<uint8_t> mask((size_t)P);
        std::vector<double> Rt0((size_t)P * 12, 0.0);
        for (int p = 0; p < P; ++p) {
            frag1[(size_t)p] = (int32_t)(rng() % (F + 4)) - 2;
            frag2[(size_t)p] = (int32_t)(rng() % (F + 4)) - 2;
            mask[(size_t)p] = rng() % 4 != 0;
            Rt0[(size_t)p * 12 + 0] = Rt0[(size_t)p * 12 + 5] = Rt0[(size_t)p * 12 + 10] = 1.0;
            for (int c = 0; c < 3; ++c) Rt0[(size_t)p * 12 + 4 * c + 3] = 0.1 * coord(rng);
        }
        for (auto& v : order2) v = (int32_t)(rng() % 600) - 40;
        std::vector<double> Rt((size_t)P * 12), rmse((size_t)P), ratio((size_t)P * 2), d2((size_t)P * Lmax);
        std::vector<int32_t> iterations((size_t)P), hits((size_t)P), idx((size_t)P * Lmax);
        std::vector<uint8_t> converged((size_t)P);
        const bool with_order = round % 2 == 0, with_mask = round % 3 != 0, with_out = round % 4 != 1, with_sums = round % 5 != 2;
        const int iters = (int)(rng() % 5);
        std::vector<double> cut_d2((size_t)P * (iters + 1)), fit_sums((size_t)P * iters * 27);
        std::vector<int32_t> cut_i((size_t)P * (iters + 1));
        const int threads = 1 + (int)(rng() % 3);
        const double inlier = round % 13 == 12 ? 1.0 : 0.3;
        int rc = usip_icp_refine_plane_f32_cpu(rows.data(), row_len, offsets.data(), F, total, perm1.data(), frag1.data(),
                                               frag2.data(), Rt0.data(), with_mask ? mask.data() : nullptr,
                                               with_order ? order2.data() : nullptr, P, Lmax, inlier, iters, 0.01, 0.0127, 0.05,
                                               Rt.data(), iterations.data(), converged.data(), rmse.data(), hits.data(),
                                               ratio.data(), with_out ? cut_d2.data() : nullptr,
                                               with_out ? cut_i.data() : nullptr, with_out ? idx.data() : nullptr,
                                               with_out ? d2.data() : nullptr, with_sums ? fit_sums.data() : nullptr, threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: refine returned %d\n", round, rc); return 1; }
        for (int p = 0; p < P; ++p) {
            if (iterations[(size_t)p] < 0 || iterations[(size_t)p] > iters) { std::printf("round %d: iterations\n", round); return 1; }
            steps += iterations[(size_t)p];
            for (int k = 0; k < 12; ++k)
                if (!std::isfinite(Rt[(size_t)p * 12 + k])) { std::printf("round %d: a pose that is not finite\n", round); return 1; }
        }
        // outside the limits: refused before anything is read
        const int bad[] = {usip_icp_refine_plane_f32_cpu(rows.data(), 5, offsets.data(), F, total, perm1.data(), frag1.data(),
                                                         frag2.data(), Rt0.data(), nullptr, nullptr, P, Lmax, 0.3, 1, 0.01,
                                                         0.01, 0.05, Rt.data(), iterations.data(), converged.data(),
                                                         rmse.data(), hits.data(), ratio.data(), nullptr, nullptr, nullptr,
                                                         nullptr, nullptr, 1),
                           usip_icp_refine_plane_f32_cpu(rows.data(), 3, offsets.data(), F, total, perm1.data(), frag1.data(),
                                                         frag2.data(), Rt0.data(), nullptr, nullptr, P, Lmax, 0.3, 1, 0.01,
                                                         0.01, 0.05, Rt.data(), iterations.data(), converged.data(),
                                                         rmse.data(), hits.data(), ratio.data(), nullptr, nullptr, nullptr,
                                                         nullptr, nullptr, 1),
                           usip_icp_refine_plane_f32_cpu(rows.data(), row_len, offsets.data(), F, total, perm1.data(),
                                                         frag1.data(), frag2.data(), Rt0.data(), nullptr, nullptr, P, Lmax, 0.3,
                                                         65, 0.01, 0.01, 0.05, Rt.data(), iterations.data(), converged.data(),
                                                         rmse.data(), hits.data(), ratio.data(), nullptr, nullptr, nullptr,
                                                         nullptr, nullptr, 1)};
        for (int rcb : bad) {
            ++calls;
            if (rcb != USIP_EINVAL) { std::printf("round %d: a call outside the limits returned %d\n", round, rcb); return 1; }
            ++refused;
        }
    }
    if (steps == 0) { std::printf("no fit ever took a step\n"); return 1; }
    std::printf("%d calls, %d refused as they must be, %d steps taken, no finding\n", calls, refused, steps);
    return 0;
}
