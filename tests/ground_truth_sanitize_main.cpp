// tests/ground_truth_sanitize_main.cpp -- a stand-alone driver of the f-18 host twins (usip_amd/csrc/ground_truth_cpu.cpp)
// for a build under -fsanitize=address,undefined (tests/test_ground_truth_cpu.py compiles and runs it): the tile-edge lengths
// (0, 1, 255, 256, 257, 513, 600) and the selection shapes (cap 7 against 6, 7, 8 and 300 near rows), with fragment ids,
// offsets, permutations, orders and counts in and out of range.  Every output array is sized exactly, so a write one element
// outside is reported (rows and perm1 carry one spare element, so that an empty bank is not a NULL).  Exit status 0: every
// call returned USIP_OK or, where the arguments are outside the limits, USIP_EINVAL.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>
#include "../include/usip_hip.h"

int main()
{
    std::mt19937_64 rng(18);
    std::uniform_real_distribution<float> coord(-0.05f, 0.05f);
    int calls = 0, refused = 0;
    for (int round = 0; round < 48; ++round) {
        const int F = 1 + (int)(rng() % 6), row_len = 3 + (int)(rng() % 3), P = 1 + (int)(rng() % 7);
        std::vector<int64_t> offsets((size_t)F + 1, 0);
        for (int f = 0; f < F; ++f) {
            const int choices[] = {0, 1, 255, 256, 257, 513, 600, 6, 7, 8, 300};
            offsets[(size_t)f + 1] = offsets[(size_t)f] + choices[rng() % 11];
        }
        const long long total = offsets[(size_t)F];
        int Lmax = 1;
        for (int f = 0; f < F; ++f) Lmax = std::max<long long>(Lmax, offsets[(size_t)f + 1] - offsets[(size_t)f]);
        if (round % 7 == 3) Lmax = std::max(1, Lmax / 2);              // fragments longer than Lmax are cut
        std::vector<float> rows((size_t)total * row_len + 1);              // (+ 1: never a NULL for an empty bank)
        for (auto& v : rows) v = round % 5 == 4 ? (float)(int)(coord(rng) * 200.f) / 200.f : coord(rng);     // duplicates
        std::vector<int32_t> perm1((size_t)total + 1);
        if (round % 3 == 0) {
            for (auto& v : perm1) v = (int32_t)(rng() % 700) - 50;      // any value: the twin clamps what it reads
        } else {                                                       // a real order along x per fragment
            for (int f = 0; f < F; ++f) {
                const long long lo = offsets[(size_t)f], n = offsets[(size_t)f + 1] - lo;
                std::iota(perm1.begin() + lo, perm1.begin() + lo + n, 0);
                std::stable_sort(perm1.begin() + lo, perm1.begin() + lo + n, [&](int32_t a, int32_t b) {
                    return rows[(size_t)(lo + a) * row_len] < rows[(size_t)(lo + b) * row_len];
                });
            }
        }
        if (round % 11 == 5) { offsets[1] = -4; offsets[(size_t)F] = total + 9; }
        std::vector<int32_t> frag1((size_t)P), frag2((size_t)P);
        std::vector<uint8_t> mask((size_t)P);
        std::vector<int64_t> ids((size_t)P);
        std::vector<double> Rt((size_t)P * 12, 0.0);
        for (int p = 0; p < P; ++p) {
            frag1[(size_t)p] = (int32_t)(rng() % (F + 4)) - 2;
            frag2[(size_t)p] = (int32_t)(rng() % (F + 4)) - 2;
            mask[(size_t)p] = rng() % 4 != 0;
            ids[(size_t)p] = (int64_t)rng();
            Rt[(size_t)p * 12 + 0] = Rt[(size_t)p * 12 + 5] = Rt[(size_t)p * 12 + 10] = 1.0;
            for (int c = 0; c < 3; ++c) Rt[(size_t)p * 12 + 4 * c + 3] = 0.05 * coord(rng);
        }
        std::vector<uint8_t> cls((size_t)P * Lmax);
        std::vector<uint64_t> key((size_t)P * Lmax);
        std::vector<int32_t> hits((size_t)P * 2);
        std::vector<double> ratio((size_t)P * 2), info((size_t)P * 36);
        const bool with_mask = round % 3 != 0, with_ids = round % 2 == 0;
        const int threads = 1 + (int)(rng() % 3), prune = round % 4 != 1;
        int rc = usip_gt_reach_f32_cpu(rows.data(), row_len, offsets.data(), F, total, perm1.data(), frag1.data(), frag2.data(),
                                       Rt.data(), with_mask ? mask.data() : nullptr, P, Lmax, 0.03, 0.006, rng(),
                                       with_ids ? ids.data() : nullptr, prune, cls.data(), hits.data(), ratio.data(), key.data(),
                                       threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: reach returned %d\n", round, rc); return 1; }
        for (int p = 0; p < P; ++p) {
            int far = 0, near = 0;
            for (int s = 0; s < Lmax; ++s) {
                const uint8_t c = cls[(size_t)p * Lmax + s];
                if (c > 2 || (c == 2) != (key[(size_t)p * Lmax + s] != ~0ull)) {
                    std::printf("round %d: a class or key out of shape\n", round);
                    return 1;
                }
                far += c >= 1;
                near += c == 2;
            }
            if (hits[(size_t)2 * p] != far || hits[(size_t)2 * p + 1] != near) {
                std::printf("round %d: hits disagree with cls\n", round);
                return 1;
            }
        }
        // the selection: cap 7 and a cap above every count; the order holds any value, the count any number
        for (const int cap : {7, 1, 65536 < Lmax ? 65536 : Lmax}) {
            std::vector<int32_t> order((size_t)P * cap), count((size_t)P);
            for (auto& v : order) v = (int32_t)(rng() % 700) - 50;
            for (int p = 0; p < P; ++p) count[(size_t)p] = round % 2 ? hits[(size_t)2 * p + 1] : (int32_t)(rng() % 900) - 100;
            rc = usip_gt_information_f32_cpu(rows.data(), row_len, offsets.data(), F, total, frag2.data(), Rt.data(), order.data(),
                                             count.data(), P, Lmax, cap, info.data(), threads);
            ++calls;
            if (rc != USIP_OK) { std::printf("round %d: information returned %d\n", round, rc); return 1; }
            for (double v : info)
                if (!(v == v)) { std::printf("round %d: a NaN in info\n", round); return 1; }
        }
        // outside the limits: refused before anything is read
        std::vector<int32_t> order(7), count((size_t)P);
        const int bad[] = {
            usip_gt_reach_f32_cpu(rows.data(), 2, offsets.data(), F, total, perm1.data(), frag1.data(), frag2.data(), Rt.data(),
                                  nullptr, P, Lmax, 0.03, 0.006, 0, nullptr, 1, cls.data(), hits.data(), ratio.data(), key.data(), 1),
            usip_gt_reach_f32_cpu(rows.data(), row_len, offsets.data(), F, total, perm1.data(), frag1.data(), frag2.data(),
                                  Rt.data(), nullptr, P, Lmax, 0.006, 0.006, 0, nullptr, 1, cls.data(), hits.data(), ratio.data(),
                                  key.data(), 1),
            usip_gt_reach_f32_cpu(rows.data(), row_len, offsets.data(), F, total, perm1.data(), frag1.data(), frag2.data(),
                                  Rt.data(), nullptr, P, Lmax, 0.03, 0.0, 0, nullptr, 1, cls.data(), hits.data(), ratio.data(),
                                  key.data(), 1),
            usip_gt_reach_f32_cpu(rows.data(), row_len, offsets.data(), F, total, perm1.data(), frag1.data(), frag2.data(),
                                  Rt.data(), nullptr, 65536, Lmax, 0.03, 0.006, 0, nullptr, 1, cls.data(), hits.data(),
                                  ratio.data(), key.data(), 1),
            usip_gt_reach_f32_cpu(rows.data(), row_len, offsets.data(), F, total, nullptr, frag1.data(), frag2.data(), Rt.data(),
                                  nullptr, P, Lmax, 0.03, 0.006, 0, nullptr, 1, cls.data(), hits.data(), ratio.data(), key.data(), 1),
            usip_gt_information_f32_cpu(rows.data(), row_len, offsets.data(), F, total, frag2.data(), Rt.data(), order.data(),
                                        count.data(), P, Lmax, 0, info.data(), 1),
            usip_gt_information_f32_cpu(rows.data(), row_len, offsets.data(), F, total, frag2.data(), Rt.data(), order.data(),
                                        count.data(), P, Lmax, 65537, info.data(), 1),
            usip_gt_information_f32_cpu(rows.data(), row_len, offsets.data(), F, total, frag2.data(), Rt.data(), nullptr,
                                        count.data(), P, Lmax, 7, info.data(), 1)};
        for (int rcb : bad) {
            ++calls;
            if (rcb != USIP_EINVAL) { std::printf("round %d: a call outside the limits returned %d\n", round, rcb); return 1; }
            ++refused;
        }
    }
    std::printf("%d calls, %d refused as they must be, no finding\n", calls, refused);
    return 0;
}
