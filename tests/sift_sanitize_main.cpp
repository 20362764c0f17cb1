// tests/sift_sanitize_main.cpp -- a stand-alone driver of the f-17 host twin (usip_amd/csrc/sift_cpu.cpp) for a build under
// -fsanitize=address,undefined (tests/test_sift_cpu.py compiles and runs it): random frames with counts in and out of range,
// ties (coordinates on a coarse lattice, so cells, distances and DoG values repeat), non-finite coordinates, cells outside the
// key range, every S, supplied and axis fields; the stages are chained as usip_amd/baselines.py chains them and also fed raw
// frames.  Every array is sized exactly, so a read or write one element outside is reported.  Exit status 0: every call
// returned USIP_OK or, where the arguments are outside the limits, USIP_EINVAL.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "../include/usip_hip.h"

int main()
{
    std::mt19937_64 rng(17);
    std::uniform_real_distribution<float> coord(-3.f, 3.f);
    int calls = 0, refused = 0;
    for (int round = 0; round < 60; ++round) {
        const int sizes[] = {1, 2, 24, 25, 26, 255, 256, 257, 515};
        const int B = 1 + (int)(rng() % 3), N = sizes[rng() % 9];
        std::vector<float> pc((size_t)B * 3 * N), field((size_t)B * N);
        for (auto& v : pc) v = round % 5 == 4 ? (float)(int)(coord(rng) * 2.f) / 2.f : coord(rng);       // ties
        for (auto& v : field) v = coord(rng);
        if (round % 9 == 8) pc[rng() % pc.size()] = NAN;
        if (round % 9 == 7) pc[rng() % pc.size()] = INFINITY;
        if (round % 9 == 6) pc[rng() % pc.size()] = 3.0e30f;              // a cell index far outside the key range
        std::vector<int32_t> count((size_t)B);
        for (auto& c : count) c = (int32_t)(rng() % (N + 6)) - 3;         // below 0 and above N: clamped
        const bool with_count = round % 3 != 0, supplied = round % 2 == 1;
        const int threads = 1 + (int)(rng() % 3), S = 4 + (int)(rng() % 8), axis = (int)(rng() % 3);
        const double leaf = round % 7 == 6 ? 100.0 : 0.125 * (double)(1 + rng() % 4), contrast = 0.01 * (double)(rng() % 4);
        const int32_t* cnt = with_count ? count.data() : nullptr;
        std::vector<double> sigma2((size_t)S);
        for (int s = 0; s < S; ++s) sigma2[s] = leaf * leaf * std::pow(2.0, 2.0 * (s - 1) / (double)(S - 3));

        std::vector<int64_t> keys((size_t)B * N);
        std::vector<float> cloud((size_t)B * 3 * N), cfield((size_t)B * N);
        std::vector<int32_t> ccount((size_t)B);
        int rc = usip_sift_voxel_keys_f32_cpu(pc.data(), cnt, B, N, leaf, keys.data());
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: keys returned %d\n", round, rc); return 1; }
        rc = usip_sift_voxel_average_f32_cpu(pc.data(), supplied ? field.data() : nullptr, axis, keys.data(), B, N, cloud.data(),
                                             cfield.data(), ccount.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: average returned %d\n", round, rc); return 1; }
        for (int f = 0; f < B; ++f)
            if (ccount[f] < 0 || ccount[f] > (with_count && count[f] < N ? (count[f] < 0 ? 0 : count[f]) : N)) {
                std::printf("round %d: %d cells from %d points\n", round, ccount[f], with_count ? count[f] : N);
                return 1;
            }
        // the octave cloud, and on odd rounds the raw frame with its raw count (non-finite rows included)
        const bool raw = round % 4 == 3;
        const float* p = raw ? pc.data() : cloud.data();
        const float* fl = raw ? field.data() : cfield.data();
        const int32_t* c = raw ? cnt : ccount.data();
        std::vector<double> dog((size_t)B * (S - 1) * N);
        std::vector<int32_t> idx((size_t)B * N * 25), scale((size_t)B * N);
        std::vector<uint8_t> mask((size_t)B * N);
        rc = usip_sift_dog_f32_cpu(p, fl, c, B, N, S, sigma2.data(), dog.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: dog returned %d\n", round, rc); return 1; }
        rc = usip_sift_nearest_f32_cpu(p, c, B, N, idx.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: nearest returned %d\n", round, rc); return 1; }
        if (round % 6 == 5) idx[rng() % idx.size()] = round % 12 == 5 ? -9 : 1 << 30;      // a wrong list: clamped, not followed
        rc = usip_sift_extrema_f32_cpu(dog.data(), idx.data(), c, B, N, S, contrast, mask.data(), scale.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: extrema returned %d\n", round, rc); return 1; }
        for (size_t i = 0; i < mask.size(); ++i)
            if (mask[i] > 1 || scale[i] < 0 || scale[i] > S - 3 || (mask[i] != 0) != (scale[i] != 0)) {
                std::printf("round %d: mask %d, scale %d at %zu\n", round, mask[i], scale[i], i);
                return 1;
            }
        double e[3] = {-4.5, -0.3, 0.0}, eo[3];
        // outside the limits: refused before anything is read
        std::vector<double> down(sigma2);
        down[1] = down[0] * 0.5;
        const int bad[] = {
            usip_sift_voxel_keys_f32_cpu(pc.data(), nullptr, B, N, 0.0, keys.data()),
            usip_sift_voxel_keys_f32_cpu(pc.data(), nullptr, B, N, (double)NAN, keys.data()),
            usip_sift_voxel_keys_f32_cpu(pc.data(), nullptr, B, N, (double)INFINITY, keys.data()),
            usip_sift_voxel_keys_f32_cpu(pc.data(), nullptr, 65536, N, 0.5, keys.data()),
            usip_sift_voxel_keys_f32_cpu(pc.data(), nullptr, B, (1 << 20) + 1, 0.5, keys.data()),
            usip_sift_voxel_average_f32_cpu(pc.data(), nullptr, 3, keys.data(), B, N, cloud.data(), cfield.data(), ccount.data(), 1),
            usip_sift_voxel_average_f32_cpu(pc.data(), nullptr, -1, keys.data(), B, N, cloud.data(), cfield.data(), ccount.data(), 1),
            usip_sift_voxel_average_f32_cpu(pc.data(), nullptr, 0, nullptr, B, N, cloud.data(), cfield.data(), ccount.data(), 1),
            usip_sift_dog_f32_cpu(p, fl, c, B, N, 3, sigma2.data(), dog.data(), 1),
            usip_sift_dog_f32_cpu(p, fl, c, B, N, 12, sigma2.data(), dog.data(), 1),
            usip_sift_dog_f32_cpu(p, fl, c, B, N, S, down.data(), dog.data(), 1),
            usip_sift_dog_f32_cpu(p, fl, c, B, N, S, nullptr, dog.data(), 1),
            usip_sift_dog_f32_cpu(p, nullptr, c, B, N, S, sigma2.data(), dog.data(), 1),
            usip_sift_nearest_f32_cpu(p, c, 0, N, idx.data(), 1),
            usip_sift_nearest_f32_cpu(p, c, B, N, nullptr, 1),
            usip_sift_extrema_f32_cpu(dog.data(), idx.data(), c, B, N, S, -0.1, mask.data(), scale.data(), 1),
            usip_sift_extrema_f32_cpu(dog.data(), idx.data(), c, B, N, S, (double)NAN, mask.data(), scale.data(), 1),
            usip_sift_extrema_f32_cpu(dog.data(), idx.data(), c, B, N, 3, 0.1, mask.data(), scale.data(), 1),
            usip_sift_exp_f64_cpu(e, -1, eo)};
        for (int rcb : bad) {
            ++calls;
            if (rcb != USIP_EINVAL) { std::printf("round %d: a call outside the limits returned %d\n", round, rcb); return 1; }
            ++refused;
        }
        if (usip_sift_exp_f64_cpu(e, 3, eo) != USIP_OK || eo[2] != 1.0 || !(eo[0] > 0.0111 && eo[0] < 0.0112)) {
            std::printf("round %d: sift_exp gives %g, %g, %g\n", round, eo[0], eo[1], eo[2]);
            return 1;
        }
        ++calls;
    }
    std::printf("%d calls, %d refused as they must be, no finding\n", calls, refused);
    return 0;
}
