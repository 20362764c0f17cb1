// tests/cgf_sanitize_main.cpp -- a stand-alone driver of the f-22 host twin (usip_amd/csrc/cgf_loss_cpu.cpp) for a build under
// -fsanitize=address,undefined (tests/test_cgf_loss_cpu.py compiles and runs it): random batch elements with M and C at and
// around the lane and workgroup widths, explicit and Philox draws, keypoints with ties and non-finite coordinates, non-finite
// descriptors and sigmas, and -- between the selection and the loss -- indices overwritten with values far outside 0 .. M-1,
// which the loss and the backward must clamp.  Every array is sized exactly, so a read or write one element outside is
// reported.  Exit status 0: every call returned USIP_OK or, where the arguments are outside the limits, USIP_EINVAL, and every
// selected index lies in 0 .. M-1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "../include/usip_hip.h"

int main()
{
    std::mt19937_64 rng(22);
    std::uniform_real_distribution<float> coord(-2.f, 2.f), unif(0.f, 1.f);
    int calls = 0, refused = 0;
    for (int round = 0; round < 60; ++round) {
        const int ms[] = {1, 2, 3, 63, 64, 65, 130, 257}, cs[] = {1, 3, 64, 65, 130};
        const int B = 1 + (int)(rng() % 3), M = ms[rng() % 8], C = cs[rng() % 5], threads = 1 + (int)(rng() % 4);
        const size_t BM = (size_t)B * M;
        std::vector<float> akp(BM * 3), pkp(BM * 3), ad(BM * C), pd(BM * C), sigma(BM), grad(BM);
        for (auto& v : akp) v = round % 5 == 4 ? (float)(int)(coord(rng) * 2.f) / 2.f : coord(rng);          // ties
        for (auto& v : pkp) v = round % 5 == 4 ? (float)(int)(coord(rng) * 2.f) / 2.f : coord(rng);
        if (round % 7 == 6) { akp[rng() % akp.size()] = NAN; pkp[rng() % pkp.size()] = INFINITY; }
        for (auto& v : ad) v = coord(rng);
        for (auto& v : pd) v = coord(rng);
        if (round % 6 == 5) { ad[rng() % ad.size()] = NAN; pd[rng() % pd.size()] = -INFINITY; }
        if (round % 4 == 3) for (int c = 0; c < C; ++c) pd[(size_t)c * M] = ad[(size_t)c * M];               // a zero distance
        for (auto& v : sigma) v = 1.5f * unif(rng);
        if (round % 8 == 7) sigma[rng() % sigma.size()] = NAN;
        if (round % 9 == 8) for (auto& v : sigma) v = 2.f;                                                   // no weight at all
        for (auto& v : grad) v = coord(rng);
        const bool explicit_draws = round % 2 == 0;
        std::vector<float> u1(explicit_draws ? BM * M : 0), u2(u1.size()), u3(explicit_draws ? BM : 0);
        for (auto& v : u1) v = unif(rng);
        for (auto& v : u2) v = unif(rng);
        for (auto& v : u3) v = unif(rng);
        const double radius = round % 3 == 0 ? 100.0 : (round % 3 == 1 ? 1e-3 : 1.5);                       // all inside, none, mixed
        std::vector<int32_t> sel(BM * 3);
        std::vector<uint8_t> has(BM), take_far(BM);
        int rc = usip_cgf_select_f32_cpu(akp.data(), pkp.data(), B, M, radius, explicit_draws ? u1.data() : nullptr,
                                         explicit_draws ? u2.data() : nullptr, explicit_draws ? u3.data() : nullptr, rng(), rng(),
                                         rng(), sel.data(), has.data(), take_far.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: the selection returned %d\n", round, rc); return 1; }
        for (size_t k = 0; k < sel.size(); ++k)
            if (sel[k] < 0 || sel[k] >= M || has[k / 3] > 1 || take_far[k / 3] > 1) {
                std::printf("round %d: index %d of %d\n", round, sel[k], M);
                return 1;
            }
        if (round % 3 == 2) {                                             // indices from anywhere: clamped
            sel[rng() % sel.size()] = -7;
            sel[rng() % sel.size()] = INT32_MAX;
            sel[rng() % sel.size()] = M;
            sel[rng() % sel.size()] = INT32_MIN;
        }
        std::vector<float> loss(BM), active((size_t)B), d_anc(BM * C), d_pos(BM * C);
        std::vector<double> dist(BM * 2), coef(BM);
        rc = usip_cgf_loss_f32_cpu(ad.data(), pd.data(), sigma.data(), sel.data(), has.data(), take_far.data(), B, M, C, 0.5, 1.0,
                                   loss.data(), active.data(), dist.data(), coef.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: the loss returned %d\n", round, rc); return 1; }
        rc = usip_cgf_loss_backward_f32_cpu(ad.data(), pd.data(), sel.data(), take_far.data(), dist.data(), coef.data(),
                                            grad.data(), B, M, C, d_anc.data(), d_pos.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: the backward returned %d\n", round, rc); return 1; }
        if (round % 6 != 5 && round % 7 != 6 && round % 8 != 7)           // finite inputs: finite outputs
            for (size_t k = 0; k < d_anc.size(); ++k)
                if (!std::isfinite(d_anc[k]) || !std::isfinite(d_pos[k]) || !std::isfinite(loss[k / C])) {
                    std::printf("round %d: a non-finite result from finite inputs\n", round);
                    return 1;
                }
        // outside the limits: refused before anything is read
        const float *AK = akp.data(), *PK = pkp.data(), *AD = ad.data(), *PD = pd.data(), *SG = sigma.data(), *G = grad.data();
        int32_t* S = sel.data();
        uint8_t *H = has.data(), *T = take_far.data();
        const int bad[] = {
            usip_cgf_select_f32_cpu(AK, PK, 0, M, 1.0, nullptr, nullptr, nullptr, 0, 0, 0, S, H, T, 1),
            usip_cgf_select_f32_cpu(AK, PK, B, 0, 1.0, nullptr, nullptr, nullptr, 0, 0, 0, S, H, T, 1),
            usip_cgf_select_f32_cpu(AK, PK, B, 65536, 1.0, nullptr, nullptr, nullptr, 0, 0, 0, S, H, T, 1),
            usip_cgf_select_f32_cpu(AK, PK, B, M, 0.0, nullptr, nullptr, nullptr, 0, 0, 0, S, H, T, 1),
            usip_cgf_select_f32_cpu(AK, PK, B, M, (double)NAN, nullptr, nullptr, nullptr, 0, 0, 0, S, H, T, 1),
            usip_cgf_select_f32_cpu(AK, PK, B, M, 1.0, AK, nullptr, nullptr, 0, 0, 0, S, H, T, 1),
            usip_cgf_select_f32_cpu(nullptr, PK, B, M, 1.0, nullptr, nullptr, nullptr, 0, 0, 0, S, H, T, 1),
            usip_cgf_select_f32_cpu(AK, PK, B, M, 1.0, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, H, T, 1),
            usip_cgf_loss_f32_cpu(AD, PD, SG, S, H, T, B, M, 0, 0.5, 1.0, loss.data(), active.data(), dist.data(), coef.data(), 1),
            usip_cgf_loss_f32_cpu(AD, PD, SG, S, H, T, B, M, 4097, 0.5, 1.0, loss.data(), active.data(), dist.data(), coef.data(), 1),
            usip_cgf_loss_f32_cpu(AD, PD, SG, S, H, T, B, 65536, C, 0.5, 1.0, loss.data(), active.data(), dist.data(), coef.data(), 1),
            usip_cgf_loss_f32_cpu(AD, PD, nullptr, S, H, T, B, M, C, 0.5, 1.0, loss.data(), active.data(), dist.data(), coef.data(), 1),
            usip_cgf_loss_f32_cpu(AD, PD, SG, S, H, T, B, M, C, 0.5, 1.0, loss.data(), active.data(), nullptr, coef.data(), 1),
            usip_cgf_loss_backward_f32_cpu(AD, PD, S, T, dist.data(), coef.data(), G, B, M, 0, d_anc.data(), d_pos.data(), 1),
            usip_cgf_loss_backward_f32_cpu(AD, PD, S, T, dist.data(), coef.data(), G, 0, M, C, d_anc.data(), d_pos.data(), 1),
            usip_cgf_loss_backward_f32_cpu(AD, PD, S, T, dist.data(), coef.data(), nullptr, B, M, C, d_anc.data(), d_pos.data(), 1),
            usip_cgf_loss_backward_f32_cpu(AD, PD, S, T, dist.data(), coef.data(), G, B, M, C, d_anc.data(), nullptr, 1)};
        for (int rcb : bad) {
            ++calls;
            if (rcb != USIP_EINVAL) { std::printf("round %d: a call outside the limits returned %d\n", round, rcb); return 1; }
            ++refused;
        }
    }
    std::printf("%d calls, %d refused as they must be, no finding\n", calls, refused);
    return 0;
}
