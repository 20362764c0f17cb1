// tests/unit_sanitize_main.cpp -- a stand-alone driver of the f-25 host twin (usip_amd/csrc/unit_columns_cpu.cpp) for a build
// under -fsanitize=address,undefined (tests/test_unit_columns_cpu.py compiles and runs it): random shapes with C and M at and
// around the lane width, zero columns, non-finite values, huge values, one to several threads.  Every array is sized exactly,
// so a read or write one element outside is reported.  Exit status 0: every call returned USIP_OK or, where the arguments are
// outside the limits, USIP_EINVAL; finite inputs gave finite outputs of unit length.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "../include/usip_hip.h"

int main()
{
    std::mt19937_64 rng(25);
    std::uniform_real_distribution<float> value(-2.f, 2.f);
    int calls = 0, refused = 0;
    for (int round = 0; round < 80; ++round) {
        const int cs[] = {0, 1, 3, 64, 65, 130}, ms[] = {1, 2, 63, 64, 65, 130};
        const int B = (int)(rng() % 4), C = cs[rng() % 6], M = ms[rng() % 6], threads = 1 + (int)(rng() % 5);
        const size_t rows = (size_t)B * M, total = rows * C;
        const size_t nt = total ? total : 1, nr = rows ? rows : 1;        // (an empty vector may hand out NULL, which is refused)
        std::vector<float> x(nt), g(nt), out(nt), dx(nt), norm(nr);
        for (auto& v : x) v = value(rng);
        for (auto& v : g) v = value(rng);
        const bool finite = round % 4 != 3;
        if (total && round % 3 == 1)                                      // a zero column
            for (int c = 0; c < C; ++c) x[(size_t)c * M] = 0.f;
        if (total && round % 5 == 2)                                      // a huge column
            for (int c = 0; c < C; ++c) x[(size_t)c * M + (M - 1)] = 1e30f;
        if (total && !finite) {
            x[rng() % total] = NAN;
            x[rng() % total] = INFINITY;
            g[rng() % total] = -INFINITY;
        }
        const float eps = round % 7 == 6 ? 0.f : 1e-5f;
        int rc = usip_unit_columns_f32_cpu(x.data(), B, C, M, eps, out.data(), norm.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: the forward returned %d\n", round, rc); return 1; }
        rc = usip_unit_columns_backward_f32_cpu(g.data(), x.data(), norm.data(), B, C, M, eps, dx.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: the backward returned %d\n", round, rc); return 1; }
        if (finite && eps > 0.f)
            for (size_t r = 0; r < rows && C > 0; ++r) {
                const size_t b = r / M, m = r % M;
                double s = 0.0;
                for (int c = 0; c < C; ++c) {
                    const float o = out[(b * C + c) * M + m], d = dx[(b * C + c) * M + m];
                    if (!std::isfinite(o) || !std::isfinite(d)) { std::printf("round %d: a non-finite result\n", round); return 1; }
                    s += (double)o * o;
                }
                if (norm[r] > 1.f && std::fabs(std::sqrt(s) - 1.0) > 1e-4) {
                    std::printf("round %d: a column of length %g\n", round, std::sqrt(s));
                    return 1;
                }
            }
        // outside the limits: refused before anything is read
        const float *X = x.data(), *G = g.data(), *N = norm.data();
        float *O = out.data(), *D = dx.data(), *W = norm.data();
        const int bad[] = {usip_unit_columns_f32_cpu(X, -1, C, M, eps, O, W, 1),
                           usip_unit_columns_f32_cpu(X, B, -1, M, eps, O, W, 1),
                           usip_unit_columns_f32_cpu(X, B, C, -1, eps, O, W, 1),
                           usip_unit_columns_f32_cpu(X, B, C, M, -1.f, O, W, 1),
                           usip_unit_columns_f32_cpu(X, B, C, M, NAN, O, W, 1),
                           usip_unit_columns_f32_cpu(nullptr, B, C, M, eps, O, W, 1),
                           usip_unit_columns_f32_cpu(X, B, C, M, eps, nullptr, W, 1),
                           usip_unit_columns_f32_cpu(X, B, C, M, eps, O, nullptr, 1),
                           usip_unit_columns_backward_f32_cpu(G, X, N, -1, C, M, eps, D, 1),
                           usip_unit_columns_backward_f32_cpu(G, X, N, B, C, -5, eps, D, 1),
                           usip_unit_columns_backward_f32_cpu(G, X, N, B, C, M, -1.f, D, 1),
                           usip_unit_columns_backward_f32_cpu(nullptr, X, N, B, C, M, eps, D, 1),
                           usip_unit_columns_backward_f32_cpu(G, nullptr, N, B, C, M, eps, D, 1),
                           usip_unit_columns_backward_f32_cpu(G, X, nullptr, B, C, M, eps, D, 1),
                           usip_unit_columns_backward_f32_cpu(G, X, N, B, C, M, eps, nullptr, 1)};
        for (int rcb : bad) {
            ++calls;
            if (rcb != USIP_EINVAL) { std::printf("round %d: a call outside the limits returned %d\n", round, rcb); return 1; }
            ++refused;
        }
    }
    std::printf("%d calls, %d refused as they must be, no finding\n", calls, refused);
    return 0;
}
