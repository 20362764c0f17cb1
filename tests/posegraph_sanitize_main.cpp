// tests/posegraph_sanitize_main.cpp -- a stand-alone driver of the f-14 host twin (usip_amd/csrc/posegraph_cpu.cpp) for a
// build under -fsanitize=address,undefined (tests/test_posegraph_cpu.py compiles and runs it): random graphs and banks with
// fragment ids, counts and neighbour indices in and out of range.  Every array is sized exactly, so a read or write one
// element outside is reported.  Exit status 0: every call returned USIP_OK or, where the arguments are outside the limits,
// USIP_EINVAL, and nothing that left a call is a NaN.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "../include/usip_hip.h"

namespace {

std::mt19937_64 rng(14);

double unit() { return std::uniform_real_distribution<double>(-1.0, 1.0)(rng); }

// a rotation about a random axis by `angle`, and a translation of length up to `shift`
void random_pose(double angle, double shift, double* Rt)
{
    double a[3] = {unit(), unit(), unit()};
    const double n = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) + 1e-9;
    for (double& v : a) v /= n;
    const double c = std::cos(angle), s = std::sin(angle), t = 1.0 - c;
    const double R[9] = {t * a[0] * a[0] + c, t * a[0] * a[1] - s * a[2], t * a[0] * a[2] + s * a[1],
                         t * a[0] * a[1] + s * a[2], t * a[1] * a[1] + c, t * a[1] * a[2] - s * a[0],
                         t * a[0] * a[2] - s * a[1], t * a[1] * a[2] + s * a[0], t * a[2] * a[2] + c};
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) Rt[4 * r + k] = R[3 * r + k];
        Rt[4 * r + 3] = shift * unit();
    }
}

bool all_finite(const std::vector<double>& v)
{
    for (double x : v)
        if (!(x - x == 0.0)) return false;
    return true;
}

}  // namespace

int main()
{
    int calls = 0, refused = 0;
    // ---------------------------------------------------------------- the optimiser
    for (int round = 0; round < 40; ++round) {
        const int S = 1 + (int)(rng() % 3), Nmax = 2 + (int)(rng() % 9);
        const int Ecap = Nmax * (Nmax - 1) / 2, Emax = 1 + (int)(rng() % Ecap);
        std::vector<int32_t> n((size_t)S), ecount((size_t)S), ei((size_t)S * Emax, 0), ej((size_t)S * Emax, 0);
        std::vector<double> X((size_t)S * Emax * 12, 0.0), info((size_t)S * Emax * 36, 0.0), T0((size_t)S * Nmax * 12, 0.0);
        for (int s = 0; s < S; ++s) {
            const int ns = 2 + (int)(rng() % (Nmax - 1));
            n[(size_t)s] = ns;
            int e = 0;
            for (int i = 0; i < ns && e < Emax; ++i)                    // sorted by construction; the chain first of every row
                for (int j = i + 1; j < ns && e < Emax; ++j)
                    if (j == i + 1 || rng() % 3 == 0) {
                        ei[(size_t)s * Emax + e] = i;
                        ej[(size_t)s * Emax + e] = j;
                        double* x = &X[((size_t)s * Emax + e) * 12];
                        random_pose(round % 5 == 4 ? 3.141592653589793 : 0.3 * unit(), 0.5, x);
                        if (round % 7 == 6 && e == 1) for (int k = 0; k < 12; ++k) x[k] = 0.0;     // no rotation at all
                        double* L = &info[((size_t)s * Emax + e) * 36];
                        const double w = round % 9 == 8 && e == 0 ? 0.0 : 100.0 + 900.0 * std::fabs(unit());
                        for (int k = 0; k < 6; ++k) L[7 * k] = k < 3 ? w : 2.0 * w;
                        ++e;
                    }
            ecount[(size_t)s] = e;
            for (int k = 0; k < ns; ++k) random_pose(0.2 * k, 1.0, &T0[((size_t)s * Nmax + k) * 12]);
        }
        std::vector<double> T((size_t)S * Nmax * 12), w1((size_t)S * Emax), w2((size_t)S * Emax), f((size_t)S * Emax),
            last((size_t)S * 2);
        std::vector<uint8_t> kept((size_t)S * Emax);
        std::vector<int32_t> done((size_t)S * 2), status((size_t)S);
        const int it1 = (int)(rng() % 5), it2 = (int)(rng() % 3), threads = 1 + (int)(rng() % 3);
        int rc = usip_posegraph_optimize_f64_cpu(n.data(), ecount.data(), ei.data(), ej.data(), X.data(), info.data(), T0.data(),
                                                 S, Nmax, Emax, 0.04, 0.25, it1, it2, T.data(), w1.data(), w2.data(), f.data(),
                                                 kept.data(), done.data(), last.data(), status.data(), threads);
        ++calls;
        if (rc != USIP_OK) { std::printf("round %d: optimize returned %d\n", round, rc); return 1; }
        if (!all_finite(T) || !all_finite(w1) || !all_finite(w2) || !all_finite(f) || !all_finite(last)) {
            std::printf("round %d: a value that is not finite left the call\n", round);
            return 1;
        }
        for (int s = 0; s < S; ++s)
            if (status[(size_t)s] < 0 || status[(size_t)s] > 3 || done[(size_t)2 * s] > it1 || done[(size_t)2 * s + 1] > it2) {
                std::printf("round %d: status %d\n", round, status[(size_t)s]);
                return 1;
            }
        // out of shape: refused before anything is indexed
        std::vector<int32_t> nb = n, eb = ecount, eib = ei, ejb = ej;
        const int which = round % 5;
        if (which == 0) nb[0] = Nmax + 1;
        if (which == 1) eb[0] = Emax + 1;
        if (which == 2) eib[0] = -3;
        if (which == 3) ejb[0] = 1000;
        if (which == 4) { eib[0] = 1; ejb[0] = 0; }
        const int bad[] = {
            usip_posegraph_optimize_f64_cpu(nb.data(), eb.data(), eib.data(), ejb.data(), X.data(), info.data(), T0.data(), S,
                                            Nmax, Emax, 0.04, 0.25, 1, 1, T.data(), w1.data(), w2.data(), f.data(), kept.data(),
                                            done.data(), last.data(), status.data(), 1),
            usip_posegraph_optimize_f64_cpu(n.data(), ecount.data(), ei.data(), ej.data(), X.data(), info.data(), T0.data(), S,
                                            Nmax, Ecap + 1, 0.04, 0.25, 1, 1, T.data(), w1.data(), w2.data(), f.data(),
                                            kept.data(), done.data(), last.data(), status.data(), 1),
            usip_posegraph_optimize_f64_cpu(n.data(), ecount.data(), ei.data(), ej.data(), X.data(), info.data(), T0.data(), S,
                                            Nmax, Emax, 0.0, 0.25, 1, 1, T.data(), w1.data(), w2.data(), f.data(), kept.data(),
                                            done.data(), last.data(), status.data(), 1),
            usip_posegraph_optimize_f64_cpu(n.data(), ecount.data(), ei.data(), ej.data(), X.data(), info.data(), T0.data(), S,
                                            Nmax, Emax, 0.04, 0.25, 257, 1, T.data(), w1.data(), w2.data(), f.data(),
                                            kept.data(), done.data(), last.data(), status.data(), 1),
            usip_posegraph_optimize_f64_cpu(n.data(), ecount.data(), ei.data(), ej.data(), X.data(), info.data(), T0.data(), S,
                                            Nmax, Emax, 0.04, 0.25, 1, 1, T.data(), nullptr, w2.data(), f.data(), kept.data(),
                                            done.data(), last.data(), status.data(), 1)};
        for (int rcb : bad) {
            ++calls;
            if (rcb != USIP_EINVAL) { std::printf("round %d: a call outside the limits returned %d\n", round, rcb); return 1; }
            ++refused;
        }
    }
    // ---------------------------------------------------------------- the information matrix
    std::uniform_real_distribution<float> coord(-0.5f, 0.5f);
    for (int round = 0; round < 40; ++round) {
        const int F = 1 + (int)(rng() % 5), row_len = 3 + (int)(rng() % 3), P = 1 + (int)(rng() % 6);
        std::vector<int64_t> offsets((size_t)F + 1, 0);
        for (int f = 0; f < F; ++f) {
            const int choices[] = {0, 1, 3, 255, 256, 257, 40, 515};
            offsets[(size_t)f + 1] = offsets[(size_t)f] + choices[rng() % 8];
        }
        const long long total = offsets[(size_t)F];
        int Lmax = 1;
        for (int f = 0; f < F; ++f) Lmax = std::max<long long>(Lmax, offsets[(size_t)f + 1] - offsets[(size_t)f]);
        if (round % 7 == 3) Lmax = std::max(1, Lmax / 2);
        std::vector<float> rows((size_t)total * row_len + 1);
        for (auto& v : rows) v = coord(rng);
        if (round % 11 == 5) { offsets[1] = -4; offsets[(size_t)F] = total + 9; }
        std::vector<int32_t> frag1((size_t)P), frag2((size_t)P), idx((size_t)P * Lmax), count((size_t)P);
        std::vector<uint8_t> mask((size_t)P);
        std::vector<double> d2((size_t)P * Lmax), info((size_t)P * 36);
        for (int p = 0; p < P; ++p) {
            frag1[(size_t)p] = (int32_t)(rng() % (F + 4)) - 2;
            frag2[(size_t)p] = (int32_t)(rng() % (F + 4)) - 2;
            mask[(size_t)p] = rng() % 4 != 0;
        }
        for (auto& v : idx) v = (int32_t)(rng() % 700) - 50;            // any value: the twin clamps what it reads
        for (auto& v : d2) v = 0.005 * std::fabs(unit());
        const int threads = 1 + (int)(rng() % 3);
        int rc = usip_icp_information_f32_cpu(rows.data(), row_len, offsets.data(), F, total, frag1.data(), frag2.data(),
                                              idx.data(), d2.data(), round % 3 ? mask.data() : nullptr, P, Lmax, 0.05,
                                              info.data(), count.data(), threads);
        ++calls;
        if (rc != USIP_OK || !all_finite(info)) { std::printf("round %d: information returned %d\n", round, rc); return 1; }
        for (int p = 0; p < P; ++p)
            if (count[(size_t)p] < 0 || count[(size_t)p] > Lmax || info[(size_t)p * 36] != (double)count[(size_t)p]) {
                std::printf("round %d: a count out of range\n", round);
                return 1;
            }
        const int bad[] = {usip_icp_information_f32_cpu(rows.data(), 2, offsets.data(), F, total, frag1.data(), frag2.data(),
                                                        idx.data(), d2.data(), nullptr, P, Lmax, 0.05, info.data(),
                                                        count.data(), 1),
                           usip_icp_information_f32_cpu(rows.data(), row_len, offsets.data(), F, total, frag1.data(),
                                                        frag2.data(), idx.data(), d2.data(), nullptr, P, Lmax, 0.0, info.data(),
                                                        count.data(), 1),
                           usip_icp_information_f32_cpu(rows.data(), row_len, offsets.data(), F, total, frag1.data(),
                                                        frag2.data(), idx.data(), d2.data(), nullptr, 65536, Lmax, 0.05,
                                                        info.data(), count.data(), 1),
                           usip_icp_information_f32_cpu(rows.data(), row_len, offsets.data(), F, total, frag1.data(),
                                                        frag2.data(), nullptr, d2.data(), nullptr, P, Lmax, 0.05, info.data(),
                                                        count.data(), 1)};
        for (int rcb : bad) {
            ++calls;
            if (rcb != USIP_EINVAL) { std::printf("round %d: a call outside the limits returned %d\n", round, rcb); return 1; }
            ++refused;
        }
    }
    std::printf("%d calls, %d refused as they must be, no finding\n", calls, refused);
    return 0;
}
