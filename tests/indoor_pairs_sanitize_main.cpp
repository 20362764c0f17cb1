// tests/indoor_pairs_sanitize_main.cpp -- a stand-alone program over the host twin of the indoor pair builder
// (usip_amd/csrc/indoor_pairs_cpu.cpp), built by tests/test_indoor_pairs_cpu.py with -fsanitize=address,undefined and run as
// a child process.  Every buffer is a std::vector of exactly the size the interface documents, so a read or write past an
// end is an AddressSanitizer report.  It links nothing else of the package and is never loaded into Python.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../include/usip_hip.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

struct Bank {
    std::vector<float> rows;
    std::vector<int64_t> offsets;
    std::vector<int32_t> pairs, modes;
    std::vector<double> icp;
    usip_indoor_pairs_bank c;
};

Bank make_bank(std::mt19937_64& rng, const std::vector<int>& lens, int row_len, int S)
{
    Bank b;
    std::normal_distribution<float> nd(0.f, 1.f);
    b.offsets.push_back(0);
    long long min_rows = 1LL << 40;
    for (int n : lens) {
        for (long long i = 0; i < (long long)n * row_len; ++i) b.rows.push_back(nd(rng));
        b.offsets.push_back(b.offsets.back() + n);
        if (n < min_rows) min_rows = n;
    }
    for (int s = 0; s < S; ++s) {
        b.pairs.push_back((int32_t)(rng() % lens.size()));
        b.pairs.push_back((int32_t)(rng() % lens.size()));
        b.modes.push_back((int32_t)(s % 3));
        const double a = 0.3 * nd(rng), cs = std::cos(a), sn = std::sin(a);
        const double m[12] = {cs, -sn, 0, nd(rng), sn, cs, 0, nd(rng), 0, 0, 1, nd(rng)};
        b.icp.insert(b.icp.end(), m, m + 12);
    }
    b.c = usip_indoor_pairs_bank{b.rows.data(), b.offsets.data(), b.pairs.data(), b.icp.data(), b.modes.data(),
                                 b.pairs.data(), (int)lens.size(), S, min_rows};
    return b;
}

usip_indoor_pairs_recipe make_recipe(int N, int M, int Cs, int n_sub, int row_len, int mode, int variant)
{
    usip_indoor_pairs_recipe r = {};
    r.cloud.aug_scale_lo = 0.9; r.cloud.aug_scale_hi = 1.1; r.cloud.shift_range = 1.0;
    r.cloud.pert_sigma = 0.12; r.cloud.pert_clip = 0.36;
    r.cloud.dst_scale_thre = 0.2; r.cloud.dst_shift_thre = 0.5;
    r.cloud.N = N; r.cloud.M = M; r.cloud.Cs = Cs; r.cloud.n_sub = n_sub; r.cloud.row_len = row_len;
    r.cloud.rot_horizontal = variant & 1; r.cloud.rot_3d = (variant >> 1) & 1; r.cloud.rot_perturbation = (variant >> 2) & 1;
    r.cloud.translation_perturbation = (variant >> 3) & 1;
    r.cloud.dst_rot_type = r.cloud.rot_3d ? 3 : (r.cloud.rot_horizontal ? 2 : 0);
    r.cloud.dst_rot_perturbation = r.cloud.rot_perturbation;
    r.icp_moves_normals = variant & 1;
    r.mode = mode;
    return r;
}

struct Out {
    std::vector<float> pc[2], sn[2], node[2], R, scale, shift;
    std::vector<int32_t> rows, slots;
    usip_indoor_pairs_out c;
    Out(int P, int N, int M, int Cs)
    {
        for (int i = 0; i < 2; ++i) {
            pc[i].assign((size_t)P * 3 * N, NAN); sn[i].assign((size_t)P * Cs * N, NAN); node[i].assign((size_t)P * 3 * M, NAN);
        }
        R.assign((size_t)P * 9, NAN); scale.assign(P, NAN); shift.assign((size_t)P * 3, NAN);
        rows.assign((size_t)2 * P * N, -1); slots.assign((size_t)2 * P * M, -1);
        c = usip_indoor_pairs_out{{pc[0].data(), pc[1].data()}, {sn[0].data(), sn[1].data()}, {node[0].data(), node[1].data()},
                                  R.data(), scale.data(), shift.data(), rows.data(), slots.data()};
    }
    bool all_written() const
    {
        for (int i = 0; i < 2; ++i) {
            for (float v : pc[i]) if (std::isnan(v)) return false;
            for (float v : sn[i]) if (std::isnan(v)) return false;
            for (float v : node[i]) if (std::isnan(v)) return false;
        }
        for (float v : R) if (std::isnan(v)) return false;
        for (float v : scale) if (std::isnan(v)) return false;
        for (float v : shift) if (std::isnan(v)) return false;
        for (int32_t v : rows) if (v < 0) return false;
        for (int32_t v : slots) if (v < 0) return false;
        return true;
    }
};

}  // namespace

int main()
{
    std::mt19937_64 rng(26);
    // frames longer than N, shorter (fix_idx layout) and of a single row; shapes that are no power of two
    const std::vector<int> lens = {140, 97, 33, 1, 260};
    const int shapes[3][4] = {{128, 8, 4, 64}, {100, 33, 3, 50}, {96, 1, 4, 1}};     // N, M, Cs, n_sub
    for (int sh = 0; sh < 3; ++sh) {
        const int N = shapes[sh][0], M = shapes[sh][1], Cs = shapes[sh][2], ns = shapes[sh][3], row_len = 7, S = 9, P = 4;
        Bank b = make_bank(rng, lens, row_len, S);
        const int32_t ids[4] = {0, 4, 8, 5};
        for (int mode = 0; mode < 4; ++mode)
            for (int variant = 0; variant < 16; variant += 5) {
                const usip_indoor_pairs_recipe r = make_recipe(N, M, Cs, ns, row_len, mode, variant);
                Out a(P, N, M, Cs), t(P, N, M, Cs);
                CHECK(usip_indoor_pairs_build_f32_cpu(&r, nullptr, &b.c, ids, P, 3, 5, 8, &a.c, 1) == 0);
                CHECK(usip_indoor_pairs_build_f32_cpu(&r, nullptr, &b.c, ids, P, 3, 5, 8, &t.c, 3) == 0);
                CHECK(a.all_written() && t.all_written());
                CHECK(a.pc[0] == t.pc[0] && a.pc[1] == t.pc[1] && a.sn[0] == t.sn[0] && a.node[0] == t.node[0] &&
                      a.node[1] == t.node[1] && a.rows == t.rows && a.slots == t.slots);
                // explicit draws, some indices far out of range: clamped, never followed outside a buffer
                std::vector<int32_t> rows((size_t)P * 2 * N), cand((size_t)P * 2 * ns), first((size_t)P * 2);
                std::vector<double> params((size_t)P * USIP_PAIRS_NPARAM);
                for (auto& v : rows) v = (int32_t)(rng() % 400) - 50;
                for (auto& v : cand) v = (int32_t)(rng() % (2 * N)) - N / 2;
                for (auto& v : first) v = (int32_t)(rng() % (2 * ns)) - 1;
                for (auto& v : params) v = (double)(rng() % 1000) / 1000.0 * 3.0 - 1.0;
                usip_indoor_pairs_draws d = {};
                d.cloud.rows = rows.data(); d.cloud.cand = cand.data(); d.cloud.first = first.data();
                d.cloud.params = params.data();
                Out e(P, N, M, Cs);
                CHECK(usip_indoor_pairs_build_f32_cpu(&r, &d, &b.c, ids, P, 0, 0, 0, &e.c, 2) == 0);
                CHECK(e.all_written());
                d.cloud.params = nullptr;
                CHECK(usip_indoor_pairs_build_f32_cpu(&r, &d, &b.c, ids, P, 0, 0, 0, &e.c, 1) < 0);
            }
        // refusals
        usip_indoor_pairs_recipe r = make_recipe(N, M, Cs, ns, row_len, 0, 5);
        Out o(P, N, M, Cs);
        const int32_t bad_ids[4] = {0, 9, 1, 2};
        CHECK(usip_indoor_pairs_build_f32_cpu(&r, nullptr, &b.c, bad_ids, P, 0, 0, 0, &o.c, 1) < 0);
        CHECK(usip_indoor_pairs_build_f32_cpu(&r, nullptr, &b.c, ids, 0, 0, 0, 0, &o.c, 1) == 0);
        CHECK(usip_indoor_pairs_build_f32_cpu(&r, nullptr, &b.c, ids, -1, 0, 0, 0, &o.c, 1) < 0);
        CHECK(usip_indoor_pairs_build_f32_cpu(&r, nullptr, nullptr, ids, P, 0, 0, 0, &o.c, 1) < 0);
        CHECK(usip_indoor_pairs_build_f32_cpu(nullptr, nullptr, &b.c, ids, P, 0, 0, 0, &o.c, 1) < 0);
        usip_indoor_pairs_recipe q = r;
        q.mode = 4;
        CHECK(usip_indoor_pairs_build_f32_cpu(&q, nullptr, &b.c, ids, P, 0, 0, 0, &o.c, 1) < 0);
        q = r; q.cloud.Cs = 2;
        CHECK(usip_indoor_pairs_build_f32_cpu(&q, nullptr, &b.c, ids, P, 0, 0, 0, &o.c, 1) < 0);
        q = r; q.cloud.Cs = 5;
        CHECK(usip_indoor_pairs_build_f32_cpu(&q, nullptr, &b.c, ids, P, 0, 0, 0, &o.c, 1) < 0);
        q = r; q.cloud.pc_sigma = 0.01;
        CHECK(usip_indoor_pairs_build_f32_cpu(&q, nullptr, &b.c, ids, P, 0, 0, 0, &o.c, 1) < 0);
        q = r; q.cloud.train = 1;
        CHECK(usip_indoor_pairs_build_f32_cpu(&q, nullptr, &b.c, ids, P, 0, 0, 0, &o.c, 1) < 0);
        q = r; q.mode = 3;
        usip_indoor_pairs_bank nb = b.c;
        nb.sample_mode = nullptr;
        CHECK(usip_indoor_pairs_build_f32_cpu(&q, nullptr, &nb, ids, P, 0, 0, 0, &o.c, 1) < 0);
        nb = b.c; nb.min_rows = 0;
        CHECK(usip_indoor_pairs_build_f32_cpu(&r, nullptr, &nb, ids, P, 0, 0, 0, &o.c, 1) < 0);
        nb = b.c; nb.num_samples = 0;
        CHECK(usip_indoor_pairs_build_f32_cpu(&r, nullptr, &nb, ids, P, 0, 0, 0, &o.c, 1) < 0);
        std::vector<int32_t> wrong = b.pairs;
        wrong[3] = (int32_t)lens.size();
        nb = b.c; nb.pairs = nb.pairs_host = wrong.data();
        CHECK(usip_indoor_pairs_build_f32_cpu(&r, nullptr, &nb, ids, P, 0, 0, 0, &o.c, 1) < 0);
        usip_indoor_pairs_out no = o.c;
        no.node[1] = nullptr;
        CHECK(usip_indoor_pairs_build_f32_cpu(&r, nullptr, &b.c, ids, P, 0, 0, 0, &no, 1) < 0);
        no = o.c; no.rows = nullptr; no.node_slots = nullptr;                       // the optional outputs
        CHECK(usip_indoor_pairs_build_f32_cpu(&r, nullptr, &b.c, ids, P, 0, 0, 0, &no, 1) == 0);
    }
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
