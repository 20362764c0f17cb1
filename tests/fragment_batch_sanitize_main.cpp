// tests/fragment_batch_sanitize_main.cpp -- a stand-alone program over the host twin of the evaluation fragment builder
// (usip_amd/csrc/fragment_batch_cpu.cpp), built by tests/test_fragment_batch_cpu.py with -fsanitize=address,undefined and run
// as a child process.  Every buffer is a std::vector of exactly B clouds -- the host twin writes clouds 0..B-1 only, odd B
// included -- so a read or write past an end is an AddressSanitizer report.  It links nothing else of the package and is
// never loaded into Python.
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
    usip_fragment_batch_bank c;
};

Bank make_bank(std::mt19937_64& rng, const std::vector<int>& lens, int row_len)
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
    b.c = usip_fragment_batch_bank{b.rows.data(), b.offsets.data(), (int)lens.size(), min_rows};
    return b;
}

usip_pairs_recipe make_recipe(int N, int M, int Cs, int n_sub, int row_len)
{
    usip_pairs_recipe r = {};
    r.N = N; r.M = M; r.Cs = Cs; r.n_sub = n_sub; r.row_len = row_len;
    return r;
}

struct Out {
    std::vector<float> pc, sn, node;
    std::vector<int32_t> rows, slots;
    usip_fragment_batch_out c;
    Out(int B, int N, int M, int Cs)
    {
        pc.assign((size_t)B * 3 * N, NAN); sn.assign((size_t)B * Cs * N, NAN); node.assign((size_t)B * 3 * M, NAN);
        rows.assign((size_t)B * N, -1); slots.assign((size_t)B * M, -1);
        c = usip_fragment_batch_out{pc.data(), sn.data(), node.data(), rows.data(), slots.data()};
    }
    bool all_written() const
    {
        for (float v : pc) if (std::isnan(v)) return false;
        for (float v : sn) if (std::isnan(v)) return false;
        for (float v : node) if (std::isnan(v)) return false;
        for (int32_t v : rows) if (v < 0) return false;
        for (int32_t v : slots) if (v < 0) return false;
        return true;
    }
};

}  // namespace

int main()
{
    std::mt19937_64 rng(27);
    // fragments longer than N, shorter (fix_idx layout) and of a single row; shapes that are no power of two
    const std::vector<int> lens = {140, 97, 33, 1, 260};
    const int shapes[3][4] = {{128, 8, 4, 64}, {100, 33, 3, 50}, {96, 1, 4, 1}};     // N, M, Cs, n_sub
    for (int sh = 0; sh < 3; ++sh) {
        const int N = shapes[sh][0], M = shapes[sh][1], Cs = shapes[sh][2], ns = shapes[sh][3], row_len = 7;
        Bank b = make_bank(rng, lens, row_len);
        const usip_pairs_recipe r = make_recipe(N, M, Cs, ns, row_len);
        const int32_t ids[5] = {0, 4, 3, 2, 2};
        for (int B = 1; B <= 5; ++B) {
            Out a(B, N, M, Cs), t(B, N, M, Cs);
            CHECK(usip_fragment_batch_build_f32_cpu(&r, nullptr, &b.c, ids, B, 3, 5, &a.c, 1) == 0);
            CHECK(usip_fragment_batch_build_f32_cpu(&r, nullptr, &b.c, ids, B, 3, 5, &t.c, 3) == 0);
            CHECK(a.all_written() && t.all_written());
            CHECK(a.pc == t.pc && a.sn == t.sn && a.node == t.node && a.rows == t.rows && a.slots == t.slots);
            // explicit draws, some indices far out of range: clamped, never followed outside a buffer
            std::vector<int32_t> rows((size_t)B * N), cand((size_t)B * ns), first((size_t)B);
            for (auto& v : rows) v = (int32_t)(rng() % 400) - 50;
            for (auto& v : cand) v = (int32_t)(rng() % (2 * N)) - N / 2;
            for (auto& v : first) v = (int32_t)(rng() % (2 * ns)) - 1;
            usip_fragment_batch_draws d = {rows.data(), cand.data(), first.data()};
            Out e(B, N, M, Cs);
            CHECK(usip_fragment_batch_build_f32_cpu(&r, &d, &b.c, ids, B, 0, 0, &e.c, 2) == 0);
            CHECK(e.all_written());
            d.first = nullptr;
            CHECK(usip_fragment_batch_build_f32_cpu(&r, &d, &b.c, ids, B, 0, 0, &e.c, 1) < 0);
        }
        // a fragment's outputs do not depend on the batch: ids[3] == ids[4] == 2
        Out five(5, N, M, Cs), one(1, N, M, Cs);
        CHECK(usip_fragment_batch_build_f32_cpu(&r, nullptr, &b.c, ids, 5, 3, 5, &five.c, 1) == 0);
        CHECK(usip_fragment_batch_build_f32_cpu(&r, nullptr, &b.c, ids + 4, 1, 3, 5, &one.c, 1) == 0);
        for (int q = 3; q < 5; ++q)
            for (size_t i = 0; i < one.pc.size(); ++i) CHECK(five.pc[(size_t)q * 3 * N + i] == one.pc[i]);
        // refusals
        const int B = 4;
        Out o(B, N, M, Cs);
        const int32_t bad_ids[4] = {0, 5, 1, 2}, neg_ids[4] = {0, -1, 1, 2};
        CHECK(usip_fragment_batch_build_f32_cpu(&r, nullptr, &b.c, bad_ids, B, 0, 0, &o.c, 1) < 0);
        CHECK(usip_fragment_batch_build_f32_cpu(&r, nullptr, &b.c, neg_ids, B, 0, 0, &o.c, 1) < 0);
        CHECK(usip_fragment_batch_build_f32_cpu(&r, nullptr, &b.c, ids, 0, 0, 0, &o.c, 1) == 0);
        CHECK(usip_fragment_batch_build_f32_cpu(&r, nullptr, &b.c, ids, -1, 0, 0, &o.c, 1) < 0);
        CHECK(usip_fragment_batch_build_f32_cpu(&r, nullptr, nullptr, ids, B, 0, 0, &o.c, 1) < 0);
        CHECK(usip_fragment_batch_build_f32_cpu(nullptr, nullptr, &b.c, ids, B, 0, 0, &o.c, 1) < 0);
        usip_pairs_recipe q = r;
        q.train = 1;
        CHECK(usip_fragment_batch_build_f32_cpu(&q, nullptr, &b.c, ids, B, 0, 0, &o.c, 1) < 0);
        q = r; q.sn_last = 1;
        CHECK(usip_fragment_batch_build_f32_cpu(&q, nullptr, &b.c, ids, B, 0, 0, &o.c, 1) < 0);
        q = r; q.height_scaling = 1;
        CHECK(usip_fragment_batch_build_f32_cpu(&q, nullptr, &b.c, ids, B, 0, 0, &o.c, 1) < 0);
        q = r; q.enu_to_cam = 1;
        CHECK(usip_fragment_batch_build_f32_cpu(&q, nullptr, &b.c, ids, B, 0, 0, &o.c, 1) < 0);
        q = r; q.Cs = 5;
        CHECK(usip_fragment_batch_build_f32_cpu(&q, nullptr, &b.c, ids, B, 0, 0, &o.c, 1) < 0);
        q = r; q.M = ns + 1;
        CHECK(usip_fragment_batch_build_f32_cpu(&q, nullptr, &b.c, ids, B, 0, 0, &o.c, 1) < 0);
        usip_fragment_batch_bank nb = b.c;
        nb.min_rows = 0;
        CHECK(usip_fragment_batch_build_f32_cpu(&r, nullptr, &nb, ids, B, 0, 0, &o.c, 1) < 0);
        nb = b.c; nb.num_fragments = 0;
        CHECK(usip_fragment_batch_build_f32_cpu(&r, nullptr, &nb, ids, B, 0, 0, &o.c, 1) < 0);
        std::vector<int64_t> hollow = b.offsets;                                    // fragment 1 emptied, min_rows left stale
        hollow[2] = hollow[1];
        nb = b.c; nb.offsets = hollow.data();
        const int32_t into[4] = {0, 1, 2, 3};
        CHECK(usip_fragment_batch_build_f32_cpu(&r, nullptr, &nb, into, B, 0, 0, &o.c, 1) < 0);
        usip_fragment_batch_out no = o.c;
        no.node = nullptr;
        CHECK(usip_fragment_batch_build_f32_cpu(&r, nullptr, &b.c, ids, B, 0, 0, &no, 1) < 0);
        no = o.c; no.rows = nullptr; no.node_slots = nullptr;                       // the optional outputs
        CHECK(usip_fragment_batch_build_f32_cpu(&r, nullptr, &b.c, ids, B, 0, 0, &no, 1) == 0);
    }
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
