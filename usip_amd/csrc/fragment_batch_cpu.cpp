// usip_amd/csrc/fragment_batch_cpu.cpp -- host twin of csrc/fragment_batch.hip: the same draws and gathers
// (csrc/fragment_batch_math.h) on host pointers, the per-cloud stage through csrc/cloud_stage_host.h.  num_threads splits
// the fragments; every fragment writes its own rows of every output, so the result does not depend on the split.  Only
// clouds 0..B-1 are computed: the device's repeated last cloud of an odd batch has no counterpart.  Never reached from the
// device entry points.
#include <thread>
#include "cloud_stage_host.h"
#include "fragment_batch_math.h"

using namespace usip_fragment_batch;

namespace {

template <class Src>
void build_host(const usip_pairs_recipe& recipe, const Src& src, const usip_fragment_batch_bank& b, const int32_t* ids,
                int B, const usip_fragment_batch_out& out, int num_threads)
{
    const usip_pairs_recipe r = stage_recipe(recipe);
    const int P = (B + 1) / 2;
    double T[T_SIZE];
    identity_table(T);
    std::vector<int32_t> cloud_frag((size_t)2 * P);
    for (int q = 0; q < 2 * P; ++q) cloud_frag[q] = clampi(ids[q < B ? q : B - 1], 0, b.num_fragments - 1);
    const FragmentView v{T, b.offsets, cloud_frag.data(), b.num_fragments};
    const long long half = P;
    const CloudOut o{{out.pc, out.pc + half * 3 * r.N}, {out.sn, out.sn + half * r.Cs * r.N},
                     {out.node, out.node + half * 3 * r.M}, out.rows, out.node_slots};
    const int nt = num_threads < 1 ? 1 : (num_threads > B ? B : num_threads);
    if (nt <= 1) {
        for (int q = 0; q < B; ++q) cloud_host(r, src, v, b.rows, P, q, o);
        return;
    }
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t)
        pool.emplace_back([&, t] { for (int q = t; q < B; q += nt) cloud_host(r, src, v, b.rows, P, q, o); });
    for (auto& th : pool) th.join();
}

}  // namespace

extern "C" int usip_fragment_batch_build_f32_cpu(const usip_pairs_recipe* recipe, const usip_fragment_batch_draws* draws,
                                                 const usip_fragment_batch_bank* bank, const int32_t* ids, int B,
                                                 uint64_t seed, uint64_t step, const usip_fragment_batch_out* out,
                                                 int num_threads)
{
    const int rc = fragment_args_ok(recipe, bank, ids, ids, B, out);
    if (rc != 1) return rc;
    for (int i = 0; i < B; ++i)
        if (bank->offsets[ids[i] + 1] - bank->offsets[ids[i]] < 1) return USIP_EINVAL;
    if (draws) {
        if (!fragment_draws_ok(draws)) return USIP_EINVAL;
        ExplicitFragmentDraws src;
        src.d = *draws;
        src.P = (B + 1) / 2;
        src.B = B;
        src.N = recipe->N;
        src.n_sub = recipe->n_sub;
        build_host(*recipe, src, *bank, ids, B, *out, num_threads);
    } else {
        PhiloxFragmentDraws src;
        src.s = {seed, step, 0};
        src.ids = ids;
        src.P = (B + 1) / 2;
        src.B = B;
        src.num_fragments = bank->num_fragments;
        build_host(*recipe, src, *bank, ids, B, *out, num_threads);
    }
    return USIP_OK;
}
