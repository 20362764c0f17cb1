// usip_amd/csrc/indoor_pairs_cpu.cpp -- host twin of csrc/indoor_pairs.hip: the same draws and arithmetic
// (csrc/indoor_pairs_math.h) on host pointers, the per-cloud stage through csrc/cloud_stage_host.h.  num_threads splits the
// pairs; every pair writes its own rows of every output, so the result does not depend on the split.  Never reached from
// the device entry points.
#include <thread>
#include "cloud_stage_host.h"
#include "indoor_pairs_math.h"

using namespace usip_indoor_pairs;

namespace {

template <class Src>
void build_host(const usip_indoor_pairs_recipe& r, const Src& src, const usip_indoor_pairs_bank& b,
                const int32_t* sample_ids, int P, const usip_indoor_pairs_out& out, int num_threads)
{
    const IndoorBank bank{b.rows, b.offsets, b.pairs, b.icp, b.sample_mode, b.num_frames, b.num_samples};
    const usip_pairs_recipe stage = stage_recipe(r);
    std::vector<double> T((size_t)P * T_SIZE);
    std::vector<int32_t> cloud_frame((size_t)2 * P);
    const IndoorView v{T.data(), b.rows, b.offsets, cloud_frame.data(), b.icp, sample_ids, b.num_frames, b.num_samples,
                       r.icp_moves_normals};
    const CloudOut o{{out.pc[0], out.pc[1]}, {out.sn[0], out.sn[1]}, {out.node[0], out.node[1]}, out.rows, out.node_slots};
    auto pair = [&](int p) {
        const int s = bank.sample(sample_ids[p]);
        double* Tp = T.data() + (size_t)p * T_SIZE;
        indoor_table(r, bank.mode(r.mode, s), src, p, Tp);
        for (int i = 0; i < 9; ++i) out.R[p * 9 + i] = (float)Tp[T_RD + i];
        out.scale[p] = (float)Tp[T_DSCALE];
        for (int k = 0; k < 3; ++k) out.shift[p * 3 + k] = (float)Tp[T_DSHIFT + k];
        for (int c = 0; c < 2; ++c) {
            cloud_frame[c * P + p] = bank.frame(s, c);
            cloud_host(stage, src, v, b.rows, P, c * P + p, o);
        }
    };
    const int nt = num_threads < 1 ? 1 : (num_threads > P ? P : num_threads);
    if (nt <= 1) {
        for (int p = 0; p < P; ++p) pair(p);
        return;
    }
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t)
        pool.emplace_back([&, t] { for (int p = t; p < P; p += nt) pair(p); });
    for (auto& th : pool) th.join();
}

}  // namespace

extern "C" int usip_indoor_pairs_build_f32_cpu(const usip_indoor_pairs_recipe* recipe, const usip_indoor_pairs_draws* draws,
                                               const usip_indoor_pairs_bank* bank, const int32_t* sample_ids, int P,
                                               uint64_t seed, uint64_t step, long long pair_base,
                                               const usip_indoor_pairs_out* out, int num_threads)
{
    const int rc = indoor_args_ok(recipe, bank, sample_ids, P, out);
    if (rc != 1) return rc;
    for (int p = 0; p < P; ++p) {
        const int s = sample_ids[p];
        if (s < 0 || s >= bank->num_samples) return USIP_EINVAL;
        if (recipe->mode == MODE_SAMPLE && (bank->sample_mode[s] < MODE_TRAIN || bank->sample_mode[s] > MODE_TEST))
            return USIP_EINVAL;
        for (int c = 0; c < 2; ++c) {
            const int f = bank->pairs[2 * s + c];
            if (f < 0 || f >= bank->num_frames || bank->offsets[f + 1] - bank->offsets[f] < 1) return USIP_EINVAL;
        }
    }
    const usip_pairs_recipe& c = recipe->cloud;
    if (draws) {
        if (!indoor_draws_ok(draws)) return USIP_EINVAL;
        const ExplicitIndoorDraws src{{}, ExplicitDraws{draws->cloud, c.N, c.n_sub, c.M, c.Cs}};
        build_host(*recipe, src, *bank, sample_ids, P, *out, num_threads);
    } else {
        const PhiloxIndoorDraws src{{seed, step, pair_base}};
        build_host(*recipe, src, *bank, sample_ids, P, *out, num_threads);
    }
    return USIP_OK;
}
