// usip_amd/csrc/desc_pairs_cpu.cpp -- host twin of csrc/desc_pairs.hip: the same draws and arithmetic
// (csrc/desc_pairs_math.h) on host pointers, in the same order, the per-cloud stage through csrc/cloud_stage_host.h.
// Never reached from the device entry points.
#include "cloud_stage_host.h"
#include "desc_pairs_math.h"

using namespace usip_desc_pairs;

namespace {

template <class Src>
void build_host(const usip_desc_pairs_recipe& rd, const Src& src, const usip_desc_pairs_bank& b, const int32_t* scan_ids,
                int P, const usip_desc_pairs_out& out)
{
    const usip_pairs_recipe& r = rd.cloud;
    const PosedBank bank{b.rows, b.offsets, b.poses, b.seq_of, b.seq_start, b.num_scans, b.num_seq};
    std::vector<double> T((size_t)2 * P * T_SIZE);
    std::vector<int32_t> cloud_scan((size_t)2 * P);
    const CloudView v{T.data(), b.offsets, cloud_scan.data(), b.num_scans};
    const CloudOut o{{out.pc[0], out.pc[1]}, {out.sn[0], out.sn[1]}, {out.node[0], out.node[1]}, out.rows, out.node_slots};
    int fails = 0;
    for (int p = 0; p < P; ++p) {
        const int a = bank.scan(scan_ids[p]);
        const int pos = select_positive(bank, rd.positive_radius, src, p, a);
        cloud_scan[p] = a;
        cloud_scan[P + p] = pos;
        out.pos_id[p] = pos;
        out.anc_seq[p] = bank.seq(a);
        for (int i = 0; i < 16; ++i) {
            out.anc_pose[p * 16 + i] = (float)bank.poses[(long long)a * 16 + i];
            out.pos_pose[p * 16 + i] = (float)bank.poses[(long long)pos * 16 + i];
        }
        if (rd.mine) {
            int fail;
            out.neg_idx[p] = mine_negative(bank, rd.negative_radius, src, scan_ids, P, p, fail);
            fails += fail;
        }
        const double us = src.scale_u(p);
        for (int c = 0; c < 2; ++c) {
            double u[CLOUD_U];
            src.cloud_params(p, c, u);
            cloud_table(r, us, u, T.data() + (size_t)(c * P + p) * T_SIZE);
            cloud_host(r, src, v, b.rows, P, c * P + p, o);
        }
    }
    if (rd.mine) out.neg_fail[0] = fails;
}

}  // namespace

extern "C" int usip_desc_pairs_build_f32_cpu(const usip_desc_pairs_recipe* recipe, const usip_desc_pairs_draws* draws,
                                             const usip_desc_pairs_bank* bank, const int32_t* scan_ids, int P,
                                             uint64_t seed, uint64_t step, long long pair_base,
                                             const usip_desc_pairs_out* out)
{
    const int rc = desc_args_ok(recipe, bank, scan_ids, P, out);
    if (rc != 1) return rc;
    for (int p = 0; p < P; ++p)
        if (scan_ids[p] < 0 || scan_ids[p] >= bank->num_scans) return USIP_EINVAL;
    for (int s = 0; s < bank->num_scans; ++s)
        if (bank->offsets[s + 1] - bank->offsets[s] < recipe->cloud.N) return USIP_EINVAL;
    const usip_pairs_recipe& c = recipe->cloud;
    if (draws) {
        if (!desc_draws_ok(recipe, draws)) return USIP_EINVAL;
        const ExplicitDescDraws src{ExplicitDraws{draws->cloud, c.N, c.n_sub, c.M, c.Cs}, draws->params, draws->tries,
                                    draws->neg_pick, draws->T};
        build_host(*recipe, src, *bank, scan_ids, P, *out);
    } else {
        const PhiloxDescDraws src{{seed, step, pair_base}};
        build_host(*recipe, src, *bank, scan_ids, P, *out);
    }
    return USIP_OK;
}
