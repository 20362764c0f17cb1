// usip_amd/csrc/pairs_cpu.cpp -- host twin of csrc/pairs.hip: the same draws and arithmetic
// (csrc/pairs_math.h) on host pointers, the per-cloud stage through csrc/cloud_stage_host.h.  Never reached from the
// device entry points.
#include "cloud_stage_host.h"

using namespace usip_pairs;

namespace {

template <class Src>
void build_host(const usip_pairs_recipe& r, const Src& src, const float* bank, const int64_t* offsets, int num_scans,
                const int32_t* scan_ids, int P, const usip_pairs_out& out)
{
    std::vector<double> T((size_t)P * T_SIZE);
    const PairView v{T.data(), offsets, scan_ids, num_scans};
    const CloudOut o{{out.pc[0], out.pc[1]}, {out.sn[0], out.sn[1]}, {out.node[0], out.node[1]}, out.rows, out.node_slots};
    for (int p = 0; p < P; ++p) {
        double* Tp = T.data() + (size_t)p * T_SIZE;
        pair_table(r, src, p, Tp);
        for (int i = 0; i < 9; ++i) out.R[p * 9 + i] = (float)Tp[T_RD + i];
        out.scale[p] = (float)Tp[T_DSCALE];
        for (int k = 0; k < 3; ++k) out.shift[p * 3 + k] = (float)Tp[T_DSHIFT + k];
        for (int c = 0; c < 2; ++c) cloud_host(r, src, v, bank, P, c * P + p, o);
    }
}

}  // namespace

extern "C" int usip_pairs_build_f32_cpu(const usip_pairs_recipe* recipe, const usip_pairs_draws* draws, const float* bank,
                                        const int64_t* offsets, int num_scans, const int32_t* scan_ids, int P,
                                        uint64_t seed, uint64_t step, long long pair_base, const usip_pairs_out* out)
{
    if (!recipe_ok(recipe) || P < 0 || num_scans < 1) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!bank || !offsets || !scan_ids || !out || !out->pc[0] || !out->pc[1] || !out->sn[0] || !out->sn[1] ||
        !out->node[0] || !out->node[1] || !out->R || !out->scale || !out->shift)
        return USIP_EINVAL;
    for (int p = 0; p < P; ++p) {
        if (scan_ids[p] < 0 || scan_ids[p] >= num_scans) return USIP_EINVAL;
        const long long n = offsets[scan_ids[p] + 1] - offsets[scan_ids[p]];
        if (n < 1 || (recipe->require_full && n < recipe->N)) return USIP_EINVAL;
    }
    if (draws) {
        if (!draws->rows || !draws->cand || !draws->first || !draws->params ||
            (recipe->train && (!draws->jit_pc || !draws->jit_sn || !draws->jit_node)))
            return USIP_EINVAL;
        const ExplicitDraws src{*draws, recipe->N, recipe->n_sub, recipe->M, recipe->Cs};
        build_host(*recipe, src, bank, offsets, num_scans, scan_ids, P, *out);
    } else {
        const PhiloxDraws src{{seed, step, pair_base}};
        build_host(*recipe, src, bank, offsets, num_scans, scan_ids, P, *out);
    }
    return USIP_OK;
}
