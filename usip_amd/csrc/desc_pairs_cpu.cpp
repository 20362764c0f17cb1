// usip_amd/csrc/desc_pairs_cpu.cpp -- host twin of csrc/desc_pairs.hip: the same draws and arithmetic
// (csrc/desc_pairs_math.h) on host pointers, in the same order, with a float64 farthest-point sampling loop in numpy's
// order (FarthestSampler.sample, data/kitti_descriptor_loader.py:70-84).  Never reached from the device entry points.
#include <cmath>
#include <vector>
#include "desc_pairs_math.h"

using namespace usip_desc_pairs;

namespace {

// out[0] = first, then k-1 times the first arg-max of the running minimum of (dx*dx + dy*dy) + dz*dz in float64
// (the loop of csrc/pairs_cpu.cpp, which keeps its own copy private)
void fps_host(const float* pts, int n, int first, int k, int32_t* out)
{
    std::vector<double> dist((size_t)n, INFINITY);
    int cur = first;
    out[0] = cur;
    for (int it = 1; it < k; ++it) {
        const double cx = pts[cur], cy = pts[n + cur], cz = pts[2 * n + cur];
        double best = -1.0;
        int bi = 0;
        for (int j = 0; j < n; ++j) {
            const double dx = cx - (double)pts[j], dy = cy - (double)pts[n + j], dz = cz - (double)pts[2 * n + j];
            const double d = (dx * dx + dy * dy) + dz * dz;
            dist[j] = d < dist[j] ? d : dist[j];
            if (dist[j] > best) { best = dist[j]; bi = j; }
        }
        out[it] = cur = bi;
    }
}

template <class Src>
void build_host(const usip_desc_pairs_recipe& rd, const Src& src, const usip_desc_pairs_bank& b, const int32_t* scan_ids,
                int P, const usip_desc_pairs_out& out)
{
    const usip_pairs_recipe& r = rd.cloud;
    const int N = r.N, M = r.M, ns = r.n_sub, Cs = r.Cs;
    const PosedBank bank{b.rows, b.offsets, b.poses, b.seq_of, b.seq_start, b.num_scans, b.num_seq};
    std::vector<double> T((size_t)T_SIZE);
    std::vector<float> cand((size_t)3 * ns);
    std::vector<int32_t> fps((size_t)M);
    int fails = 0;
    for (int p = 0; p < P; ++p) {
        const int a = bank.scan(scan_ids[p]);
        const int pos = select_positive(bank, rd.positive_radius, src, p, a);
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
            const int q = c * P + p, s = c == 0 ? a : pos;
            const long long o0 = bank.offsets[s], n = bank.offsets[s + 1] - o0;
            double u[CLOUD_U];
            src.cloud_params(p, c, u);
            cloud_table(r, us, u, T.data());
            float* pc = out.pc[c] + (long long)p * 3 * N;
            float* sn = out.sn[c] + (long long)p * Cs * N;
            for (int j = 0; j < N; ++j) {
                const long long row = src.row(p, c, n, N, j);
                const float* rp = bank.rows + (o0 + row) * r.row_len;
                float xyz[3], sv[MAX_CS], o[3];
                load_row(r, rp, xyz, sv);
                double zp[4] = {0, 0, 0, 0}, zs[MAX_CS] = {0, 0, 0, 0, 0, 0, 0, 0};
                if (r.train) {
                    src.jit_pc(p, c, N, j, zp);
                    src.jit_sn(p, c, N, Cs, j, zs);
                }
                finish_xyz(r, T.data(), 0, xyz, zp, r.pc_sigma, r.pc_clip, true, o);
                finish_sn(r, T.data(), 0, sv, zs);
                for (int k = 0; k < 3; ++k) pc[(long long)k * N + j] = o[k];
                for (int k = 0; k < Cs; ++k) sn[(long long)k * N + j] = sv[k];
                if (out.rows) out.rows[(long long)q * N + j] = (int32_t)row;
            }
            for (int i = 0; i < ns; ++i) {
                const long long row = src.row(p, c, n, N, src.cand(p, c, N, i));
                const float* cp = bank.rows + (o0 + row) * r.row_len;
                for (int k = 0; k < 3; ++k) cand[(size_t)k * ns + i] = cp[k];
            }
            fps_host(cand.data(), ns, src.first(p, c, ns), M, fps.data());
            float* node = out.node[c] + (long long)p * 3 * M;
            for (int m = 0; m < M; ++m) {
                const int ci = fps[m];
                const float xyz[3] = {cand[ci], cand[ns + ci], cand[2 * ns + ci]};
                double z[4] = {0, 0, 0, 0};
                if (r.train) src.jit_node(p, c, M, m, z);
                float o[3];
                finish_xyz(r, T.data(), 0, xyz, z, r.node_sigma, r.node_clip, false, o);
                for (int k = 0; k < 3; ++k) node[(long long)k * M + m] = o[k];
                if (out.node_slots) out.node_slots[(long long)q * M + m] = src.cand(p, c, N, ci);
            }
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
        const PhiloxDescDraws src{seed, step, pair_base};
        build_host(*recipe, src, *bank, scan_ids, P, *out);
    }
    return USIP_OK;
}
