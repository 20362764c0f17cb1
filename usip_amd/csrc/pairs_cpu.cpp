// usip_amd/csrc/pairs_cpu.cpp -- host twin of csrc/pairs.hip: the same draws and arithmetic
// (csrc/pairs_math.h) on host pointers, with its own float64 farthest-point sampling loop in numpy's order
// (FarthestSampler.sample, data/kitti_detector_loader.py:69-83).  Never reached from the device entry points.
#include <cmath>
#include <vector>
#include "pairs_math.h"

using namespace usip_pairs;

namespace {

// out[0] = first, then k-1 times the first arg-max of the running minimum of (dx*dx + dy*dy) + dz*dz in float64
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
void build_host(const usip_pairs_recipe& r, const Src& src, const float* bank, const int64_t* offsets, int num_scans,
                const int32_t* scan_ids, int P, const usip_pairs_out& out)
{
    const int N = r.N, M = r.M, ns = r.n_sub, Cs = r.Cs;
    std::vector<double> T((size_t)T_SIZE);
    std::vector<float> cand((size_t)3 * ns);
    std::vector<int32_t> fps((size_t)M);
    for (int p = 0; p < P; ++p) {
        double u[USIP_PAIRS_NPARAM];
        src.params(p, u);
        pair_table(r, u, T.data());
        for (int i = 0; i < 9; ++i) out.R[p * 9 + i] = (float)T[T_RD + i];
        out.scale[p] = (float)T[T_DSCALE];
        for (int k = 0; k < 3; ++k) out.shift[p * 3 + k] = (float)T[T_DSHIFT + k];
        int s = scan_ids[p];
        s = s < 0 ? 0 : (s >= num_scans ? num_scans - 1 : s);
        const long long o0 = offsets[s], n = offsets[s + 1] - o0;
        for (int c = 0; c < 2; ++c) {
            const int q = c * P + p;
            float* pc = out.pc[c] + (long long)p * 3 * N;
            float* sn = out.sn[c] + (long long)p * Cs * N;
            for (int j = 0; j < N; ++j) {
                const long long row = src.row(p, c, n, N, j);
                const float* rp = bank + (o0 + row) * r.row_len;
                float xyz[3], sv[MAX_CS], o[3];
                load_row(r, rp, xyz, sv);
                raw_xyz(T.data(), rp, xyz);
                double zp[4] = {0, 0, 0, 0}, zs[MAX_CS] = {0, 0, 0, 0, 0, 0, 0, 0};
                if (r.train) {
                    src.jit_pc(p, c, N, j, zp);
                    src.jit_sn(p, c, N, Cs, j, zs);
                }
                finish_xyz(r, T.data(), c, xyz, zp, r.pc_sigma, r.pc_clip, true, o);
                finish_sn(r, T.data(), c, sv, zs);
                for (int k = 0; k < 3; ++k) pc[(long long)k * N + j] = o[k];
                for (int k = 0; k < Cs; ++k) sn[(long long)k * N + j] = sv[k];
                if (out.rows) out.rows[(long long)q * N + j] = (int32_t)row;
            }
            for (int i = 0; i < ns; ++i) {
                const long long row = src.row(p, c, n, N, src.cand(p, c, N, i));
                float cx[3];
                raw_xyz(T.data(), bank + (o0 + row) * r.row_len, cx);
                for (int k = 0; k < 3; ++k) cand[(size_t)k * ns + i] = cx[k];
            }
            fps_host(cand.data(), ns, src.first(p, c, ns), M, fps.data());
            float* node = out.node[c] + (long long)p * 3 * M;
            for (int m = 0; m < M; ++m) {
                const int ci = fps[m];
                const float xyz[3] = {cand[ci], cand[ns + ci], cand[2 * ns + ci]};
                double z[4] = {0, 0, 0, 0};
                if (r.train) src.jit_node(p, c, M, m, z);
                float o[3];
                finish_xyz(r, T.data(), c, xyz, z, r.node_sigma, r.node_clip, false, o);
                for (int k = 0; k < 3; ++k) node[(long long)k * M + m] = o[k];
                if (out.node_slots) out.node_slots[(long long)q * M + m] = src.cand(p, c, N, ci);
            }
        }
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
        const PhiloxDraws src{seed, step, pair_base};
        build_host(*recipe, src, bank, offsets, num_scans, scan_ids, P, *out);
    }
    return USIP_OK;
}
