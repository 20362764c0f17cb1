// usip_amd/csrc/posegraph_cpu.cpp -- host twin of csrc/posegraph.hip: the same decisions and arithmetic
// (csrc/posegraph_math.h) on host pointers, as plain loops: the information sums in the device's order (LANES strided partial
// sums, then the binary tree), the factorisation entry by entry, every inner sum in ascending index.  num_threads splits the
// pairs or the scenes.  Never reached from the device entry points.
#include <cmath>
#include <cstring>
#include <vector>
#include "bank.h"
#include "host_split.h"
#include "posegraph_math.h"
#include "../../include/usip_hip.h"

using namespace usip_pg;
using usip_frag::info_fill;
using usip_frag::info_terms;
using usip_frag::radius_sq_hi;
using usip_frag::within;
using usip_bank::bank_ok;
using usip_bank::fragment_range;
using usip_bank::Range;
using usip_host::split;
using usip_reg::tree_sum;

namespace {

struct Scene {
    const int32_t* ei;
    const int32_t* ej;
    const double* X;
    const double* info;
    double* T;
    uint8_t* kept;
    int n, E, M;
    std::vector<double> lt, blocks, wbuf, g, x;
    std::vector<int> start, list;
};

void edge_pass(Scene& sc, bool weights_only, double tau2, bool stage2, double* wout, double* fout)
{
    for (int e = 0; e < sc.E; ++e) {
        const int i = clamp_index(sc.ei[e], sc.n), j = clamp_index(sc.ej[e], sc.n);
        double E[12], r[6];
        residual(sc.T + i * 12, sc.T + j * 12, sc.X + (long long)e * 12, E, r);
        const double* L = sc.info + (long long)e * 36;
        const double f = energy(L, r);
        const bool odometry = j == i + 1;
        double w = weight(f, L[0], tau2, odometry);
        if (stage2 && !odometry && sc.kept[e] == 0) w = 0.0;
        if (weights_only) {
            wout[e] = w;
            if (fout) fout[e] = energy_out(f);
        } else {
            sc.wbuf[(size_t)e] = w;
            if (w > 0.0) edge_blocks(E, r, L, w, sc.blocks.data() + (size_t)e * EDGE_W);
        }
    }
}

void assemble(Scene& sc)
{
    const int M = sc.M, n = sc.n;
    std::fill(sc.lt.begin(), sc.lt.end(), 0.0);
    for (int a = 1; a < n; ++a)
        for (int q = 0; q < 42; ++q) {
            const int r = q < 36 ? q / 6 : q - 36, c = q < 36 ? q % 6 : 0;
            if (q < 36 && r < c) continue;
            double sum = 0.0;
            for (int at = sc.start[(size_t)a]; at < sc.start[(size_t)a + 1]; ++at) {
                const int e = sc.list[(size_t)at];
                if (!(sc.wbuf[(size_t)e] > 0.0)) continue;
                const double* blk = sc.blocks.data() + (size_t)e * EDGE_W;
                const bool first = sc.ei[e] == a;
                sum += q < 36 ? blk[(first ? B_II : B_JJ) + 6 * r + c] : blk[(first ? G_I : G_J) + r];
            }
            if (q < 36) sc.lt[(size_t)(6 * (a - 1) + c) * M + 6 * (a - 1) + r] = sum;
            else sc.g[(size_t)(6 * (a - 1) + r)] = sum;
        }
    for (int e = 0; e < sc.E; ++e) {
        const int i = clamp_index(sc.ei[e], n), j = clamp_index(sc.ej[e], n);
        if (i < 1 || !(sc.wbuf[(size_t)e] > 0.0)) continue;
        for (int q = 0; q < 36; ++q)
            sc.lt[(size_t)(6 * (i - 1) + q % 6) * M + 6 * (j - 1) + q / 6] = sc.blocks[(size_t)e * EDGE_W + B_JI + q];
    }
}

// x = H^-1 g; the status of the step
int solve(Scene& sc)
{
    const int M = sc.M;
    double* lt = sc.lt.data();
    for (int j = 0; j < M; ++j) {
        double* colj = lt + (size_t)j * M;
        for (int i = j; i < M; ++i) {
            double v = colj[i];
            for (int k = 0; k < j; ++k) v -= lt[(size_t)k * M + i] * lt[(size_t)k * M + j];
            colj[i] = v;
        }
        const double d = colj[j];
        if (!(usip_fgr::finite(d) && d > 0.0)) return ST_PIVOT;
        const double piv = std::sqrt(d);
        colj[j] = piv;
        for (int i = j + 1; i < M; ++i) colj[i] = colj[i] / piv;
    }
    double* x = sc.x.data();
    for (int i = 0; i < M; ++i) {
        double v = sc.g[(size_t)i];
        for (int k = 0; k < i; ++k) v -= lt[(size_t)k * M + i] * x[k];
        x[i] = v / lt[(size_t)i * M + i];
    }
    for (int i = M - 1; i >= 0; --i) {
        double v = x[i];
        for (int k = M - 1; k > i; --k) v -= lt[(size_t)i * M + k] * x[k];
        x[i] = v / lt[(size_t)i * M + i];
    }
    bool inf = false, far = false;
    for (int i = 0; i < M; ++i) {
        inf = inf || !usip_fgr::finite(x[i]);
        far = far || (i % 6 >= 3 && std::fabs(x[i]) > PI);
    }
    return inf ? ST_NOT_FINITE : (far ? ST_ANGLE : ST_OK);
}

}  // namespace

extern "C" int usip_icp_information_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags,
                                            long long total_rows, const int32_t* frag1, const int32_t* frag2,
                                            const int32_t* idx, const double* d2, const uint8_t* mask, int P, int Lmax,
                                            double radius, double* info, int32_t* count, int num_threads)
{
    if (!bank_ok(rows, row_len, offsets, num_frags, total_rows, P, Lmax) || !(radius > 0.0)) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!frag1 || !frag2 || !idx || !d2 || !info || !count) return USIP_EINVAL;
    const double r2hi = radius_sq_hi(radius);
    split(P, num_threads, [&](int lo, int hi) {
        std::vector<double> buf((size_t)LANES * 10);
        double (*part)[10] = reinterpret_cast<double (*)[10]>(buf.data());
        for (int p = lo; p < hi; ++p) {
            const Range r1 = fragment_range(offsets, num_frags, total_rows, frag1[p], Lmax);
            const Range r2 = fragment_range(offsets, num_frags, total_rows, frag2[p], Lmax);
            const bool live = !(mask && mask[p] == 0) && r1.n >= 1;
            const int n2 = live ? r2.n : 0;
            const float* rows1 = rows + r1.first * row_len;
            for (int l = 0; l < LANES; ++l) {
                double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                int mine = 0;
                for (int i = l; i < n2; i += LANES)
                    if (within(d2[(long long)p * Lmax + i], radius, r2hi)) {
                        const float* a = rows1 + (long long)clamp_index(idx[(long long)p * Lmax + i], r1.n) * row_len;
                        double t[9];
                        info_terms((double)a[0], (double)a[1], (double)a[2], t);
                        for (int k = 0; k < 9; ++k) s[k] += t[k];
                        ++mine;
                    }
                for (int k = 0; k < 9; ++k) part[l][k] = s[k];
                part[l][9] = (double)mine;
            }
            tree_sum<10>(part);
            double sum[9];
            for (int k = 0; k < 9; ++k) sum[k] = part[0][k];
            const int n = (int)part[0][9];
            info_fill(sum, n, info + (long long)p * 36);
            count[p] = n;
        }
    });
    return USIP_OK;
}

extern "C" int usip_posegraph_optimize_f64_cpu(const int32_t* n, const int32_t* ecount, const int32_t* edge_i,
                                               const int32_t* edge_j, const double* X, const double* info, const double* T0,
                                               int S, int Nmax, int Emax, double tau2, double prune, int iterations1,
                                               int iterations2, double* T, double* weight1, double* weight2, double* energy,
                                               uint8_t* kept, int32_t* iterations_done, double* last_step, int32_t* status,
                                               int num_threads)
{
    if (!shape_ok(S, Nmax, Emax) || !(tau2 > 0.0) || !(tau2 - tau2 == 0.0) || !(prune >= 0.0 && prune <= 1.0) ||
        iterations1 < 0 || iterations1 > MAX_ITERATIONS || iterations2 < 0 || iterations2 > MAX_ITERATIONS)
        return USIP_EINVAL;
    if (S == 0) return USIP_OK;
    if (!n || !ecount || !edge_i || !edge_j || !X || !info || !T0 || !T || !weight1 || !weight2 || !energy || !kept ||
        !iterations_done || !last_step || !status)
        return USIP_EINVAL;
    for (int s = 0; s < S; ++s) {                                      // host pointers: a graph out of shape is refused here
        if (n[s] < 2 || n[s] > Nmax || ecount[s] < 0 || ecount[s] > Emax) return USIP_EINVAL;
        for (int e = 0; e < ecount[s]; ++e)
            if (!edge_ok(edge_i + (long long)s * Emax, edge_j + (long long)s * Emax, e, n[s])) return USIP_EINVAL;
    }
    const size_t SE = (size_t)S * Emax;
    std::memset(T, 0, sizeof(double) * (size_t)S * Nmax * 12);
    std::memset(weight1, 0, sizeof(double) * SE);
    std::memset(weight2, 0, sizeof(double) * SE);
    std::memset(energy, 0, sizeof(double) * SE);
    std::memset(kept, 0, SE);
    std::memset(iterations_done, 0, sizeof(int32_t) * (size_t)S * 2);
    std::memset(last_step, 0, sizeof(double) * (size_t)S * 2);
    std::memset(status, 0, sizeof(int32_t) * (size_t)S);
    split(S, num_threads, [&](int lo, int hi) {
        Scene sc;
        for (int s = lo; s < hi; ++s) {
            sc.ei = edge_i + (long long)s * Emax;
            sc.ej = edge_j + (long long)s * Emax;
            sc.X = X + (long long)s * Emax * 12;
            sc.info = info + (long long)s * Emax * 36;
            sc.T = T + (long long)s * Nmax * 12;
            sc.kept = kept + (long long)s * Emax;
            sc.n = n[s];
            sc.E = ecount[s];
            sc.M = 6 * (sc.n - 1);
            const int M = sc.M, E = sc.E;
            sc.lt.assign((size_t)M * M, 0.0);
            sc.blocks.assign((size_t)E * EDGE_W + 1, 0.0);
            sc.wbuf.assign((size_t)E + 1, 0.0);
            sc.g.assign((size_t)M, 0.0);
            sc.x.assign((size_t)M, 0.0);
            sc.start.assign((size_t)sc.n + 1, 0);
            sc.list.clear();
            for (int k = 0; k < sc.n * 12; ++k) sc.T[k] = T0[(long long)s * Nmax * 12 + k];
            for (int a = 0; a < sc.n; ++a) {
                for (int e = 0; e < E; ++e)
                    if (sc.ei[e] == a || sc.ej[e] == a) sc.list.push_back(e);
                sc.start[(size_t)a + 1] = (int)sc.list.size();
            }
            int st = ST_OK;
            for (int stage = 0; stage < 2; ++stage) {
                const int iterations = stage == 0 ? iterations1 : iterations2;
                int done = 0;
                double last = 0.0;
                for (int it = 0; it < iterations && st == ST_OK; ++it) {
                    edge_pass(sc, false, tau2, stage == 1, nullptr, nullptr);
                    assemble(sc);
                    st = solve(sc);
                    if (st != ST_OK) break;
                    double step = 0.0;
                    for (int a = 1; a < sc.n; ++a) {
                        double d[6];
                        for (int k = 0; k < 6; ++k) d[k] = -sc.x[(size_t)(6 * (a - 1) + k)];
                        apply_update(sc.T + a * 12, d);
                    }
                    for (int k = 0; k < M; ++k) step = max_nan(step, std::fabs(sc.x[(size_t)k]));
                    last = step;
                    done = it + 1;
                }
                iterations_done[2 * s + stage] = done;
                last_step[2 * s + stage] = last;
                double* wout = (stage == 0 ? weight1 : weight2) + (long long)s * Emax;
                edge_pass(sc, true, tau2, stage == 1, wout, stage == 1 ? energy + (long long)s * Emax : nullptr);
                if (stage == 0)
                    for (int e = 0; e < E; ++e)
                        sc.kept[e] = (clamp_index(sc.ej[e], sc.n) == clamp_index(sc.ei[e], sc.n) + 1 || wout[e] >= prune) ? 1 : 0;
            }
            status[s] = st;
        }
    });
    return USIP_OK;
}
