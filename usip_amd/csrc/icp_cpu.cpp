// usip_amd/csrc/icp_cpu.cpp -- host twin of csrc/icp.hip: the same decisions and arithmetic
// (csrc/icp_math.h) on host pointers.  The nearest-neighbour search is the plain loop over ALL rows of fragment 1 in
// ascending row order -- which is what proves the device's walk; the trim is a sort of (bit pattern, row); every sum is
// taken in the device's order (LANES strided partial sums, then the binary tree).  num_threads splits the pairs.  Never
// reached from the device entry points.  The point-to-plane metric (csrc/icp_plane_math.h) is the same loop
// with another fit.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "bank.h"
#include "host_split.h"
#include "icp_math.h"
#include "icp_plane_math.h"
#include "../../include/usip_hip.h"

using namespace usip_reg;
using namespace usip_frag;
using namespace usip_icp;
using namespace usip_bank;

namespace {

struct Pair {
    const float* rows1;
    const float* rows2;
    int n1, n2;
};

Pair pair_of(const Bank& bank, const int32_t* frag1, const int32_t* frag2, int p, int Lmax)
{
    const Range r1 = bank.range(frag1[p], Lmax);
    const Range r2 = bank.range(frag2[p], Lmax);
    return {bank.rows + r1.first * bank.row_len, bank.rows + r2.first * bank.row_len, r1.n, r2.n};
}

// one pass under Rt: the slots of order2 (NULL: the rows) name the queries, as the device's lanes do
void nearest_of(const Bank& bank, const Pair& pr, const double* Rt, const int32_t* order2, int32_t* idx, double* d2)
{
    for (int s = 0; s < pr.n2; ++s) {
        const int i = order2 ? clamp_index(order2[s], pr.n2) : s;
        const float* b = pr.rows2 + (long long)i * bank.row_len;
        const double b0 = (double)b[0], b1 = (double)b[1], b2 = (double)b[2];
        const double qx = xform(Rt, 0, b0, b1, b2), qy = xform(Rt, 1, b0, b1, b2), qz = xform(Rt, 2, b0, b1, b2);
        double best = INFINITY;
        int brow = 0x7fffffff;
        for (int j = 0; j < pr.n1; ++j) {
            const float* a = pr.rows1 + (long long)j * bank.row_len;
            const double v = sqdist3(qx, qy, qz, (double)a[0], (double)a[1], (double)a[2]);
            if (better(v, j, best, brow)) { best = v; brow = j; }
        }
        idx[i] = brow;
        d2[i] = best;
    }
}

// the cut (d2*, i*): the m-th smallest of (bit pattern, row)
void cut_of(const double* d2, int n2, int m, std::vector<std::pair<unsigned long long, int>>& key, unsigned long long* cut,
            int* icut)
{
    key.resize((size_t)n2);
    for (int i = 0; i < n2; ++i) key[(size_t)i] = {bits_of(d2[i]), i};
    std::nth_element(key.begin(), key.begin() + (m - 1), key.end());
    *cut = key[(size_t)m - 1].first;
    *icut = key[(size_t)m - 1].second;
}


struct Scratch {
    std::vector<std::pair<unsigned long long, int>> key;
    std::vector<double> part, lanes;
    Scratch() : part((size_t)LANES * 10) {}
    double (*parts())[10] { return reinterpret_cast<double (*)[10]>(part.data()); }
};

// the fit of the kept rows: lane l adds the kept rows l, l + LANES, ... in ascending order, then the tree
void fit_of(const Bank& bank, const Pair& pr, const int32_t* idx, const double* d2, unsigned long long cut, int icut, int m,
            Scratch& sc, double Rn[12])
{
    double (*part)[10] = sc.parts();
    const int row_len = bank.row_len;
    for (int l = 0; l < LANES; ++l) {
        double s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = l; i < pr.n2; i += LANES)
            if (kept(bits_of(d2[i]), i, cut, icut)) {
                const float* a = pr.rows1 + (long long)clamp_index(idx[i], pr.n1) * row_len;
                const float* b = pr.rows2 + (long long)i * row_len;
                for (int k = 0; k < 3; ++k) { s[k] += (double)a[k]; s[3 + k] += (double)b[k]; }
            }
        for (int k = 0; k < 10; ++k) part[l][k] = s[k];
    }
    tree_sum<6>(part);
    double ca[3], cb[3];
    for (int k = 0; k < 3; ++k) { ca[k] = part[0][k] / (double)m; cb[k] = part[0][3 + k] / (double)m; }
    for (int l = 0; l < LANES; ++l) {
        double B[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = l; i < pr.n2; i += LANES)
            if (kept(bits_of(d2[i]), i, cut, icut)) {
                const float* a = pr.rows1 + (long long)clamp_index(idx[i], pr.n1) * row_len;
                const float* b = pr.rows2 + (long long)i * row_len;
                const double x[3] = {(double)a[0] - ca[0], (double)a[1] - ca[1], (double)a[2] - ca[2]};
                const double y[3] = {(double)b[0] - cb[0], (double)b[1] - cb[1], (double)b[2] - cb[2]};
                accumulate(B, x, y);
            }
        for (int k = 0; k < 10; ++k) part[l][k] = B[k];
    }
    tree_sum<10>(part);
    double B[10];
    for (int k = 0; k < 10; ++k) B[k] = part[0][k];
    transform_from(B, ca, cb, Rn);
}

// the fit under the plane metric (f-28): the lanes' 27 partial sums, the tree in the device's rounds of nine columns, the
// solve and the step.  S: the 27 sums.  false: the solve failed.
bool fit_plane_of(const Bank& bank, const Pair& pr, const double* Rt, const int32_t* idx, const double* d2,
                  unsigned long long cut, int icut, Scratch& sc, double S[PLANE_SUMS], double Rn[12])
{
    double (*part)[10] = sc.parts();
    const int row_len = bank.row_len;
    sc.lanes.assign((size_t)LANES * PLANE_SUMS, 0.0);
    for (int l = 0; l < LANES; ++l) {
        double* s = sc.lanes.data() + (size_t)l * PLANE_SUMS;
        for (int i = l; i < pr.n2; i += LANES)
            if (kept(bits_of(d2[i]), i, cut, icut)) {
                const float* a = pr.rows1 + (long long)clamp_index(idx[i], pr.n1) * row_len;
                const float* b = pr.rows2 + (long long)i * row_len;
                const double b0 = (double)b[0], b1 = (double)b[1], b2 = (double)b[2];
                plane_terms(s, xform(Rt, 0, b0, b1, b2), xform(Rt, 1, b0, b1, b2), xform(Rt, 2, b0, b1, b2), a);
            }
    }
    for (int base = 0; base < PLANE_SUMS; base += 9) {
        for (int l = 0; l < LANES; ++l)
            for (int k = 0; k < 9; ++k) part[l][k] = sc.lanes[(size_t)l * PLANE_SUMS + base + k];
        tree_sum<9>(part);
        for (int k = 0; k < 9; ++k) S[base + k] = part[0][k];
    }
    double x[6];
    const bool ok = plane_solve(S, x);
    if (ok) plane_step(Rt, x, Rn);                                     // (a failed solve's x may hold anything)
    return ok;
}

}  // namespace

extern "C" int usip_icp_nearest_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags,
                                        long long total_rows, const int32_t* perm1, const int32_t* frag1,
                                        const int32_t* frag2, const double* Rt, const uint8_t* mask, const int32_t* order2,
                                        int P, int Lmax, int32_t* idx, double* d2, int num_threads)
{
    if (!(bank_ok(rows, row_len, offsets, num_frags, total_rows, P, Lmax) && perm1)) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!frag1 || !frag2 || !Rt || !idx || !d2) return USIP_EINVAL;
    const Bank bank{rows, offsets, row_len, num_frags, total_rows};
    std::memset(idx, 0, sizeof(int32_t) * (size_t)P * (size_t)Lmax);
    std::memset(d2, 0, sizeof(double) * (size_t)P * (size_t)Lmax);
    usip_host::split(P, num_threads, [&](int lo, int hi) {
        for (int p = lo; p < hi; ++p) {
            if (mask && mask[p] == 0) continue;
            const Pair pr = pair_of(bank, frag1, frag2, p, Lmax);
            if (pr.n1 < 1 || pr.n2 < 1) continue;
            nearest_of(bank, pr, Rt + (long long)p * 12, order2 ? order2 + (long long)p * Lmax : nullptr,
                       idx + (long long)p * Lmax, d2 + (long long)p * Lmax);
        }
    });
    return USIP_OK;
}

// Both entries of the loop; only the fit differs with the metric.  fit_sums: the plane metric's optional record.
static int refine_loop(bool plane, const float* rows, int row_len, const int64_t* offsets, int num_frags, long long total_rows,
                       const int32_t* perm1, const int32_t* frag1, const int32_t* frag2, const double* Rt0,
                       const uint8_t* mask, const int32_t* order2, int P, int Lmax, double inlier_ratio, int max_iterations,
                       double tol_t, double tol_c, double align_radius, double* Rt_out, int32_t* iterations,
                       uint8_t* converged, double* rmse, int32_t* hits, double* ratio, double* cut_d2, int32_t* cut_i_out,
                       int32_t* idx_out, double* d2_out, double* fit_sums, int num_threads)
{
    if (!(bank_ok(rows, row_len, offsets, num_frags, total_rows, P, Lmax) && perm1) || (plane && row_len < 6))
        return USIP_EINVAL;
    if (!(inlier_ratio > 0.0 && inlier_ratio <= 1.0) || max_iterations < 0 || max_iterations > MAX_ITERATIONS ||
        !(tol_t >= 0.0) || !(tol_c >= 0.0) || !(align_radius > 0.0))
        return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!frag1 || !frag2 || !Rt0 || !Rt_out || !iterations || !converged || !rmse || !hits || !ratio ||
        (cut_d2 == nullptr) != (cut_i_out == nullptr))
        return USIP_EINVAL;
    const int slots = max_iterations + 1;
    if (cut_d2) {
        std::memset(cut_d2, 0, sizeof(double) * (size_t)P * (size_t)slots);
        std::memset(cut_i_out, 0, sizeof(int32_t) * (size_t)P * (size_t)slots);
    }
    if (fit_sums && max_iterations > 0) std::memset(fit_sums, 0, sizeof(double) * (size_t)P * (size_t)max_iterations * PLANE_SUMS);
    const Bank bank{rows, offsets, row_len, num_frags, total_rows};
    const double r2hi = radius_sq_hi(align_radius);
    if (idx_out) std::memset(idx_out, 0, sizeof(int32_t) * (size_t)P * (size_t)Lmax);
    if (d2_out) std::memset(d2_out, 0, sizeof(double) * (size_t)P * (size_t)Lmax);
    usip_host::split(P, num_threads, [&](int lo, int hi) {
        Scratch sc;
        std::vector<int32_t> idx;
        std::vector<double> d2;
        for (int p = lo; p < hi; ++p) {
            double* Rt = Rt_out + (long long)p * 12;
            for (int k = 0; k < 12; ++k) Rt[k] = Rt0[(long long)p * 12 + k];
            iterations[p] = 0;
            converged[p] = 0;
            rmse[p] = 0.0;
            hits[p] = 0;
            ratio[2 * p] = ratio[2 * p + 1] = 0.0;
            const Pair pr = pair_of(bank, frag1, frag2, p, Lmax);
            if ((mask && mask[p] == 0) || pr.n1 < 1 || pr.n2 < 1) continue;
            const int32_t* order = order2 ? order2 + (long long)p * Lmax : nullptr;
            const int m = trim_count(inlier_ratio, pr.n2);
            idx.assign((size_t)pr.n2, 0);                              // rows no query names read as zeros, as the device's
            d2.assign((size_t)pr.n2, 0.0);
            double h[6] = {0, 0, 0, 0, 0, 0};
            unsigned long long cut;
            int icut;
            for (int k = 1; k <= max_iterations; ++k) {
                nearest_of(bank, pr, Rt, order, idx.data(), d2.data());
                cut_of(d2.data(), pr.n2, m, sc.key, &cut, &icut);
                if (cut_d2) {
                    cut_d2[(long long)p * slots + k - 1] = double_of(cut);
                    cut_i_out[(long long)p * slots + k - 1] = icut;
                }
                double Rn[12], dt, dc;
                bool ok;
                if (plane) {
                    double S[PLANE_SUMS];
                    ok = fit_plane_of(bank, pr, Rt, idx.data(), d2.data(), cut, icut, sc, S, Rn);
                    if (fit_sums)
                        std::memcpy(fit_sums + ((long long)p * max_iterations + k - 1) * PLANE_SUMS, S, sizeof(S));
                } else {
                    fit_of(bank, pr, idx.data(), d2.data(), cut, icut, m, sc, Rn);
                    ok = finite12(Rn);
                }
                if (!ok) break;
                pose_delta(Rn, Rt, &dt, &dc);
                for (int e = 0; e < 12; ++e) Rt[e] = Rn[e];
                push(h, dt);
                push(h + 3, dc);
                iterations[p] = k;
                if (recent_mean(h, k) <= tol_t && recent_mean(h + 3, k) <= tol_c) {
                    converged[p] = 1;
                    break;
                }
            }
            nearest_of(bank, pr, Rt, order, idx.data(), d2.data());
            cut_of(d2.data(), pr.n2, m, sc.key, &cut, &icut);
            if (cut_d2) {
                cut_d2[(long long)p * slots + max_iterations] = double_of(cut);
                cut_i_out[(long long)p * slots + max_iterations] = icut;
            }
            double (*part)[10] = sc.parts();
            int found = 0;
            for (int l = 0; l < LANES; ++l) {
                double sum = 0.0;
                for (int i = l; i < pr.n2; i += LANES)
                    if (kept(bits_of(d2[(size_t)i]), i, cut, icut)) sum += d2[(size_t)i];
                part[l][0] = sum;
            }
            for (int i = 0; i < pr.n2; ++i) found += within(d2[(size_t)i], align_radius, r2hi) ? 1 : 0;
            tree_sum<1>(part);
            hits[p] = found;
            ratio[2 * p] = (double)found / (double)pr.n1;
            ratio[2 * p + 1] = (double)found / (double)pr.n2;
            rmse[p] = std::sqrt(part[0][0] / (double)m);
            if (idx_out) std::memcpy(idx_out + (long long)p * Lmax, idx.data(), sizeof(int32_t) * (size_t)pr.n2);
            if (d2_out) std::memcpy(d2_out + (long long)p * Lmax, d2.data(), sizeof(double) * (size_t)pr.n2);
        }
    });
    return USIP_OK;
}

extern "C" int usip_icp_refine_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags,
                                       long long total_rows, const int32_t* perm1, const int32_t* frag1,
                                       const int32_t* frag2, const double* Rt0, const uint8_t* mask, const int32_t* order2,
                                       int P, int Lmax, double inlier_ratio, int max_iterations, double tol_t, double tol_c,
                                       double align_radius, double* Rt_out, int32_t* iterations, uint8_t* converged,
                                       double* rmse, int32_t* hits, double* ratio, double* cut_d2, int32_t* cut_i_out,
                                       int32_t* idx_out, double* d2_out, int num_threads)
{
    return refine_loop(false, rows, row_len, offsets, num_frags, total_rows, perm1, frag1, frag2, Rt0, mask, order2, P, Lmax,
                       inlier_ratio, max_iterations, tol_t, tol_c, align_radius, Rt_out, iterations, converged, rmse, hits,
                       ratio, cut_d2, cut_i_out, idx_out, d2_out, nullptr, num_threads);
}

extern "C" int usip_icp_refine_plane_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags,
                                             long long total_rows, const int32_t* perm1, const int32_t* frag1,
                                             const int32_t* frag2, const double* Rt0, const uint8_t* mask,
                                             const int32_t* order2, int P, int Lmax, double inlier_ratio, int max_iterations,
                                             double tol_t, double tol_c, double align_radius, double* Rt_out,
                                             int32_t* iterations, uint8_t* converged, double* rmse, int32_t* hits,
                                             double* ratio, double* cut_d2, int32_t* cut_i_out, int32_t* idx_out,
                                             double* d2_out, double* fit_sums, int num_threads)
{
    return refine_loop(true, rows, row_len, offsets, num_frags, total_rows, perm1, frag1, frag2, Rt0, mask, order2, P, Lmax,
                       inlier_ratio, max_iterations, tol_t, tol_c, align_radius, Rt_out, iterations, converged, rmse, hits,
                       ratio, cut_d2, cut_i_out, idx_out, d2_out, fit_sums, num_threads);
}
