// usip_amd/csrc/ground_truth_cpu.cpp -- host twin of csrc/ground_truth.hip: the same arithmetic
// (csrc/ground_truth_math.h over csrc/fragments_math.h) on host pointers.  The reach twin tests the rows of fragment 1 for
// every row of fragment 2 in ascending row order (prune = 0: all of them; otherwise outward along x until the gap alone
// reaches `far`); the information twin adds in the device's order (256 strided partial sums, then the binary tree).  Never
// reached from the device entry points.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "bank.h"
#include "ground_truth_math.h"
#include "host_split.h"
#include "../../include/usip_hip.h"

using namespace usip_gt;
using namespace usip_frag;
using namespace usip_bank;
using usip_host::split;
using usip_reg::clamp_count;
using usip_reg::clamp_index;
using usip_reg::tree_sum;

extern "C" int usip_gt_reach_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags,
                                     long long total_rows, const int32_t* perm1, const int32_t* frag1, const int32_t* frag2,
                                     const double* Rt, const uint8_t* mask, int P, int Lmax, double far_radius,
                                     double near_radius, uint64_t seed, const int64_t* pair_ids, int prune, uint8_t* cls,
                                     int32_t* hits, double* ratio, uint64_t* key, int num_threads)
{
    if (!bank_ok(rows, row_len, offsets, num_frags, total_rows, P, Lmax) || !(near_radius > 0.0) ||
        !(far_radius > near_radius))
        return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!perm1 || !frag1 || !frag2 || !Rt || !cls || !hits || !ratio || !key) return USIP_EINVAL;
    const double far2hi = radius_sq_hi(far_radius), near2hi = radius_sq_hi(near_radius);
    split(P, num_threads, [&](long long lo, long long hi) {
        std::vector<double> a;                                         // fragment 1 along x: x[n1], y[n1], z[n1]
        for (long long p = lo; p < hi; ++p) {
            uint8_t* c = cls + p * Lmax;
            uint64_t* k = key + p * Lmax;
            std::memset(c, 0, (size_t)Lmax);
            std::fill(k, k + Lmax, KEY_NONE);
            hits[2 * p] = hits[2 * p + 1] = 0;
            ratio[2 * p] = ratio[2 * p + 1] = 0.0;
            if (mask && mask[p] == 0) continue;
            const Range r1 = fragment_range(offsets, num_frags, total_rows, frag1[p], Lmax);
            const Range r2 = fragment_range(offsets, num_frags, total_rows, frag2[p], Lmax);
            const int n1 = r1.n, n2 = r2.n;
            if (n1 < 1 || n2 < 1) continue;
            const double* G = Rt + p * 12;
            a.assign((size_t)3 * n1, 0.0);
            for (int s = 0; s < n1; ++s) {
                const float* row = rows + (r1.first + (prune ? safe_index(perm1[r1.first + s], n1) : s)) * row_len;
                for (int d = 0; d < 3; ++d) a[(size_t)d * n1 + s] = (double)row[d];
            }
            const double* ax = a.data();
            const double* ay = ax + n1;
            const double* az = ay + n1;
            const uint64_t id = pair_ids ? (uint64_t)pair_ids[p] : (uint64_t)p;
            int reached = 0, close = 0;
            for (int i = 0; i < n2; ++i) {
                const float* b = rows + (r2.first + i) * row_len;
                const double b0 = (double)b[0], b1 = (double)b[1], b2 = (double)b[2];
                const double qx = xform(G, 0, b0, b1, b2), qy = xform(G, 1, b0, b1, b2), qz = xform(G, 2, b0, b1, b2);
                double best = INFINITY;
                if (!prune) {
                    for (int j = 0; j < n1; ++j) best = std::min(best, sqdist3(qx, qy, qz, ax[j], ay[j], az[j]));
                } else {
                    const int s = (int)(std::lower_bound(ax, ax + n1, qx) - ax);
                    for (int j = s; j < n1 && !beyond(ax[j] - qx, far_radius); ++j)
                        best = std::min(best, sqdist3(qx, qy, qz, ax[j], ay[j], az[j]));
                    for (int j = s - 1; j >= 0 && !beyond(qx - ax[j], far_radius); --j)
                        best = std::min(best, sqdist3(qx, qy, qz, ax[j], ay[j], az[j]));
                }
                c[i] = reach_class(best, far_radius, far2hi, near_radius, near2hi);
                if (c[i] == 2) k[i] = selection_key(seed, id, (uint64_t)i);
                reached += c[i] >= 1;
                close += c[i] == 2;
            }
            hits[2 * p] = reached;
            hits[2 * p + 1] = close;
            ratio[2 * p] = (double)reached / (double)n1;
            ratio[2 * p + 1] = (double)reached / (double)n2;
        }
    });
    return USIP_OK;
}

extern "C" int usip_gt_information_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags,
                                           long long total_rows, const int32_t* frag2, const double* Rt, const int32_t* order,
                                           const int32_t* count, int P, int Lmax, int cap, double* info, int num_threads)
{
    if (!bank_ok(rows, row_len, offsets, num_frags, total_rows, P, Lmax) || cap < 1 || cap > CAP_MAX) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!frag2 || !Rt || !order || !count || !info) return USIP_EINVAL;
    split(P, num_threads, [&](long long lo, long long hi) {
        std::vector<double> buf((size_t)LANES * 10);
        double (*part)[10] = reinterpret_cast<double (*)[10]>(buf.data());
        for (long long p = lo; p < hi; ++p) {
            const Range r2 = fragment_range(offsets, num_frags, total_rows, frag2[p], Lmax);
            const int n = r2.n >= 1 ? clamp_count(count, (int)p, cap) : 0;
            const double* G = Rt + p * 12;
            const float* rows2 = rows + r2.first * row_len;
            for (int l = 0; l < LANES; ++l) {
                double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                int mine = 0;
                for (int at = l; at < n; at += LANES) {
                    const float* b = rows2 + (long long)clamp_index(order[p * cap + at], r2.n) * row_len;
                    const double b0 = (double)b[0], b1 = (double)b[1], b2 = (double)b[2];
                    double t[9];
                    gt_terms(xform(G, 0, b0, b1, b2), xform(G, 1, b0, b1, b2), xform(G, 2, b0, b1, b2), t);
                    for (int k = 0; k < 9; ++k) s[k] += t[k];
                    ++mine;
                }
                for (int k = 0; k < 9; ++k) part[l][k] = s[k];
                part[l][9] = (double)mine;
            }
            tree_sum<10>(part);
            double sum[9];
            for (int k = 0; k < 9; ++k) sum[k] = part[0][k];
            info_fill(sum, (int)part[0][9], info + p * 36);
        }
    });
    return USIP_OK;
}
