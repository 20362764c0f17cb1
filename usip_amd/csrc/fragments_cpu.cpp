// usip_amd/csrc/fragments_cpu.cpp -- host twin of csrc/fragments.hip: the same arithmetic
// (csrc/fragments_math.h over csrc/registration_math.h) on host pointers.  RANSAC is csrc/registration_cpu.cpp's; the sums
// here run in the device's order (REFIT_LANES strided partial sums, then the binary tree).  Never reached from the device
// entry points.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "bank.h"
#include "fragments_math.h"
#include "host_split.h"
#include "../../include/usip_hip.h"

using namespace usip_reg;
using namespace usip_frag;
using namespace usip_bank;
using namespace usip_host;

namespace {

template <int K>
void knn_host(const float* a, const float* b, const int32_t* a_count, const int32_t* b_count, float* dist, int32_t* idx,
              int32_t* valid, int B, int C, int Ma, int Nb, int num_threads)
{
    for (int bi = 0; bi < B; ++bi) {
        const int nb = clamp_count(b_count, bi, Nb);
        valid[bi] = nb < K ? nb : K;
    }
    split((long long)B * Ma, num_threads, [=](long long lo, long long hi) {
        for (long long r = lo; r < hi; ++r) {
            const int bi = (int)(r / Ma), i = (int)(r - (long long)bi * Ma);
            const int na = clamp_count(a_count, bi, Ma), nb = clamp_count(b_count, bi, Nb);
            const float* ab = a + (long long)bi * C * Ma;
            const float* bb = b + (long long)bi * C * Nb;
            TopK<K> list;
            list.clear();
            if (i < na)
                for (int j = 0; j < nb; ++j) {
                    float s = 0.f;
                    for (int c = 0; c < C; ++c) {
                        const float df = ab[(long long)c * Ma + i] - bb[(long long)c * Nb + j];
                        s = std::fmaf(df, df, s);
                    }
                    list.offer(std::sqrt(s), j);
                }
            for (int s = 0; s < K; ++s) {
                const bool have = list.j[s] != 0x7fffffff;
                dist[r * K + s] = have ? list.d[s] : INFINITY;
                idx[r * K + s] = have ? list.j[s] : 0;
            }
        }
    });
}

// queries q[3][nq] against the database d[3][nd] sorted along x: the number of queries with a point within the radius
int count_hits(const std::vector<double>& q, int nq, const std::vector<double>& d, int nd, double radius, bool prune,
               int num_threads)
{
    const double r2hi = radius_sq_hi(radius);
    std::vector<int> found((size_t)clamp_threads(num_threads), 0);     // a slot per range
    const double* dx = d.data();
    const double* dy = dx + nd;
    const double* dz = dy + nd;
    split_numbered(nq, num_threads, [&](long long lo, long long hi, int w) {
        int mine = 0;
        for (long long i = lo; i < hi; ++i) {
            const double xi = q[i], yi = q[(size_t)nq + i], zi = q[(size_t)2 * nq + i];
            bool hit = false;
            if (!prune) {
                for (int j = 0; j < nd && !hit; ++j) hit = within(sqdist3(xi, yi, zi, dx[j], dy[j], dz[j]), radius, r2hi);
            } else {
                const int s = (int)(std::lower_bound(dx, dx + nd, xi) - dx);
                for (int j = s; j < nd && !hit; ++j) {                 // outward, until the x-gap alone reaches the radius
                    if (beyond(dx[j] - xi, radius)) break;
                    hit = within(sqdist3(xi, yi, zi, dx[j], dy[j], dz[j]), radius, r2hi);
                }
                for (int j = s - 1; j >= 0 && !hit; --j) {
                    if (beyond(xi - dx[j], radius)) break;
                    hit = within(sqdist3(xi, yi, zi, dx[j], dy[j], dz[j]), radius, r2hi);
                }
            }
            mine += hit ? 1 : 0;
        }
        found[w] = mine;
    });
    int total = 0;
    for (int mine : found) total += mine;
    return total;
}

}  // namespace

extern "C" int usip_knn_nd_counted_f32_cpu(const float* a, const float* b, const int32_t* a_count, const int32_t* b_count,
                                           int k, float* dist, int32_t* idx, int32_t* valid, int B, int C, int Ma, int Nb,
                                           int num_threads)
{
    if (B < 0 || B > 65535 || C < 1 || Ma < 0 || Nb < 1 || k < 1 || k > KMAX) return USIP_EINVAL;
    if ((long long)B * Ma == 0) return USIP_OK;
    if (!a || !b || !a_count || !b_count || !dist || !idx || !valid) return USIP_EINVAL;
    switch (k) {
#define USIP_TOPK_CASE(k_) \
    case k_: knn_host<k_>(a, b, a_count, b_count, dist, idx, valid, B, C, Ma, Nb, num_threads); return USIP_OK
        USIP_TOPK_CASE(1); USIP_TOPK_CASE(2); USIP_TOPK_CASE(3); USIP_TOPK_CASE(4);
        USIP_TOPK_CASE(5); USIP_TOPK_CASE(6); USIP_TOPK_CASE(7); USIP_TOPK_CASE(8);
#undef USIP_TOPK_CASE
    }
    return USIP_EINVAL;
}

extern "C" int usip_match_union_i32_cpu(const int32_t* nn12, const int32_t* nn21, const int32_t* a_count,
                                        const int32_t* p_count, int P, int Ma, int Mp, int k, int32_t* pairs, int32_t* count)
{
    if (P < 0 || P > 65535 || Ma < 1 || Mp < 1 || k < 1 || k > KMAX) return USIP_EINVAL;
    if ((long long)k * ((long long)Ma + Mp) > UNION_MAX) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!nn12 || !nn21 || !a_count || !p_count || !pairs || !count) return USIP_EINVAL;
    const int Cmax = k * (Ma + Mp);
    std::vector<uint32_t> key;
    for (int p = 0; p < P; ++p) {
        const int na = clamp_count(a_count, p, Ma), np = clamp_count(p_count, p, Mp);
        const int k12 = np < k ? np : k, k21 = na < k ? na : k;
        const int32_t* A = nn12 + (long long)p * Ma * k;
        const int32_t* Q = nn21 + (long long)p * Mp * k;
        key.clear();
        for (int i = 0; i < na; ++i)
            for (int c = 0; c < k12; ++c) key.push_back((uint32_t)(i * Mp + clamp_index(A[(long long)i * k + c], Mp)));
        for (int q = 0; q < np; ++q)
            for (int c = 0; c < k21; ++c) key.push_back((uint32_t)(clamp_index(Q[(long long)q * k + c], Ma) * Mp + q));
        std::sort(key.begin(), key.end());
        key.erase(std::unique(key.begin(), key.end()), key.end());
        int32_t* out = pairs + (long long)p * Cmax * 2;
        std::memset(out, 0, (size_t)Cmax * 2 * sizeof(int32_t));
        for (size_t e = 0; e < key.size(); ++e) {
            const int i = (int)(key[e] / (uint32_t)Mp);
            out[2 * e] = i;
            out[2 * e + 1] = (int)key[e] - i * Mp;
        }
        count[p] = (int)key.size();
    }
    return USIP_OK;
}

extern "C" int usip_information_f32_cpu(const float* x, const uint8_t* mask, int P, int Nmax, double* info)
{
    if (P < 0 || P > 65535 || Nmax < 1 || Nmax > NMAX) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!x || !mask || !info) return USIP_EINVAL;
    std::vector<double> part_store((size_t)REFIT_LANES * 10);
    double (*part)[10] = reinterpret_cast<double (*)[10]>(part_store.data());
    for (int p = 0; p < P; ++p) {
        const float* a = x + (long long)p * 3 * Nmax;
        const uint8_t* m = mask + (long long)p * Nmax;
        int n = 0;
        for (int l = 0; l < REFIT_LANES; ++l) {
            double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int i = l; i < Nmax; i += REFIT_LANES)
                if (m[i]) {
                    double t[9];
                    info_terms((double)a[i], (double)a[(long long)Nmax + i], (double)a[2LL * Nmax + i], t);
                    for (int k = 0; k < 9; ++k) s[k] += t[k];
                    ++n;
                }
            for (int k = 0; k < 9; ++k) part[l][k] = s[k];
            part[l][9] = 0.0;
        }
        tree_sum<9>(part);
        double sum[9];
        for (int k = 0; k < 9; ++k) sum[k] = part[0][k];
        info_fill(sum, n, info + (long long)p * 36);
    }
    return USIP_OK;
}

extern "C" int usip_overlap_keys_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags,
                                         long long total_rows, const int32_t* frag2, const double* Rt, int P, int Lmax,
                                         double* keys)
{
    if (!bank_ok(rows, row_len, offsets, num_frags, total_rows, P, Lmax)) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!frag2 || !Rt || !keys) return USIP_EINVAL;
    for (int p = 0; p < P; ++p) {
        const Range r = fragment_range(offsets, num_frags, total_rows, frag2[p], Lmax);
        for (int s = 0; s < Lmax; ++s) {
            double v = INFINITY;
            if (s < r.n) {
                const float* row = rows + (r.first + s) * row_len;
                v = xform(Rt + (long long)p * 12, 0, (double)row[0], (double)row[1], (double)row[2]);
            }
            keys[(long long)p * Lmax + s] = v;
        }
    }
    return USIP_OK;
}

extern "C" int usip_overlap_ratio_f32_cpu(const float* rows, int row_len, const int64_t* offsets, int num_frags,
                                          long long total_rows, const int32_t* frag1, const int32_t* frag2, const double* Rt,
                                          const int32_t* perm1, const int32_t* perm2, int P, int Lmax, double radius,
                                          int prune, int32_t* hits, double* ratio, int num_threads)
{
    if (!bank_ok(rows, row_len, offsets, num_frags, total_rows, P, Lmax) || !(radius > 0.0)) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!frag1 || !frag2 || !Rt || !perm1 || !perm2 || !hits || !ratio) return USIP_EINVAL;
    std::vector<double> a, b;
    for (int p = 0; p < P; ++p) {
        const Range r1 = fragment_range(offsets, num_frags, total_rows, frag1[p], Lmax);
        const Range r2 = fragment_range(offsets, num_frags, total_rows, frag2[p], Lmax);
        const double* G = Rt + (long long)p * 12;
        a.assign((size_t)3 * r1.n, 0.0);                               // both in their sorted order
        b.assign((size_t)3 * r2.n, 0.0);
        for (int s = 0; s < r1.n; ++s) {
            const float* row = rows + (r1.first + safe_index(perm1[r1.first + s], r1.n)) * row_len;
            for (int c = 0; c < 3; ++c) a[(size_t)c * r1.n + s] = (double)row[c];
        }
        for (int s = 0; s < r2.n; ++s) {
            const float* row = rows + (r2.first + safe_index(perm2[(long long)p * Lmax + s], r2.n)) * row_len;
            for (int c = 0; c < 3; ++c)
                b[(size_t)c * r2.n + s] = xform(G, c, (double)row[0], (double)row[1], (double)row[2]);
        }
        hits[2 * p] = r2.n > 0 ? count_hits(a, r1.n, b, r2.n, radius, prune != 0, num_threads) : 0;
        hits[2 * p + 1] = r1.n > 0 ? count_hits(b, r2.n, a, r1.n, radius, prune != 0, num_threads) : 0;
        ratio[2 * p] = r1.n > 0 ? (double)hits[2 * p] / (double)r1.n : 0.0;
        ratio[2 * p + 1] = r2.n > 0 ? (double)hits[2 * p + 1] / (double)r2.n : 0.0;
    }
    return USIP_OK;
}
