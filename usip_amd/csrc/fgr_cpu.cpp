// usip_amd/csrc/fgr_cpu.cpp -- host twin of csrc/fgr.hip: the same draws and arithmetic (csrc/fgr_math.h)
// on host pointers.  The trials run as the sequential loop they replay; every sum is taken in the device's order (LANES
// strided partial sums, then the binary tree).  num_threads splits the pairs.  Never reached from the device entry points.
#include <cmath>
#include <cstring>
#include <vector>
#include "fgr_math.h"
#include "host_split.h"
#include "../../include/usip_hip.h"

using namespace usip_fgr;

namespace {

bool shape_ok(int P, int M) { return P >= 0 && P <= 65535 && M >= 1 && M <= MMAX; }

struct TuplesOut {
    int32_t* mutual;
    int32_t* mutual_count;
    double* norm;
    int32_t* rows;
    int32_t* row_count;
    int32_t* trials_walked;
    int32_t* triples_out;
    int T_out;
};

// u f64 [nc][6]: the mutual rows, normalised
void normalise_rows(const float* a, const float* b, const int32_t* mutual, int nc, int M, const double* norm, double* u)
{
    for (int c = 0; c < nc; ++c) {
        const int i = usip_reg::clamp_index(mutual[2 * c], M), j = usip_reg::clamp_index(mutual[2 * c + 1], M);
        for (int k = 0; k < 3; ++k) {
            u[6 * c + k] = ((double)a[(long long)k * M + i] - norm[k]) / norm[6];
            u[6 * c + 3 + k] = ((double)b[(long long)k * M + j] - norm[3 + k]) / norm[6];
        }
    }
}

template <class Src>
void tuples_range(const float* kp1, const float* kp2, const int32_t* n1p, const int32_t* n2p, const int32_t* nn12,
                  const int32_t* nn21, int M, const Src& src, const TuplesOut& out, int lo, int hi)
{
    std::vector<double> u((size_t)MMAX * 6), part(LANES);
    for (int p = lo; p < hi; ++p) {
        const int n1 = clamp_count(n1p, p, M), n2 = clamp_count(n2p, p, M);
        const float* a = kp1 + (long long)p * 3 * M;
        const float* b = kp2 + (long long)p * 3 * M;
        const int32_t* f12 = nn12 + (long long)p * M;
        const int32_t* f21 = nn21 + (long long)p * M;
        int32_t* mutual = out.mutual + (long long)p * M * 2;
        double* norm = out.norm + (long long)p * 8;
        int32_t* rows = out.rows + (long long)p * ROWS_MAX;
        std::memset(mutual, 0, sizeof(int32_t) * 2 * (size_t)M);
        std::memset(rows, 0, sizeof(int32_t) * ROWS_MAX);
        int nc = 0;
        for (int i = 0; i < n1; ++i) {
            const int j = f12[i];
            if (j >= 0 && j < n2 && f21[j] == i) {
                mutual[2 * nc] = i;
                mutual[2 * nc + 1] = j;
                ++nc;
            }
        }
        for (int c = 0; c < 6; ++c) {
            const float* x = (c < 3 ? a : b) + (long long)(c % 3) * M;
            const int n = c < 3 ? n1 : n2;
            for (int l = 0; l < LANES; ++l) {
                double s = 0.0;
                for (int i = l; i < n; i += LANES) s += (double)x[i];
                part[l] = s;
            }
            norm[c] = n > 0 ? tree256(part.data()) / (double)n : 0.0;
        }
        double scale = 0.0;
        for (int i = 0; i < n1; ++i)
            scale = max_nan(scale, norm3((double)a[i] - norm[0], (double)a[(long long)M + i] - norm[1],
                                         (double)a[2LL * M + i] - norm[2]));
        for (int i = 0; i < n2; ++i)
            scale = max_nan(scale, norm3((double)b[i] - norm[3], (double)b[(long long)M + i] - norm[4],
                                         (double)b[2LL * M + i] - norm[5]));
        norm[6] = scale;
        norm[7] = 0.0;
        int kept = 0, walked = 0;
        if (scale_ok(scale)) {
            normalise_rows(a, b, mutual, nc, M, norm, u.data());
            const int T = src.trials(nc);
            walked = T;
            for (int t = 0; t < T; ++t) {
                int idx[3];
                src.get(p, t, nc, idx);
                if (out.triples_out && t < out.T_out) {
                    int32_t* d = out.triples_out + ((long long)p * out.T_out + t) * 3;
                    d[0] = idx[0]; d[1] = idx[1]; d[2] = idx[2];
                }
                if (!tuple_ok(&u[6 * idx[0]], &u[6 * idx[1]], &u[6 * idx[2]])) continue;
                rows[3 * kept] = idx[0];
                rows[3 * kept + 1] = idx[1];
                rows[3 * kept + 2] = idx[2];
                if (++kept == TUPLE_CAP) {
                    walked = t + 1;
                    break;
                }
            }
        }
        out.mutual_count[p] = nc;
        out.row_count[p] = 3 * kept;
        out.trials_walked[p] = walked;
    }
}

void optimize_range(const float* kp1, const float* kp2, const int32_t* mutual_all, const int32_t* mutual_count,
                    const double* norm_all, const int32_t* rows_all, const int32_t* row_count, int M, double threshold,
                    double* Rt_out, uint8_t* valid, uint8_t* inlier_mask, int32_t* inliers, int lo, int hi)
{
    std::vector<double> u((size_t)MMAX * 6), part((size_t)NSUM * LANES);
    std::vector<int> row(ROWS_MAX);
    for (int p = lo; p < hi; ++p) {
        const int nc = clamp_count(mutual_count, p, M), nr = clamp_count(row_count, p, ROWS_MAX);
        const float* a = kp1 + (long long)p * 3 * M;
        const float* b = kp2 + (long long)p * 3 * M;
        const int32_t* mutual = mutual_all + (long long)p * M * 2;
        const double* norm = norm_all + (long long)p * 8;
        const int32_t* rows = rows_all + (long long)p * ROWS_MAX;
        bool ok = scale_ok(norm[6]) && nr >= MIN_ROWS && nc >= 1;
        Pose pose;
        pose_identity(pose);
        if (ok) {
            normalise_rows(a, b, mutual, nc, M, norm, u.data());
            for (int r = 0; r < nr; ++r) row[r] = usip_reg::clamp_index(rows[r], nc);
            double par = 1.0;
            for (int it = 0; it < ITERATIONS; ++it) {
                par = next_par(par, it);
                for (int l = 0; l < LANES; ++l) {
                    double S[NSUM];
                    for (int k = 0; k < NSUM; ++k) S[k] = 0.0;
                    for (int r = l; r < nr; r += LANES) sums_of_row(S, pose, &u[6 * row[r]], par);
                    for (int k = 0; k < NSUM; ++k) part[(size_t)k * LANES + l] = S[k];
                }
                double Ss[NSUM], x[6];
                for (int k = 0; k < NSUM; ++k) Ss[k] = tree256(&part[(size_t)k * LANES]);
                ok = solve6(Ss, x);
                if (!ok) break;
                apply_step(pose, x);
            }
        }
        double Rt[12];
        if (ok) denormalise(pose, norm, Rt);
        else identity_Rt(Rt);
        for (int k = 0; k < 12; ++k) Rt_out[(long long)p * 12 + k] = Rt[k];
        valid[p] = ok ? 1 : 0;
        uint8_t* mask = inlier_mask + (long long)p * M;
        int count = 0;
        for (int c = 0; c < M; ++c) {
            bool in = false;
            if (ok && c < nc) {
                const int i = usip_reg::clamp_index(mutual[2 * c], M), j = usip_reg::clamp_index(mutual[2 * c + 1], M);
                in = usip_reg::residual(Rt, (double)a[i], (double)a[(long long)M + i], (double)a[2LL * M + i], (double)b[j],
                                        (double)b[(long long)M + j], (double)b[2LL * M + j]) < threshold;
            }
            mask[c] = in ? 1 : 0;
            count += in ? 1 : 0;
        }
        inliers[p] = count;
    }
}

}  // namespace

extern "C" int usip_fgr_tuples_f32_cpu(const float* kp1, const float* kp2, const int32_t* n1, const int32_t* n2,
                                       const int32_t* nn12, const int32_t* nn21, int P, int M, uint64_t seed,
                                       const int64_t* pair_ids, const int32_t* triples, int T, int32_t* mutual,
                                       int32_t* mutual_count, double* norm, int32_t* rows, int32_t* row_count,
                                       int32_t* trials_walked, int32_t* triples_out, int T_out, int num_threads)
{
    if (!shape_ok(P, M) || (triples && T < 1) || (triples_out && T_out < 1)) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!kp1 || !kp2 || !n1 || !n2 || !nn12 || !nn21 || !mutual || !mutual_count || !norm || !rows || !row_count ||
        !trials_walked)
        return USIP_EINVAL;
    const TuplesOut out{mutual, mutual_count, norm, rows, row_count, trials_walked, triples_out, triples_out ? T_out : 0};
    if (triples) {
        const ExplicitTriples src{triples, T};
        usip_host::split(P, num_threads, [&](int lo, int hi) { tuples_range(kp1, kp2, n1, n2, nn12, nn21, M, src, out, lo, hi); });
    } else {
        const PhiloxTriples src{seed, pair_ids};
        usip_host::split(P, num_threads, [&](int lo, int hi) { tuples_range(kp1, kp2, n1, n2, nn12, nn21, M, src, out, lo, hi); });
    }
    return USIP_OK;
}

extern "C" int usip_fgr_tuples_explicit_f32_cpu(const float* kp1, const float* kp2, const int32_t* n1, const int32_t* n2,
                                                const int32_t* nn12, const int32_t* nn21, int P, int M, const int32_t* triples,
                                                int T, int32_t* mutual, int32_t* mutual_count, double* norm, int32_t* rows,
                                                int32_t* row_count, int32_t* trials_walked, int num_threads)
{
    if (!triples) return USIP_EINVAL;
    return usip_fgr_tuples_f32_cpu(kp1, kp2, n1, n2, nn12, nn21, P, M, 0, nullptr, triples, T, mutual, mutual_count, norm, rows,
                                   row_count, trials_walked, nullptr, 0, num_threads);
}

extern "C" int usip_fgr_optimize_f32_cpu(const float* kp1, const float* kp2, const int32_t* mutual,
                                         const int32_t* mutual_count, const double* norm, const int32_t* rows,
                                         const int32_t* row_count, int P, int M, double threshold, double* Rt, uint8_t* valid,
                                         uint8_t* inlier_mask, int32_t* inliers, int num_threads)
{
    if (!shape_ok(P, M)) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!kp1 || !kp2 || !mutual || !mutual_count || !norm || !rows || !row_count || !Rt || !valid || !inlier_mask || !inliers)
        return USIP_EINVAL;
    usip_host::split(P, num_threads, [&](int lo, int hi) {
        optimize_range(kp1, kp2, mutual, mutual_count, norm, rows, row_count, M, threshold, Rt, valid, inlier_mask, inliers,
                       lo, hi);
    });
    return USIP_OK;
}

extern "C" int usip_fgr_sincos_f64_cpu(const double* x, int n, double* sin_out, double* cos_out)
{
    if (n < 0) return USIP_EINVAL;
    if (n == 0) return USIP_OK;
    if (!x || !sin_out || !cos_out) return USIP_EINVAL;
    for (int i = 0; i < n; ++i) fgr_sincos(x[i], sin_out + i, cos_out + i);
    return USIP_OK;
}
