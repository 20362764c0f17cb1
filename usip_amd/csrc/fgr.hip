// usip_amd/csrc/fgr.hip -- Fast Global Registration of fragment pairs on the device: the second registrator
// of the reference's indoor evaluation (evaluation/matlab/eval_indoor/fgr/register2FragmentsFGR.m), batched over pairs, one
// workgroup per pair, no launch synchronises.  csrc/fgr_math.h has the arithmetic, which the host twin (csrc/fgr_cpu.cpp)
// shares; include/usip_hip.h (f-12) is the contract.
//
//   fgr_tuples_kernel     256 lanes.  The mutual rows by a workgroup scan (one ballot per wave, then across the waves); the
//                         two means (lane-strided sums, the binary tree) and the scale; the mutual rows' normalised float64
//                         coordinates staged in LDS (48 KB at the limit); then the trials in chunks of 256, in trial order:
//                         one lane per trial, the accept flags scanned the same way, accepted rows written at their scanned
//                         offsets.  The workgroup leaves at the chunk in which the cap fills or the trials end -- the
//                         sequential loop of the original replayed in parallel, as ransac_select_kernel replays ransac.m.
//   fgr_optimize_kernel   256 lanes.  The mutual rows' normalised coordinates staged once in LDS with the tuple rows' 16-bit
//                         indices beside them; the 64 Gauss-Newton steps run inside the kernel.  Per step: every lane adds
//                         its rows into 19 register sums and writes them to LDS; barrier; wave w reduces the sums w, w + 4,
//                         ... (lane l: (p[l] + p[l + 128]) + (p[l + 64] + p[l + 192]), then shuffles for the strides 32 .. 1:
//                         the contract's tree); barrier; every lane solves the 6 x 6 system itself -- the same instructions
//                         on the same values, so all agree and every branch on the result is workgroup-uniform.  The inlier
//                         mask over the mutual rows at the end.
#include "common.h"
#include "fgr_math.h"

using namespace usip_fgr;

namespace {

constexpr int WAVES = LANES / USIP_WAVE;

struct TuplesOut {
    int32_t* mutual;           // [P][M][2]
    int32_t* mutual_count;     // [P]
    double* norm;              // [P][8]
    int32_t* rows;             // [P][ROWS_MAX]
    int32_t* row_count;        // [P]
    int32_t* trials_walked;    // [P]
    int32_t* triples_out;      // [P][T_out][3], optional
    int T_out;
};

// Exclusive scan of one flag per lane over the workgroup: offset of this lane's flag, the workgroup's total.  wave_tot: four
// ints in LDS; the caller puts a barrier between two calls.
__device__ __forceinline__ int block_scan(bool flag, int* wave_tot, int* total)
{
    const unsigned long long mask = __ballot(flag);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wave_tot[w] = __popcll(mask);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) {
        const int c = wave_tot[k];
        before += k < w ? c : 0;
        all += c;
    }
    *total = all;
    return before + usip_mbcnt(mask);
}

template <class Src>
__global__ __launch_bounds__(LANES) void fgr_tuples_kernel(const float* __restrict__ kp1, const float* __restrict__ kp2,
                                                           const int32_t* __restrict__ n1p, const int32_t* __restrict__ n2p,
                                                           const int32_t* __restrict__ nn12, const int32_t* __restrict__ nn21,
                                                           int M, Src src, TuplesOut out)
{
    __shared__ double u[MMAX][6];                          // the mutual rows, normalised; before that the reductions' partials
    __shared__ uint32_t s_mut[MMAX];                       // i | j << 16
    __shared__ double s_norm[8];
    __shared__ int s_wave[WAVES];
    __shared__ int s_fill;
    double (*part)[6] = u;
    const int p = blockIdx.x, l = threadIdx.x;
    const int n1 = clamp_count(n1p, p, M), n2 = clamp_count(n2p, p, M);
    const float* a = kp1 + (long long)p * 3 * M;
    const float* b = kp2 + (long long)p * 3 * M;
    const int32_t* f12 = nn12 + (long long)p * M;
    const int32_t* f21 = nn21 + (long long)p * M;
    int32_t* mutual = out.mutual + (long long)p * M * 2;
    if (l == 0) s_fill = 0;

    // 1. the mutual rows, ascending i
    int nc = 0;
    for (int base = 0; base < n1; base += LANES) {
        const int i = base + l;
        int j = -1;
        if (i < n1) j = f12[i];
        const bool hit = i < n1 && j >= 0 && j < n2 && f21[j] == i;
        int total;
        const int at = nc + block_scan(hit, s_wave, &total);
        if (hit) {
            s_mut[at] = (uint32_t)i | ((uint32_t)j << 16);
            mutual[2 * at] = i;
            mutual[2 * at + 1] = j;
        }
        nc += total;
        __syncthreads();
    }
    for (int c = nc + l; c < M; c += LANES) { mutual[2 * c] = 0; mutual[2 * c + 1] = 0; }

    // 2. the means of ALL keypoints of either fragment, then the scale
    {
        double s[6] = {0, 0, 0, 0, 0, 0};
        for (int i = l; i < n1; i += LANES)
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] += (double)a[(long long)c * M + i];
        for (int i = l; i < n2; i += LANES)
#pragma unroll
            for (int c = 0; c < 3; ++c) s[3 + c] += (double)b[(long long)c * M + i];
#pragma unroll
        for (int c = 0; c < 6; ++c) part[l][c] = s[c];
        for (int st = LANES / 2; st > 0; st >>= 1) {
            __syncthreads();
            if (l < st)
#pragma unroll
                for (int c = 0; c < 6; ++c) part[l][c] += part[l + st][c];
        }
        __syncthreads();
        if (l < 6) s_norm[l] = (l < 3 ? n1 : n2) > 0 ? part[0][l] / (double)(l < 3 ? n1 : n2) : 0.0;
        __syncthreads();
        double best = 0.0;
        for (int i = l; i < n1; i += LANES)
            best = max_nan(best, norm3((double)a[i] - s_norm[0], (double)a[(long long)M + i] - s_norm[1],
                                       (double)a[2LL * M + i] - s_norm[2]));
        for (int i = l; i < n2; i += LANES)
            best = max_nan(best, norm3((double)b[i] - s_norm[3], (double)b[(long long)M + i] - s_norm[4],
                                       (double)b[2LL * M + i] - s_norm[5]));
        part[l][0] = best;
        for (int st = LANES / 2; st > 0; st >>= 1) {
            __syncthreads();
            if (l < st) part[l][0] = max_nan(part[l][0], part[l + st][0]);
        }
        __syncthreads();
        if (l == 0) { s_norm[6] = part[0][0]; s_norm[7] = 0.0; }
        __syncthreads();
        if (l < 8) out.norm[(long long)p * 8 + l] = s_norm[l];
    }
    const double scale = s_norm[6];
    const bool usable = scale_ok(scale);                   // workgroup-uniform
    __syncthreads();                                       // part (= u) has been read

    // 3. the mutual rows, normalised
    for (int c = l; c < nc; c += LANES) {
        const int i = (int)(s_mut[c] & 0xffffu), j = (int)(s_mut[c] >> 16);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            u[c][k] = ((double)a[(long long)k * M + i] - s_norm[k]) / scale;
            u[c][3 + k] = ((double)b[(long long)k * M + j] - s_norm[3 + k]) / scale;
        }
    }
    __syncthreads();

    // 4. the trials, a chunk of one workgroup width at a time
    const int T = usable ? src.trials(nc) : 0;
    int32_t* rows = out.rows + (long long)p * ROWS_MAX;
    int kept = 0, walked = T;
    for (int base = 0; base < T; base += LANES) {
        const int t = base + l;
        bool acc = false;
        int idx[3] = {0, 0, 0};
        if (t < T) {
            src.get(p, t, nc, idx);
            acc = tuple_ok(u[idx[0]], u[idx[1]], u[idx[2]]);
        }
        int total;
        const int k = kept + block_scan(acc, s_wave, &total);
        if (acc && k < TUPLE_CAP) {
            rows[3 * k] = idx[0];
            rows[3 * k + 1] = idx[1];
            rows[3 * k + 2] = idx[2];
            if (k == TUPLE_CAP - 1) s_fill = t + 1;
        }
        kept += total;
        __syncthreads();
        const int fill = s_fill;
        if (out.triples_out && t < T && t < out.T_out && (fill == 0 || t < fill)) {
            int32_t* d = out.triples_out + ((long long)p * out.T_out + t) * 3;
            d[0] = idx[0]; d[1] = idx[1]; d[2] = idx[2];
        }
        if (fill != 0) { walked = fill; break; }           // workgroup-uniform
    }
    kept = kept < TUPLE_CAP ? kept : TUPLE_CAP;
    for (int i = 3 * kept + l; i < ROWS_MAX; i += LANES) rows[i] = 0;
    if (l == 0) {
        out.mutual_count[p] = nc;
        out.row_count[p] = 3 * kept;
        out.trials_walked[p] = walked;
    }
}

__global__ __launch_bounds__(LANES) void fgr_optimize_kernel(const float* __restrict__ kp1, const float* __restrict__ kp2,
                                                             const int32_t* __restrict__ mutual_all,
                                                             const int32_t* __restrict__ mutual_count,
                                                             const double* __restrict__ norm_all,
                                                             const int32_t* __restrict__ rows_all,
                                                             const int32_t* __restrict__ row_count, int M, double threshold,
                                                             double* __restrict__ Rt_out, uint8_t* __restrict__ valid,
                                                             uint8_t* __restrict__ inlier_mask, int32_t* __restrict__ inliers)
{
    __shared__ double u[MMAX][6];                          // 49 152 B
    __shared__ double part[NSUM][LANES];                   // 38 912 B
    __shared__ double sums[NSUM];
    __shared__ double s_Rt[12];
    __shared__ uint16_t s_row[ROWS_MAX];                   // 6 000 B
    __shared__ int s_inl;
    const int p = blockIdx.x, l = threadIdx.x;
    const int lane = l & 63, w = __builtin_amdgcn_readfirstlane(l >> 6);
    const int nc = clamp_count(mutual_count, p, M);
    const int nr = clamp_count(row_count, p, ROWS_MAX);
    const float* a = kp1 + (long long)p * 3 * M;
    const float* b = kp2 + (long long)p * 3 * M;
    const int32_t* mutual = mutual_all + (long long)p * M * 2;
    const double* norm = norm_all + (long long)p * 8;
    const int32_t* rows = rows_all + (long long)p * ROWS_MAX;
    const double scale = norm[6];
    bool ok = scale_ok(scale) && nr >= MIN_ROWS && nc >= 1;    // workgroup-uniform, here and below
    if (l == 0) s_inl = 0;

    if (ok) {
        for (int c = l; c < nc; c += LANES) {
            const int i = usip_reg::clamp_index(mutual[2 * c], M), j = usip_reg::clamp_index(mutual[2 * c + 1], M);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                u[c][k] = ((double)a[(long long)k * M + i] - norm[k]) / scale;
                u[c][3 + k] = ((double)b[(long long)k * M + j] - norm[3 + k]) / scale;
            }
        }
        for (int r = l; r < nr; r += LANES) s_row[r] = (uint16_t)usip_reg::clamp_index(rows[r], nc);
    }
    __syncthreads();

    Pose pose;
    pose_identity(pose);
    double par = 1.0;
    if (ok) {
        for (int it = 0; it < ITERATIONS; ++it) {
            par = next_par(par, it);
            double S[NSUM];
#pragma unroll
            for (int k = 0; k < NSUM; ++k) S[k] = 0.0;
            for (int r = l; r < nr; r += LANES) sums_of_row(S, pose, u[s_row[r]], par);
#pragma unroll
            for (int k = 0; k < NSUM; ++k) part[k][l] = S[k];
            __syncthreads();
            for (int k = w; k < NSUM; k += WAVES) {
                double v = (part[k][lane] + part[k][lane + 128]) + (part[k][lane + 64] + part[k][lane + 192]);
#pragma unroll
                for (int st = 32; st > 0; st >>= 1) v += __shfl_down(v, st);
                if (lane == 0) sums[k] = v;
            }
            __syncthreads();
            double Ss[NSUM], x[6];
#pragma unroll
            for (int k = 0; k < NSUM; ++k) Ss[k] = sums[k];
            ok = solve6(Ss, x);
            if (!ok) break;
            apply_step(pose, x);
        }
    }

    if (l == 0) {
        double Rt[12];
        if (ok) denormalise(pose, norm, Rt);
        else identity_Rt(Rt);
#pragma unroll
        for (int k = 0; k < 12; ++k) { s_Rt[k] = Rt[k]; Rt_out[(long long)p * 12 + k] = Rt[k]; }
        valid[p] = ok ? 1 : 0;
    }
    __syncthreads();
    double Rt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = s_Rt[k];
    int mine = 0;
    uint8_t* mask = inlier_mask + (long long)p * M;
    for (int c = l; c < M; c += LANES) {
        bool in = false;
        if (ok && c < nc) {
            const int i = usip_reg::clamp_index(mutual[2 * c], M), j = usip_reg::clamp_index(mutual[2 * c + 1], M);
            in = usip_reg::residual(Rt, (double)a[i], (double)a[(long long)M + i], (double)a[2LL * M + i], (double)b[j],
                                    (double)b[(long long)M + j], (double)b[2LL * M + j]) < threshold;
        }
        mask[c] = in ? 1 : 0;
        mine += in ? 1 : 0;
    }
    if (mine) atomicAdd(&s_inl, mine);
    __syncthreads();
    if (l == 0) inliers[p] = s_inl;
}

bool shape_ok(int P, int M) { return P >= 0 && P <= 65535 && M >= 1 && M <= MMAX; }

template <class Src>
int launch_tuples(const float* kp1, const float* kp2, const int32_t* n1, const int32_t* n2, const int32_t* nn12,
                  const int32_t* nn21, int P, int M, const Src& src, const TuplesOut& out, hipStream_t stream)
{
    USIP_LAUNCH(fgr_tuples_kernel<Src>, dim3(P), dim3(LANES), 0, stream, kp1, kp2, n1, n2, nn12, nn21, M, src, out);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}

}  // namespace

extern "C" int usip_fgr_tuples_f32(const float* kp1, const float* kp2, const int32_t* n1, const int32_t* n2,
                                   const int32_t* nn12, const int32_t* nn21, int P, int M, uint64_t seed,
                                   const int64_t* pair_ids, int32_t* mutual, int32_t* mutual_count, double* norm,
                                   int32_t* rows, int32_t* row_count, int32_t* trials_walked, int32_t* triples_out, int T_out,
                                   void* stream)
{
    if (!shape_ok(P, M) || (triples_out && T_out < 1)) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!kp1 || !kp2 || !n1 || !n2 || !nn12 || !nn21 || !mutual || !mutual_count || !norm || !rows || !row_count ||
        !trials_walked)
        return USIP_EINVAL;
    const TuplesOut out{mutual, mutual_count, norm, rows, row_count, trials_walked, triples_out, triples_out ? T_out : 0};
    return launch_tuples(kp1, kp2, n1, n2, nn12, nn21, P, M, PhiloxTriples{seed, pair_ids}, out, (hipStream_t)stream);
}

extern "C" int usip_fgr_tuples_explicit_f32(const float* kp1, const float* kp2, const int32_t* n1, const int32_t* n2,
                                            const int32_t* nn12, const int32_t* nn21, int P, int M, const int32_t* triples,
                                            int T, int32_t* mutual, int32_t* mutual_count, double* norm, int32_t* rows,
                                            int32_t* row_count, int32_t* trials_walked, void* stream)
{
    if (!shape_ok(P, M) || T < 1) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!kp1 || !kp2 || !n1 || !n2 || !nn12 || !nn21 || !triples || !mutual || !mutual_count || !norm || !rows ||
        !row_count || !trials_walked)
        return USIP_EINVAL;
    const TuplesOut out{mutual, mutual_count, norm, rows, row_count, trials_walked, nullptr, 0};
    return launch_tuples(kp1, kp2, n1, n2, nn12, nn21, P, M, ExplicitTriples{triples, T}, out, (hipStream_t)stream);
}

extern "C" int usip_fgr_optimize_f32(const float* kp1, const float* kp2, const int32_t* mutual, const int32_t* mutual_count,
                                     const double* norm, const int32_t* rows, const int32_t* row_count, int P, int M,
                                     double threshold, double* Rt, uint8_t* valid, uint8_t* inlier_mask, int32_t* inliers,
                                     void* stream)
{
    if (!shape_ok(P, M)) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!kp1 || !kp2 || !mutual || !mutual_count || !norm || !rows || !row_count || !Rt || !valid || !inlier_mask || !inliers)
        return USIP_EINVAL;
    USIP_LAUNCH(fgr_optimize_kernel, dim3(P), dim3(LANES), 0, (hipStream_t)stream, kp1, kp2, mutual, mutual_count, norm, rows,
                row_count, M, threshold, Rt, valid, inlier_mask, inliers);
    USIP_LAUNCH_CHECK();
    return USIP_OK;
}
