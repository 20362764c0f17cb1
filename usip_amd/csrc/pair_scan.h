// usip_amd/csrc/pair_scan.h -- the two index-order pair scans of the step, as wave-level device functions.
//
// ball_query_coords.hip and nearest.hip run them for every row; cell_grid.hip runs them, inside its own launches,
// for the rows its grid cannot answer.  One copy of each loop, so both routes give the same bits.
#pragma once
#include "common.h"
#include <cmath>
#include <limits>

// Largest float T with sqrt_rn(T) <= radius (host sqrtf and the device's __fsqrt_rn are both
// correctly rounded IEEE operations, so the threshold can be derived on the host).
static inline float usip_sqrt_threshold(float radius)
{
    if (!(radius >= 0.0f)) return -1.0f;     // negative or NaN radius: sqrt(s) <= r never holds
    if (std::isinf(radius)) return radius;
    float t = radius * radius;
    if (std::isinf(t)) t = std::numeric_limits<float>::max();
    for (int i = 0; i < 8 && sqrtf(t) > radius; ++i) t = std::nextafterf(t, -1.0f);
    for (int i = 0; i < 8; ++i) {
        const float up = std::nextafterf(t, std::numeric_limits<float>::infinity());
        if (!std::isinf(up) && sqrtf(up) <= radius) t = up; else break;
    }
    return t;
}

// Ball query, index order: a wave owns the R node rows m0 .. m0+R-1 of one cloud (nb [3][M], xb [3][N]), streams the
// cloud once for all of them and keeps the first K hits (s <= T) of row r in lists[r * K ..]; count[r] = hits seen
// (>= K: the row is full; rows past M start full).  Stops as soon as every row is full.
template <bool VEC, int R>
__device__ __forceinline__ void usip_ball_scan_rows(const float* __restrict__ nb, const float* __restrict__ xb,
                                                    int* lists, int (&count)[R], float T, int K, int M, int N,
                                                    int m0, int lane)
{
    float ax[R], ay[R], az[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int m = min(m0 + r, M - 1);
        ax[r] = nb[m]; ay[r] = nb[M + m]; az[r] = nb[2 * M + m];
        count[r] = (m0 + r < M) ? 0 : K;                  // rows past the end are "done"
    }
    if (m0 < M) {
        constexpr int STEP = VEC ? 256 : 64;
        // The scan is bound by load latency (one L2 round trip per 256 points if the loads are issued where
        // they are used): the next block of points is fetched, from a clamped address, before the current one
        // is tested.
        float4 nx = make_float4(0, 0, 0, 0), ny = nx, nz = nx;
        if (VEC) {
            const int i = min(lane * 4, N - 4);
            nx = *reinterpret_cast<const float4*>(xb + i);
            ny = *reinterpret_cast<const float4*>(xb + N + i);
            nz = *reinterpret_cast<const float4*>(xb + 2 * N + i);
        }
        for (int base = 0; base < N; base += STEP) {
            bool done = true;
#pragma unroll
            for (int r = 0; r < R; ++r) done = done && (count[r] >= K);
            if (done) break;
            unsigned bits[R];
            unsigned any = 0;
            if (VEC) {
                const int i = base + lane * 4;
                const float4 px = nx, py = ny, pz = nz;
                const bool ok = i < N;
                {
                    const int in = min(i + STEP, N - 4);
                    nx = *reinterpret_cast<const float4*>(xb + in);
                    ny = *reinterpret_cast<const float4*>(xb + N + in);
                    nz = *reinterpret_cast<const float4*>(xb + 2 * N + in);
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    // two points per packed instruction (same arithmetic, bit for bit)
                    const usip_f32x2 rx = {ax[r], ax[r]}, ry = {ay[r], ay[r]}, rz = {az[r], az[r]};
                    const usip_f32x2 s01 = usip_sqdist2(rx, ry, rz, usip_f32x2{px.x, px.y}, usip_f32x2{py.x, py.y},
                                                        usip_f32x2{pz.x, pz.y});
                    const usip_f32x2 s23 = usip_sqdist2(rx, ry, rz, usip_f32x2{px.z, px.w}, usip_f32x2{py.z, py.w},
                                                        usip_f32x2{pz.z, pz.w});
                    unsigned h = (s01.x <= T ? 1u : 0u) | (s01.y <= T ? 2u : 0u) | (s23.x <= T ? 4u : 0u) |
                                 (s23.y <= T ? 8u : 0u);
                    bits[r] = (ok && count[r] < K) ? h : 0u;
                    any |= bits[r];
                }
            } else {
                const int i = base + lane;
                const bool ok = i < N;
                const float px = ok ? xb[i] : 0.f, py = ok ? xb[N + i] : 0.f, pz = ok ? xb[2 * N + i] : 0.f;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    unsigned h = usip_sqdist(ax[r], ay[r], az[r], px, py, pz) <= T ? 1u : 0u;
                    bits[r] = (ok && count[r] < K) ? h : 0u;
                    any |= bits[r];
                }
            }
            if (__ballot(any != 0u) == 0ull) continue;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                int* list = lists + r * K;
                if (VEC) {
                    unsigned long long m0b = __ballot(bits[r] & 1u), m1b = __ballot(bits[r] & 2u);
                    unsigned long long m2b = __ballot(bits[r] & 4u), m3b = __ballot(bits[r] & 8u);
                    if ((m0b | m1b | m2b | m3b) == 0ull) continue;
                    int p = count[r] + usip_mbcnt(m0b) + usip_mbcnt(m1b) + usip_mbcnt(m2b) + usip_mbcnt(m3b);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (bits[r] & (1u << j)) {
                            if (p < K) list[p] = base + lane * 4 + j;
                            ++p;
                        }
                    }
                    count[r] += __popcll(m0b) + __popcll(m1b) + __popcll(m2b) + __popcll(m3b);
                } else {
                    unsigned long long mb = __ballot(bits[r] & 1u);
                    if (mb == 0ull) continue;
                    int p = count[r] + usip_mbcnt(mb);
                    if ((bits[r] & 1u) && p < K) list[p] = base + lane;
                    count[r] += __popcll(mb);
                }
            }
        }
    }
}

// The rows' output, after a workgroup barrier behind whatever filled the lists: the first min(count, K) entries,
// repeated cyclically; zeros for an empty ball.  orow0 = out + (b * M + m0) * K.
template <int R>
__device__ __forceinline__ void usip_ball_write_rows(const int* lists, const int (&count)[R], int32_t* orow0, int K,
                                                     int M, int m0, int lane)
{
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int m = m0 + r;
        if (m < M) {
            const int u = min(count[r], K);
            int32_t* orow = orow0 + (long long)r * K;
            for (int j = lane; j < K; j += 64) orow[j] = (u > 0) ? lists[r * K + (j % u)] : 0;
        }
    }
}

// Nearest candidate, index order: a wave owns the R queries i0 .. i0+R-1 of one cloud (ab [3][Ma]) and scans the
// candidates [jbeg, jend) of bb [3][Nb].  In lane 0, d[r] = min_j sqrt(s_j) and j[r] = the FIRST index attaining it
// (0x7fffffff for an empty or all-NaN chunk).
template <int R>
__device__ __forceinline__ void usip_nearest_scan(const float* __restrict__ ab, const float* __restrict__ bb,
                                                  int Ma, int Nb, int jbeg, int jend, int i0, int lane,
                                                  float (&best_d)[R], int (&best_j)[R])
{
    float ax[R], ay[R], az[R], best_s[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = min(i0 + r, Ma - 1);
        ax[r] = ab[i]; ay[r] = ab[Ma + i]; az[r] = ab[2 * Ma + i];
        best_s[r] = __builtin_inff(); best_d[r] = __builtin_inff(); best_j[r] = 0x7fffffff;
    }
    static_assert(R % 2 == 0, "queries are processed in pairs");
    usip_f32x2 qx[R / 2], qy[R / 2], qz[R / 2];
#pragma unroll
    for (int r = 0; r < R / 2; ++r) {
        qx[r] = usip_f32x2{ax[2 * r], ax[2 * r + 1]};
        qy[r] = usip_f32x2{ay[2 * r], ay[2 * r + 1]};
        qz[r] = usip_f32x2{az[2 * r], az[2 * r + 1]};
    }
    // The reference-exact rule -- the correctly rounded sqrt of every candidate that improves a lane's running minimum of
    // the SQUARED distance, first index kept on equal distances -- cost 70 of the kernel's 95 us: some lane of the wave
    // improves in more than half of the iterations, and hipcc predicates the sqrt into all of them.  Instead (r03):
    //   * one branch-free scan keeps, per lane and query, the strict running minimum s0 of the squared distance with its
    //     index j0 and the minimum it replaced, s1.  min_j sqrt(s_j) = sqrt(min_j s_j) (the rounded sqrt is monotone), and
    //     every candidate whose sqrt rounds to that value has s_j <= smin (1 + 2^-22 + ...): only candidates with
    //     s_j <= thr = smin (1 + 2^-20) can be the answer.  The FIRST of them is a strict running minimum of its lane
    //     (everything before it in the lane lies above thr), and the qualifying running minima of a lane are the tail
    //     of its sequence: if s1 > thr the lane's only qualifying candidate is (s0, j0);
    //   * a wave in which some lane has s1 <= thr as well (two candidates within 1e-6 of the minimum in one lane, or an
    //     empty / all-NaN chunk) settles the question by the exact scan below.
    // UNR candidates per lane and iteration, all their loads issued before the first is used (one candidate per iteration
    // was a chain of L2 latencies); the tail repeats the chunk's last candidate, which is never a strict improvement.
    constexpr int UNR = 4;
    float s1[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { best_s[r] = __builtin_inff(); s1[r] = __builtin_inff(); }
    for (int j0 = jbeg + lane; j0 < jend; j0 += 64 * UNR) {
        float bx[UNR], by[UNR], bz[UNR];
        int jj[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            jj[u] = min(j0 + 64 * u, jend - 1);
            bx[u] = bb[jj[u]]; by[u] = bb[Nb + jj[u]]; bz[u] = bb[2 * Nb + jj[u]];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const usip_f32x2 cx = {bx[u], bx[u]}, cy = {by[u], by[u]}, cz = {bz[u], bz[u]};
#pragma unroll
            for (int r2 = 0; r2 < R / 2; ++r2) {
                const usip_f32x2 s2 = usip_sqdist2(qx[r2], qy[r2], qz[r2], cx, cy, cz);   // two queries per packed instruction
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int r = 2 * r2 + h;
                    const float sq = h ? s2.y : s2.x;
                    const bool lt = sq < best_s[r];                                // false for NaN
                    s1[r] = lt ? best_s[r] : s1[r];
                    best_s[r] = lt ? sq : best_s[r];
                    best_j[r] = lt ? jj[u] : best_j[r];
                }
            }
        }
    }
    float thr[R];
    bool ambiguous = false;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float m = best_s[r];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fminf(m, __shfl_xor(m, off));
        thr[r] = m * 1.00000095367431640625f;                  // 1 + 2^-20
        ambiguous = ambiguous || s1[r] <= thr[r];
        if (best_s[r] <= thr[r]) best_d[r] = sqrtf(best_s[r]);  // this lane's candidate (j0 is its index already)
        else best_j[r] = 0x7fffffff;
    }
    if (__any(ambiguous)) {
        // exact scan of the chunk: every candidate with s <= thr, in ascending order within a lane
#pragma unroll
        for (int r = 0; r < R; ++r) { best_d[r] = __builtin_inff(); best_j[r] = 0x7fffffff; }
        for (int j = jbeg + lane; j < jend; j += 64) {
            const float bx = bb[j], by = bb[Nb + j], bz = bb[2 * Nb + j];
            const usip_f32x2 cx = {bx, bx}, cy = {by, by}, cz = {bz, bz};
#pragma unroll
            for (int r2 = 0; r2 < R / 2; ++r2) {
                const usip_f32x2 s2 = usip_sqdist2(qx[r2], qy[r2], qz[r2], cx, cy, cz);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int r = 2 * r2 + h;
                    const float sq = h ? s2.y : s2.x;
                    if (sq <= thr[r]) {
                        const float d = sqrtf(sq);
                        if (d < best_d[r]) { best_d[r] = d; best_j[r] = j; }
                    }
                }
            }
        }
    }
    // wave reduction: smaller distance wins, then lower index (== first occurrence overall)
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float d = best_d[r];
        int j = best_j[r];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_down(d, off);
            const int oj = __shfl_down(j, off);
            if (od < d || (od == d && oj < j)) { d = od; j = oj; }
        }
        best_d[r] = d;
        best_j[r] = j;
    }
}
