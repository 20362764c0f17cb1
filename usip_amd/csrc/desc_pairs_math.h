// usip_amd/csrc/desc_pairs_math.h -- the arithmetic of one descriptor training pair, shared by the kernels of
// csrc/desc_pairs.hip and the host twin of csrc/desc_pairs_cpu.cpp.  The per-slot work is csrc/pairs_math.h's cloud stage
// (cloud_point, cloud_node) seen through CloudView: no transform; what is new here is the choice of the positive scan, the
// mining of negatives, a table per CLOUD, and the parameter draws, with stream tags of their own.
//
// Reference semantics (data/kitti_descriptor_loader.py):
//   get_nearby_instance_unagumented_np   :154-203, the narrowing rejection search (select_positive)
//   mine_negative_sample                 :278-317 (mine_negative)
//   augment                              :205-276: ONE scale for the pair; per cloud yaw, rand(3), randn(3), the three jitter
//                                        blocks and the shift, in that order; the arithmetic of the detector loader's augment
#pragma once
#include "pairs_math.h"

namespace usip_desc_pairs {

using namespace usip_pairs;

// Stream tags (counter word 1 = tag << 8 | cloud); f-5 uses 1-8, the per-slot streams here are f-5's + DTAG0 (17-22).
enum : uint32_t {
    DTAG0 = 16,
    DTAG_PARAM_U = 23,    // cloud c, elements 0, 1: that cloud's uniforms; cloud 0, element 2: the pair's scale
    DTAG_PARAM_N = 24,    // cloud c, element 0: that cloud's perturbation normals
    DTAG_TRY = 25,        // element = try number of the positive search: word 0
    DTAG_NEG = 26,        // element 0: the negative pick, word 0
};
constexpr int CLOUD_U = 10;       // params per cloud, from index 1 + CLOUD_U * c

// One cloud's table (pairs_math.h's layout; no height scale, and the transform's entries stay zero: CloudView::dst is 0).
USIP_HD void cloud_table(const usip_pairs_recipe& r, double u_scale, const double* u, double* T)
{
    augment_table(r, u, u_scale, u + 7, T);
    T[T_HEIGHT] = 1.0;
    for (int i = T_HEIGHT_ON; i < T_SIZE; ++i) T[i] = 0.0;
}

// The descriptor's pair: one table per cloud, the scan chosen on the device (anchor or positive), no transform, and no
// fix_idx layout (a scan shorter than N is refused).
struct CloudView {
    const double* tab;          // [2P][T_SIZE]
    const int64_t* offsets;
    const int32_t* cloud_scan;  // [2P]
    int num_scans;

    USIP_HD const double* table(int q, int) const { return tab + (long long)q * T_SIZE; }
    USIP_HD void scan(int q, int, long long& o0, long long& n) const
    {
        const int s = clampi(cloud_scan[q], 0, num_scans - 1);
        o0 = offsets[s];
        n = offsets[s + 1] - o0;
    }
    USIP_HD static int dst(int) { return 0; }
    USIP_HD static bool usable(long long n, int N) { return n >= N; }
    USIP_HD static void move(int, int, double*) {}
    USIP_HD static void move_sn(int, int, float*) {}
    template <class Src>
    USIP_HD static void node_xyz(const usip_pairs_recipe&, const Src&, int, int, int, int, double*) {}
    USIP_HD static bool f32_array(int) { return true; }
    USIP_HD static void post(int, const double*, float*, bool) {}
};

struct PosedBank {
    const float* rows;
    const int64_t* offsets;
    const double* poses;
    const int32_t* seq_of;
    const int32_t* seq_start;
    int num_scans, num_seq;

    USIP_HD int scan(int s) const { return clampi(s, 0, num_scans - 1); }
    USIP_HD int seq(int scan_id) const { return clampi(seq_of[scan_id], 0, num_seq - 1); }
};

// get_nearby_instance_unagumented_np: the bank-global scan chosen for anchor scan a of pair p
template <class Src>
USIP_HD int select_positive(const PosedBank& b, double thr, const Src& src, int p, int a)
{
    const int q = b.seq(a), s0 = b.seq_start[q], n = b.seq_start[q + 1] - s0, ia = a - s0;
    if (ia < 0 || ia >= n) return a;                        // a seq_start that is not the host's copy: never outside the bank
    const int interval = (int)(thr / 0.8 * 2);
    int lo = ia - interval < 0 ? 0 : ia - interval;
    int hi = ia + interval > n - 1 ? n - 1 : ia + interval;
    const double* A = b.poses + (long long)a * 16;
    for (int counter = 0; counter < 3 * interval && lo <= hi; ++counter) {
        const int t = src.try_index(p, counter, lo, hi, ia);
        const double* B = b.poses + (long long)b.scan(s0 + t) * 16;
        const double dx = B[3] - A[3], dy = B[7] - A[7], dz = B[11] - A[11];
        if (sqrt((dx * dx + dy * dy) + dz * dz) < thr) return b.scan(s0 + t);
        if (t < ia) lo = t + 1; else hi = t - 1;
    }
    return a;
}

// the reference's candidate test between anchors i and j of one call
USIP_HD bool negative_candidate(const PosedBank& b, double thr, int ai, int aj)
{
    if (b.seq(ai) != b.seq(aj)) return true;
    const double* A = b.poses + (long long)ai * 16;
    const double* B = b.poses + (long long)aj * 16;
    const double dx = (double)(float)B[3] - (double)(float)A[3], dy = (double)(float)B[7] - (double)(float)A[7],
                 dz = (double)(float)B[11] - (double)(float)A[11];
    return sqrt((dx * dx + dy * dy) + dz * dz) > thr;
}

// mine_negative_sample for anchor i: the index j picked, or 0 with fail = 1
template <class Src>
USIP_HD long long mine_negative(const PosedBank& b, double thr, const Src& src, const int32_t* scan_ids, int P, int i,
                                int& fail)
{
    const int ai = b.scan(scan_ids[i]);
    int count = 0;
    for (int j = 0; j < P; ++j)
        if (j != i && negative_candidate(b, thr, ai, b.scan(scan_ids[j]))) ++count;
    fail = count == 0;
    if (count == 0) return 0;
    const int pick = src.neg_pick(i, count);
    int k = 0;
    for (int j = 0; j < P; ++j)
        if (j != i && negative_candidate(b, thr, ai, b.scan(scan_ids[j])) && k++ == pick) return j;
    return 0;
}

// ----------------------------------------------------------------------------------------------- sources of draws
struct PhiloxDescDraws : PhiloxSlots<DTAG0> {
    // word 0 of (DTAG_PARAM_U, cloud 0, element 2): the pair's scale uniform
    USIP_HD double scale_u(int p) const
    {
        uint64_t b[4];
        pairs_block(seed, step, gp(p), DTAG_PARAM_U, 0, 2, b);
        return u53(b[0]);
    }
    // cloud c's CLOUD_U draws: (DTAG_PARAM_U, c, element 0) = yaw, rand(3); element 1 words 0..2 = the shift uniforms;
    // (DTAG_PARAM_N, c, element 0) normals 0..2 = the perturbation
    USIP_HD void cloud_params(int p, int c, double* u) const
    {
        uint64_t b[4];
        double z[4];
        pairs_block(seed, step, gp(p), DTAG_PARAM_U, c, 0, b);
        u[0] = u53(b[0]); u[1] = u53(b[1]); u[2] = u53(b[2]); u[3] = u53(b[3]);
        pairs_block(seed, step, gp(p), DTAG_PARAM_N, c, 0, b);
        normal4(b, z);
        u[4] = z[0]; u[5] = z[1]; u[6] = z[2];
        pairs_block(seed, step, gp(p), DTAG_PARAM_U, c, 1, b);
        u[7] = u53(b[0]); u[8] = u53(b[1]); u[9] = u53(b[2]);
    }
    USIP_HD int try_index(int p, int counter, int lo, int hi, int) const
    {
        uint64_t b[4];
        pairs_block(seed, step, gp(p), DTAG_TRY, 0, (uint64_t)counter, b);
        return clampi(lo + (int)(u53(b[0]) * (double)(hi - lo + 1)), lo, hi);
    }
    USIP_HD int neg_pick(int p, int count) const
    {
        uint64_t b[4];
        pairs_block(seed, step, gp(p), DTAG_NEG, 0, 0, b);
        return clampi((int)(u53(b[0]) * (double)count), 0, count - 1);
    }
};

// The recorded draws.  Indices are clamped into range: a bad fixture gives wrong values, never an access outside the bank.
struct ExplicitDescDraws {
    ExplicitDraws cloud;
    const double* par;
    const int32_t* tries;
    const int32_t* pick;
    int T;

    USIP_HD double scale_u(int p) const { return par[(long long)p * USIP_DESC_PAIRS_NPARAM]; }
    USIP_HD void cloud_params(int p, int c, double* u) const
    {
#pragma unroll
        for (int i = 0; i < CLOUD_U; ++i) u[i] = par[(long long)p * USIP_DESC_PAIRS_NPARAM + 1 + CLOUD_U * c + i];
    }
    USIP_HD long long row(int p, int c, long long n, int N, int j) const { return cloud.row(p, c, n, N, j); }
    USIP_HD int cand(int p, int c, int N, int i) const { return cloud.cand(p, c, N, i); }
    USIP_HD int first(int p, int c, int n_sub) const { return cloud.first(p, c, n_sub); }
    USIP_HD void jit_pc(int p, int c, int N, int j, double* z) const { cloud.jit_pc(p, c, N, j, z); }
    USIP_HD void jit_sn(int p, int c, int N, int Cs, int j, double* z) const { cloud.jit_sn(p, c, N, Cs, j, z); }
    USIP_HD void jit_node(int p, int c, int M, int m, double* z) const { cloud.jit_node(p, c, M, m, z); }
    USIP_HD int try_index(int p, int counter, int lo, int hi, int ia) const
    {
        return clampi(counter < T ? tries[(long long)p * T + counter] : ia, lo, hi);
    }
    USIP_HD int neg_pick(int p, int count) const { return clampi(pick[p], 0, count - 1); }
};

inline bool desc_recipe_ok(const usip_desc_pairs_recipe* r)
{
    if (!r || !recipe_ok(&r->cloud)) return false;
    const usip_pairs_recipe& c = r->cloud;
    if (c.sn_last || c.height_scaling || c.enu_to_cam || c.dst_rot_type || c.dst_rot_perturbation) return false;
    if (!(r->positive_radius > 0.0) || !(r->negative_radius > 0.0)) return false;
    return true;
}

// The checks both entry points share; 1 = go on, else the value to return.
inline int desc_args_ok(const usip_desc_pairs_recipe* r, const usip_desc_pairs_bank* b, const int32_t* scan_ids, int P,
                        const usip_desc_pairs_out* o)
{
    if (!desc_recipe_ok(r) || !b || P < 0 || b->num_scans < 1 || b->num_seq < 1) return USIP_EINVAL;
    if (b->min_rows < r->cloud.N) return USIP_EINVAL;
    if (r->mine && P < 2) return USIP_EINVAL;
    if (!b->seq_start_host || b->seq_start_host[0] != 0 || b->seq_start_host[b->num_seq] != b->num_scans)
        return USIP_EINVAL;
    for (int q = 0; q < b->num_seq; ++q)
        if (b->seq_start_host[q + 1] <= b->seq_start_host[q]) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!b->rows || !b->offsets || !b->poses || !b->seq_of || !b->seq_start || !scan_ids) return USIP_EINVAL;
    if (!o || !o->pc[0] || !o->pc[1] || !o->sn[0] || !o->sn[1] || !o->node[0] || !o->node[1] || !o->anc_pose ||
        !o->pos_pose || !o->anc_seq || !o->pos_id || (r->mine && (!o->neg_idx || !o->neg_fail)))
        return USIP_EINVAL;
    return 1;
}

inline bool desc_draws_ok(const usip_desc_pairs_recipe* r, const usip_desc_pairs_draws* d)
{
    if (!d || !d->cloud.rows || !d->cloud.cand || !d->cloud.first || !d->params || !d->tries || d->T < 1) return false;
    if (r->mine && !d->neg_pick) return false;
    if (r->cloud.train && (!d->cloud.jit_pc || !d->cloud.jit_sn || !d->cloud.jit_node)) return false;
    return true;
}

}  // namespace usip_desc_pairs
