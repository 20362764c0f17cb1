// usip_amd/csrc/indoor_pairs_math.h -- the arithmetic of one indoor descriptor training pair, shared by the
// kernels of csrc/indoor_pairs.hip and the host twin of csrc/indoor_pairs_cpu.cpp.  The per-slot work is csrc/pairs_math.h's
// cloud stage seen through IndoorView: one table per pair (as the detector's), one frame per cloud, the positive takes the
// table's transform, and -- what neither other builder has -- the anchor is first moved by the sample's ICP matrix.
//
// Reference semantics (data/scenenn_descriptor_loader.py):
//   get_instance_unaugmented_np   :101-118, the row choice of both frames (fix_idx layout below N rows)
//   __getitem__ :239-240          anc_pc = hom2cart(icp . cart2hom(anc_pc)') in float64, from there on a float64 array;
//                                 anc_sn[:, 0:3] = the same expression, translation included, assigned into the f32 array
//   :243-248                      N/2 candidates, FPS on the un-augmented coordinates (the anchor's: after the move)
//   augment :120-187              ONE parameter set for both clouds; the jitter is drawn but never added; val:
//                                 augment_rot_only :189-228 (rotations only); test: nothing
//   :266-278                      transform_pc_pytorch on the positive in every mode
#pragma once
#include "pairs_math.h"

namespace usip_indoor_pairs {

using namespace usip_pairs;

constexpr uint32_t ITAG0 = 32;              // stream tags 33-40: f-5's layout, none shared with f-5 (1-8) or f-8 (17-26)
enum { MODE_TRAIN = 0, MODE_VAL = 1, MODE_TEST = 2, MODE_SAMPLE = 3 };

// rows 0..2 of the 4x4 matrix on [x y z 1] (translate = false: on [x y z 0], the rotation part); the last row is 0 0 0 1,
// so hom2cart divides by 1
USIP_HD void icp_move(const double* m, double x[3], bool translate)
{
    const double a = x[0], b = x[1], c = x[2];
    for (int i = 0; i < 3; ++i) {
        const double rot = dot3(m[4 * i], m[4 * i + 1], m[4 * i + 2], a, b, c);
        x[i] = translate ? rot + m[4 * i + 3] : rot;
    }
}

// transform_pc_pytorch on one column vector as torch.matmul sums it on the reference's host path (a 3x3 by 3xN sgemm):
// r0 p0 rounded, then one fused multiply-add per further term; * scale, + shift as pairs_math.h's transform3.  The
// detector builder's transform3 keeps its own order; the indoor fixtures hold the positive to the reference's bits.
USIP_HD void transform3_fma(const double* T, float p[3], bool shift_scale)
{
    float o[3];
    for (int i = 0; i < 3; ++i) {
        const float r0 = (float)T[T_RD + 3 * i], r1 = (float)T[T_RD + 3 * i + 1], r2 = (float)T[T_RD + 3 * i + 2];
        o[i] = fmaf(r2, p[2], fmaf(r1, p[1], r0 * p[0]));
    }
    for (int i = 0; i < 3; ++i)
        p[i] = shift_scale ? o[i] * (float)T[T_DSCALE] + (float)T[T_DSHIFT + i] : o[i];
}

struct IndoorBank {
    const float* rows;
    const int64_t* offsets;
    const int32_t* pairs;
    const double* icp;
    const int32_t* sample_mode;
    int num_frames, num_samples;

    USIP_HD int sample(int s) const { return clampi(s, 0, num_samples - 1); }
    USIP_HD int frame(int s, int c) const { return clampi(pairs[2 * s + c], 0, num_frames - 1); }
    USIP_HD int mode(int recipe_mode, int s) const
    {
        return recipe_mode == MODE_SAMPLE ? clampi(sample_mode[s], MODE_TRAIN, MODE_TEST) : recipe_mode;
    }
};

// The pair's table under mode (train, val or test): pair_table with the mode's scale and shift rules and no height scale.
// The cloud stage runs with train = 1 unless the whole call is in test mode, so a val or test sample of a mixed call is
// left untouched through the table alone: scale 1, and a shift of -0.0 (x + -0.0 is x for every x, -0.0 included) wherever
// the reference adds none.
template <class Src>
USIP_HD void indoor_table(const usip_indoor_pairs_recipe& r, int mode, const Src& src, int p, double* T)
{
    usip_pairs_recipe c = r.cloud;
    c.train = mode != MODE_TEST;
    c.height_scaling = 0;
    if (mode != MODE_TRAIN) {
        c.aug_scale_lo = c.aug_scale_hi = 1.0;
        c.translation_perturbation = 0;
    }
    pair_table(c, src, p, T);
    if (!c.translation_perturbation)
        for (int k = 0; k < 3; ++k) T[T_SHIFT + k] = -0.0;
}

// The recipe the cloud stage runs with.
inline usip_pairs_recipe stage_recipe(const usip_indoor_pairs_recipe& r)
{
    usip_pairs_recipe c = r.cloud;
    c.train = r.mode != MODE_TEST;
    c.height_scaling = c.enu_to_cam = c.sn_last = 0;
    return c;
}

// One table per pair, one frame per cloud (read from the workspace), cloud 1 takes the transform (post), cloud 0 the
// ICP move.
struct IndoorView {
    const double* tab;          // [P][T_SIZE]
    const float* bank;          // the frames' rows: an anchor's node is recomputed from its row (node_xyz)
    const int64_t* offsets;
    const int32_t* cloud_frame; // [2P]
    const double* icp;          // [S][12]
    const int32_t* sample_ids;  // [P]
    int num_frames, num_samples, moves_normals;

    USIP_HD const double* table(int, int p) const { return tab + (long long)p * T_SIZE; }
    USIP_HD void scan(int q, int, long long& o0, long long& n) const
    {
        const int s = clampi(cloud_frame[q], 0, num_frames - 1);
        o0 = offsets[s];
        n = offsets[s + 1] - o0;
    }
    USIP_HD static int dst(int) { return 0; }               // the positive's transform is post's
    USIP_HD static bool usable(long long n, int) { return n >= 1; }
    USIP_HD static bool f32_array(int c) { return c == 1; }
    USIP_HD static void post(int c, const double* T, float* x, bool full)
    {
        if (c == 1) transform3_fma(T, x, full);
    }
    USIP_HD const double* matrix(int p) const { return icp + 12LL * clampi(sample_ids[p], 0, num_samples - 1); }
    USIP_HD void move(int p, int c, double* x) const
    {
        if (c == 0) icp_move(matrix(p), x, true);
    }
    USIP_HD void move_sn(int p, int c, float* s) const
    {
        if (c != 0) return;
        double a[3] = {s[0], s[1], s[2]};
        icp_move(matrix(p), a, moves_normals != 0);
        for (int k = 0; k < 3; ++k) s[k] = (float)a[k];
    }
    // The anchor's node: FPS chose among the float32 roundings of the moved points; the node itself is the float64 move of
    // the bank row, rounded once at the end of augment as the reference's float64 node is.
    template <class Src>
    USIP_HD void node_xyz(const usip_pairs_recipe& r, const Src& src, int q, int p, int c, int ci, double* x) const
    {
        if (c != 0) return;
        long long o0, n;
        scan(q, p, o0, n);
        if (n < 1) return;
        const float* row = bank + (o0 + src.row(p, c, n, r.N, src.cand(p, c, r.N, ci))) * r.row_len;
        x[0] = row[0]; x[1] = row[1]; x[2] = row[2];
        move(p, c, x);
    }
};

// ----------------------------------------------------------------------------------------------- sources of draws
// The reference draws its three jitter blocks and never adds them (:171-173): no such draw is made here, at compile time
// -- these members shadow PhiloxSlots' -- and the cloud stage adds -0.0 (sigma 0 times it, clipped, is -0.0 again).
struct NoJitter {
    USIP_HD static void jit_pc(int, int, int, int, double* z) { z[0] = z[1] = z[2] = -0.0; }
    USIP_HD static void jit_sn(int, int, int, int Cs, int, double* z) { for (int k = 0; k < Cs; ++k) z[k] = -0.0; }
    USIP_HD static void jit_node(int, int, int, int, double* z) { z[0] = z[1] = z[2] = -0.0; }
};

struct PhiloxIndoorDraws : PhiloxSlots<ITAG0> {
    // PhiloxDraws::params (csrc/pairs_math.h) on this builder's streams: half h of the pair's draws, u[12 h .. 12 h + 12)
    USIP_HD void params(int p, int h, double* u) const
    {
        uint64_t b[4];
#pragma unroll
        for (int e = 3 * h; e < 3 * h + 3; ++e) {
            pairs_block(seed, step, gp(p), ITAG0 + TAG_PARAM_U, 0, e, b);
#pragma unroll
            for (int i = 0; i < 4; ++i) u[4 * e + i] = u53(b[i]);
        }
        double z[4];
        pairs_block(seed, step, gp(p), ITAG0 + TAG_PARAM_N, 0, h, b);
        normal4(b, z);
        double* n = u + (h ? 15 : 4);
        n[0] = z[0]; n[1] = z[1]; n[2] = z[2];
    }
    USIP_HD static void jit_pc(int a, int b, int c, int d, double* z) { NoJitter::jit_pc(a, b, c, d, z); }
    USIP_HD static void jit_sn(int a, int b, int c, int Cs, int e, double* z) { NoJitter::jit_sn(a, b, c, Cs, e, z); }
    USIP_HD static void jit_node(int a, int b, int c, int d, double* z) { NoJitter::jit_node(a, b, c, d, z); }
};

struct ExplicitIndoorDraws : NoJitter {
    ExplicitDraws cloud;

    USIP_HD void params(int p, int h, double* u) const { cloud.params(p, h, u); }
    USIP_HD long long row(int p, int c, long long n, int N, int j) const { return cloud.row(p, c, n, N, j); }
    USIP_HD int cand(int p, int c, int N, int i) const { return cloud.cand(p, c, N, i); }
    USIP_HD int first(int p, int c, int n_sub) const { return cloud.first(p, c, n_sub); }
};

inline bool indoor_recipe_ok(const usip_indoor_pairs_recipe* r)
{
    if (!r || !recipe_ok(&r->cloud)) return false;
    const usip_pairs_recipe& c = r->cloud;
    if (c.train || c.sn_last || c.height_scaling || c.enu_to_cam || c.require_full || c.Cs < 3) return false;
    if (c.pc_sigma != 0.0 || c.sn_sigma != 0.0 || c.node_sigma != 0.0) return false;
    if (!(c.pc_clip >= 0.0) || !(c.sn_clip >= 0.0) || !(c.node_clip >= 0.0)) return false;
    if (r->mode < MODE_TRAIN || r->mode > MODE_SAMPLE || (r->icp_moves_normals != 0 && r->icp_moves_normals != 1)) return false;
    return true;
}

// The checks both entry points share; 1 = go on, else the value to return.
inline int indoor_args_ok(const usip_indoor_pairs_recipe* r, const usip_indoor_pairs_bank* b, const int32_t* sample_ids,
                          int P, const usip_indoor_pairs_out* o)
{
    if (!indoor_recipe_ok(r) || !b || P < 0 || b->num_samples < 1 || b->num_frames < 1 || b->min_rows < 1) return USIP_EINVAL;
    if (r->mode == MODE_SAMPLE && !b->sample_mode) return USIP_EINVAL;
    if (b->pairs_host)
        for (long long i = 0; i < 2LL * b->num_samples; ++i)
            if (b->pairs_host[i] < 0 || b->pairs_host[i] >= b->num_frames) return USIP_EINVAL;
    if (P == 0) return USIP_OK;
    if (!b->rows || !b->offsets || !b->pairs || !b->icp || !sample_ids) return USIP_EINVAL;
    if (!o || !o->pc[0] || !o->pc[1] || !o->sn[0] || !o->sn[1] || !o->node[0] || !o->node[1] || !o->R || !o->scale ||
        !o->shift)
        return USIP_EINVAL;
    return 1;
}

inline bool indoor_draws_ok(const usip_indoor_pairs_draws* d)
{
    return d && d->cloud.rows && d->cloud.cand && d->cloud.first && d->cloud.params;
}

}  // namespace usip_indoor_pairs
