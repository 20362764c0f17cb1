// usip_amd/csrc/fragment_batch_math.h -- the arithmetic of one evaluation fragment, shared by the kernels of
// csrc/fragment_batch.hip and the host twin of csrc/fragment_batch_cpu.cpp.  The per-slot work is csrc/pairs_math.h's cloud
// stage seen through FragmentView: one fragment per cloud, one identity table for all of them, every hook empty and
// train = 0, so a point, its sn channels and a node are the bank row's own float32 values.
//
// Reference semantics (evaluation/redwood_loader.py, data/match3d_eval_loader.py):
//   get_instance_unaugmented_np   redwood :85-92: N rows without replacement, the fix_idx layout below N rows;
//                                 match3d :83: the same choice, which raises below N rows -- Redwood's branch serves both
//   __getitem__                   N/2 of the N slots without replacement, FarthestSampler.sample on them (first index
//                                 random), pc / sn / node .astype(float32): gathers of the file's float32 values
#pragma once
#include "indoor_pairs_math.h"

namespace usip_fragment_batch {

using namespace usip_pairs;

constexpr uint32_t FTAG0 = 48;              // stream tags 49-51: none shared with f-5 (1-8), f-8 (17-26) or f-26 (33-40)

// Cloud q of the stage's 2P is position min(q, B - 1) of the call: with B odd the last cloud repeats the last fragment.
USIP_HD int position(int P, int B, int p, int c) { return clampi(c * P + p, 0, B - 1); }

// The identity table: no stage, scale 1, no height scaling, R = I.  With train = 0 and dst = 0 only T_HEIGHT_ON is read.
USIP_HD void identity_table(double* T)
{
    for (int i = 0; i < T_SIZE; ++i) T[i] = 0.0;
    T[T_SCALE] = T[T_HEIGHT] = T[T_DSCALE] = 1.0;
    T[T_RD] = T[T_RD + 4] = T[T_RD + 8] = 1.0;
}

// One table for every cloud, one fragment per cloud (read from cloud_frag [2P]), nothing moved and nothing transformed.
struct FragmentView {
    const double* tab;          // [T_SIZE]
    const int64_t* offsets;
    const int32_t* cloud_frag;  // [2P]
    int num_fragments;

    USIP_HD const double* table(int, int) const { return tab; }
    USIP_HD void scan(int q, int, long long& o0, long long& n) const
    {
        const int s = clampi(cloud_frag[q], 0, num_fragments - 1);
        o0 = offsets[s];
        n = offsets[s + 1] - o0;
    }
    USIP_HD static int dst(int) { return 0; }
    USIP_HD static bool usable(long long n, int) { return n >= 1; }
    USIP_HD static void move(int, int, double*) {}
    USIP_HD static void move_sn(int, int, float*) {}
    template <class Src>
    USIP_HD static void node_xyz(const usip_pairs_recipe&, const Src&, int, int, int, int, double*) {}
    USIP_HD static bool f32_array(int) { return true; }
    USIP_HD static void post(int, const double*, float*, bool) {}
};

// ----------------------------------------------------------------------------------------------- sources of draws
// Philox: f-5's CHOICE / CAND / FIRST streams at tag base 48 with the fragment's id in the bank where f-5 has the pair,
// and cloud 0: the draws do not depend on the batch.  ids [B] is read per slot (one cached word).
struct PhiloxFragmentDraws : usip_indoor_pairs::NoJitter {
    PhiloxSlots<FTAG0> s;       // base 0: gp(id) = id
    const int32_t* ids;
    int P, B, num_fragments;

    USIP_HD int frag(int p, int c) const { return clampi(ids[position(P, B, p, c)], 0, num_fragments - 1); }
    USIP_HD long long row(int p, int c, long long n, int N, int j) const { return s.row(frag(p, c), 0, n, N, j); }
    USIP_HD int cand(int p, int c, int N, int i) const { return s.cand(frag(p, c), 0, N, i); }
    USIP_HD int first(int p, int c, int n_sub) const { return s.first(frag(p, c), 0, n_sub); }
};

// The recorded draws, per position of the call; indices are clamped into range as ExplicitDraws' are.
struct ExplicitFragmentDraws : usip_indoor_pairs::NoJitter {
    usip_fragment_batch_draws d;
    int P, B, N, n_sub;

    USIP_HD long long row(int p, int c, long long n, int, int j) const
    {
        const long long v = d.rows[(long long)position(P, B, p, c) * N + j];
        return v < 0 ? 0 : (v >= n ? n - 1 : v);
    }
    USIP_HD int cand(int p, int c, int, int i) const
    {
        return clampi(d.cand[(long long)position(P, B, p, c) * n_sub + i], 0, N - 1);
    }
    USIP_HD int first(int p, int c, int) const { return clampi(d.first[position(P, B, p, c)], 0, n_sub - 1); }
};

inline bool fragment_recipe_ok(const usip_pairs_recipe* r)
{
    return recipe_ok(r) && !r->train && !r->sn_last && !r->height_scaling && !r->enu_to_cam && !r->require_full;
}

// The recipe the cloud stage runs with: the shape fields, every flag off.
inline usip_pairs_recipe stage_recipe(const usip_pairs_recipe& r)
{
    usip_pairs_recipe c = r;
    c.rot_horizontal = c.rot_3d = c.rot_perturbation = c.translation_perturbation = 0;
    c.dst_rot_type = c.dst_rot_perturbation = 0;
    return c;
}

// The checks every entry point shares; 1 = go on, else the value to return.
inline int fragment_args_ok(const usip_pairs_recipe* r, const usip_fragment_batch_bank* b, const int32_t* ids,
                            const int32_t* ids_host, int B, const usip_fragment_batch_out* o)
{
    if (!fragment_recipe_ok(r) || !b || B < 0 || b->num_fragments < 1 || b->min_rows < 1) return USIP_EINVAL;
    if (ids_host)
        for (int i = 0; i < B; ++i)
            if (ids_host[i] < 0 || ids_host[i] >= b->num_fragments) return USIP_EINVAL;
    if (B == 0) return USIP_OK;
    if (!b->rows || !b->offsets || !ids || !o || !o->pc || !o->sn || !o->node) return USIP_EINVAL;
    return 1;
}

inline bool fragment_draws_ok(const usip_fragment_batch_draws* d) { return d && d->rows && d->cand && d->first; }

}  // namespace usip_fragment_batch
