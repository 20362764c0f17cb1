/* include/usip_hip_fragment_batch.h -- the part of the C ABI that builds evaluation batches from indoor fragments
 * (SURVEY 8 f-27).  include/usip_hip.h includes it after usip_hip_indoor_pairs.h, inside its extern "C" block and after the
 * f-5 structs it builds on: include that header, never this one alone.  usip_amd/_lib.py reads it as it reads usip_hip.h
 * (STRUCTS_INCLUDED, SIGNATURES_INCLUDED). */
#ifndef USIP_HIP_H
#error "include usip_hip.h, which includes this header"
#endif
#ifndef USIP_HIP_FRAGMENT_BATCH_H
#define USIP_HIP_FRAGMENT_BATCH_H

/* ------------------------------------------------------------------ f-27  evaluation batches from indoor fragments
 * Replaces RedwoodLoader.__getitem__ (evaluation/redwood_loader.py:73-127) and Match3DEvalLoader.__getitem__
 * (data/match3d_eval_loader.py:78-103): B fragments of a bank resident in device memory, each written as the detector and
 * the descriptor consume it in evaluation.  No augmentation and no transform: pc, sn and node are gathers of bank rows.
 *
 * bank: f-5's rows f32 [rows][row_len] (x y z nx ny nz curvature ...) and offsets i64 [num_fragments + 1].  ids i32 [B]
 * (device): which fragment each cloud of the call is (clamped); ids_host, where given, is the host's copy, on which the id
 * range is checked.
 * Per fragment, f-5's per-slot work: N slots drawn without replacement (fewer rows than N: the fix_idx layout of
 * RedwoodLoader :88-92 -- Match3DEvalLoader would raise there, this is Redwood's for both), sn = columns 3..3+Cs, n_sub of
 * the N slots are the FPS candidates, the first FPS index is random, usip_fps_f32 on the float32 candidates gives M nodes.
 * recipe: f-5's; only N, M, Cs, n_sub and row_len are read.  train, sn_last, height_scaling, enu_to_cam and require_full must
 * be 0.
 * The cloud stage addresses clouds in two halves of P, so every buffer of `out` and the workspace hold B2 = 2 * ceil(B / 2)
 * clouds: with B odd, cloud B2 - 1 repeats fragment ids[B - 1] (under explicit draws: its draws too) and is the caller's to
 * drop.  Outputs: pc f32 [B2][3][N], sn f32 [B2][Cs][N], node f32 [B2][3][M]; optional rows i32 [B2][N] (fragment-relative
 * row of every slot), node_slots i32 [B2][M] (the slot every node came from).
 * Randomness (usip_fragment_batch_build_f32): f-5's CHOICE / CAND / FIRST streams at tag base 48 (49-51), none shared with
 * f-5 (1-8), f-8 (17-26) or f-26 (33-40), with the FRAGMENT'S ID where f-5 has the pair and cloud 0: a fragment gets the
 * same points and nodes whatever batch it rides in and wherever in it.  usip_fragment_batch_apply_f32 takes the draws
 * explicitly, per position of the call: rows i32 [B][N], cand i32 [B][n_sub], first i32 [B].
 * USIP_EINVAL: f-5's shape rules, a set flag among the five above, num_fragments < 1, an empty fragment (min_rows < 1), an
 * id out of range (where ids_host is given), B < 0. */
typedef struct usip_fragment_batch_bank {
    const float* rows;
    const int64_t* offsets;
    int num_fragments;
    long long min_rows;                        /* the fewest rows of any fragment */
} usip_fragment_batch_bank;
typedef struct usip_fragment_batch_draws {
    const int32_t* rows;
    const int32_t* cand;
    const int32_t* first;
} usip_fragment_batch_draws;
typedef struct usip_fragment_batch_out {
    float* pc;
    float* sn;
    float* node;
    int32_t* rows;          /* optional (NULL) */
    int32_t* node_slots;    /* optional (NULL) */
} usip_fragment_batch_out;
long long usip_fragment_batch_workspace_bytes(const usip_pairs_recipe* recipe, int B);
/* Byte offset of one part: 0 the one f64 identity table, 1 the FPS candidates f32 [B2][3][n_sub], 2 the first FPS indices
 * i32 [B2], 3 the FPS picks i32 [B2][M], 4 every cloud's fragment id i32 [B2], 5 the total. */
long long usip_fragment_batch_workspace_offset(const usip_pairs_recipe* recipe, int B, int part);
int usip_fragment_batch_build_f32(const usip_pairs_recipe* recipe, const usip_fragment_batch_bank* bank, const int32_t* ids,
                                  const int32_t* ids_host, int B, uint64_t seed, uint64_t step,
                                  const usip_fragment_batch_out* out, void* workspace, void* stream);
int usip_fragment_batch_apply_f32(const usip_pairs_recipe* recipe, const usip_fragment_batch_draws* draws,
                                  const usip_fragment_batch_bank* bank, const int32_t* ids, const int32_t* ids_host, int B,
                                  const usip_fragment_batch_out* out, void* workspace, void* stream);
/* HOST twin (every pointer on the host, draws NULL = Philox): the same arithmetic in the same order, its own float64 FPS;
 * num_threads splits the fragments.  Only clouds 0..B-1 are written: its buffers need hold no more than B clouds. */
int usip_fragment_batch_build_f32_cpu(const usip_pairs_recipe* recipe, const usip_fragment_batch_draws* draws,
                                      const usip_fragment_batch_bank* bank, const int32_t* ids, int B, uint64_t seed,
                                      uint64_t step, const usip_fragment_batch_out* out, int num_threads);

#endif /* USIP_HIP_FRAGMENT_BATCH_H */
