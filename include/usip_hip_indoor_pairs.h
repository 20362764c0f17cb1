/* include/usip_hip_indoor_pairs.h -- the part of the C ABI that builds indoor descriptor batches.
 * include/usip_hip.h includes it after f-8, inside its extern "C" block and after the f-5 structs it builds on: include that
 * header, never this one alone.  usip_amd/_lib.py reads it as it reads usip_hip.h (STRUCTS_INCLUDED, SIGNATURES_INCLUDED). */
#ifndef USIP_HIP_H
#error "include usip_hip.h, which includes this header"
#endif
#ifndef USIP_HIP_INDOOR_PAIRS_H
#define USIP_HIP_INDOOR_PAIRS_H

/* ------------------------------------------------------------------ f-26  indoor descriptor batches (SceneNN pairs)
 * Replaces SceneNNDescriptorLoader.__getitem__ (data/scenenn_descriptor_loader.py:230-289) with its augment / augment_rot_only
 * (:120-228) and transform_pc_pytorch: P (anchor, positive) pairs of recorded frames, the anchor first moved into the
 * positive's frame by the sample's 4x4 ICP matrix, written as IndoorDescriptorStep.step consumes them.
 *
 * bank: f-5's rows / offsets over the FRAMES (num_frames of them), plus the samples: pairs i32 [S][2] (anchor frame,
 * positive frame), icp f64 [S][12] (rows 0..2 of the 4x4 matrix; a matrix whose last row is not exactly 0 0 0 1 is refused
 * where the bank is made, so hom2cart's division is by 1 and is not performed), sample_mode i32 [S] or NULL (read with recipe
 * mode 3).  pairs_host / icp_host are the host's copies of pairs (the entry points check the frame ids on them) and may be
 * NULL for the host twin, which checks its own.  sample_ids i32 [P]: which sample each pair of the call is (clamped).
 * Per pair, with f-5's per-slot work (fix_idx layout for a frame shorter than N, n_sub FPS candidates, usip_fps_f32 on the
 * un-augmented float32 candidates):
 *   anchor (cloud 0): xyz <- ((m0 x + m1 y) + m2 z) + m3 per row of icp in float64, and stays float64 through augment to ONE
 *     rounding; its FPS candidates are the float32 roundings of the moved points, its nodes are recomputed in float64 from
 *     the bank row FPS chose.  sn[0:3] goes through the same expression and is rounded to float32 at once; with
 *     icp_moves_normals = 1 (the reference) the translation m3 is added to the normals too, with 0 only the rotation part.
 *   positive (cloud 1): the frame's float32 array as f-5's src cloud holds it, then transform_pc_pytorch (R, scale, shift
 *     are the outputs, f-5's dst).
 *   ONE augmentation parameter set for both clouds.  mode 0 train: augment (rotation stages, scale U(lo, hi), shift under
 *     translation_perturbation; the jitter is drawn by the reference but never added: the three sigmas must be 0 and no
 *     jitter draw is made or read).  mode 1 val: the rotation stages only.  mode 2 test: none.  mode 3: sample_mode[s] of
 *     each sample (0, 1 or 2).
 * cloud holds f-5's fields; train, sn_last, height_scaling, enu_to_cam and require_full must be 0 (the mode decides), Cs >= 3.
 * Outputs: pc[c] f32 [P][3][N], sn[c] f32 [P][Cs][N], node[c] f32 [P][3][M] (0 anchor, 1 positive), R f32 [P][3][3], scale
 * f32 [P][1], shift f32 [P][3][1]; optional rows i32 [2][P][N], node_slots i32 [2][P][M].
 * Randomness (usip_indoor_pairs_build_f32): f-5's layout of streams at tag base 32 (33-40): none shared with f-5 (1-8) or
 * f-8 (17-26).  usip_indoor_pairs_apply_f32 takes f-5's explicit draws (jit_* unused, may be NULL).
 * USIP_EINVAL: f-5's shape rules, the fields above, S < 1, a frame id out of range (where pairs_host is given), an empty
 * frame (min_rows < 1), mode outside 0..3, mode 3 without sample_mode. */
typedef struct usip_indoor_pairs_recipe {
    usip_pairs_recipe cloud;
    int icp_moves_normals;                     /* 1: the reference adds the ICP translation to sn[0:3]; 0: rotation only */
    int mode;                                  /* 0 train, 1 val, 2 test, 3 per sample (bank sample_mode) */
} usip_indoor_pairs_recipe;
typedef struct usip_indoor_pairs_bank {
    const float* rows;
    const int64_t* offsets;
    const int32_t* pairs;
    const double* icp;
    const int32_t* sample_mode;                /* optional (NULL) */
    const int32_t* pairs_host;                 /* optional (NULL): host copy of pairs */
    int num_frames, num_samples;
    long long min_rows;                        /* the fewest rows of any frame */
} usip_indoor_pairs_bank;
typedef struct usip_indoor_pairs_draws {
    usip_pairs_draws cloud;                    /* rows, cand, first, params as f-5; jit_pc, jit_sn, jit_node unused */
} usip_indoor_pairs_draws;
typedef struct usip_indoor_pairs_out {
    float* pc[2];
    float* sn[2];
    float* node[2];
    float* R;
    float* scale;
    float* shift;
    int32_t* rows;          /* optional (NULL) */
    int32_t* node_slots;    /* optional (NULL) */
} usip_indoor_pairs_out;
long long usip_indoor_pairs_workspace_bytes(const usip_indoor_pairs_recipe* recipe, int P);
/* Byte offset of one part: 0 the per-pair f64 tables [P], 1 the un-augmented FPS candidates f32 [2P][3][n_sub] (anchors
 * 0..P-1, then positives), 2 the first FPS indices i32 [2P], 3 the FPS picks i32 [2P][M], 4 every cloud's frame id i32 [2P],
 * 5 the total. */
long long usip_indoor_pairs_workspace_offset(const usip_indoor_pairs_recipe* recipe, int P, int part);
int usip_indoor_pairs_build_f32(const usip_indoor_pairs_recipe* recipe, const usip_indoor_pairs_bank* bank,
                                const int32_t* sample_ids, int P, uint64_t seed, uint64_t step, long long pair_base,
                                const usip_indoor_pairs_out* out, void* workspace, void* stream);
int usip_indoor_pairs_apply_f32(const usip_indoor_pairs_recipe* recipe, const usip_indoor_pairs_draws* draws,
                                const usip_indoor_pairs_bank* bank, const int32_t* sample_ids, int P,
                                const usip_indoor_pairs_out* out, void* workspace, void* stream);
/* HOST twin (every pointer on the host, draws NULL = Philox): the same arithmetic in the same order, its own float64 FPS;
 * num_threads splits the pairs. */
int usip_indoor_pairs_build_f32_cpu(const usip_indoor_pairs_recipe* recipe, const usip_indoor_pairs_draws* draws,
                                    const usip_indoor_pairs_bank* bank, const int32_t* sample_ids, int P, uint64_t seed,
                                    uint64_t step, long long pair_base, const usip_indoor_pairs_out* out, int num_threads);

#endif /* USIP_HIP_INDOOR_PAIRS_H */
