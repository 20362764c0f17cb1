// usip_amd/csrc/pairs_math.h -- the arithmetic of one training pair, shared by the kernels of csrc/pairs.hip
// and the host twin of csrc/pairs_cpu.cpp.  Two sources of draws feed it through the same interface: PhiloxDraws (training)
// and ExplicitDraws (the reference's recorded draws, tests/golden/pairs_cases.npz), so the fixtures test the code that trains.
// cloud_point / cloud_node are the per-cloud stage of BOTH builders (f-5 and the descriptor's f-8, csrc/desc_pairs_math.h):
// one thread of csrc/cloud_stage.h's kernels or one iteration of csrc/cloud_stage_host.h's loops, told apart by a View.
//
// Reference semantics (data/kitti_detector_loader.py, data/oxford_detector_loader.py, data/augmentation.py):
//   angles2rotation_matrix  R = Rz (Ry Rx), float64
//   augment                 p <- p @ R per active stage (2d yaw, 3d, perturbation; row vectors, float64), + jitter,
//                           * scale, + shift, one rounding to f32 at the end.  With NO rotation stage the points stay
//                           the f32 array read from the scan: rounded after the jitter += (added in float64), after
//                           * scale (an f32 product: numpy multiplies an f32 array by a Python float in f32) and after
//                           += shift; nodes come out of FPS in float64 and always take the float64 path.  sn[0:3] is
//                           rotated too, but assigned into the f32 array after every stage, and its jitter is added in
//                           float64 and rounded (it is an in-place f32 +=); sn is never scaled
//   transform_pc_pytorch    R, scale, shift of the dst view: f32 R p (torch.matmul), * scale, + shift, on pc, sn[0:3], node
//   height scaling          Oxford, ENU z *= U(0.25, 1.2) in f32 (numpy multiplies an f32 array by a Python float in f32)
//   coordinate_ENU_to_cam   (x, y, z) <- (x, -z, y) on pc, sn[0:3] and node, after FPS
#pragma once
#include <math.h>
#include "pairs_rng.h"
#include "../../include/usip_hip.h"

namespace usip_pairs {

// per-pair float64 table written by the params stage
enum {
    T_STAGE = 0,        // 3 rotation matrices of augment, 9 each, row-major
    T_NSTAGE = 27,
    T_SCALE = 28,       // augment scale
    T_SHIFT = 29,       // 3: augment shift (0 without translation_perturbation)
    T_HEIGHT = 32,      // height scale (an f32 value), T_HEIGHT_ON = 1 when applied
    T_HEIGHT_ON = 33,
    T_RD = 34,          // 9: transform R (f32 values)
    T_DSCALE = 43,      // transform scale (f32 value)
    T_DSHIFT = 44,      // 3: transform shift (f32 values)
    T_SIZE = 48,
};
constexpr int MAX_CS = 8;
constexpr int MAX_ROW = 16;

USIP_HD double dot3(double a0, double a1, double a2, double b0, double b1, double b2)
{
    return (a0 * b0 + a1 * b1) + a2 * b2;                 // contraction is off
}

USIP_HD void mat3mul(const double A[9], const double B[9], double C[9])
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = dot3(A[3 * i], A[3 * i + 1], A[3 * i + 2], B[j], B[3 + j], B[6 + j]);
}

// angles2rotation_matrix (augmentation.py:15-28)
USIP_HD void rotation(double ax, double ay, double az, double R[9])
{
    const double cx = cos(ax), sx = sin(ax), cy = cos(ay), sy = sin(ay), cz = cos(az), sz = sin(az);
    const double Rx[9] = {1, 0, 0, 0, cx, -sx, 0, sx, cx};
    const double Ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy};
    const double Rz[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1};
    double A[9];
    mat3mul(Ry, Rx, A);
    mat3mul(Rz, A, R);
}

USIP_HD double clip(double v, double c) { return v < -c ? -c : (v > c ? c : v); }
USIP_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
USIP_HD double uniform(double lo, double hi, double u) { return lo + (hi - lo) * u; }    // numpy: low + (high - low) * u

// augment's part of a table, T[0 .. T_SHIFT + 3): rot = the yaw uniform, rand(3), randn(3); one scale and three shift uniforms
USIP_HD void augment_table(const usip_pairs_recipe& r, const double* rot, double u_scale, const double* u_shift, double* T)
{
    const double pi = 3.141592653589793;
    int ns = 0;
    if (r.train) {
        if (r.rot_horizontal) rotation(0.0, rot[0] * 2 * pi, 0.0, T + 9 * ns++);           // np.random.uniform() * 2 * np.pi
        if (r.rot_3d) rotation(rot[1] * pi * 2, rot[2] * pi * 2, rot[3] * pi * 2, T + 9 * ns++);   // np.random.rand(3) * np.pi * 2
        if (r.rot_perturbation)
            rotation(clip(r.pert_sigma * rot[4], r.pert_clip), clip(r.pert_sigma * rot[5], r.pert_clip),
                     clip(r.pert_sigma * rot[6], r.pert_clip), T + 9 * ns++);
    }
    for (int i = 9 * ns; i < 27; ++i) T[i] = 0.0;
    T[T_NSTAGE] = ns;
    T[T_SCALE] = r.train ? uniform(r.aug_scale_lo, r.aug_scale_hi, u_scale) : 1.0;
    for (int k = 0; k < 3; ++k)
        T[T_SHIFT + k] = (r.train && r.translation_perturbation) ? uniform(-r.shift_range, r.shift_range, u_shift[k]) : 0.0;
}

// Pair p's USIP_PAIRS_NPARAM raw draws u (layout in include/usip_hip.h) -> T.  The draws come in two halves, each where it
// is used and every index a constant, so that on the device u stays in registers and the halves share them.
template <class Src>
USIP_HD void pair_table(const usip_pairs_recipe& r, const Src& src, int p, double* T)
{
    const double pi = 3.141592653589793;
    double u[USIP_PAIRS_NPARAM];
    src.params(p, 0, u);                                   // u[0 .. 12): augment and height scale
    augment_table(r, u, u[7], u + 8, T);
    const bool height = r.train && r.height_scaling;
    T[T_HEIGHT] = height ? (double)(float)uniform(r.height_lo, r.height_hi, u[11]) : 1.0;
    T[T_HEIGHT_ON] = height ? 1.0 : 0.0;
    src.params(p, 1, u);                                   // u[12 .. 24): the dst transform
    double ax = 0, ay = 0, az = 0;
    if (r.dst_rot_type == 2) {
        ay = u[12] * 2 * pi;
    } else if (r.dst_rot_type == 3) {
        ax = u[12] * 2 * pi; ay = u[13] * 2 * pi; az = u[14] * 2 * pi;
    }
    if (r.dst_rot_perturbation) {
        const double c = 3 * 0.06;
        ax += clip(0.06 * u[15], c); ay += clip(0.06 * u[16], c); az += clip(0.06 * u[17], c);
    }
    double Rd[9];
    rotation(ax, ay, az, Rd);
    for (int i = 0; i < 9; ++i) T[T_RD + i] = (double)(float)Rd[i];
    T[T_DSCALE] = (double)(float)uniform(1.0 - r.dst_scale_thre, 1.0 + r.dst_scale_thre, u[18]);
    for (int k = 0; k < 3; ++k) T[T_DSHIFT + k] = (double)(float)uniform(-r.dst_shift_thre, r.dst_shift_thre, u[19 + k]);
    for (int i = T_DSHIFT + 3; i < T_SIZE; ++i) T[i] = 0.0;
}

// The un-augmented coordinates FPS sees: the row's x y z, Oxford's height scaling applied (ENU frame).
USIP_HD void raw_xyz(const double* T, const float* row, float p[3])
{
    p[0] = row[0];
    p[1] = row[1];
    p[2] = T[T_HEIGHT_ON] != 0.0 ? row[2] * (float)T[T_HEIGHT] : row[2];
}

// transform_pc_pytorch on one column vector: f32 R p, * scale, + shift
USIP_HD void transform3(const double* T, float p[3], bool shift_scale)
{
    float o[3];
    for (int i = 0; i < 3; ++i) {
        const float r0 = (float)T[T_RD + 3 * i], r1 = (float)T[T_RD + 3 * i + 1], r2 = (float)T[T_RD + 3 * i + 2];
        o[i] = (r0 * p[0] + r1 * p[1]) + r2 * p[2];
    }
    for (int i = 0; i < 3; ++i)
        p[i] = shift_scale ? o[i] * (float)T[T_DSCALE] + (float)T[T_DSHIFT + i] : o[i];
}

// A point (f32_array: the reference holds it in the scan's f32 array) or a node (float64 out of FPS): ENU -> cam,
// augment (train) with jitter z[3] * sigma clipped, rounded as the reference rounds, then dst's transform.
template <class Move>
USIP_HD void finish_xyz(const usip_pairs_recipe& r, const double* T, int cloud, const float in[3], const double z[3],
                        double sigma, double clp, bool f32_array, float out[3], const Move& move)
{
    double p[3] = {in[0], in[1], in[2]};
    move(p);                                               // the float64 entry: a View's own frame (empty but for IndoorView)
    if (r.enu_to_cam) { const double y = p[1]; p[1] = -p[2]; p[2] = y; }
    if (r.train && f32_array && (int)T[T_NSTAGE] == 0) {
        for (int k = 0; k < 3; ++k) {
            float q = (float)(p[k] + clip(sigma * z[k], clp));                 // pc_np += jitter (in-place f32)
            q = q * (float)T[T_SCALE];                                         // pc_np * scale (f32)
            out[k] = r.translation_perturbation ? (float)((double)q + T[T_SHIFT + k]) : q;   // pc_np += shift
        }
        if (cloud == 1) transform3(T, out, true);
        return;
    }
    if (r.train) {
        const int ns = (int)T[T_NSTAGE];
        for (int s = 0; s < ns; ++s) {
            const double* R = T + T_STAGE + 9 * s;
            const double q0 = dot3(p[0], p[1], p[2], R[0], R[3], R[6]);
            const double q1 = dot3(p[0], p[1], p[2], R[1], R[4], R[7]);
            const double q2 = dot3(p[0], p[1], p[2], R[2], R[5], R[8]);
            p[0] = q0; p[1] = q1; p[2] = q2;
        }
        for (int k = 0; k < 3; ++k) p[k] = (p[k] + clip(sigma * z[k], clp)) * T[T_SCALE] + T[T_SHIFT + k];
    }
    for (int k = 0; k < 3; ++k) out[k] = (float)p[k];
    if (cloud == 1) transform3(T, out, true);
}

// The sn channels of a point: ENU -> cam on 0:3, augment (train), dst's rotation on 0:3.
USIP_HD void finish_sn(const usip_pairs_recipe& r, const double* T, int cloud, float* s, const double* z)
{
    const int Cs = r.Cs;
    if (r.enu_to_cam) { const float y = s[1]; s[1] = -s[2]; s[2] = y; }
    if (r.train) {
        if (Cs >= 3) {
            const int ns = (int)T[T_NSTAGE];
            for (int st = 0; st < ns; ++st) {
                const double* R = T + T_STAGE + 9 * st;
                const double a = s[0], b = s[1], c = s[2];
                s[0] = (float)dot3(a, b, c, R[0], R[3], R[6]);
                s[1] = (float)dot3(a, b, c, R[1], R[4], R[7]);
                s[2] = (float)dot3(a, b, c, R[2], R[5], R[8]);
            }
        }
        for (int k = 0; k < Cs; ++k) s[k] = (float)((double)s[k] + clip(r.sn_sigma * z[k], r.sn_clip));
    }
    if (cloud == 1 && Cs >= 3) transform3(T, s, false);
}

// Load one scan row's columns 0..2 and the sn columns.
USIP_HD void load_row(const usip_pairs_recipe& r, const float* row, float xyz[3], float* s)
{
    xyz[0] = row[0]; xyz[1] = row[1]; xyz[2] = row[2];
    if (r.sn_last) {
        s[0] = row[r.row_len - 1];
    } else {
        for (int k = 0; k < r.Cs; ++k) s[k] = row[3 + k];
    }
}

// fix_idx layout of a scan with n < N rows: slot j < F = q n is j % n (q whole copies), the rest a random draw of N - F
USIP_HD long long fix_copies(long long n, int N)
{
    if (n >= N) return 0;
    return (N - n + n - 1) / n;                 // smallest q >= 1 with n + q n >= N
}

// ----------------------------------------------------------------------------------------------- sources of draws
// The per-slot Philox draws of one cloud, streams TAG0 + TAG_CHOICE .. TAG0 + TAG_JIT_NODE: TAG0 = 0 for the detector's
// pairs, 16 for the descriptor's (csrc/desc_pairs_math.h), so the two builders share no draw.
template <uint32_t TAG0>
struct PhiloxSlots {
    uint64_t seed, step;
    long long base;

    USIP_HD uint64_t gp(int p) const { return (uint64_t)(base + p); }
    USIP_HD PairsPerm perm(int p, int c, uint32_t tag, uint64_t n) const
    {
        uint64_t b[4];
        pairs_block(seed, step, gp(p), TAG0 + tag, c, 0, b);
        PairsPerm q;
        q.init(b, n);
        return q;
    }
    // scan-relative row of slot j
    USIP_HD long long row(int p, int c, long long n, int N, int j) const
    {
        const PairsPerm q = perm(p, c, TAG_CHOICE, (uint64_t)n);
        const long long F = fix_copies(n, N) * n;
        return j < F ? j % n : (long long)q((uint64_t)(j - F));
    }
    USIP_HD int cand(int p, int c, int N, int i) const { return (int)perm(p, c, TAG_CAND, (uint64_t)N)((uint64_t)i); }
    USIP_HD int first(int p, int c, int n_sub) const { return (int)perm(p, c, TAG_FIRST, (uint64_t)n_sub)(0); }
    USIP_HD void jit_pc(int p, int c, int, int j, double* z) const
    {
        uint64_t b[4];
        pairs_block(seed, step, gp(p), TAG0 + TAG_JIT_PC, c, (uint64_t)j, b);
        normal4(b, z);
    }
    USIP_HD void jit_sn(int p, int c, int, int Cs, int j, double* z) const
    {
        uint64_t b[4];
        double t[4];
        for (int e = 0; 4 * e < Cs; ++e) {
            pairs_block(seed, step, gp(p), TAG0 + TAG_JIT_SN, c, 2 * (uint64_t)j + e, b);
            normal4(b, t);
            for (int k = 0; k < 4 && 4 * e + k < Cs; ++k) z[4 * e + k] = t[k];
        }
    }
    USIP_HD void jit_node(int p, int c, int, int m, double* z) const
    {
        uint64_t b[4];
        pairs_block(seed, step, gp(p), TAG0 + TAG_JIT_NODE, c, (uint64_t)m, b);
        normal4(b, z);
    }
};

struct PhiloxDraws : PhiloxSlots<0> {
    // half h of the pair's draws, u[12 h .. 12 h + 12): uniforms, then the perturbation normals over u[4..6] / u[15..17]
    USIP_HD void params(int p, int h, double* u) const
    {
        uint64_t b[4];
#pragma unroll
        for (int e = 3 * h; e < 3 * h + 3; ++e) {
            pairs_block(seed, step, gp(p), TAG_PARAM_U, 0, e, b);
#pragma unroll
            for (int i = 0; i < 4; ++i) u[4 * e + i] = u53(b[i]);
        }
        double z[4];
        pairs_block(seed, step, gp(p), TAG_PARAM_N, 0, h, b);
        normal4(b, z);
        double* n = u + (h ? 15 : 4);
        n[0] = z[0]; n[1] = z[1]; n[2] = z[2];
    }
};

// The recorded draws (layouts in include/usip_hip.h).  Indices are clamped into range: a bad fixture gives wrong values,
// never an access outside the bank.
struct ExplicitDraws {
    usip_pairs_draws d;
    int N, n_sub, M, Cs;

    USIP_HD void params(int p, int h, double* u) const
    {
#pragma unroll
        for (int i = 12 * h; i < 12 * h + 12; ++i) u[i] = d.params[(long long)p * USIP_PAIRS_NPARAM + i];
    }
    USIP_HD long long row(int p, int c, long long n, int, int j) const
    {
        const long long v = d.rows[((long long)p * 2 + c) * N + j];
        return v < 0 ? 0 : (v >= n ? n - 1 : v);
    }
    USIP_HD int cand(int p, int c, int, int i) const
    {
        return clampi(d.cand[((long long)p * 2 + c) * n_sub + i], 0, N - 1);
    }
    USIP_HD int first(int p, int c, int) const
    {
        return clampi(d.first[p * 2 + c], 0, n_sub - 1);
    }
    USIP_HD void jit_pc(int p, int c, int, int j, double* z) const
    {
        for (int k = 0; k < 3; ++k) z[k] = d.jit_pc[(((long long)p * 2 + c) * N + j) * 3 + k];
    }
    USIP_HD void jit_sn(int p, int c, int, int, int j, double* z) const
    {
        for (int k = 0; k < Cs; ++k) z[k] = d.jit_sn[(((long long)p * 2 + c) * N + j) * Cs + k];
    }
    USIP_HD void jit_node(int p, int c, int, int m, double* z) const
    {
        for (int k = 0; k < 3; ++k) z[k] = d.jit_node[(((long long)p * 2 + c) * M + m) * 3 + k];
    }
};

// ------------------------------------------------------------------------------------------------ the cloud stage
// Cloud q = c * P + p is cloud c (0 or 1) of pair p.  A View tells the two builders apart:
//   table(q, p)           the cloud's float64 table
//   scan(q, p, o0, n)     its scan's first bank row and row count
//   dst(c)                1 where the cloud takes the table's transform
//   usable(n, N)          false for a scan the entry points refuse on the host (min_rows)
//   move(p, c, x)         float64 coordinates out of raw_xyz -> the cloud's own frame (empty but for the indoor builder's
//   move_sn(p, c, s)      ICP move, csrc/indoor_pairs_math.h; the normals' counterpart, rounded to float32)
//   node_xyz(...)         a node's float64 coordinates, preset to candidate ci's float32 ones (empty likewise)
//   f32_array(c)          whether the reference holds the cloud's points in a float32 array when augment begins
//   post(c, T, x, full)   after finish_xyz / finish_sn, on a point or node (full) or on sn[0:3]: a transform of the View's own
struct CloudOut {
    float* pc[2];           // [P][3][N] per cloud of the pair
    float* sn[2];           // [P][Cs][N]
    float* node[2];         // [P][3][M]
    int32_t* rows;          // [2P][N] or null
    int32_t* node_slots;    // [2P][M] or null
};

// The detector's pair: one table per pair, the scan from the call's ids, cloud 1 takes the dst transform.
struct PairView {
    const double* tab;      // [P][T_SIZE]
    const int64_t* offsets;
    const int32_t* scan_ids;
    int num_scans;

    USIP_HD const double* table(int, int p) const { return tab + (long long)p * T_SIZE; }
    USIP_HD void scan(int, int p, long long& o0, long long& n) const
    {
        const int s = clampi(scan_ids[p], 0, num_scans - 1);
        o0 = offsets[s];
        n = offsets[s + 1] - o0;
    }
    USIP_HD static int dst(int c) { return c; }
    USIP_HD static bool usable(long long n, int) { return n >= 1; }
    USIP_HD static void move(int, int, double*) {}
    USIP_HD static void move_sn(int, int, float*) {}
    template <class Src>
    USIP_HD static void node_xyz(const usip_pairs_recipe&, const Src&, int, int, int, int, double*) {}
    USIP_HD static bool f32_array(int) { return true; }
    USIP_HD static void post(int, const double*, float*, bool) {}
};

// Slot j of cloud q: slot -> scan row through the keyed bijection (or the fix_idx layout), one row load, augment and
// transform, pc / sn written transposed; slots j < n_sub first write the un-augmented FPS candidate j of cd [3][n_sub]
// (first: written after the slot's own work, the Philox kernel holds enough across it to spill scalar registers).
template <class Src, class View>
USIP_HD void cloud_point(const usip_pairs_recipe& r, const Src& src, const View& v, const float* bank, int P, int q, int j,
                         const CloudOut& out, float* cd)
{
    const int N = r.N, c = q / P, p = q - c * P;
    long long o0, n;
    v.scan(q, p, o0, n);
    if (!v.usable(n, N)) return;
    const double* T = v.table(q, p);
    if (j < r.n_sub) {
        const long long crow = src.row(p, c, n, N, src.cand(p, c, N, j));
        float cx[3];
        raw_xyz(T, bank + (o0 + crow) * r.row_len, cx);
        double cm[3] = {cx[0], cx[1], cx[2]};
        v.move(p, c, cm);
        for (int k = 0; k < 3; ++k) cd[(long long)k * r.n_sub + j] = (float)cm[k];
    }
    const long long row = src.row(p, c, n, N, j);
    const float* rp = bank + (o0 + row) * r.row_len;
    float xyz[3], s[MAX_CS];
    load_row(r, rp, xyz, s);
    raw_xyz(T, rp, xyz);
    double zp[4] = {0, 0, 0, 0}, zs[MAX_CS];
    for (int k = 0; k < MAX_CS; ++k) zs[k] = 0.0;
    if (r.train) {
        src.jit_pc(p, c, N, j, zp);
        src.jit_sn(p, c, N, r.Cs, j, zs);
    }
    v.move_sn(p, c, s);
    float o[3];
    finish_xyz(r, T, v.dst(c), xyz, zp, r.pc_sigma, r.pc_clip, v.f32_array(c), o, [&](double* x) { v.move(p, c, x); });
    finish_sn(r, T, v.dst(c), s, zs);
    v.post(c, T, o, true);
    if (r.Cs >= 3) v.post(c, T, s, false);
    float* pc = out.pc[c] + (long long)p * 3 * N;
    float* sn = out.sn[c] + (long long)p * r.Cs * N;
    for (int k = 0; k < 3; ++k) pc[(long long)k * N + j] = o[k];
    for (int k = 0; k < r.Cs; ++k) sn[(long long)k * N + j] = s[k];
    if (out.rows) out.rows[(long long)q * N + j] = (int32_t)row;
}

// Node m of cloud q: the candidate FPS chose (fps [M], indices into cd), augment with its own jitter, transform.
template <class Src, class View>
USIP_HD void cloud_node(const usip_pairs_recipe& r, const Src& src, const View& v, int P, int q, int m, const float* cd,
                        const int32_t* fps, const CloudOut& out)
{
    const int M = r.M, ns = r.n_sub, c = q / P, p = q - c * P;
    const double* T = v.table(q, p);
    const int ci = clampi(fps[m], 0, ns - 1);
    const float xyz[3] = {cd[ci], cd[ns + ci], cd[2 * ns + ci]};
    double z[4] = {0, 0, 0, 0};
    if (r.train) src.jit_node(p, c, M, m, z);
    float o[3];
    finish_xyz(r, T, v.dst(c), xyz, z, r.node_sigma, r.node_clip, false, o,
               [&](double* x) { v.node_xyz(r, src, q, p, c, ci, x); });
    v.post(c, T, o, true);
    float* node = out.node[c] + (long long)p * 3 * M;
    for (int k = 0; k < 3; ++k) node[(long long)k * M + m] = o[k];
    if (out.node_slots) out.node_slots[(long long)q * M + m] = src.cand(p, c, r.N, ci);
}

// Shape rules shared by the device and host entry points.
inline bool recipe_ok(const usip_pairs_recipe* r)
{
    if (!r) return false;
    if (r->N < 1 || r->M < 1 || r->Cs < 1 || r->Cs > MAX_CS || r->n_sub < 1 || r->row_len > MAX_ROW) return false;
    if (r->n_sub > 16384 || r->M > r->n_sub || r->n_sub > r->N) return false;
    if (r->sn_last ? (r->Cs != 1 || r->row_len < 4) : (3 + r->Cs > r->row_len)) return false;
    if (r->enu_to_cam && (r->Cs < 3 || r->sn_last)) return false;
    if (r->dst_rot_type != 0 && r->dst_rot_type != 2 && r->dst_rot_type != 3) return false;
    return true;
}

}  // namespace usip_pairs
