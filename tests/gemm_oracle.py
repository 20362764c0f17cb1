"""Plain references of the shared-MLP product family (csrc/shared_mlp.hip, shared_mlp_bf16.hip, shared_mlp_x3.hip,
gemm_x2d.hip, gemm_x2f.hip, narrow_fwd.hip and the weight-gradient kernels) and the operands their tests share.  numpy on
the CPU only; independent of the library (usip_amd is not imported here).

The method: operands for which the product is EXACT.  Every kernel of the family multiplies 16-bit planes (or fp32 values) on
the matrix cores and accumulates in fp32.  The builders here hand out operands such that
  * every element is reproduced exactly by the planes its form keeps,
  * every plane pair the form drops has a zero factor,
  * every product is an integer multiple of one unit u = a_unit * v_unit and sum |products| (+ |bias| + |row bias|) stays
    below 2^24 u for every output element,
so the result is the fp64 product whatever the accumulation order, tile shape, wave layout or K split, and that product is an
fp32 number: a form is right iff its output EQUALS want.astype(float32) elementwise.  The same is asserted for the statistics
partials (sum Y, sum Y^2), the weight-gradient tiles and the fork add.

What the model of the operand preparation restates, and where it was read:
  pow2_scale            split_common.h::pow2_scale
  weight scale          shared_mlp_x3.hip::x2h_weight_scale: pow2_scale(max|A|, X2H_TOP - 1): max|A| 2^e in [2^13, 2^14)
  forward bound         shared_mlp_x3.hip::gemm_x3p_kernel (NPL == 2, PRO_AFFINE_RELU), gemm_x2d.hip, gemm_x2f.hip:
                        max_k |c0| / invstd * sqrt(nb P) + |fma(mean, c0, c1)|, scale pow2_scale(bound, X2H_TOP)
  backward bound        the same places: max of coef4[4][0 .. ceil(K / 64))
  fp16 two-plane split  split_common.h::split_pair_h (RNE twice)
  bf16 three-plane      split_common.h::split_pair (RNE three times)
  plane pairs           PLANE_PAIRS below
A builder's big values sit in channel PAIRS (probe, canceller): the probe's weight (or streamed element) has its low planes
populated, the canceller is minus almost that, and both meet the same small factor -- the output is then a SMALL number whose
value depends on the low-plane product, so the statistics (sum Y^2) stay exact too."""
import math

import numpy as np

X2H_TOP = 15                                  # split_common.h
XBK = 16                                      # k per stage
X2H_PARTS = 32                                # partial maxima behind a two-plane image: trailer floats [4, 4 + 32)

# (weight plane, streamed plane) pairs a form multiplies; 0 = high plane.
#   x2h  shared_mlp_x3.hip USIP_X3_FIRST_HALF / SECOND_HALF with NPL == 2: (1,0) (0,1) | (0,0); the same three in
#        gemm_x2d.hip, gemm_x2f.hip, gemm_x2r_kernel and wgrad_x3_kernel<.., 2> / wgrad_x2l_kernel (USIP_X3W_*)
#   x3   the same macros with NPL == 3: (2,0) (0,2) (1,1) | (1,0) (0,1) (0,0); shared_mlp_bf16.hip NS == 3 keeps the same six
#   a    one plane: the bf16 mode (operands rounded to bf16) -- and fp32, which needs no split at all
PLANE_PAIRS = {
    "x2h": ((1, 0), (0, 1), (0, 0)),
    "x3": ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)),
    "a": ((0, 0),),
}
NPLANES = {"x2h": 2, "x3": 3, "a": 1}


# ------------------------------------------------------------------------------------------------ number formats
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def exact32(v64, what):
    """the float32 of a float64 array, asserted to be that number"""
    v64 = np.asarray(v64, np.float64)
    out = v64.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v64), "%s is not exact in float32" % what
    return out


def pow2_scale(bound, top):
    """split_common.h::pow2_scale -> float32 power of two"""
    b = int(bits(np.float32(bound)).reshape(-1)[0])
    eb = (b >> 23) & 0xff
    e = top - (eb - 126)
    e = max(-60, min(60, e))
    if eb == 255:
        e = 0
    return np.float32(2.0 ** e)


def weight_scale(A):
    """2^e with max|A| 2^e in [2^13, 2^14); an all-zero operand gets 2^60"""
    mx = np.float32(np.abs(np.asarray(A, np.float32)).max()) if np.size(A) else np.float32(0)
    return pow2_scale(mx, X2H_TOP - 1)


def forward_bound(coef, nb, P):
    """the kernel's bound of relu(fma(x, c0, c1)) from coef = [4][K] (scale, shift, mean, invstd), one float32 operation after
    the other as the kernels write it (the library is built without contraction: usip_amd/build.py):
    fabsf(c0) / invstd * sqrtf((float)nb * (float)P) + fabsf(fmaf(mean, c0, c1))"""
    c = np.asarray(coef, np.float32)
    rn = np.sqrt(np.float32(nb) * np.float32(P), dtype=np.float32)
    first = (np.abs(c[0]) / c[3]).astype(np.float32)
    prod = (first * rn).astype(np.float32)
    mean_term = np.abs((c[2].astype(np.float64) * c[0].astype(np.float64) + c[1].astype(np.float64)).astype(np.float32))
    return np.float32((prod + mean_term).astype(np.float32).max())


def invstd_for_bound(target, nb, P):
    """an invstd (float32) with fl(fl(1 / invstd) * sqrtf(nb P)) == target exactly, or None: lets a fixture put the bound the
    kernel derives from a channel with |c0| = 1 on a short dyadic whatever the sample count"""
    rn = np.sqrt(np.float32(nb) * np.float32(P), dtype=np.float32)
    start = int(bits(np.float32(float(rn) / float(target))).reshape(-1)[0])
    cand = (start + np.arange(-4096, 4097)).astype(np.uint32).view(np.float32)
    q = (np.float32(1.0) / cand).astype(np.float32)
    hit = np.flatnonzero((q * rn).astype(np.float32) == np.float32(target))
    return None if hit.size == 0 else np.float32(cand[hit[0]])


def backward_bound(coef4, K):
    """max of row 4 of coef4 over ceil(K / 64) entries"""
    c = np.asarray(coef4, np.float32)
    return np.float32(c[4, :(K + 63) // 64].max())


def rne_bf16(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32"""
    u = bits(x).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def split2h(x):
    """split_pair_h: float32 -> (hi, lo) float16 planes"""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def split3(x):
    """split_pair: float32 -> (h, m, l) bf16 planes held as float32"""
    x = np.asarray(x, np.float32)
    h = rne_bf16(x)
    r1 = (x - h).astype(np.float32)
    m = rne_bf16(r1)
    r2 = (r1 - m).astype(np.float32)
    return h, m, rne_bf16(r2)


def planes_of(form, x_scaled):
    """the planes `form` keeps of an (already scaled) float32 operand, as float64 arrays; asserts that they are zero or NORMAL
    numbers of their format and sum back to the operand exactly"""
    x = np.asarray(x_scaled, np.float32)
    if form == "x2h":
        pl = [p.astype(np.float64) for p in split2h(x)]
        tiny = 2.0 ** -14
    elif form == "x3":
        pl = [p.astype(np.float64) for p in split3(x)]
        tiny = 2.0 ** -126
    else:
        pl = [rne_bf16(x).astype(np.float64)]
        tiny = 2.0 ** -126
    for p in pl:
        assert np.all(np.isfinite(p)), "a plane overflows its format"
        assert np.all((p == 0) | (np.abs(p) >= tiny)), "a plane value is subnormal in its format"
    assert np.array_equal(sum(pl), x.astype(np.float64)), "the planes of form %s do not reproduce the operand" % form
    return pl


def dropped_pairs_zero(form, a_planes, v_planes):
    """every pair the form drops has a zero factor in every channel k.  a_planes [M,K], v_planes [nb,K,P]"""
    kept = set(PLANE_PAIRS[form])
    n = NPLANES[form]
    for i in range(n):
        for j in range(n):
            if (i, j) in kept:
                continue
            a_nz = np.any(a_planes[i] != 0, axis=0)                           # [K]
            v_nz = np.any(v_planes[j] != 0, axis=(0, 2))
            if np.any(a_nz & v_nz):
                return False
    return True


# ------------------------------------------------------------------------------------------------ prologues, products
def pool_dz(dp, arg, group):
    """PRO_BN_BWD_POOL's synthesised dZ[b][k][p] = (p % group == arg[b][k][p / group]) ? dp[b][k][p / group] : 0"""
    nb, K, Gn = dp.shape
    P = Gn * group
    pos = np.arange(P) % group
    hit = np.repeat(arg, group, axis=2) == pos[None, None, :]
    return np.where(hit, np.repeat(np.asarray(dp, np.float64), group, axis=2), 0.0)


def prologue(pro, X, X2=None, coef=None, pool=None):
    """pro(X) in float64: 0 none | 1 relu(fma(x, c0, c1)) | 2 fma(c0, [fma(y, c0, c1) > 0 ? dZ : 0], fma(c2, y, c3)) with
    x = dZ, X2 = y (mlp_common.h::pro_apply) | 3 the same with dZ from pool = (dpooled, arg, group)"""
    if pro == 0:
        return np.asarray(X, np.float64)
    c = np.asarray(coef, np.float64)
    col = lambda r: c[r][None, :, None]                                      # noqa: E731
    if pro == 1:
        return np.maximum(np.asarray(X, np.float64) * col(0) + col(1), 0.0)
    y = np.asarray(X2, np.float64)
    dz = pool_dz(*pool) if pro == 3 else np.asarray(X, np.float64)
    on = (y * col(0) + col(1)) > 0.0
    return col(0) * np.where(on, dz, 0.0) + (col(2) * y + col(3))


def product(A, V, bias=None, rowbias=None, rb_group=1):
    """Y[b] = A . V[b] + bias + rowbias[b][:, p // rb_group] in float64.  A [M,K], V [nb,K,P]"""
    Y = np.matmul(np.asarray(A, np.float64), np.asarray(V, np.float64))
    if bias is not None:
        Y = Y + np.asarray(bias, np.float64)[None, :, None]
    if rowbias is not None:
        Y = Y + np.repeat(np.asarray(rowbias, np.float64), rb_group, axis=2)
    return Y


def fork_add(Y, dp, arg, group):
    """the FORK add: Y[b][m][g * group + arg[b][m][g]] += dp[b][m][g]"""
    out = np.array(Y, np.float64)
    nb, M, Gn = dp.shape
    b, m, g = np.meshgrid(np.arange(nb), np.arange(M), np.arange(Gn), indexing="ij")
    out[b, m, g * group + arg] += np.asarray(dp, np.float64)
    return out


def stats_by_tile(Y, tile):
    """[2][M][nb * ceil(P / tile)]: (sum Y, sum Y^2) of every `tile` positions (mlp_common.h::gemm_epilogue: slot tn = b * tpc
    + position tile; usip_mlp_gemm_tiles: 256 positions at M <= 64, 128 above)"""
    nb, M, P = Y.shape
    tpc = (P + tile - 1) // tile
    out = np.zeros((2, M, nb * tpc))
    for b in range(nb):
        for t in range(tpc):
            seg = Y[b, :, t * tile:(t + 1) * tile]
            out[0, :, b * tpc + t] = seg.sum(axis=1)
            out[1, :, b * tpc + t] = (seg * seg).sum(axis=1)
    return out


def x2r_walk(nb, P, cap=512):
    """gemm_x2r_kernel's tile walk: tiles of 64 positions numbered b * tpc + t, workgroup w of G = min(total, 512) takes tiles
    w, w + G, ...  -> (G, [list of (b, t) per workgroup])"""
    tpc = (P + 63) // 64
    total = nb * tpc
    G = min(total, cap)
    return G, [[divmod(t, tpc) for t in range(w, total, G)] for w in range(G)]


def stats_x2r(Y, cap=512):
    """[2][M][G]: one slot per persistent workgroup of gemm_x2r_kernel (cap 512); narrow_fwd_kernel walks its 64-position tiles
    the same way with G = usip_mlp_narrow_forward_blocks (768 at M 64, 512 at M 128)"""
    nb, M, P = Y.shape
    G, walk = x2r_walk(nb, P, cap)
    out = np.zeros((2, M, G))
    for w, tiles in enumerate(walk):
        for b, t in tiles:
            seg = Y[b, :, t * 64:(t + 1) * 64]
            out[0, :, w] += seg.sum(axis=1)
            out[1, :, w] += (seg * seg).sum(axis=1)
    return out


# ------------------------------------------------------------------------------------------------ the split weight image
def lds_off(row, half):
    """split_common.h::lds_off: byte offset of (row, 16-B half) inside a [rows][16 x 16-bit] plane"""
    return row * 32 + ((half ^ (row >> 3)) & 1) * 16


def image_bytes(M, K, bm, npl):
    return ((M + bm - 1) // bm) * ((K + XBK - 1) // XBK) * npl * bm * 32


def image_ref(A, bm, form):
    """The image usip_mlp_split3_f32 (form x3) / usip_mlp_split2h_f32 (x2h) writes for A [M,K] with bm-row tiles: uint16 array
    (stage order (mt, ks, plane), each plane [bm][16] through lds_off, zero beyond M x K) and, for x2h, the scale that belongs
    in trailer float 0.  shared_mlp_x3.hip::split3_tiles_kernel."""
    A = np.asarray(A, np.float32)
    M, K = A.shape
    npl = NPLANES[form]
    nmt, nks = (M + bm - 1) // bm, (K + XBK - 1) // XBK
    pad = np.zeros((nmt * bm, nks * XBK), np.float32)
    pad[:M, :K] = A
    scale = weight_scale(A) if form == "x2h" else np.float32(1.0)
    if form == "x2h":
        pl = [p.view(np.uint16) for p in split2h(pad * scale)]
    else:
        pl = [(bits(p) >> 16).astype(np.uint16).reshape(pad.shape) for p in split3(pad)]
    out = np.zeros(image_bytes(M, K, bm, npl) // 2, np.uint16)
    rows = np.arange(bm)
    for mt in range(nmt):
        for ks in range(nks):
            for s in range(npl):
                base = ((mt * nks + ks) * npl + s) * bm * 16                  # in 16-bit units
                blk = pl[s][mt * bm:(mt + 1) * bm, ks * XBK:(ks + 1) * XBK]
                for half in range(2):
                    off = (rows * 32 + ((half ^ (rows >> 3)) & 1) * 16) // 2
                    for i in range(8):
                        out[base + off + i] = blk[:, half * 8 + i]
    return out, scale


# ------------------------------------------------------------------------------------------------ exactness claims
def assert_exact_product(A, V, unit_log2, bias=None, rowbias=None, rb_group=1):
    """sum_k |A V| + |bias| + |row bias| < 2^24 units of 2^-unit_log2 for every output, every term a multiple of the unit
    -> want (float64), asserted to be an fp32 number"""
    s = 2.0 ** unit_log2
    a, v = np.abs(np.asarray(A, np.float64)), np.abs(np.asarray(V, np.float64))
    # a conservative statement of "every product is a multiple of u": the operands are multiples of units whose product is u
    tot = np.matmul(a, v)
    if bias is not None:
        tot = tot + np.abs(np.asarray(bias, np.float64))[None, :, None]
    if rowbias is not None:
        tot = tot + np.repeat(np.abs(np.asarray(rowbias, np.float64)), rb_group, axis=2)
    assert np.array_equal(tot * s, np.round(tot * s)), "a term is no multiple of the unit"
    assert float(tot.max(initial=0.0)) * s < 2.0 ** 24, "sum |products| reaches 2^24 units"
    want = product(A, V, bias, rowbias, rb_group)
    exact32(want, "the product")
    return want


def assert_exact_sums(terms, unit_log2, axis, what):
    """sum |terms| < 2^24 units along axis, terms multiples of the unit"""
    s = 2.0 ** unit_log2
    t = np.abs(np.asarray(terms, np.float64)) * s
    assert np.array_equal(t, np.round(t)), "%s: a term is no multiple of the unit" % what
    assert float(t.sum(axis=axis).max(initial=0.0)) < 2.0 ** 24, "%s reaches 2^24 units" % what


def assert_exact_stats(Y, unit_log2):
    """sum Y and sum Y^2 over ALL positions of a channel (hence over every slot) stay below 2^24 units"""
    assert_exact_sums(np.moveaxis(Y, 1, 0).reshape(Y.shape[1], -1), unit_log2, 1, "sum Y")
    assert_exact_sums(np.moveaxis(Y * Y, 1, 0).reshape(Y.shape[1], -1), 2 * unit_log2, 1, "sum Y^2")


def operand_record(form, A, V, a_scale=1.0, v_scale=1.0):
    """Asserts the plane claims of (A, V) for `form` and returns which value classes they hold:
    b = low planes populated in the weights, c = in the streamed operand."""
    ap = planes_of(form, (np.asarray(A, np.float64) * float(a_scale)).astype(np.float32))
    vp = planes_of(form, exact32(np.asarray(V, np.float64) * float(v_scale), "the scaled streamed operand"))
    assert dropped_pairs_zero(form, ap, vp), "a dropped plane pair has two nonzero factors"
    rec = dict(a_low=[bool(np.any(p != 0)) for p in ap[1:]], v_low=[bool(np.any(p != 0)) for p in vp[1:]])
    rec["class_b"] = all(rec["a_low"]) if ap[1:] else False
    rec["class_c"] = all(rec["v_low"]) if vp[1:] else False
    # channels whose low-plane products are kept AND nonzero, by 16-k stage: a kernel that forgets a stage's low plane fails
    if form != "a":
        kb = np.any(ap[1] != 0, axis=0) & np.any(vp[0] != 0, axis=(0, 2))
        kc = np.any(vp[1] != 0, axis=(0, 2)) & np.any(ap[0] != 0, axis=0)
        rec["b_channels"], rec["c_channels"] = np.flatnonzero(kb).tolist(), np.flatnonzero(kc).tolist()
        # ... and by tile of 64 positions: how many tiles (per cloud) meet no weights-low / no streamed-low product
        a_lo, a_hi = np.any(ap[1] != 0, axis=0), np.any(ap[0] != 0, axis=0)
        b_hit = np.any((vp[0] != 0) & a_lo[None, :, None], axis=1)             # [nb, P]
        c_hit = np.any((vp[1] != 0) & a_hi[None, :, None], axis=1)
        edges = np.arange(0, b_hit.shape[1], 64)
        rec["tiles_without_b"] = int((np.add.reduceat(b_hit, edges, axis=1) == 0).sum())
        rec["tiles_without_c"] = int((np.add.reduceat(c_hit, edges, axis=1) == 0).sum())
    return rec


# ------------------------------------------------------------------------------------------------ builders
def _big(form, j, kind=0):
    """(value with its low planes populated, canceller) as integers; value - canceller is 1, 2 or 3"""
    if form == "x2h":
        v = [2048 + 2 * (j % 32) + 1, 4096 + 4 * (j % 32) + 1, 8192 + 8 * (j % 32) + 5][(j + kind) % 3]
    else:
        v = (1 << 17) + 257 + 2 * (j % 100)
    return v, v - (1 + j % 3)


def special_positions(P):
    s = sorted({p for p in (0, 1, 63, 64, 127, 128, 129, 255, 256, 257, P // 2, P - 2, P - 1) if 0 <= p < P})
    return s


def probe_channels(form, K):
    """[(kind, k, k + 1)]: channel pairs that carry the big values: 'b' weights, 'c' streamed operand, 'd' (x3) both mid
    planes, 't' (x2h) the bound-tight element.  Every 16-k stage gets a b and a c pair, and so do the last four channels."""
    if form == "a" or K < 8:
        return []
    out, used = [], set()

    def add(kind, k):
        if k >= 0 and k + 1 < K and k not in used and k + 1 not in used:
            out.append((kind, k, k + 1))
            used.update((k, k + 1))
    for s0 in range(0, K, XBK):
        add("b" if (s0 // XBK) % 2 == 0 else "c", s0)
        add("c" if (s0 // XBK) % 2 == 0 else "b", s0 + 2)
    add("b", K - 4)
    add("c", K - 2)
    add("t" if form == "x2h" else "d", 6)
    return out


def _design(form, M, K, nb, P, rng, signed, pair_pos=None, tile_pos=None):
    """integer operands: A [M,K], V [nb,K,P] and roles.  pair_pos(kind, i) -> positions (per cloud) of probe pair i, tile_pos
    (kind, i) -> one more in every tile of 64 positions (the smallest tile of the family: every tile of every kernel, and
    every visit of a persistent workgroup, then meets a weights-low and a streamed-low product)."""
    A = np.zeros((M, K), np.int64)
    V = np.zeros((nb, K, P), np.int64)
    probes = probe_channels(form, K)
    taken = {k for _, k0, k1 in probes for k in (k0, k1)}
    free = [k for k in range(K) if k not in taken]
    k_off = free[0] if len(free) > 2 else None
    k_on = free[1] if len(free) > 2 else None
    samples = nb * P
    want_terms = 2.0 if samples <= 4096 else (1.0 if samples <= 65536 else 0.5)
    dens = min(1.0, math.sqrt(want_terms / max(len(free), 1)))
    for k in free:
        A[:, k] = rng.integers(-2, 3, M) * (rng.random(M) < dens)
        hi = 4 if samples <= 4096 else 3
        v = rng.integers(1, hi, (nb, P)) * (rng.random((nb, P)) < dens)
        if signed:
            v = v * rng.choice([-1, 1], (nb, P))
        V[:, k, :] = v
    if k_off is not None:
        V[:, k_off, :] = 0
        A[:, k_off] = rng.choice([-2, -1, 1, 2], M)
        V[:, k_on, :] = rng.integers(1, 3, (nb, P))
        A[:, k_on] = rng.choice([-1, 0, 1], M)
    spec = special_positions(P)
    roles = dict(probes=probes, k_off=k_off, k_on=k_on, special={}, tight=None)
    rows = np.arange(M)
    for i, (kind, k0, k1) in enumerate(probes):
        pos = pair_pos(kind, i) if pair_pos else [spec[(i + 3 * j) % len(spec)] for j in range(3)]
        if kind in ("b", "c"):                                  # ... and one position in EVERY tile of 64 positions
            pos = list(pos) + (tile_pos(kind, i) if tile_pos else
                               [t * 64 + (7 * i + 13 * t) % min(64, P - t * 64) for t in range((P + 63) // 64)])
        pos = sorted(set(pos))
        roles["special"][(kind, k0)] = pos
        sgn = -1 if (signed and i % 2) else 1
        if kind == "b":
            big = np.array([_big(form, int(m) + i) for m in rows])
            A[:, k0], A[:, k1] = big[:, 0] * sgn, -big[:, 1] * sgn
            for b in range(nb):
                V[b, k0, pos] = V[b, k1, pos] = 1 + (b + i) % 2
        elif kind == "c":
            s = np.array([[1, -1, 2, -2, 0][(int(m) + i) % 5] for m in rows])
            A[:, k0], A[:, k1] = s, -s
            for b in range(nb):
                for j, p in enumerate(pos):
                    v, c = _big(form, 7 * i + 3 * j + b, kind=j)
                    V[b, k0, p], V[b, k1, p] = v * sgn, c * sgn
        elif kind == "d":                                      # x3: mid plane x mid plane, at one position
            A[:, k0], A[:, k1] = 257 + 2 * (rows % 2), -256
            V[0, k0, pos[0]] = V[0, k1, pos[0]] = 259 * sgn
        elif kind == "t":                                      # filled by the caller (it knows the bound)
            s = np.array([[1, -1][(int(m) + i) % 2] for m in rows])
            A[:, k0], A[:, k1] = s, -s
            roles["tight"] = (k0, k1, pos[0])
    return A, V, roles


def _neg_zero(x, idx):
    x = np.array(x, np.float32)
    if x.size:
        x.reshape(-1)[idx % x.size] = np.float32(-0.0)
    return x


def gemm_fixture(form, pro, nb, K, M, P, seed=0, bias=True, rb_group=0, stats_tile=0, pool_group=0, a_log2=17, v_log2=3,
                 fork_group=0, x2r_stats=False, red_group=None):
    """Operands of one exact GEMM case -> dict(A [M,K] f32, X / X2 / coef / pool, bias, rowbias, want f32 [nb,M,P], stats, record).

    form: which planes the operands may populate ("a", "x2h", "x3"); pro 0..3.  A = A_int 2^-a_log2, pro(X) = V_int 2^-v_log2,
    unit of the output u = 2^-(a_log2 + v_log2).  For form x2h with pro >= 1 the coefficients are such that the kernel's own
    scale of the streamed operand is 2^v_log2 (so V_int are the scaled values it splits)."""
    rng = np.random.default_rng(seed * 7919 + K * 131 + M * 17 + P + pro)
    signed = pro != 1
    au, vu = 2.0 ** -a_log2, 2.0 ** -v_log2
    ulog = a_log2 + v_log2
    u = 2.0 ** -ulog
    pair_pos = None
    if pro == 3:
        # the synthesised dZ has ONE nonzero position per run of pool_group: probe pairs take whole runs' arg positions
        runs = P // pool_group
        arg = rng.integers(0, pool_group, (nb, K, runs))

        def pair_pos(kind, i):
            return [((i * 5 + j * 3) % runs) * pool_group + int((i + j) % pool_group) for j in range(3)]

        def tile_pos(kind, i):
            out = []
            for t in range((P + 63) // 64):
                r0, r1 = (t * 64 + pool_group - 1) // pool_group, min(runs, ((t + 1) * 64) // pool_group)
                if r1 > r0:                                     # a run that lies inside the tile
                    out.append((r0 + (i + t) % (r1 - r0)) * pool_group + (3 * i + t) % pool_group)
            return out
    Ai, Vi, roles = _design(form, M, K, nb, P, rng, signed, pair_pos, tile_pos if pro == 3 else None)
    rec = dict(form=form, pro=pro, shape=(nb, K, M, P), equals_bound=False, bound_tight=False, relu_off=False, relu_on=False,
               mask_tie=False, below_bound=False)
    fx = dict(pool=None, X2=None, coef=None, bound=None)
    v_scale = 1.0

    # ---- the bound and the element at it (two-plane forms, pro >= 1)
    bound_int = None
    if form == "x2h" and pro >= 1:
        if pro == 1:
            r = int(math.floor(math.log2(math.sqrt(nb * P))))
            j = 14 - v_log2 - r
            bound_shift = j                                   # |c0| / invstd = 2^j
            # channel K / 2 (c0 = 1, c1 = 2 units) gets the invstd that puts the derived bound on 2^14 + 2 units exactly
            tight_invstd = invstd_for_bound((1 << 14) * vu, nb, P) if K > 1 else None
            bound_int = (1 << 14) + 2 if tight_invstd is not None else None
        else:
            bound_int = (1 << 14) + 2 * (seed % 2)
        if roles["tight"] is not None:
            k0, k1, p = roles["tight"]
            vt = bound_int if bound_int is not None else (1 << 14)
            if pro == 3:
                p = roles["special"][("t", k0)][0]
            Vi[0, k0, p], Vi[0, k1, p] = vt, vt - 64
            rec["bound_tight"], rec["equals_bound"], rec["below_bound"] = True, bound_int is not None, True
    A = exact32(Ai * au, "A")
    if M * K > 3:
        A = _neg_zero(A, 1) if Ai.reshape(-1)[1 % Ai.size] == 0 else A
    Vt = Vi * vu                                               # the target pro(X), float64

    # ---- raw operands behind the prologue
    if pro == 0:
        X = exact32(Vt, "X")
        zeros = np.flatnonzero(Vi.reshape(-1) == 0)
        if zeros.size:
            X.reshape(-1)[zeros[::3]] = np.float32(-0.0)
        rec["neg_zero"] = bool(zeros.size)
    elif pro == 1:
        c0 = (2.0 ** rng.integers(-1, 3, K)) * np.where(np.arange(K) % 5 == 2, -1.0, 1.0)
        c1i = rng.integers(-2, 3, K)
        if K > 1:
            c1i[K // 2], c0[K // 2] = 2, 1.0                    # the channel the bound comes from
        c1 = c1i * vu
        T = Vi.astype(np.float64)
        off = Vi == 0
        T[off] = -rng.integers(0, 4, int(off.sum()))            # pre-activation 0 (the tie: relu gives 0) or below
        rec["mask_tie"] = bool(np.any(T[off] == 0))
        X = exact32((T * vu - c1[None, :, None]) / c0[None, :, None], "X")
        if form == "x2h":
            invstd = np.abs(c0) / 2.0 ** (bound_shift - 1)      # the others: at most half the bound (+ |c1|)
            if bound_int is not None:
                invstd[K // 2] = tight_invstd
            else:
                invstd[K // 2] = np.abs(c0[K // 2]) / 2.0 ** bound_shift
        else:
            invstd = np.ones(K)
        fx["coef"] = exact32(np.stack([c0, c1, np.zeros(K), invstd]), "coef")
        if roles["k_off"] is not None:
            rec["relu_off"] = bool(np.all(Vi[:, roles["k_off"], :] == 0))
            rec["relu_on"] = bool(np.all(Vi[:, roles["k_on"], :] > 0))
    else:
        yu = 2.0 ** -2
        c0 = (2.0 ** rng.integers(-1, 2, K)) * np.where(np.arange(K) % 5 == 2, -1.0, 1.0)
        y0 = rng.integers(-2, 3, K) * yu
        c1 = -c0 * y0
        c2i, c3i = rng.integers(-1, 2, K), rng.integers(-1, 2, K)
        for kind, k0, k1 in roles["probes"]:                    # big weights: no base value, or the outputs grow large
            if kind in ("b", "d"):
                c2i[[k0, k1]] = 0
                c3i[[k0, k1]] = 0
        c2, c3 = c2i * (vu / yu), c3i * vu
        yi = rng.integers(-4, 5, (nb, K, P))
        y = yi * yu
        on = (y * c0[None, :, None] + c1[None, :, None]) > 0
        # wherever the target is not the small base value the mask must be on: move y across the threshold there
        base_i = c2i[None, :, None] * yi + c3i[None, :, None]
        need = (Vi != 0) & ~on
        step = np.sign(c0)[None, :, None] * np.ones_like(y)
        y = np.where(need, y0[None, :, None] + step * yu, y)
        yi = np.round(y / yu).astype(np.int64)
        on = (y * c0[None, :, None] + c1[None, :, None]) > 0
        base_i = c2i[None, :, None] * yi + c3i[None, :, None]
        rec["mask_tie"] = bool(np.any((y * c0[None, :, None] + c1[None, :, None]) == 0))
        if roles["k_off"] is not None:                          # a channel whose mask is off / on everywhere
            ko, kn = roles["k_off"], roles["k_on"]
            y[:, ko, :] = y0[ko] - np.sign(c0[ko]) * yu * rng.integers(0, 3, (nb, P))
            y[:, kn, :] = y0[kn] + np.sign(c0[kn]) * yu * rng.integers(1, 3, (nb, P))
            yi = np.round(y / yu).astype(np.int64)
            on = (y * c0[None, :, None] + c1[None, :, None]) > 0
            base_i = c2i[None, :, None] * yi + c3i[None, :, None]
            rec["relu_off"], rec["relu_on"] = bool(not on[:, ko, :].any()), bool(on[:, kn, :].all())
        dz = np.where(on, (Vi - base_i) * vu / c0[None, :, None], 5.0 * vu)       # 5 units where the mask hides it
        if pro == 3:
            g = pool_group
            for (kind, k0), plist in roles["special"].items():
                k1 = k0 + 1
                for p in plist:
                    arg[:, k0, p // g] = arg[:, k1, p // g] = p % g
            dp = np.take_along_axis(dz.reshape(nb, K, P // g, g), arg[..., None], axis=3)[..., 0]
            fx["pool"] = (exact32(dp, "dpooled"), arg.astype(np.int32), g)
            X = None
            rec["arg_first"], rec["arg_last"] = bool(np.any(arg == 0)), bool(np.any(arg == g - 1))
        else:
            X = exact32(dz, "dZ")
        fx["X2"] = exact32(y, "y")
        coef = np.zeros((5, K))
        coef[0], coef[1], coef[2], coef[3] = c0, c1, c2, c3
        if form == "x2h":
            nent = (K + 63) // 64
            B = bound_int * vu
            coef[4, :] = B * 2.0 ** 20                          # entries the kernel must not read
            coef[4, :nent] = B / 4
            coef[4, nent - 1] = B
        fx["coef"] = exact32(coef, "coef4")
    fx["X"] = X

    # ---- what the prologue really yields, the scale the kernel will derive, the plane claims
    V = prologue(pro, X, fx["X2"], fx["coef"], fx["pool"])
    if pro in (0, 1):
        assert np.array_equal(V, Vt), "the raw operand does not give the designed pro(X)"
    a_scale = 1.0
    if form == "x2h":
        a_scale = float(weight_scale(A))
        if pro >= 1:
            bnd = forward_bound(fx["coef"], nb, P) if pro == 1 else backward_bound(fx["coef"], K)
            fx["bound"] = float(bnd)
            v_scale = float(pow2_scale(bnd, X2H_TOP))
            assert float(np.abs(V).max()) <= float(bnd), "max |pro(X)| exceeds the bound the kernel derives"
            assert v_scale == 2.0 ** v_log2, "the kernel's scale is not the designed one"
            if rec["equals_bound"]:
                assert float(np.abs(V).max()) == float(bnd), "no element sits at the bound"
            rec["below_bound"] = bool(np.any((np.abs(V) > 0) & (np.abs(V) <= float(bnd) * (1 - 2.0 ** -8))))
        else:
            v_scale = 1.0
    rec.update(operand_record(form, A, V, a_scale, v_scale))
    rec["a_scale"], rec["v_scale"] = a_scale, v_scale
    rec["neg"] = bool(np.any(V < 0)) or bool(np.any(A < 0))
    rec["zeros"] = bool(np.any(V == 0)) and bool(np.any(A == 0))

    # ---- epilogue operands and the exact result
    bvec = exact32(rng.integers(-3, 4, M) * u, "bias") if bias else None
    rb = None
    if rb_group:
        rb = exact32(rng.integers(-2, 3, (nb, M, P // rb_group)) * u, "rowbias")
        edges = [t for t in range(128, P, 128) if t % rb_group]
        rec["rb_straddles_tile"] = bool(edges)                  # a group with positions on both sides of a tile edge
        rec["rb_groups_differ"] = bool(rb.shape[2] < 2 or np.all(np.any(rb[:, :, 1:] != rb[:, :, :-1], axis=(0, 1))))
    want = assert_exact_product(A, V, ulog, bvec, rb, max(rb_group, 1))
    fx.update(A=A, bias=bvec, rowbias=rb, rb_group=rb_group, unit_log2=ulog)
    if fork_group:
        fdp = exact32(rng.integers(-3, 4, (nb, M, P // fork_group)) * u, "fork dpooled")
        farg = rng.integers(0, fork_group, (nb, M, P // fork_group))
        farg[:, :, 0], farg[:, :, -1] = 0, fork_group - 1       # first position of a cloud, last position of a cloud
        farg[:, ::2, 0] = fork_group - 1
        farg[:, ::2, -1] = 0
        for t in range(256, P, 256):                           # ... and of every 256-position tile
            farg[:, 1::2, t // fork_group], farg[:, 1::2, t // fork_group - 1] = 0, fork_group - 1
        fdp[:, :, 0] = np.where(fdp[:, :, 0] == 0, u, fdp[:, :, 0])
        fdp[:, :, -1] = np.where(fdp[:, :, -1] == 0, -u, fdp[:, :, -1])
        want = fork_add(want, fdp, farg, fork_group)
        assert_exact_sums(np.stack([np.abs(want), np.abs(np.repeat(fdp, fork_group, axis=2))]), ulog, 0, "fork add")
        fx["fork"] = (fdp, farg.astype(np.int32), fork_group)
        rec["fork_arg_first"], rec["fork_arg_last"] = bool(np.any(farg == 0)), bool(np.any(farg == fork_group - 1))
    fx["want"] = exact32(want, "Y")
    if red_group is not None:
        fx["red"] = red_fixture(want, ulog, red_group, rng)
        rec["red_mask_tie"], rec["red_mask_off"] = fx["red"]["tie"], fx["red"]["off"]
    fx["stats"] = None
    if stats_tile or x2r_stats:
        assert_exact_stats(want, ulog)
        st = stats_x2r(want, int(x2r_stats)) if x2r_stats else stats_by_tile(want, stats_tile)
        fx["stats"] = exact32(st, "stats")
        rec["stats_slots"] = st.shape[2]
        cols = st.reshape(-1, st.shape[2]).T                    # no two slots hold the same partials: a misplaced one shows
        rec["stats_slots_differ"] = bool(len(np.unique(cols, axis=0)) == st.shape[2])
    fx["record"] = rec
    return fx


def red_fixture(dX, unit_log2, red_group, rng):
    """The `red` epilogue of gemm_x2d_kernel (gemm_x2d.hip::epilogue_x2d_fast, RED): dX [nb,M,P] is the gradient of the
    activated output of the layer with pre-BN tensor y and coefficients (scale, shift, mean, invstd); per tile of 128
    positions and channel, sum d and sum d * ((y - mean) * invstd) with d = dX where fma(y, scale, shift) > 0, the maximum of
    |d| per (tile, 256 channels), and per run of red_group positions sum d and sum y.
    -> dict(y, coef [4,M], sums [2][tiles][M], maxima [tiles * M / 256], gsum [2][nb][M][P / red_group] or None)"""
    nb, M, P = dX.shape
    yu = 0.25
    scale = (2.0 ** rng.integers(-1, 2, M)) * np.where(np.arange(M) % 3 == 1, -1.0, 1.0)
    y0 = rng.integers(-2, 3, M) * yu
    mean = rng.integers(-2, 3, M) * yu
    invstd = 2.0 ** rng.integers(-1, 2, M)
    y = rng.integers(-4, 5, (nb, M, P)) * yu
    pre = y * scale[None, :, None] - (scale * y0)[None, :, None]
    on = pre > 0
    d = np.where(on, dX, 0.0)
    xhat = (y - mean[None, :, None]) * invstd[None, :, None]
    tiles = nb * (P // 128)
    dt = d.reshape(nb, M, P // 128, 128)
    assert_exact_sums(dt, unit_log2, 3, "red sum d")
    assert_exact_sums(dt * xhat.reshape(dt.shape), unit_log2 + 3, 3, "red sum d xhat")
    sums = np.stack([dt.sum(3), (dt * xhat.reshape(dt.shape)).sum(3)])                 # [2][nb][M][tpc]
    sums = np.moveaxis(sums, 2, 3).reshape(2, tiles, M)
    mx = np.abs(dt).reshape(nb, M // 256, 256, P // 128, 128).max(axis=(2, 4))         # [nb][M/256][tpc]
    maxima = np.moveaxis(mx, 1, 2).reshape(-1)
    gsum = None
    if red_group:
        dg, yg = d.reshape(nb, M, P // red_group, red_group), y.reshape(nb, M, P // red_group, red_group)
        assert_exact_sums(dg, unit_log2, 3, "gsum d")
        gsum = exact32(np.stack([dg.sum(3), yg.sum(3)]), "gsum")
    coef = exact32(np.stack([scale, -scale * y0, mean, invstd]), "red coef")
    return dict(y=exact32(y, "red y"), coef=coef, sums=exact32(sums, "red sums"), maxima=exact32(maxima, "red maxima"),
                gsum=gsum, tie=bool(np.any(pre == 0)), off=bool(np.any(~on & (dX != 0))))


def at_storage(A, lda, a_offset, a_trans=False, fill=3.0):
    """the matrix operand as the library stores it: K-major At [K][lda] with A[m][k] = At[k][a_offset + m], or (a_trans) [M][lda]
    with A[m][k] = At[m][a_offset + k]; the columns outside the operand hold `fill` (never read)"""
    M, K = A.shape
    if a_trans:
        At = np.full((M, lda), fill, np.float32)
        At[:, a_offset:a_offset + K] = A
    else:
        At = np.full((K, lda), fill, np.float32)
        At[:, a_offset:a_offset + M] = A.T
    return At


# ------------------------------------------------------------------------------------------------ weight gradient
def wgrad_fixture(form, pro, nb, M, N, P, seed=0, pool_group=0, xpro=False, g_log2=3, x_log2=3):
    """dW[m][n] = sum_{b,p} pro(G)[b][m][p] * xpro(X)[b][n][p] with FEW nonzero values (the contraction runs over thousands of
    positions): -> dict(G, G2, coef4, pool, X, xcoef, want [M,N] f32, record).  The operands are positions-major twins of the
    GEMM's: `V` = pro(G) [nb,M,P] plays the streamed operand, Xp = xpro(X) [nb,N,P] the other one; both are prepared on the
    fly, so both may hold low planes -- per POSITION at most one of them (a dropped pair needs a zero factor per contraction
    index)."""
    rng = np.random.default_rng(seed * 104729 + M * 31 + N * 7 + P + pro)
    gu, xu = 2.0 ** -g_log2, 2.0 ** -x_log2
    ulog = g_log2 + x_log2
    signed_x = not xpro
    Gi = np.zeros((nb, M, P), np.int64)
    Xi = np.zeros((nb, N, P), np.int64)
    dens = min(1.0, 24.0 / P)
    Gi[:] = rng.integers(-2, 3, Gi.shape) * (rng.random(Gi.shape) < dens)
    xv = rng.integers(1, 3, Xi.shape) * (rng.random(Xi.shape) < dens)
    Xi[:] = xv * (rng.choice([-1, 1], Xi.shape) if signed_x else 1)
    rec = dict(form=form, pro=pro, shape=(nb, M, N, P), class_g_low=False, class_x_low=False)
    if pro == 3:
        runs = P // pool_group
        arg = rng.integers(0, pool_group, (nb, M, runs))
    if form != "a" and P >= 8:
        # probe position pairs (p, p + 1): at p the G column is big and X small, at p + 1 the canceller; likewise for X
        spec = [p for p in special_positions(P) if p + 1 < P and p % 2 == 0]
        if pro == 3:
            spec = [r * pool_group for r in range(0, runs, max(1, runs // 6))]
        for i, p in enumerate(spec):
            b = i % nb
            if pro == 3:
                pp = (p, p + pool_group) if p + pool_group < P else None
                if pp is None:
                    continue
            else:
                pp = (p, p + 1)
            Gi[b, :, pp[0]] = Gi[b, :, pp[1]] = 0
            Xi[b, :, pp[0]] = Xi[b, :, pp[1]] = 0
            if i % 2 == 0:
                big = np.array([_big(form, m + i) for m in range(M)])
                Gi[b, :, pp[0]], Gi[b, :, pp[1]] = big[:, 0], -big[:, 1]
                s = np.array([[1, 2, 0, 1][(n + i) % 4] for n in range(N)]) * (1 if not signed_x or i % 4 == 0 else -1)
                Xi[b, :, pp[0]] = Xi[b, :, pp[1]] = s
                rec["class_g_low"] = True
            else:
                big = np.array([_big(form, n + i) for n in range(N)])
                Xi[b, :, pp[0]], Xi[b, :, pp[1]] = big[:, 0], big[:, 1]
                s = np.array([[1, -1, 2, 0][(m + i) % 4] for m in range(M)])
                Gi[b, :, pp[0]], Gi[b, :, pp[1]] = s, -s
                rec["class_x_low"] = True
            if pro == 3:
                arg[b, :, pp[0] // pool_group] = 0
                arg[b, :, pp[1] // pool_group] = 0
    fx = dict(G=None, G2=None, coef4=None, pool=None, xcoef=None, bound=None, xbound=None)
    g_scale = x_scale = 1.0
    # ---- G behind its prologue
    if pro == 0:
        fx["G"] = exact32(Gi * gu, "G")
    else:
        yu = 2.0 ** -2
        c0 = (2.0 ** rng.integers(-1, 2, M)) * np.where(np.arange(M) % 5 == 2, -1.0, 1.0)
        y0 = rng.integers(-2, 3, M) * yu
        c1 = -c0 * y0
        c2i, c3i = rng.integers(-1, 2, M), np.zeros(M, np.int64)
        c2 = c2i * (gu / yu)
        yi = rng.integers(-4, 5, (nb, M, P)) * (rng.random((nb, M, P)) < dens)
        y = yi * yu
        act = lambda yy: (yy * c0[None, :, None] + c1[None, :, None]) > 0        # noqa: E731
        need = (Gi != 0) & ~act(y)
        y = np.where(need, y0[None, :, None] + np.sign(c0)[None, :, None] * yu, y)
        yi = np.round(y / yu).astype(np.int64)
        on = act(y)
        rec["mask_tie"] = bool(np.any((y * c0[None, :, None] + c1[None, :, None]) == 0))
        base_i = c2i[None, :, None] * yi
        if pro == 3:
            # only the arg position of a run carries a gradient: everything else is the base value
            pos = np.arange(P) % pool_group
            hit = np.repeat(arg, pool_group, axis=2) == pos[None, None, :]
            Gi = np.where(hit & on, Gi, base_i)
        else:
            Gi = np.where(on, Gi, base_i)
        dz = np.where(on, (Gi - base_i) * gu / c0[None, :, None], 5.0 * gu)
        if pro == 3:
            dp = np.take_along_axis(dz.reshape(nb, M, runs, pool_group), arg[..., None], axis=3)[..., 0]
            fx["pool"] = (exact32(dp, "dpooled"), arg.astype(np.int32), pool_group)
        else:
            fx["G"] = exact32(dz, "dZ")
        fx["G2"] = exact32(y, "y")
        coef = np.zeros((5, M))
        coef[0], coef[1], coef[2] = c0, c1, c2
        gb = float(np.abs(Gi).max()) * gu
        B = 2.0 ** math.ceil(math.log2(max(gb, gu))) if form == "x2h" else 1.0
        nent = (M + 63) // 64
        coef[4, :] = B * 2.0 ** 20
        coef[4, :nent] = B / 2
        coef[4, 0] = B
        fx["coef4"] = exact32(coef, "coef4")
    V = prologue(pro, fx["G"], fx["G2"], fx["coef4"], fx["pool"])
    assert np.array_equal(V, Gi * gu), "the raw operands do not give the designed pro(G)"
    # ---- X behind its prologue
    if xpro:
        s0 = (2.0 ** rng.integers(-1, 2, N)) * np.where(np.arange(N) % 5 == 2, -1.0, 1.0)
        s1i = rng.integers(-2, 3, N)
        T = Xi.astype(np.float64)
        off = Xi == 0
        T[off] = -rng.integers(0, 3, int(off.sum()))
        Xraw = exact32((T * xu - (s1i * xu)[None, :, None]) / s0[None, :, None], "X")
        xb = float(np.abs(Xi).max()) * xu
        Bx = 2.0 ** math.ceil(math.log2(max(xb, xu)) + 1)
        rn = math.sqrt(nb * P)
        jx = math.floor(math.log2(Bx / rn))
        invstd = np.abs(s0) / 2.0 ** jx
        fx["xcoef"] = exact32(np.stack([s0, s1i * xu, np.zeros(N), invstd]), "xcoef")
        fx["X"] = Xraw
        Xp = np.maximum(Xraw.astype(np.float64) * s0[None, :, None] + (s1i * xu)[None, :, None], 0.0)
        assert np.array_equal(Xp, Xi * xu)
    else:
        fx["X"] = exact32(Xi * xu, "X")
        Xp = Xi * xu
    if form == "x2h" and pro >= 2 and xpro:                   # (what the two-plane kernels take; else the values go unscaled)
        fx["bound"] = float(backward_bound(fx["coef4"], M))
        g_scale = float(pow2_scale(fx["bound"], X2H_TOP))
        fx["xbound"] = float(forward_bound(fx["xcoef"], nb, P))
        x_scale = float(pow2_scale(fx["xbound"], X2H_TOP))
        assert float(np.abs(V).max()) <= fx["bound"] and float(np.abs(Xp).max()) <= fx["xbound"]
    # ---- plane claims: positions are the contraction index; (g planes, x planes) per position
    gp = planes_of(form, exact32(V * g_scale, "scaled pro(G)"))
    xp = planes_of(form, exact32(Xp * x_scale, "scaled X"))
    kept = set(PLANE_PAIRS[form])
    for i in range(NPLANES[form]):
        for j in range(NPLANES[form]):
            if (i, j) not in kept:
                g_nz, x_nz = np.any(gp[i] != 0, axis=1), np.any(xp[j] != 0, axis=1)          # [nb, P]
                assert not np.any(g_nz & x_nz), "a dropped plane pair has two nonzero factors"
    flat = lambda t: np.moveaxis(t, 1, 0).reshape(t.shape[1], -1)              # noqa: E731
    tot = (flat(np.abs(V)) @ flat(np.abs(Xp)).T) * 2.0 ** ulog
    assert np.array_equal(tot, np.round(tot)) and float(tot.max()) < 2.0 ** 24, "sum |products| reaches 2^24 units"
    want = flat(V) @ flat(Xp).T
    fx["want"] = exact32(want, "dW")
    rec["nonzero_out"] = int(np.count_nonzero(want))
    fx["record"] = rec
    return fx


# ------------------------------------------------------------------------------------------------ the weight-gradient segment plans
def wgrad_plan(M, N, P, nb):
    """shared_mlp.hip::wgrad_plan -> (seglen, segs, tiles): the slicing of the 64 x 64 / 128 x 128 tile kernels"""
    small = M <= 64 and N <= 64
    bm = 64 if small else 128
    tiles = ((M + bm - 1) // bm) * ((N + bm - 1) // bm)
    want = max(1, 1024 // tiles)
    per_cloud = max(1, (want + nb - 1) // nb)
    sl = ((((P + per_cloud - 1) // per_cloud) + 31) // 32) * 32
    if sl < 512:
        floor_sl = 512
        while floor_sl > 64 and tiles * nb * ((P + floor_sl - 1) // floor_sl) < 256:
            floor_sl //= 2
        sl = max(sl, floor_sl)
    return sl, (P + sl - 1) // sl, tiles


def wgrad_x3_plan(M, N, P, nb):
    """shared_mlp_x3.hip::wgrad_x3_plan (default knobs): the slicing of the 256 x 256 tile kernels"""
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    want = max(1, 256 // tiles)
    per_cloud = max(1, (want + nb - 1) // nb)
    sl = ((((P + per_cloud - 1) // per_cloud) + 31) // 32) * 32
    floor_sl = 512
    while floor_sl > 128 and tiles * nb * ((P + floor_sl - 1) // floor_sl) < 192:
        floor_sl //= 2
    sl = max(sl, floor_sl)
    return sl, (P + sl - 1) // sl, tiles
