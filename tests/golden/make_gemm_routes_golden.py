"""Which kernels ops.mlp_gemm launches, pinned at one commit: tests/golden/gemm_routes_parent.json.

The shared-MLP GEMM family picks its kernel from the call: the matmul mode, the shape, the prologue, what the epilogue has
to add.  This fixture holds, for one call per route, what the library's launch log (usip_launch_log) reported at the commit
BEFORE the rejected forms of that family and their knobs were retired: every kernel name with its workgroup count, in
order (the weight split first, the GEMM last).  tests/test_f32x2_mode_gpu.py issues the same calls and compares.

Every row is the smallest shape that takes its route.  Where the library has a query for the decision the position count is
searched with it (usip_mlp_gemm_f32x3_used, usip_mlp_x3p_tile_rows, usip_mlp_narrow_forward_blocks, usip_mlp_gemm_tiles; the
fork and `red` rows assert theirs), so a threshold that moves changes the row's shape, which the fixture holds too, and the
test fails instead of following it.  The two streaming-kernel rows need 3072 / 2048 tiles of 64 positions -- more than any
other row, because usip_mlp_narrow_forward_blocks refuses fewer.

Inputs are not stored: they come from seeded generators, and the fixture holds a SHA-256 of them.

    python tests/golden/make_gemm_routes_golden.py      (on the GPU; regenerating it moves the pin: do that only on purpose)
"""
import functools
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PATH = os.path.join(HERE, "gemm_routes_parent.json")
DEV = "cuda:0"


def _lib():
    from usip_amd import _lib as L
    return L.lib()


def _smallest_p(step, ok):
    """The smallest multiple of `step` positions (one cloud) for which ok(P) holds."""
    P = step
    while not ok(P):
        P += step
        assert P <= 1 << 20, "no position count takes this route"
    return P


def rows():
    """-> [dict(name, mode, knob, nb, K, M, P, pro, stats, bias, rb, pool, a_trans, fork, red)], the table.
    rb / pool / fork: a group size or 0; red: None or the red_group; knob: the value of x2_direct."""
    lib = _lib()
    used = lambda M, K: (lambda P: bool(lib.usip_mlp_gemm_f32x3_used(M, K, P, 1)))                       # noqa: E731
    wide = lambda M, K: (lambda P: bool(lib.usip_mlp_gemm_f32x3_used(M, K, P, 1))                        # noqa: E731
                         and lib.usip_mlp_x3p_tile_rows(M, P, 1) == 256)
    narrow = lambda M: (lambda P: lib.usip_mlp_narrow_forward_blocks(M, 64, P, 1) > 0)                   # noqa: E731
    out = []

    def row(name, mode, nb, K, M, P, pro=1, stats=True, bias=True, rb=0, pool=0, a_trans=False, fork=0, red=None, knob=0):
        out.append(dict(name=name, mode=mode, knob=knob, nb=nb, K=K, M=M, P=P, pro=pro, stats=stats, bias=bias, rb=rb,
                        pool=pool, a_trans=a_trans, fork=fork, red=red))

    # fp32 MFMA tile kernel, its four geometries (shared_mlp.hip: 32 / 64 rows per workgroup at M <= 64, the 128-row
    # workgroup with one / two row tiles per wave below / from 512 tiles)
    row("f32 M32 few tiles", "f32", 1, 16, 32, 256, pro=0)
    row("f32 M64", "f32", 1, 16, 64, 256, pro=0)
    row("f32 M128 few tiles", "f32", 1, 16, 128, 128, pro=0)
    row("f32 M656 many tiles", "f32", 1, 16, 656, _smallest_p(128, lambda P: lib.usip_mlp_gemm_tiles(656, P, 1) * 6 >= 512), pro=0)
    row("bf16", "bf16", 1, 16, 128, 128, pro=0)
    # f32x3: the kernel that splits both operands itself (a transposed matrix operand, K beyond the split images' 640)
    row("f32x3 a_trans", "f32x3", 1, 128, 128, _smallest_p(128, used(128, 128)), pro=0, a_trans=True)
    row("f32x3 K656", "f32x3", 1, 656, 128, _smallest_p(128, used(128, 656)), pro=0)
    row("x3p 128-row tiles", "f32x3", 1, 128, 128, _smallest_p(128, used(128, 128)), pro=0)
    row("x3p 256-row tiles", "f32x3", 1, 128, 256, _smallest_p(128, wide(256, 128)), pro=0)
    row("x2h 128-row tiles", "f32x2", 1, 256, 128, _smallest_p(128, used(128, 256)))
    # gemm_x2f: whole 256 x 256 tiles, K % 64 == 0
    Pf = _smallest_p(256, wide(256, 128))
    row("x2f forward stats", "f32x2", 1, 128, 256, Pf)
    row("x2f forward", "f32x2", 1, 128, 256, Pf, stats=False)
    row("x2f forward row bias", "f32x2", 1, 128, 256, Pf, rb=16)
    row("x2f pro2", "f32x2", 1, 128, 256, Pf, pro=2, stats=False, bias=False)
    row("x2f pro3", "f32x2", 1, 128, 256, Pf, pro=3, stats=False, bias=False, pool=16)
    # gemm_x2d by input: what gemm_x2f refuses
    row("x2d K272", "f32x2", 1, 272, 256, _smallest_p(256, wide(256, 272)))
    row("x2d K tail", "f32x2", 1, 136, 256, _smallest_p(256, wide(256, 136)))
    row("x2d odd stage count", "f32x2", 1, 144, 256, _smallest_p(256, wide(256, 144)))
    row("x2d even stage count", "f32x2", 1, 160, 256, _smallest_p(256, wide(256, 160)))
    assert lib.usip_mlp_gemm_f32x3_used(300, 256, 8200, 2) and lib.usip_mlp_x3p_tile_rows(300, 8200, 2) == 256
    row("x2d general epilogue", "f32x2", 2, 256, 300, 8200)
    Pd = _smallest_p(256, wide(256, 160))
    row("x2d direct pro2", "f32x2", 1, 160, 256, Pd, pro=2, stats=False, bias=False)
    row("x2d direct pro3", "f32x2", 1, 160, 256, Pd, pro=3, stats=False, bias=False, pool=16)
    row("x2f fork", "f32x2", 1, 128, 256, Pf, pro=2, stats=False, bias=False, fork=16)
    row("x2d red", "f32x2", 1, 128, 256, Pf, pro=2, stats=False, bias=False, red=0)
    row("x2d red group 16", "f32x2", 1, 128, 256, Pf, pro=2, stats=False, bias=False, red=16)
    # gemm_x2r: M, K <= 128
    Pr = _smallest_p(128, used(128, 128))
    row("x2r forward", "f32x2", 1, 128, 128, Pr)
    row("x2r row bias", "f32x2", 1, 128, 128, Pr, rb=32)
    row("x2r pro2", "f32x2", 1, 128, 128, Pr, pro=2, stats=False, bias=False)
    row("x2r pro3", "f32x2", 1, 128, 128, Pr, pro=3, stats=False, bias=False, pool=16)
    row("x2r 64 -> 128", "f32x2", 1, 64, 128, 65536, rb=64)                  # (ops.mlp_gemm: nb * P >= 65536)
    row("narrow_fwd M64", "f32", 1, 64, 64, _smallest_p(64, narrow(64)))
    row("narrow_fwd M128", "f32", 1, 64, 128, _smallest_p(64, narrow(128)))
    # the references the tests obtain through knob x2_direct
    row("x2f forward stats, x2_direct 1", "f32x2", 1, 128, 256, Pf, knob=1)
    row("x2f forward stats, x2_direct 12", "f32x2", 1, 128, 256, Pf, knob=12)
    row("x2d direct pro2, x2_direct 8", "f32x2", 1, 160, 256, Pd, pro=2, stats=False, bias=False, knob=8)
    assert len({r["name"] for r in out}) == len(out)
    return out


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _randn(seed, *shape):
    import torch
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _arg(seed, group, *shape):
    import torch
    return torch.randint(0, group, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int32)


def host_inputs(r):
    """The seeded host tensors of a row, by role (shared between rows of one shape: the caches above)."""
    nb, K, M, P = r["nb"], r["K"], r["M"], r["P"]
    s = K * 1000003 + M * 10007 + nb * 101 + P
    t = dict(A=_randn(s, M, K) if r["a_trans"] else _randn(s, K, M), X=_randn(s + 1, nb, K, P), v=_randn(s + 2, 3, max(K, M)))
    if r["pro"] == 2:
        t["dZ"] = _randn(s + 3, nb, K, P)
    if r["pool"]:
        t["dp"], t["arg"] = _randn(s + 4, nb, K, P // r["pool"]), _arg(s + 5, r["pool"], nb, K, P // r["pool"])
    if r["rb"]:
        t["rb"] = _randn(s + 6, nb, M, P // r["rb"])
    if r["fork"]:
        t["fdp"], t["farg"] = _randn(s + 7, nb, M, P // r["fork"]), _arg(s + 8, r["fork"], nb, M, P // r["fork"])
    if r["red"] is not None:
        t["yprev"] = _randn(s + 9, nb, M, P)
    return t


def digest(table):
    h, seen = hashlib.sha256(), set()
    for r in table:
        for k, v in sorted(host_inputs(r).items()):
            if id(v) not in seen:                              # a tensor shared between rows counts once
                seen.add(id(v))
                h.update(("%s %s %s|" % (r["name"], k, tuple(v.shape))).encode())
                h.update(v.numpy().tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------ one call
def _bn_coef(y, gamma, beta, eps=1e-5):
    import torch
    mu, var = y.double().mean(dim=(0, 2)), y.double().var(dim=(0, 2), unbiased=False)
    istd = (1.0 / torch.sqrt(var + eps)).float()
    sc = gamma * istd
    return torch.stack([sc, beta - mu.float() * sc, mu.float(), istd]).contiguous()


def launches(r):
    """Issue the row's ops.mlp_gemm call once -> [[kernel name, workgroups], ...] as the launch log holds them."""
    import ctypes
    from usip_amd import ops
    lib = _lib()
    nb, K, M, P, pro = r["nb"], r["K"], r["M"], r["P"], r["pro"]
    h = {k: v.to(DEV) for k, v in host_inputs(r).items()}
    prev = ops.set_matmul_mode(r["mode"])
    try:
        A = h["A"] * (2.0 / K) ** 0.5
        X = h["X"] * 1.7 + 0.2
        gamma, beta = 1 + 0.3 * h["v"][0, :K].contiguous(), 0.3 * h["v"][1, :K].contiguous()
        kw = dict(pro=pro, want_stats=r["stats"], a_trans=r["a_trans"], tag="fwd" if pro < 2 else "dgrad")
        if r["bias"]:
            kw["bias"] = 0.1 * h["v"][2, :M].contiguous()
        if r["rb"]:
            kw.update(rowbias=h["rb"], rb_group=r["rb"])
        if pro >= 1:
            cf = _bn_coef(X, gamma, beta)
            ops.declare_samples(cf, nb * P)
            kw["coef"] = cf
        if pro == 2:                                           # X is the layer's pre-BN output, dZ its incoming gradient
            kw.update(X2=X, coef=ops.bn_backward_reduce(h["dZ"], X, cf, cf[2].contiguous(), cf[3].contiguous(), gamma, True)[2])
            X = h["dZ"]
        if pro == 3:
            G = r["pool"]
            kw.update(X2=X, pool=(h["dp"], h["arg"], G),
                      coef=ops.bn_pool_backward_reduce(h["dp"], h["arg"], X.view(nb, K, P // G, G), cf, cf[2].contiguous(),
                                                       cf[3].contiguous(), gamma, True)[2])
            X = None
        if r["fork"]:
            assert lib.usip_mlp_gemm_x2h_fork_supported(M, K, P, nb, r["fork"]) == 1, r["name"]
            kw["fork"] = (h["fdp"], h["farg"], r["fork"])
        if r["red"] is not None:
            assert lib.usip_mlp_gemm_x2d_red_tiles(M, K, P, nb, r["red"]) > 0, r["name"]
            yp = h["yprev"] * 1.5 - 0.2
            kw.update(red=(yp, _bn_coef(yp, 1 + 0.3 * h["v"][0, :M].contiguous(), 0.3 * h["v"][1, :M].contiguous())),
                      red_group=r["red"])
        lib.usip_set_tuning(b"x2_direct", r["knob"])
        lib.usip_launch_log(1)
        try:
            res = ops.mlp_gemm(A, X, **kw)
            got, wg = [], ctypes.c_uint(0)
            while (name := lib.usip_launch_log_entry(len(got), ctypes.byref(wg))) is not None:
                got.append([name.decode(), int(wg.value)])
        finally:
            lib.usip_launch_log(0)
            lib.usip_set_tuning(b"x2_direct", 0)
        if r["fork"]:
            assert res[2] is True, r["name"]
        if r["red"] is not None:
            assert res[2] is not None, r["name"]
        return got
    finally:
        ops.set_matmul_mode(prev)


def save(out):
    """One row per line."""
    with open(PATH, "w") as f:
        f.write('{"inputs_sha256": %s,\n "rows": {\n' % json.dumps(out["inputs_sha256"]))
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in out["rows"].items()))
        f.write("\n }}\n")


def main():
    import torch
    table = rows()
    out = dict(inputs_sha256=digest(table), rows={})
    for r in table:
        got = launches(r)
        torch.cuda.synchronize()
        out["rows"][r["name"]] = dict(call=r, launches=got)
        print(r["name"], "| nb %d K %d M %d P %d |" % (r["nb"], r["K"], r["M"], r["P"]),
              "; ".join("%s x%d" % (n.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0], w) for n, w in got))
    save(out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
