"""Bits of the baseline detectors' host twins pinned at one commit: tests/golden/baseline_walk_parent_bits.npz.

The device kernels are held to the host twins (tests/test_iss_gpu.py, tests/test_harris_gpu.py, tests/test_sift_gpu.py), but
twin and device share the *_math.h headers and could drift together.  This fixture holds what the twins computed at the commit
BEFORE the ascending walk's body (csrc/ascending_walk.h) and the twins' frame loop (csrc/frames_host.h) became one each:
tests/test_iss_cpu.py, tests/test_harris_cpu.py and tests/test_sift_cpu.py hold today's twins to it bit for bit, the three GPU
files the device.

Inputs are not stored: they come from the seeded generator below (case), and the fixture holds a SHA-256 of them, so a
generator that has moved fails the test instead of moving the expectation.  Every case has B = 2 frames; frame 0 is live to
its end, frame 1 has a count of its own.

  n1 .. n515        N = 1, 255, 256, 257, 515 (the tile boundary, a partial last tile, three tiles): coordinates uniform in
                    [-3, 3], frame 1 on a half-unit lattice (exact ties in x and in distance), count = [N, N - 3]
  n515_constant_x   the same at one x: a run of equal x longer than two tiles, the walk's search and break never fire
  n1030_r0.5, n1030_r100   x uniform in [0, 10], y and z in [-0.5, 0.5]: five tiles; at radius 0.5 a middle workgroup skips
                    tiles on both sides, at 100 every tile is walked
  c0, cneg, cover   257 points with count[0] = 0 (an all-dead frame beside a live one), -2 and N + 3: all clamped
  nonfinite         257 points, a NaN y in one live row and a +inf z in another of either frame (x stays finite: where a NaN
                    sorts along x is no part of any contract)
  m24, m25, m26     64 slots with 24 / 25 / 26 live rows in frame 1: below, at and above the SIFT stages' MIN_POINTS
Per case: iss_keypoints_cpu (mask, saliency, neighbours) and harris_keypoints_cpu (mask, response, members, normals; "harris"
everywhere, "noble", "lowe" and "tomasi" on n257) at the case's radius; sift_nearest_cpu, and sift_dog_cpu + sift_extrema_cpu
at S = 4 over the z axis (on n257 and m24 .. m26 also at S = 11 over a supplied field) with the scales chosen so that the
walk's radius is about the case's; sift_keypoints_cpu's four results on n515.  On n1030_r0.5 also tiles_visited of the three
kernels that report it, from the closed form (the twins do not walk tiles): workgroup w visits the tiles from the first whose
largest x is within r of its smallest query x to the last whose smallest x is within r of its largest.

Float outputs are stored as their bit patterns with every NaN as one pattern (which NaN an invalid operation gives is the
machine's, not the contract's), integers as they are.  An array of more than FULL bytes is stored as the SHA-256 of that form:
equal digests are equal bits, and the file stays below tile_walk_parent_bits.npz.

    python tests/golden/make_baseline_walk_golden.py       (regenerating it moves the pin: do that only on purpose)
"""
import functools
import hashlib
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PATH = os.path.join(HERE, "baseline_walk_parent_bits.npz")
FULL = 8192                                                             # bytes up to which an output is stored entry by entry
TILE = 256
MIN_POINTS = 25
THREADS = 8
MIN_CONTRAST = 0.01
HARRIS_EXTRA = ("noble", "lowe", "tomasi")                              # on n257, beside "harris"
SIFT_FLAT = dict(min_scale=0.5, n_octaves=2, n_scales_per_octave=3, min_contrast=0.02, field="z")   # sift_keypoints on n515
VISITS = "n1030_r0.5"

# name -> (N, kind, radius, count)
CASES = {}
for _n in (1, 255, 256, 257, 515):
    CASES["n%d" % _n] = (_n, "uniform", 1.5, (_n, _n - 3))
CASES["n515_constant_x"] = (515, "constant_x", 1.5, (515, 512))
CASES["n1030_r0.5"] = (1030, "slab", 0.5, (1030, 1027))
CASES["n1030_r100"] = (1030, "slab", 100.0, (1030, 1027))
CASES["c0"] = (257, "uniform", 1.5, (0, 257))
CASES["cneg"] = (257, "uniform", 1.5, (-2, 257))
CASES["cover"] = (257, "uniform", 1.5, (260, 254))
CASES["nonfinite"] = (257, "nonfinite", 1.5, (257, 254))
for _m in (24, 25, 26):
    CASES["m%d" % _m] = (64, "uniform", 3.0, (64, _m))
WIDE = ("n257", "m24", "m25", "m26")                                    # also S = 11 over a supplied field


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (pc f32 [2,3,N], count i32 [2], supplied field f32 [2,N], radius); nobody writes into them"""
    N, kind, radius, count = CASES[name]
    g = np.random.default_rng(zlib.crc32(name.encode()))
    pc = g.uniform(-3.0, 3.0, (2, 3, N)).astype(np.float32)
    if kind == "slab":
        pc[:, 0] = g.uniform(0.0, 10.0, (2, N)).astype(np.float32)
        pc[:, 1:] = g.uniform(-0.5, 0.5, (2, 2, N)).astype(np.float32)
    pc[1] = np.round(pc[1] * 2) / 2
    if kind == "constant_x":
        pc[:, 0] = np.float32(1.25)
    if kind == "nonfinite":
        for b in range(2):
            pc[b, 1, 5 + b], pc[b, 2, 140 + b] = np.nan, np.inf
    field = g.normal(size=(2, N)).astype(np.float32)
    for a in (pc, field):
        a.setflags(write=False)
    return pc, np.array(count, np.int32), field, radius


def sift_variants(name):
    """-> [(tag, sigma2 f64 [S], field f32 [2,N])]: the scales put the walk's radius (3 sigma_{S-1}) near the case's"""
    from usip_amd import baselines as bl
    pc, _, field, radius = case(name)
    out = [("s4", bl.sift_sigma2(radius / 12.0, 1), np.ascontiguousarray(pc[:, 2]))]
    if name in WIDE:
        out.append(("s11", bl.sift_sigma2(radius / 6.0, 8), field))
    return out


def bits(a):
    """A float output as its bit patterns, every NaN as one; everything else as it is."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return np.where(np.isnan(a), u({4: 0x7FC00000, 8: 0x7FF8000000000000}[a.dtype.itemsize]), a.view(u))


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def stored(a):
    """An output as the fixture holds it."""
    b = bits(a)
    return b if b.nbytes <= FULL else sha([np.array(b.shape, np.int64), b])


def tiles_expected(name, r, least=0):
    """tiles_visited i32 [2, tiles of N] of a walk at radius r from the closed form; a frame of fewer than `least` live
    points walks nothing."""
    pc, count, _, _ = case(name)
    N = pc.shape[2]
    out = np.zeros((2, (N + TILE - 1) // TILE), np.int32)
    for b in range(2):
        n = int(np.clip(count[b], 0, N))
        if n == 0 or n < least:
            continue
        xs = np.sort(pc[b, 0, :n].astype(np.float64), kind="stable")
        T = (n + TILE - 1) // TILE
        lo, hi = xs[np.arange(T) * TILE], xs[np.minimum(np.arange(T) * TILE + TILE - 1, n - 1)]
        out[b, :T] = [((lo[w] - hi < r) & (lo - hi[w] < r)).sum() for w in range(T)]
    return out


# ------------------------------------------------------------------------------------------------ the three detectors, per case
def _harris_methods(name):
    return ("harris",) + (HARRIS_EXTRA if name == "n257" else ())


def iss_host(name, num_threads=THREADS):
    from usip_amd import baselines as bl
    pc, count, _, r = case(name)
    out = bl.iss_keypoints_cpu(pc, count, salient_radius=r, non_max_radius=r, num_threads=num_threads)
    return {"iss_" + k: stored(v) for k, v in zip(("mask", "saliency", "neighbours"), out)}


def harris_host(name, num_threads=THREADS):
    from usip_amd import baselines as bl
    pc, count, _, r = case(name)
    got = {}
    for method in _harris_methods(name):
        out = bl.harris_keypoints_cpu(pc, count, radius=r, response=method, num_threads=num_threads)
        got.update({"%s_%s" % (method, k): stored(v) for k, v in zip(("mask", "response", "members", "normals"), out)})
    return got


def sift_host(name, num_threads=THREADS):
    from usip_amd import baselines as bl
    pc, count, _, _ = case(name)
    idx = bl.sift_nearest_cpu(pc, count, num_threads)
    got = {"sift_idx": stored(idx)}
    for tag, sigma2, field in sift_variants(name):
        dog = bl.sift_dog_cpu(pc, field, count, sigma2, num_threads)
        mask, scale = bl.sift_extrema_cpu(dog, idx, count, MIN_CONTRAST, num_threads)
        got.update({tag + "_dog": stored(dog), tag + "_mask": stored(mask), tag + "_scale_index": stored(scale)})
    if name == "n515":
        out = bl.sift_keypoints_cpu(pc, count, num_threads=num_threads, **SIFT_FLAT)
        got.update({"flat_" + k: stored(v) for k, v in zip(("candidates", "mask", "scale", "octave_count"), out)})
    return got


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.array(a)).to(dev)                        # (a copy: the cases are read-only)


def iss_device(name, dev="cuda:0"):
    from usip_amd import baselines as bl
    pc, count, _, r = case(name)
    p, c = _dev(pc, dev), _dev(count, dev)
    out = bl.iss_keypoints(p, c, salient_radius=r, non_max_radius=r)
    got = {"iss_" + k: stored(v.cpu().numpy()) for k, v in zip(("mask", "saliency", "neighbours"), out)}
    if name == VISITS:
        got["visits_radius"] = bl.iss_saliency(p, c, salient_radius=r, want_visits=True)[2].cpu().numpy()
    return got


def harris_device(name, dev="cuda:0"):
    from usip_amd import baselines as bl
    pc, count, _, r = case(name)
    p, c = _dev(pc, dev), _dev(count, dev)
    got = {}
    for method in _harris_methods(name):
        out = bl.harris_keypoints(p, c, radius=r, response=method)
        got.update({"%s_%s" % (method, k): stored(v.cpu().numpy())
                    for k, v in zip(("mask", "response", "members", "normals"), out)})
    if name == VISITS:
        got["visits_radius"] = bl.harris_response(p, c, radius=r, want_visits=True)[3].cpu().numpy()
    return got


def sift_device(name, dev="cuda:0"):
    from usip_amd import baselines as bl
    from usip_amd import ops
    pc, count, _, _ = case(name)
    p, c = _dev(pc, dev), _dev(count, dev)
    perm = bl.sort_along_x(p, c)
    idx = ops.sift_nearest(p, c, perm)
    got = {"sift_idx": stored(idx.cpu().numpy())}
    for tag, sigma2, field in sift_variants(name):
        dog, visits = ops.sift_dog(p, _dev(field, dev), c, perm, sigma2, want_visits=True)
        mask, scale = ops.sift_extrema(dog, idx, c, MIN_CONTRAST)
        got.update({tag + "_dog": stored(dog.cpu().numpy()), tag + "_mask": stored(mask.cpu().numpy()),
                    tag + "_scale_index": stored(scale.cpu().numpy())})
        if name == VISITS:
            got["visits_sift"] = visits.cpu().numpy()
    if name == "n515":
        out = bl.sift_keypoints(p, c, **SIFT_FLAT)
        got.update({"flat_" + k: stored(v.cpu().numpy()) for k, v in zip(("candidates", "mask", "scale", "octave_count"), out)})
    return got


FAMILIES = {"iss": ("iss_", "visits_radius"), "harris": ("harris_",) + tuple(m + "_" for m in HARRIS_EXTRA) + ("visits_radius",),
            "sift": ("sift_", "s4_", "s11_", "flat_", "visits_sift")}


# ------------------------------------------------------------------------------------------------ the fixture
def key(name, field):
    return "%s__%s" % (name, field)


_PINNED = {}


def check(family, name, got, what):
    """Every stored output of `family` ("iss", "harris", "sift") on case `name` against got {field: stored form}, bit for bit;
    the inputs' digest first (nothing is skipped when the generator moves).  The twins report no visits: a got without them is
    held to everything else."""
    if not _PINNED:
        _PINNED.update(np.load(PATH))
    digest = key(name, "sha256")
    assert bytes(_PINNED[digest]) == bytes(sha(case(name)[:3])), "the generator no longer gives the fixture's inputs: " + name
    want = {k[len(key(name, "")):]: v for k, v in _PINNED.items() if k.startswith(key(name, "")) and k != digest}
    want = {k: v for k, v in want.items() if k.startswith(FAMILIES[family])}
    if not any(k.startswith("visits_") for k in got):
        want = {k: v for k, v in want.items() if not k.startswith("visits_")}
    assert want and set(want) == set(got), (name, sorted(want), sorted(got))
    differ = {k: int((got[k] != e).sum()) if got[k].shape == e.shape else -1 for k, e in want.items()}
    print("%s, %s: entries that differ from the pinned bits %s" % (what, name, differ))
    for k, e in want.items():
        assert got[k].dtype == e.dtype and got[k].shape == e.shape, (name, k, got[k].dtype, e.dtype, got[k].shape, e.shape)
        assert np.array_equal(got[k], e), (what, name, k, differ[k])


def main():
    from usip_amd import baselines as bl
    out = {}
    for name in CASES:
        pc, count, field, r = case(name)
        out[key(name, "sha256")] = sha([pc, count, field])
        got = dict(iss_host(name), **harris_host(name), **sift_host(name))
        if name == VISITS:
            got["visits_radius"] = tiles_expected(name, r)
            got["visits_sift"] = tiles_expected(name, bl.sift_walk_radius(sift_variants(name)[0][1]), MIN_POINTS)
            print("  tiles visited at r = %g: %s" % (r, got["visits_radius"].tolist()))
        full = bl.iss_keypoints_cpu(pc, count, salient_radius=r, non_max_radius=r, num_threads=THREADS)
        hk = bl.harris_keypoints_cpu(pc, count, radius=r, num_threads=THREADS)
        print("%-16s iss keypoints %s salient %s; harris keypoints %s with a normal %s; sift s4 keypoints %s" % (
            name, full[0].sum(1).tolist(), (full[1] > 0).sum(1).tolist(), hk[0].sum(1).tolist(),
            (hk[2] > 0).sum(1).tolist(),
            bl.sift_extrema_cpu(bl.sift_dog_cpu(pc, sift_variants(name)[0][2], count, sift_variants(name)[0][1], THREADS),
                                bl.sift_nearest_cpu(pc, count, THREADS), count, MIN_CONTRAST, THREADS)[0].sum(1).tolist()))
        for k, v in got.items():
            out[key(name, k)] = v
    np.savez_compressed(PATH, **out)
    size = os.path.getsize(PATH)
    print("wrote", PATH, "%.0f KB, %d arrays" % (size / 1024, len(out)))
    if size > os.path.getsize(os.path.join(HERE, "tile_walk_parent_bits.npz")):
        raise SystemExit("the fixture is larger than tile_walk_parent_bits.npz")


if __name__ == "__main__":
    main()
