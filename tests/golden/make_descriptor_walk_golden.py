"""Bits of the baseline descriptors' host twins pinned at one commit: tests/golden/descriptor_walk_parent_bits.npz.

The device kernels are held to the host twins (tests/test_fpfh_gpu.py, tests/test_shot_gpu.py, tests/test_spin_gpu.py), but
twin and device share the *_math.h headers and could drift together.  This fixture holds what the twins computed at the commit
BEFORE the wave-per-keypoint walk (csrc/keypoint_walk.h) and the twins' keypoint loop (csrc/keypoints_host.h) became one each:
tests/test_fpfh_cpu.py, tests/test_shot_cpu.py and tests/test_spin_cpu.py hold today's twins to it bit for bit, the three GPU
files the device.

Inputs are not stored.  The clouds are make_baseline_walk_golden.py's (its `case`, imported, not copied): n1, n257, n515,
n515_constant_x (lo = 0 and hi = n for every keypoint in reach), n1030_r0.5 (narrow windows), n1030_r100 (the window is the
frame), c0, cneg, cover (clamped counts) and nonfinite; the keypoints come from the seeded generator below (inputs), and the
fixture holds a SHA-256 of cloud, counts, keypoints, keypoint counts and supplied axes, so a generator that has moved fails
the test instead of moving the expectation.  A case is a cloud with its entries; every entry has B = 2 frames at the cloud's own radius (also the normals'),
but n1030_r0.5 at 0.75: its second frame lies on a half-unit lattice, where d2 < 0.25 holds for coincident points alone and
no radius of 0.5 describes anything; at 0.75 a window is still 1.5 of the frame's 10 units.

  <cloud>_m<M>     M = 1, 3, 4, 5, 70 keypoints (1, 3 and 4 busy waves of a workgroup, a second workgroup with one wave, many
                   workgroups), kp_count = [M, M - M // 4].  Keypoint 0 sits beside the live point nearest the frame's centroid;
                   from M = 5 on it sits exactly ON that point, keypoint 1 has its x below the cloud by r / 2, keypoint 2 above
                   by r / 2, keypoint 3 by 10 r (an empty [lo, hi)); the others are live points moved by up to r / 4 and
                   positions uniform in the frame's box.  No keypoint is non-finite.
  n515_m5_kc0, _kcneg, _kcover   the same with kp_count = (0, M), (-2, M + 3), (M, 3)
  n515_m5_w63, _w64, _w65        the cloud thinned around keypoint 4 = (0, 0, 0): of the live rows with |x| < r the W nearest
                   the keypoint stay and the others move by 3 along x, out of the window, so that the keypoint's [lo, hi)
                   holds exactly 63, 64 and 65 rows in either frame -- asserted here by the twins' first_within semantics over a
                   numpy sort (window)
Per entry: fpfh_descriptors_cpu (desc, kp_members, fpfh; on the M = 70 entries also fpfh_spfh_cpu's spfh and members),
shot_descriptors_cpu (desc, kp_members, shot, hist, lrf, lrf_members), spin_descriptors_cpu in both structures without a
support angle (desc, kp_members, spin, hist, axes, lrf_members); on n257 and n515 also at support_angle_cos = 0.5 over estimated
normals, on n257 from M = 5 on also over supplied axes with a zero, a NaN and an inf row.

Not vacuous, checked by main(): in every frame that has a live point and a live keypoint (which leaves out n1's second frame,
the first of c0 and of cneg -- a count of -2 is a count of 0 --, and the kp_count <= 0 frames; n1 is left out whole: one point
has no member but itself) at least one keypoint has kp_members > 0 and a row that is not zero in all three descriptors, and
at least one keypoint has a SHOT frame.  main() prints the counts and exits non-zero otherwise.  No case had to be dropped for
any descriptor.

An output of a case is that output of its entries, flattened, one after the other.  Stored forms are
make_baseline_walk_golden.py's (stored: bit patterns, every NaN one pattern, more than 8 KiB as a SHA-256).

    python tests/golden/make_descriptor_walk_golden.py     (regenerating it moves the pin: do that only on purpose)
"""
import functools
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from make_baseline_walk_golden import bits, case, key, sha, stored  # noqa: E402,F401

PATH = os.path.join(HERE, "descriptor_walk_parent_bits.npz")
THREADS = 8
CLOUDS = ("n1", "n257", "n515", "n515_constant_x", "n1030_r0.5", "n1030_r100", "c0", "cneg", "cover", "nonfinite")
MS = (1, 3, 4, 5, 70)
KP_COUNTS = {"kc0": lambda M: (0, M), "kcneg": lambda M: (-2, M + 3), "kcover": lambda M: (M, 3)}
WINDOWS = (63, 64, 65)
ANGLED = ("n257", "n515")                                               # also support_angle_cos = 0.5
RADIUS = {"n1030_r0.5": 0.75}                                          # where the cloud's own radius describes nothing (docstring)
AXES = "n257"                                                           # also supplied axes, from M = 5 on
FAMILIES = ("fpfh", "shot", "spin")

# tag -> (cloud, M, variant)
ENTRIES = {"%s_m%d" % (c, m): (c, m, None) for c in CLOUDS for m in MS}
ENTRIES.update({"n515_m5_" + v: ("n515", 5, v) for v in KP_COUNTS})
ENTRIES.update({"n515_m5_w%d" % w: ("n515", 5, w) for w in WINDOWS})
CASES = {c: [t for t, e in ENTRIES.items() if e[0] == c] for c in CLOUDS}   # case -> its entries


def window(x, n, qx, r):
    """[lo, hi) of the keypoint at qx over the live rows sorted along x, as the twins search it: lo the first position with
    qx - x < r, hi the first from lo on with x - qx >= r"""
    xs = np.sort(x[:n].astype(np.float64), kind="stable")
    inside = np.flatnonzero(float(qx) - xs < r)
    lo = int(inside[0]) if len(inside) else n
    beyond = np.flatnonzero(xs[lo:] - float(qx) >= r)
    return lo, lo + int(beyond[0]) if len(beyond) else n


def _thinned(pc, count, r, rows):
    """pc with exactly `rows` live rows of either frame left in the window of the keypoint (0, 0, 0)"""
    pc = pc.copy()
    for b in range(2):
        n = int(np.clip(count[b], 0, pc.shape[2]))
        near = np.flatnonzero(np.abs(pc[b, 0, :n].astype(np.float64)) < r)
        d2 = (pc[b, :, near].astype(np.float64) ** 2).sum(1)
        away = near[np.argsort(d2, kind="stable")[rows:]]
        pc[b, 0, away] += np.where(pc[b, 0, away] < 0, np.float32(3.0), np.float32(-3.0))
        lo, hi = window(pc[b, 0], n, 0.0, r)
        assert hi - lo == rows, (b, lo, hi, rows)
    return pc


@functools.lru_cache(maxsize=None)
def inputs(tag):
    """-> (pc f32 [2,3,N], count i32 [2], keypoints f32 [2,3,M], kp_count i32 [2], radius, supplied axes f64 [2,M,3] or None);
    nobody writes into them"""
    cloud, M, variant = ENTRIES[tag]
    pc, count, _, r = case(cloud)
    r = RADIUS.get(cloud, r)
    if variant in WINDOWS:
        pc = _thinned(pc, count, r, variant)
    N = pc.shape[2]
    g = np.random.default_rng(zlib.crc32(tag.encode()))
    kp = np.zeros((2, 3, M), np.float32)
    for b in range(2):
        live = np.flatnonzero(np.isfinite(pc[b, :, :int(np.clip(count[b], 0, N))]).all(0))
        if len(live) == 0:
            continue
        p = pc[b][:, live].astype(np.float64)
        lo, hi = p.min(1), p.max(1)
        centre = p[:, np.argmin(((p - p.mean(1, keepdims=True)) ** 2).sum(0))]
        moved = p[:, g.integers(0, len(live), M)] + g.uniform(-r / 4, r / 4, (3, M))
        free = g.uniform(lo[:, None], hi[:, None], (3, M))
        kp[b] = np.where(np.arange(M) % 2 == 0, moved, free)
        kp[b, :, 0] = centre + (0.0 if M >= 5 else r / 16)
        if M >= 5:
            kp[b, 0, 1:4] = [lo[0] - r / 2, hi[0] + r / 2, hi[0] + 10 * r]
        if variant in WINDOWS:
            kp[b, :, 4] = 0.0
    kc = KP_COUNTS[variant](M) if variant in KP_COUNTS else ((M, M) if variant in WINDOWS else (M, M - M // 4))
    axes = None
    if cloud == AXES and variant is None and M >= 5:
        axes = g.normal(size=(2, M, 3)) * 3.0                           # (not of unit length)
        axes[:, 1], axes[:, 2, 1], axes[:, 3, 2] = 0.0, np.nan, np.inf
    out = (pc, np.array(count, np.int32), kp, np.array(kc, np.int32), r, axes)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def digest(name):
    """SHA-256 of every input of case `name`"""
    arrays = []
    for tag in CASES[name]:
        pc, count, kp, kc, _, axes = inputs(tag)
        arrays += [pc, count, kp, kc] + ([] if axes is None else [axes])
    return sha(arrays)


# ------------------------------------------------------------------------------------------------ the three descriptors, per entry
def _backend(dev, num_threads):
    """-> (call(name, ...) of usip_amd.baselines on the host twins or on `dev`, array -> its argument, result -> array)"""
    from usip_amd import baselines as bl
    if dev is None:
        return (lambda name, *a, **k: getattr(bl, name + "_cpu")(*a, num_threads=num_threads, **k)), (lambda a: a), (lambda a: a)
    import torch
    return (lambda name, *a, **k: getattr(bl, name)(*a, **k)), \
        (lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)), \
        (lambda t: None if t is None else t.cpu().numpy())              # (np.array: a copy, the inputs are read-only)


SPIN_FIELDS = ("desc", "kp_members", "spin", "hist", "axes", "lrf_members")


def raw(tag, family, dev=None, num_threads=THREADS):
    """{field: array} of one descriptor on one entry, from the host twins (dev None) or the device"""
    call, to, back = _backend(dev, num_threads)
    cloud, M, variant = ENTRIES[tag]
    pc, count, kp, kc, r, axes = inputs(tag)
    p, c, k, n = to(pc), to(count), to(kp), to(kc)
    got = {}
    if family == "fpfh":
        out = call("fpfh_descriptors", p, k, c, n, radius=r, normal_radius=r, want_f64=True)
        got.update(zip(("fpfh_desc", "fpfh_kp_members", "fpfh_fpfh"), out))
        if M == 70:
            got.update(zip(("fpfh_spfh", "fpfh_members"), call("fpfh_spfh", p, c, radius=r, normal_radius=r)[:2]))
    elif family == "shot":
        out = call("shot_descriptors", p, k, c, n, radius=r, normal_radius=r, want_f64=True)
        got.update(zip(("shot_desc", "shot_kp_members", "shot_shot", "shot_hist", "shot_lrf", "shot_lrf_members"), out))
    else:
        runs = [("rect", dict(structure="rectangular")), ("rad", dict(structure="radial"))]
        if cloud in ANGLED:
            runs.append(("angle", dict(support_angle_cos=0.5, normal_radius=r)))
        if axes is not None:
            runs.append(("axes", dict(axes=to(axes))))
        for name, kw in runs:
            out = call("spin_descriptors", p, k, c, n, radius=r, want_f64=True, **kw)
            got.update({"spin_%s_%s" % (name, f): v for f, v in zip(SPIN_FIELDS, out) if v is not None})
    return {f: back(v) for f, v in got.items()}


def outputs(name, family, dev=None, num_threads=THREADS):
    """{field: stored form} of one descriptor on case `name`: an output of the case is that of its entries, one after the
    other in ENTRIES' order"""
    parts = {}
    for tag in CASES[name]:
        for f, v in raw(tag, family, dev, num_threads).items():
            parts.setdefault(f, []).append(bits(v).reshape(-1))
    return {f: stored(np.concatenate(v)) for f, v in parts.items()}


def host(name, family, num_threads=THREADS):
    return outputs(name, family, None, num_threads)


def device(name, family, dev="cuda:0"):
    return outputs(name, family, dev)


# ------------------------------------------------------------------------------------------------ the fixture
_PINNED = {}


def check(family, name, got, what):
    """Every stored output of `family` on case `name` against got {field: stored form}, bit for bit; the inputs' digest first
    (nothing is skipped when the generator moves)."""
    if not _PINNED:
        _PINNED.update(np.load(PATH))
    assert bytes(_PINNED[key(name, "sha256")]) == bytes(digest(name)), "the generator no longer gives the fixture's inputs: " + name
    head = key(name, family + "_")
    want = {k[len(key(name, "")):]: v for k, v in _PINNED.items() if k.startswith(head)}
    assert want and set(want) == set(got), (name, sorted(want), sorted(got))
    differ = {k: int((got[k] != e).sum()) if got[k].shape == e.shape else -1 for k, e in want.items()}
    print("%s, %s: entries that differ from the pinned bits %s" % (what, name, differ))
    for k, e in want.items():
        assert got[k].dtype == e.dtype and got[k].shape == e.shape, (name, k, got[k].dtype, e.dtype, got[k].shape, e.shape)
        assert np.array_equal(got[k], e), (what, name, k, differ[k])


def described(tag, got):
    """per frame: (keypoints with members and a non-zero row in all three descriptors, keypoints with a SHOT frame), or None
    for a frame that has no live point or no live keypoint"""
    pc, count, kp, kc, _, _ = inputs(tag)
    out = []
    for b in range(2):
        if min(int(count[b]), int(kc[b])) <= 0:
            out.append(None)
            continue
        full = np.ones(kp.shape[2], bool)
        for members, rows in (("fpfh_kp_members", "fpfh_fpfh"), ("shot_kp_members", "shot_shot"),
                              ("spin_rect_kp_members", "spin_rect_spin"), ("spin_rad_kp_members", "spin_rad_spin")):
            full &= (got[members][b] > 0) & (got[rows][b] != 0).any(1)
        out.append((int(full.sum()), int((got["shot_lrf"][b] != 0).any(1).sum())))
    return out


def main():
    out, vacuous = {}, []
    for tag in ENTRIES:
        got = {}
        for family in FAMILIES:
            got.update(raw(tag, family))
        counts = described(tag, got)
        print("%-24s keypoints described by all three, with a SHOT frame, per frame: %s" % (tag, counts))
        if ENTRIES[tag][0] != "n1" and any(c is not None and min(c) < 1 for c in counts):
            vacuous.append(tag)
    if vacuous:
        raise SystemExit("vacuous: no keypoint of a live frame is described by all three descriptors in %s" % vacuous)
    for name in CASES:
        out[key(name, "sha256")] = digest(name)
        for family in FAMILIES:
            out.update({key(name, f): v for f, v in host(name, family).items()})
    np.savez_compressed(PATH, **out)
    size = os.path.getsize(PATH)
    print("wrote", PATH, "%.0f KB, %d arrays" % (size / 1024, len(out)))
    if size >= os.path.getsize(os.path.join(HERE, "tile_walk_parent_bits.npz")):
        raise SystemExit("the fixture is not smaller than tile_walk_parent_bits.npz")


if __name__ == "__main__":
    main()
