"""Fixtures of the indoor descriptor pair builder: tests/golden/indoor_pairs_cases.npz.

Runs the reference's OWN SceneNNDescriptorLoader (__getitem__, augment, augment_rot_only, get_instance_unaugmented_np,
data/scenenn_descriptor_loader.py:101-289) with its FarthestSampler, cart2hom, hom2cart, and atomic_rotate /
transform_pc_pytorch (data/augmentation.py), compiled out of the reference checkout with ast (the module imports
torchvision / h5py / matplotlib, absent here).  np.load and the pickle are answered from this script's own arrays, and
every np.random draw and argmax by a recorder, so the draws go into the fixture next to what the reference computed:

  choice(n, k, replace=False)   a permuted prefix, as numpy's
  randint / uniform / rand      uniform(low, high) = low + (high - low) * u, numpy's own formula; u is recorded
  randn                         standard normals (the jitter blocks are drawn, never added, and not stored)
  argmax                        recorded too: FarthestSampler's picks, i.e. the FPS indices

FPS condition.  The reference samples in float64, the builder on float32 candidates (the anchor's: the float32 roundings
of the moved points).  For every FPS round of every cloud the generator measures the relative gap between the largest
running distance and the largest value different from it (duplicated rows of a short frame tie exactly; the lowest index
wins on both sides).  A case whose smallest gap is below 1e-4 -- a thousand float32 roundings -- is REFUSED, not skipped:
change its seed until the reference alone satisfies the condition.  The smallest gap is stored (fps_min_gap).

The host twin is then run under the recorded draws, and the share of anchor values (anc_pc, anc_node, anc_sn[0:3]) that are
not bit-equal to the reference's is stored (anchor_unequal_share): np.dot sums the four-term ICP product in BLAS's order.

    python tests/golden/make_indoor_pairs_golden.py        (needs the reference checkout and the built library)
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from usip_amd import synth  # noqa: E402

REF = "/root/reference"
N, M, ROW_LEN = 1024, 32, 7
FRAME_ROWS = (1180, 1100, 700, 300)      # 700: one whole copy + a draw of 324; 300: three copies + 124
PAIRS = ((0, 1), (1, 0), (2, 0), (1, 3), (3, 2))     # sample 2: a short anchor; 3: a short positive; 4: both short
MIN_GAP = 1e-4
# name: (mode, Cs, rot_horizontal, rot_3d, rot_perturbation, translation_perturbation, samples, recorder seed)
CASES = {
    "c4_train_2dp_short": ("train", 4, 1, 0, 1, 0, [2, 3], 400),     # the reference's setting, on the short frames
    "c4_train_norot_shift": ("train", 4, 0, 0, 0, 1, [1], 401),      # the positive's f32-array path beside the anchor's f64
    "c3_train_3d": ("train", 3, 0, 1, 0, 0, [0], 402),
    "c4_val_p2": ("val", 4, 1, 0, 1, 0, [0, 1], 403),                # P = 2 with both frame orders
    "c4_test": ("test", 4, 1, 0, 1, 0, [4], 404),
}
KEYS = ("anc_pc", "anc_sn", "anc_node", "pos_pc", "pos_sn", "pos_node", "anc_R_pos", "anc_scale_pos", "anc_shift_pos")


def rigid(rng):
    """A general rigid pose: a few tenths of a radian about every axis and about a metre."""
    ax, ay, az = rng.uniform(-0.4, 0.4, 3)
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    T = np.eye(4)
    T[:3, :3] = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
                 @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    T[:3, 3] = rng.uniform(-1.0, 1.0, 3)
    return T


class Recorder:
    def __init__(self, seed):
        self.g = np.random.default_rng(seed)
        self.log = []

    def choice(self, a, size, replace=True):
        assert not replace
        r = self.g.permutation(int(a))[:size]
        self.log.append(("choice", r.copy()))
        return r

    def randint(self, n):
        v = int(self.g.integers(0, n))
        self.log.append(("randint", v))
        return v

    def uniform(self, low=0.0, high=1.0, size=None):
        u = self.g.random(size)
        self.log.append(("uniform", np.atleast_1d(u).ravel().copy()))
        v = low + (high - low) * u
        return float(v) if size is None else v

    def rand(self, *shape):
        u = self.g.random(shape)
        self.log.append(("uniform", u.ravel().copy()))
        return u

    def randn(self, *shape):
        z = self.g.standard_normal(shape).astype(np.float32).astype(np.float64)
        self.log.append(("randn", z.copy() if z.size <= 3 else None))
        return float(z) if shape == () else z


def make_np(frames, rec):
    """numpy, with load and random answered by this script and argmax recorded."""
    proxy = types.ModuleType("np_proxy")
    proxy.__dict__.update({k: getattr(np, k) for k in dir(np) if not k.startswith("__")})

    def load(path, *a, **kw):
        return frames[int(os.path.basename(path).split(".")[0])].copy()

    def argmax(x, *a, **kw):
        i = int(np.argmax(x, *a, **kw))
        rec.log.append(("argmax", i))
        return i
    proxy.load, proxy.random, proxy.argmax = load, rec, argmax
    return proxy


def extract(ns, path, names):
    tree = ast.parse(open(path).read())
    nodes = [n for n in tree.body if getattr(n, "name", None) in names]
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)


def reference(np_proxy):
    ns = {"np": np_proxy, "torch": torch, "os": os, "math": __import__("math"),
          "data": types.SimpleNamespace(Dataset=object)}
    extract(ns, os.path.join(REF, "data", "augmentation.py"),
            {"angles2rotation_matrix", "atomic_rotate", "transform_pc_pytorch"})
    extract(ns, os.path.join(REF, "data", "scenenn_descriptor_loader.py"),
            {"FarthestSampler", "cart2hom", "hom2cart", "SceneNNDescriptorLoader"})
    return ns


def loader(ns, opt, mode, pairs, icp):
    ld = ns["SceneNNDescriptorLoader"].__new__(ns["SceneNNDescriptorLoader"])
    ld.root, ld.opt, ld.mode, ld.farthest_sampler = "r", opt, mode, ns["FarthestSampler"]()
    ld.frame_folder, ld.pairs_np, ld.icp_np = "frames", pairs, icp
    return ld


def parse_item(log, lens, mode, opt):
    """One __getitem__'s draws in the layouts of include/usip_hip.h (usip_pairs_draws), for one pair; and the FPS picks."""
    pos = [0]

    def take(what):
        k, v = log[pos[0]]
        assert k == what, (pos[0], k, what)
        pos[0] += 1
        return v

    def choice_rows(n):
        if n >= N:
            return take("choice")
        fix = np.arange(n)
        while n + fix.shape[0] < N:
            fix = np.concatenate((fix, np.arange(n)))
        return np.concatenate((fix, take("choice")))
    rows = [choice_rows(lens[0]), choice_rows(lens[1])]
    cand, first, fps = [None, None], [0, 0], [None, None]
    for c in range(2):
        cand[c] = take("choice")
        first[c] = take("randint")
        fps[c] = [first[c]] + [take("argmax") for _ in range(M - 1)]
    params = np.zeros(24)
    if mode in ("train", "val"):
        params[0] = take("uniform")[0]
        params[1:4] = take("uniform")
        params[4:7] = take("randn")
    if mode == "train":
        take("randn"), take("randn"), take("randn")            # the three jitter blocks: drawn, never added
        params[7] = take("uniform")[0]
        params[8:11] = take("uniform")
    if opt.rot_3d:
        params[12:15] = [take("uniform")[0] for _ in range(3)]
    elif opt.rot_horizontal:
        params[12] = take("uniform")[0]
    if opt.rot_perturbation:
        params[15:18] = [float(take("randn")) for _ in range(3)]
    params[18] = take("uniform")[0]
    params[19:22] = take("uniform")
    assert pos[0] == len(log), (pos[0], len(log))
    d = dict(rows=np.stack(rows).astype(np.int32), cand=np.stack(cand).astype(np.int32),
             first=np.asarray(first, dtype=np.int32), params=params)
    return d, np.asarray(fps)


def fps_gap(pts, picks):
    """Smallest relative gap, over the rounds, between the largest running distance and the largest value below it."""
    pts = np.asarray(pts, dtype=np.float64)
    dist = ((pts[picks[0]] - pts) ** 2).sum(axis=1)
    worst = np.inf
    for i in range(1, len(picks)):
        top = dist.max()
        assert dist[picks[i]] == top and picks[i] == int(np.argmax(dist))
        below = dist[dist != top]
        if below.size:
            worst = min(worst, (top - below.max()) / top)
        dist = np.minimum(dist, ((pts[picks[i]] - pts) ** 2).sum(axis=1))
    return worst


def main():
    from usip_amd import indoor_pairs
    rng = np.random.default_rng(2026)
    frames = []
    for n in FRAME_ROWS:
        pc = synth.make_cloud(rng, n, "slab:3").T
        sn = synth.make_normals(rng, n, 4).T
        frames.append(np.concatenate([pc, sn], 1).astype(np.float32))
    pairs = np.asarray(PAIRS, dtype=np.int64)
    icp = np.stack([rigid(rng) for _ in PAIRS])
    out = {"frame_%d" % i: f for i, f in enumerate(frames)}
    out.update(pairs=pairs.astype(np.int32), icp=icp, N=np.int32(N), M=np.int32(M))
    min_gap, unequal, total = np.inf, 0, 0
    for name, (mode, Cs, rh, r3, pert, transl, samples, seed) in CASES.items():
        opt = types.SimpleNamespace(input_pc_num=N, node_num=M, surface_normal_len=Cs, rot_horizontal=bool(rh),
                                    rot_3d=bool(r3), rot_perturbation=bool(pert), translation_perturbation=bool(transl))
        rec = Recorder(seed)
        ld = loader(reference(make_np(frames, rec)), opt, mode, pairs, icp)
        items, draws, slots = [], [], []
        for s in samples:
            rec.log = []
            items.append(ld.__getitem__(s))
            d, fps = parse_item(rec.log, [len(frames[f]) for f in pairs[s]], mode, opt)
            # the candidates the reference sampled from, recomputed here: the anchor's moved points in float64
            anc = frames[pairs[s, 0]][d["rows"][0], 0:3]
            anc = (np.dot(icp[s], np.hstack((anc, np.ones((N, 1)))).T)).T[:, 0:3]
            clouds = (anc, frames[pairs[s, 1]][d["rows"][1], 0:3])
            gap = min(fps_gap(clouds[c][d["cand"][c]], fps[c]) for c in range(2))
            print("%s sample %d: smallest FPS gap %.3e" % (name, s, gap))
            if gap < MIN_GAP:
                raise SystemExit("%s sample %d: an FPS round is decided by a relative gap of %.3e < %.0e: change the "
                                 "case's seed" % (name, s, gap, MIN_GAP))
            min_gap = min(min_gap, gap)
            draws.append(d)
            slots.append(np.stack([d["cand"][c][fps[c]] for c in range(2)]).astype(np.int32))
        for ki, k in enumerate(KEYS):
            v = [np.asarray(it[ki].numpy() if torch.is_tensor(it[ki]) else it[ki], dtype=np.float32) for it in items]
            out["%s_%s" % (name, k)] = np.stack(v).reshape((len(items),) + {"anc_scale_pos": (1,)}.get(k, v[0].shape))
        for k in draws[0]:
            v = np.stack([d[k] for d in draws])
            out["%s_draw_%s" % (name, k)] = v.astype(np.int16) if k in ("rows", "cand") else v
        out["%s_node_slots" % name] = np.stack(slots, 1)                                            # [2][P][M]
        out["%s_ids" % name] = np.array(samples, dtype=np.int32)
        out["%s_case" % name] = np.array([indoor_pairs.MODES[mode], Cs, rh, r3, pert, transl], dtype=np.int32)
        # the host twin under the same draws: how many anchor values differ in their last bit
        recipe = indoor_pairs.IndoorPairRecipe(N=N, M=M, Cs=Cs, n_sub=N // 2, rot_horizontal=rh, rot_3d=r3,
                                               rot_perturbation=pert, translation_perturbation=transl)
        got, _, _ = indoor_pairs.build_cpu(recipe, frames, pairs, icp, samples, len(samples), mode=mode,
                                           draws={k: np.stack([d[k] for d in draws]) for k in draws[0]})
        for k, sl in (("anc_pc", slice(None)), ("anc_node", slice(None)), ("anc_sn", slice(0, 3))):
            a, b = got[k][:, sl], out["%s_%s" % (name, k)][:, sl]
            unequal += int((a.view(np.int32) != b.view(np.int32)).sum())
            total += a.size
    out["fps_min_gap"] = np.float64(min_gap)
    out["anchor_unequal_share"] = np.float64(unequal / total)
    print("smallest FPS gap %.3e; anchor values not bit-equal to the host twin's: %d of %d (%.4f%%)"
          % (min_gap, unequal, total, 100.0 * unequal / total))
    path = os.path.join(HERE, "indoor_pairs_cases.npz")
    np.savez_compressed(path, **out)
    size, cap = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "indoor_head.npz"))
    print("wrote", path, "%.0f KB (indoor_head.npz: %.0f KB)" % (size / 1024, cap / 1024))
    if size > cap:
        raise SystemExit("the fixture is larger than indoor_head.npz")


if __name__ == "__main__":
    main()
