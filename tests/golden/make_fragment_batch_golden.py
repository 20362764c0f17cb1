"""Fixtures of the evaluation fragment builder: tests/golden/fragment_batch_cases.npz.

Runs the reference's OWN RedwoodLoader.__getitem__ (evaluation/redwood_loader.py:73-127) and Match3DEvalLoader.__getitem__
(data/match3d_eval_loader.py:78-103), each with the FarthestSampler of its own file, compiled out of the reference checkout
with ast (the modules import torchvision / h5py / matplotlib, absent here).  np.load is answered from this script's own
frames, and every np.random draw and argmax by a recorder, so the draws go into the fixture next to what the reference
computed:

  choice(n, k, replace=False)   a permuted prefix, as numpy's
  randint(n)                    the first FPS index
  argmax                        FarthestSampler's picks, i.e. the FPS indices

RedwoodLoader runs on all four frames (1180, 1100, 700 and 300 rows: the last two take its fix_idx layout),
Match3DEvalLoader on the two long ones (it has no such branch and would raise).

FPS condition.  The reference samples in float64, the builder in float32.  For every FPS round of every item the generator
measures the relative gap between the largest running distance and the largest value different from it (duplicated rows of
a short frame tie exactly; the lowest index wins on both sides).  The frames are reseeded until the reference ALONE meets
the bar of 1e-4 -- a thousand float32 roundings -- in every round; the smallest gap is stored (fps_min_gap).

    python tests/golden/make_fragment_batch_golden.py        (needs the reference checkout)
"""
import ast
import os
import re
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from usip_amd import synth  # noqa: E402

REF = "/root/reference"
N, N_SUB, M, CS, ROW_LEN = 1024, 512, 32, 4, 7
FRAME_ROWS = (1180, 1100, 700, 300)      # 700: one whole copy + a draw of 324; 300: three copies + 124
MIN_GAP = 1e-4
# name: (loader, frames, recorder seed)
CASES = {"redwood": ("RedwoodLoader", (0, 1, 2, 3), 500), "match3d": ("Match3DEvalLoader", (0, 1), 501)}


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


def make_np(frames, rec):
    """numpy, with load and random answered by this script and argmax recorded."""
    proxy = types.ModuleType("np_proxy")
    proxy.__dict__.update({k: getattr(np, k) for k in dir(np) if not k.startswith("__")})

    def load(path, *a, **kw):
        return frames[int(re.findall(r"(\d+)\.npy$", os.path.basename(path))[0])].copy()

    def argmax(x, *a, **kw):
        i = int(np.argmax(x, *a, **kw))
        rec.log.append(("argmax", i))
        return i
    proxy.load, proxy.random, proxy.argmax = load, rec, argmax
    return proxy


def reference(np_proxy, path, names):
    ns = {"np": np_proxy, "torch": torch, "os": os, "data": types.SimpleNamespace(Dataset=object)}
    tree = ast.parse(open(path).read())
    nodes = [n for n in tree.body if getattr(n, "name", None) in names]
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns


def loader(kind, np_proxy, opt, num_frames):
    if kind == "RedwoodLoader":
        ns = reference(np_proxy, os.path.join(REF, "evaluation", "redwood_loader.py"), {"FarthestSampler", kind})
        ld = ns[kind].__new__(ns[kind])
        ld.scene_name_list, ld.scene_frame_num_acc = ["livingroom1"], [num_frames]
    else:
        ns = reference(np_proxy, os.path.join(REF, "data", "match3d_eval_loader.py"), {"FarthestSampler", kind})
        ld = ns[kind].__new__(ns[kind])
        ld.dataset = [(os.path.join("r", "scene", "cloud_bin_%d.npy" % i), 0, i) for i in range(num_frames)]
    ld.root, ld.opt, ld.farthest_sampler = "r", opt, ns["FarthestSampler"]()
    return ld


def parse_item(log, n):
    """One __getitem__'s draws: rows [N], cand [n_sub], first, and the FPS picks [M]."""
    pos = [0]

    def take(what):
        k, v = log[pos[0]]
        assert k == what, (pos[0], k, what)
        pos[0] += 1
        return v
    if n >= N:
        rows = take("choice")
    else:
        fix = np.arange(n)
        while n + fix.shape[0] < N:
            fix = np.concatenate((fix, np.arange(n)))
        rows = np.concatenate((fix, take("choice")))
    cand = take("choice")
    first = take("randint")
    fps = [first] + [take("argmax") for _ in range(M - 1)]
    assert pos[0] == len(log) and rows.shape == (N,) and cand.shape == (N_SUB,), (pos[0], len(log))
    return rows.astype(np.int32), cand.astype(np.int32), np.int32(first), np.asarray(fps)


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


def run(frame_seed):
    rng = np.random.default_rng(frame_seed)
    frames = []
    for n in FRAME_ROWS:
        pc = synth.make_cloud(rng, n, "slab:3").T
        sn = synth.make_normals(rng, n, 4).T
        frames.append(np.concatenate([pc, sn], 1).astype(np.float32))
    out = {"frame_%d" % i: f for i, f in enumerate(frames)}
    out.update(N=np.int32(N), n_sub=np.int32(N_SUB), M=np.int32(M), Cs=np.int32(CS), frame_seed=np.int64(frame_seed))
    opt = types.SimpleNamespace(input_pc_num=N, node_num=M, surface_normal_len=CS)
    min_gap = np.inf
    for name, (kind, ids, seed) in CASES.items():
        rec = Recorder(seed)
        ld = loader(kind, make_np(frames, rec), opt, len(frames))
        items, rows, cand, first, slots = [], [], [], [], []
        for i in ids:
            rec.log = []
            items.append(ld.__getitem__(i))
            assert items[-1][4] == i
            r, c, f, fps = parse_item(rec.log, len(frames[i]))
            min_gap = min(min_gap, fps_gap(frames[i][r, 0:3][c], fps))
            rows.append(r), cand.append(c), first.append(f), slots.append(c[fps])
        for ki, k in enumerate(("pc", "sn", "node")):
            v = np.stack([it[ki].numpy() for it in items])
            assert v.dtype == np.float32
            out["%s_%s" % (name, k)] = v
        out["%s_draw_rows" % name] = np.stack(rows).astype(np.int16)
        out["%s_draw_cand" % name] = np.stack(cand).astype(np.int16)
        out["%s_draw_first" % name] = np.asarray(first, dtype=np.int32)
        out["%s_node_slots" % name] = np.stack(slots).astype(np.int32)
        out["%s_ids" % name] = np.asarray(ids, dtype=np.int32)
    out["fps_min_gap"] = np.float64(min_gap)
    return out


def main():
    for frame_seed in range(2027, 2127):
        out = run(frame_seed)
        gap = float(out["fps_min_gap"])
        print("frame seed %d: smallest FPS gap %.3e" % (frame_seed, gap))
        if gap >= MIN_GAP:
            break
    else:
        raise SystemExit("no frame seed meets the FPS condition")
    path = os.path.join(HERE, "fragment_batch_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "%.0f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
