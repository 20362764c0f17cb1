"""Fixtures of the training-pair builder: tests/golden/pairs_cases.npz.

Runs the reference's OWN KittiLoader / OxfordLoader .__getitem__ (data/kitti_detector_loader.py:101-259,
data/oxford_detector_loader.py:99-229) with augment and transform_pc_pytorch (data/augmentation.py:15-28, :64-75,
:199-248, :266-278), compiled out of the reference checkout with ast (its modules import torchvision / h5py, absent
here).  np.load is substituted (the scans come from this script), and every np.random draw is answered by a recorder,
so the draws go into the fixture next to what the reference computed from them:

  choice(n, k, replace=False)   a permuted prefix, as numpy's
  randint / uniform / rand      uniform(low, high) = low + (high - low) * u, numpy's own formula; u is recorded
  randn                         standard normals rounded to values float32 holds exactly (stored losslessly in f32)
  argmax                        recorded too: FarthestSampler's picks, i.e. the FPS indices

    python tests/golden/make_pairs_golden.py        (needs the reference checkout)
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
N, M = 1024, 32
SCAN_ROWS = (1500, 700, 1300)        # scan 1 is shorter than N: KittiLoader's fix_idx layout
# name: (loader, Cs, train, rot_horizontal, rot_3d, rot_perturbation, translation_perturbation, scan)
CASES = {
    "k1_train": ("kitti", 1, 1, 1, 0, 0, 0, 1),
    "k4_train": ("kitti", 4, 1, 1, 0, 1, 1, 0),
    "k5_train": ("kitti", 5, 1, 0, 1, 0, 0, 2),
    "k4_test": ("kitti", 4, 0, 1, 0, 0, 0, 1),
    "o4_train": ("oxford", 4, 1, 1, 0, 0, 0, 0),
    "o5_train": ("oxford", 5, 1, 1, 0, 1, 0, 2),
    "o5_test": ("oxford", 5, 0, 1, 0, 0, 0, 2),
    "k1_norot": ("kitti", 1, 1, 0, 0, 0, 1, 0),    # no rotation stage: the points stay an f32 array through augment
}


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
        self.log.append(("randn", z.copy()))
        return float(z) if shape == () else z


def make_np(scans, rec):
    """numpy, with load and random answered by this script and argmax recorded."""
    proxy = types.ModuleType("np_proxy")
    proxy.__dict__.update({k: getattr(np, k) for k in dir(np) if not k.startswith("__")})

    def load(path, *a, **kw):
        if path.endswith(".npz"):
            return {"pose": np.eye(4)}
        return scans[int(os.path.basename(path).split(".")[0])].copy()

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
            {"angles2rotation_matrix", "atomic_rotate", "transform_pc_pytorch", "coordinate_ENU_to_cam_element",
             "coordinate_ENU_to_cam"})
    extract(ns, os.path.join(REF, "data", "kitti_detector_loader.py"), {"FarthestSampler", "KittiLoader"})
    extract(ns, os.path.join(REF, "data", "oxford_detector_loader.py"), {"OxfordLoader"})
    return ns


def loader(ns, kind, opt, mode, num_scans):
    if kind == "kitti":
        ld = ns["KittiLoader"].__new__(ns["KittiLoader"])
        ld.root, ld.seq_list, ld.folder_list, ld.accumulated_sample_num_list = "r", [0], ["f"], [num_scans]
    else:
        ld = ns["OxfordLoader"].__new__(ns["OxfordLoader"])
        ld.root, ld.is_filter_str = "r", ""
        ld.dataset = [{"file": "%06d.bin" % i, "anc_idx": i} for i in range(num_scans)]
    ld.opt, ld.mode, ld.farthest_sampler = opt, mode, ns["FarthestSampler"]()
    return ld


def parse(log, kind, n, Cs, train, opt):
    """The recorded draws in the layouts of include/usip_hip.h (usip_pairs_draws)."""
    pos = [0]

    def take(what):
        k, v = log[pos[0]]
        assert k == what, (pos[0], k, what)
        pos[0] += 1
        return v
    n_sub = int(N / 3) if kind == "kitti" else int(N / 8)
    rows, cand, first, fps = [None, None], [None, None], [0, 0], [None, None]
    params = np.zeros(24)

    def choice_rows():
        if n >= N:
            return take("choice")
        fix = np.arange(n)
        while n + fix.shape[0] < N:
            fix = np.concatenate((fix, np.arange(n)))
        return np.concatenate((fix, take("choice")))

    def fps_of(c):
        cand[c] = take("choice")
        first[c] = take("randint")
        fps[c] = [first[c]] + [take("argmax") for _ in range(M - 1)]
    if kind == "kitti":
        for c in range(2):
            rows[c] = choice_rows()
            fps_of(c)
    else:
        rows[0], rows[1] = take("choice"), take("choice")
        params[11] = take("uniform")[0]
        fps_of(0)
        fps_of(1)
    jit = {}
    if train:
        params[0] = take("uniform")[0]
        params[1:4] = take("uniform")
        params[4:7] = take("randn")
        jit["jit_pc"], jit["jit_sn"], jit["jit_node"] = take("randn"), take("randn"), take("randn")
        params[7] = take("uniform")[0]
        params[8:11] = take("uniform")
    if opt.rot_3d:
        params[12:15] = [take("uniform")[0] for _ in range(3)]
    elif opt.rot_horizontal:
        params[12] = take("uniform")[0]
    if opt.rot_perturbation:
        params[15:18] = [take("randn") for _ in range(3)]
    params[18] = take("uniform")[0]
    params[19:22] = take("uniform")
    assert pos[0] == len(log), (pos[0], len(log))
    d = dict(rows=np.stack(rows)[None].astype(np.int32), cand=np.stack(cand)[None].astype(np.int32),
             first=np.asarray(first, dtype=np.int32)[None], params=params[None])
    for k, v in jit.items():
        d[k] = v.astype(np.float32)[None]
    node_slots = np.stack([np.asarray(cand[c])[fps[c]] for c in range(2)])[:, None].astype(np.int32)
    return d, node_slots


def main():
    rng = np.random.default_rng(2024)
    scans = []
    for n in SCAN_ROWS:
        pc = synth.make_cloud(rng, n, "slab:20").T
        sn = synth.make_normals(rng, n, 5).T
        scans.append(np.concatenate([pc, sn], 1).astype(np.float32))
    out = {"scan_%d" % i: s for i, s in enumerate(scans)}
    out["N"], out["M"] = np.int32(N), np.int32(M)
    for ci, (name, (kind, Cs, train, rh, r3, pert, transl, scan)) in enumerate(CASES.items()):
        opt = types.SimpleNamespace(input_pc_num=N, node_num=M, surface_normal_len=Cs, rot_horizontal=bool(rh),
                                    rot_3d=bool(r3), rot_perturbation=bool(pert), translation_perturbation=bool(transl),
                                    radius_threshold=100, is_height_scaling=True)
        rec = Recorder(100 + ci)
        ns = reference(make_np(scans, rec))
        ld = loader(ns, kind, opt, "train" if train else "test", len(scans))
        res = ld.__getitem__(scan)
        d, node_slots = parse(rec.log, kind, len(scans[scan]), Cs, train, opt)
        keys = ("src_pc", "src_sn", "src_node", "dst_pc", "dst_sn", "dst_node", "R", "scale", "shift")
        for k, v in zip(keys, res):
            out["%s_%s" % (name, k)] = np.asarray(v.numpy() if torch.is_tensor(v) else v, dtype=np.float32)
        for k, v in d.items():
            out["%s_draw_%s" % (name, k)] = v
        out["%s_node_slots" % name] = node_slots
        out["%s_case" % name] = np.array([0 if kind == "kitti" else 1, Cs, train, rh, r3, pert, transl, scan],
                                         dtype=np.int32)
    path = os.path.join(HERE, "pairs_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "%.0f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
