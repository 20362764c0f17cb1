"""Bits of the RANSAC host twins pinned at one commit: tests/golden/ransac_parent_bits.npz.

The device kernels are held to the host twins bit for bit (tests/test_registration_gpu.py, tests/test_fragments_gpu.py), but
twin and device share csrc/registration_math.h and could drift together.  This fixture holds what the twins computed at the
commit BEFORE the f-6 and f-9 RANSAC copies were merged into one kernel pair and one twin: the f-6 twin on case A, the f-9
`_large` twin on case B.  tests/test_registration_cpu.py holds today's twin to it, tests/test_registration_gpu.py the device.

Inputs are not stored: they come from the seeded generator the tests use (tests/eval_oracle.py make_batch), and the fixture
holds a SHA-256 of x1, x2 and count, so a generator that has moved fails the test instead of moving the expectation.

  A  the <= 1024 batch of tests/test_fragments_gpu.py: counts 1024, 2, 300, 513 at Nmax = 1024, with gt (delta_t, delta_deg)
  B  chunk edges and tiny counts: 1023 .. 2049 around the 1024-row LDS chunk, 3 and 4, at Nmax = 2049

Both: 64 Philox trials, max_trials = 63, threshold 0.2.  Everything is stored as integers or as the bit patterns of float64.

    python tests/golden/make_ransac_golden.py       (regenerating it moves the pin: do that only on purpose)
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import eval_oracle as eo  # noqa: E402

PATH = os.path.join(HERE, "ransac_parent_bits.npz")
T, MAX_TRIALS, THR = 64, 63, 0.2
CASES = {
    "A": dict(batch=dict(seed=34, P=4, n=1024, T=8, counts=[1024, 2, 300, 513], noise=0.01),
              ids=[7, 8, 1000, 3], seed=5, gt=True, large=False),
    "B": dict(batch=dict(seed=91, P=8, n=2049, T=1, counts=[1023, 1024, 1025, 2047, 2048, 2049, 3, 4], noise=0.02),
              ids=list(range(100, 108)), seed=17, gt=False, large=True),
}
TRIAL_FIELDS = ("counts", "hypotheses", "triplets")
SELECT_FIELDS = ("Rt", "inlier_mask", "inliers", "trialcount", "valid", "chosen")
GT_FIELDS = ("delta_t", "delta_deg")


def inputs(name):
    """-> (x1, x2, count, gt or None, pair ids i64, Philox seed, large) of one case."""
    c = CASES[name]
    x1, x2, count, gt, _ = eo.make_batch(**c["batch"])
    return x1, x2, count, (gt if c["gt"] else None), np.asarray(c["ids"], np.int64), c["seed"], c["large"]


def digest(x1, x2, count):
    h = hashlib.sha256()
    for a in (x1, x2, count):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def bits(a):
    """An output as the fixture stores it: float64 as its bit pattern, everything else as it is."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def fields(name):
    return TRIAL_FIELDS + SELECT_FIELDS + (GT_FIELDS if CASES[name]["gt"] else ())


def collect(trials, select):
    """(counts, hypotheses, triplets), the select dict -> {field: stored form}."""
    out = dict(zip(TRIAL_FIELDS, trials))
    out.update({k: v for k, v in select.items() if v is not None})
    return {k: bits(v) for k, v in out.items()}


def host_twin(name):
    from usip_amd import evaluation as ev
    from usip_amd import fragments as fr
    x1, x2, count, gt, ids, seed, large = inputs(name)
    if large:
        trials = fr.ransac_trials_large_cpu(x1, x2, count, T, THR, seed, ids)
        select = fr.ransac_select_large_cpu(x1, x2, count, trials[0], MAX_TRIALS, THR, seed, ids)
    else:
        trials = ev.ransac_trials_cpu(x1, x2, count, T, THR, seed, ids)
        select = ev.ransac_select_cpu(x1, x2, count, trials[0], MAX_TRIALS, THR, seed, ids, gt=gt)
    return collect(trials, select)


def main():
    out = {}
    for name in CASES:
        x1, x2, count = inputs(name)[:3]
        out["%s_sha256" % name] = np.frombuffer(bytes.fromhex(digest(x1, x2, count)), np.uint8)
        got = host_twin(name)
        for k in fields(name):
            out["%s_%s" % (name, k)] = got[k]
        print(name, "valid", got["valid"].tolist(), "inliers", got["inliers"].tolist(), "trialcount",
              got["trialcount"].tolist(), "chosen", got["chosen"].tolist())
    np.savez_compressed(PATH, **out)
    size = os.path.getsize(PATH)
    print("wrote", PATH, "%.0f KB" % (size / 1024))
    if size > 100 * 1024:
        raise SystemExit("the fixture is larger than 100 KB")


if __name__ == "__main__":
    main()
