"""The unchanged GEMM and layer-backward forms at a group of 448: a size that is neither a power of two nor a divisor of a
position tile, and larger than any row-bias or pooled group of tests/gemm_cases.py / tests/layer_bwd_cases.py (128).  Fixtures
from the existing oracles (gemm_oracle.gemm_fixture, layer_bwd_oracle.layer_fixture); shared by tests/test_wide_cpu.py, which
asserts every fixture's record on the CPU, and tests/test_wide_forms_gpu.py.  No library import here.

Forward, one case per form that takes a row bias.  The shape is rb = 448 on P = 1344, nb = 2 -- the tiles of 128 and 256
positions cross the group boundaries at 448 and 896, the tiles of 64 (gemm_x2r, narrow_fwd) change group every seventh tile --
wherever the form's own launch conditions let that shape reach it:
  generic fp32 tile kernel, gemm_x3p, gemm_x2r   P = 1344, nb = 2
  gemm_x2d      256-row tiles need ceil(M / 256) nb ceil(P / 128) >= 256 (usip_mlp_x3p_tile_rows): P = 1344 with nb = 24
  gemm_x2f      whole 256-position tiles (P % 256 == 0): P = 1792 = lcm(256, 448), nb = 19; every second tile crosses a boundary
  narrow_fwd    at least 2048 tiles of 64 positions (usip_mlp_narrow_forward_blocks): P = 66304 = 148 * 448, nb = 2
Layer backward: the pooled forms of layer_bwd_x2 a group of 448 reaches (448 % 32 == 0: PG + SPLIT; with RED; with RED and the
per-neighbourhood sums) at group 448 on P = 1344, nb = 2.  narrow_bwd has no pooled form."""
from gemm_cases import BF, F32K, NF, S3, X3, XD, XF, XR  # noqa: F401
from gemm_oracle import gemm_fixture
from layer_bwd_cases import LPG, LPR
from layer_bwd_oracle import layer_bwd_blocks, layer_fixture

GROUP = 448
WIDE_GEMM_CASES = {}


def _case(name, mode, form, nb, K, M, P, kernel, wgs, **opt):
    WIDE_GEMM_CASES[name] = dict(name=name, mode=mode, form=form, pro=1, nb=nb, K=K, M=M, P=P, kernel=kernel, wgs=wgs,
                                 opt=dict(opt, rb=GROUP, stats=True))


_case("generic rb 448", "f32", "x2h", 2, 17, 129, 1344, F32K % (2, 2, 1, 1, "true", 1), 2 * 11 * 3)
_case("x3p rb 448", "f32x3", "x3", 2, 32, 129, 1344, X3 % (1, 1, 2, 2, 3, 3), 2 * 11 * 2, knobs=S3)
_case("x2r rb 448", "f32x2", "x2h", 2, 16, 128, 1344, XR % (1, 1, "true"), 2 * 21, walk=512, knobs=S3)
_case("x2d rb 448", "f32x2", "x2h", 24, 16, 256, 1344, XD % (1, 1, "false", 1, "true", "false"), 24 * 11, knobs=S3)
_case("x2f rb 448", "f32x2", "x2h", 19, 64, 256, 1792, XF % (1, 1, "false"), 19 * 7, knobs=S3)
_case("narrow_fwd rb 448", "f32", "x2h", 2, 64, 128, 66304, NF % (2, "true", "true", "true"), 512, walk=512)


def wide_gemm_fixture(name):
    c = WIDE_GEMM_CASES[name]
    o = c["opt"]
    tile = 0 if o.get("walk") else (256 if c["M"] <= 64 else 128)
    return gemm_fixture(c["form"], 1, c["nb"], c["K"], c["M"], c["P"], seed=len(name), bias=True, rb_group=GROUP,
                        stats_tile=tile, x2r_stats=o.get("walk", 0))


WIDE_LAYER_CASES = {}


def _lcase(name, kernel, **opt):
    WIDE_LAYER_CASES[name] = dict(name=name, kernel=kernel, cin=128, cout=128, nb=2, P=1344,
                                  wgs=layer_bwd_blocks(128, 128, 1344, 2), opt=dict(opt, pooled=GROUP))


_lcase("pooled PG group 448", LPG)
_lcase("pooled red group 448", LPR, red=True)
_lcase("pooled gsum group 448", LPR, red=True, gsum=True)


def wide_layer_fixture(name):
    c = WIDE_LAYER_CASES[name]
    o = c["opt"]
    return layer_fixture(128, 128, c["nb"], c["P"], pooled=GROUP, red=o.get("red", False), gsum=o.get("gsum", False),
                         seed=len(name))
