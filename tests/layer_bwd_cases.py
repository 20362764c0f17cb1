"""The exact cases of the fused layer-backward kernels (csrc/layer_bwd_x2.hip, csrc/narrow_bwd.hip): which fixture of
tests/layer_bwd_oracle.py must launch which kernel instantiation with how many workgroups.  Shared by
tests/test_layer_bwd_oracle_cpu.py (which builds every fixture and asserts its record on the CPU) and
tests/test_layer_bwd_forms_gpu.py.  No library import here."""
from layer_bwd_oracle import layer_bwd_blocks, layer_fixture, narrow_fixture, narrow_plan

# what the two dispatchers can launch (layer_bwd_x2.hip::layer_backward_x2h, narrow_bwd.hip::usip_mlp_narrow_backward_f32), as
# the launch log spells it: layer_bwd_x2_kernel<CIN, COUT, POOL, RED, NW, BP, DB, PG, SPLIT>, narrow_bwd_kernel<COUT, XPRO, RED>
LX = "layer_bwd_x2_kernel<%d, %d, %s, %s, %d, 32, %s, %s, %s>"
L64 = LX % (64, 64, "false", "false", 4, "false", "false", "false")
L64R = LX % (64, 64, "false", "true", 4, "false", "false", "false")
L64WS = "layer_bwd_x2ws_kernel<64, 64, 4, 32>"
L128 = LX % (64, 128, "false", "false", 4, "false", "false", "true")
L128R = LX % (64, 128, "false", "true", 4, "false", "false", "true")
LP = LX % (128, 128, "true", "false", 8, "true", "false", "false")          # pooled, DB, a group that is no multiple of 32
LPG = LX % (128, 128, "true", "false", 8, "true", "true", "true")           # pooled, DB + PG + SPLIT
LPR = LX % (128, 128, "true", "true", 8, "false", "true", "true")           # pooled, RED + PG + SPLIT
LAYER_DISPATCH = (L64, L64R, L64WS, L128, L128R, LP, LPG, LPR)
NK = "narrow_bwd_kernel<%d, %s, %s>"
NARROW_DISPATCH = tuple(NK % (co, x, r) for co in (64, 128) for x, r in (("false", "false"), ("true", "false"), ("true", "true")))
FINALIZE = "wsum_finalize_kernel"

# ------------------------------------------------------------------------------------------------ layer_bwd_x2
# Options: red, gsum, ws (rows of the source), pooled (group), x_rows (X as rows [0, cin) of a wider tensor), ldw / wcol (the
# operand as columns [wcol, wcol + cin) of a wider W / dW), c_entry (dx_rows: through the C entry, dX as rows of a wider tensor).
# The walks: (1, 64) two workgroups with one tile each; (3, 5504) 516 tiles on 512 workgroups -- four take a second tile, in another
# cloud; (3, 16448) 1542 tiles: three and four per workgroup.  Pooled, on 256 workgroups: (1, 192) one tile each, (3, 2880) 270
# tiles: one and two, (3, 8256) 774 tiles: three and four.
LAYER_CASES = {}


def _case(name, kernel, cin, cout, nb, P, **opt):
    assert name not in LAYER_CASES
    LAYER_CASES[name] = dict(name=name, kernel=kernel, cin=cin, cout=cout, nb=nb, P=P, wgs=layer_bwd_blocks(cin, cout, P, nb),
                             opt=opt)


_case("64x64 one tile", L64, 64, 64, 1, 64)
_case("64x64 second tile in another cloud, wider X", L64, 64, 64, 3, 5504, x_rows=96)
_case("64x64 three and four tiles, wider W", L64, 64, 64, 3, 16448, ldw=128, wcol=64)
_case("64x64 red one tile, wider dX through the C entry", L64R, 64, 64, 1, 64, red=True, c_entry=80)
_case("64x64 red second tile in another cloud", L64R, 64, 64, 3, 5504, red=True, ldw=128, wcol=64)
_case("64x64 red three and four tiles, wider X", L64R, 64, 64, 3, 16448, red=True, x_rows=96)
_case("x2ws one tile, one source row", L64WS, 64, 64, 1, 64, red=True, ws=1)
_case("x2ws second tile in another cloud, seven rows, wider X", L64WS, 64, 64, 3, 5504, red=True, ws=7, x_rows=96)
_case("x2ws three and four tiles, eight rows, wider W", L64WS, 64, 64, 3, 16448, red=True, ws=8, ldw=128, wcol=64)
_case("x2ws two tiles per workgroup, three rows", L64WS, 64, 64, 2, 16384, red=True, ws=3)
_case("64x128 one tile", L128, 64, 128, 1, 64)
_case("64x128 second tile in another cloud, wider W", L128, 64, 128, 3, 5504, ldw=128, wcol=64)
_case("64x128 three and four tiles", L128, 64, 128, 3, 16448)
_case("64x128 red one tile, wider X", L128R, 64, 128, 1, 64, red=True, x_rows=96)
_case("64x128 red second tile in another cloud", L128R, 64, 128, 3, 5504, red=True)
_case("64x128 red three and four tiles, wider dX through the C entry", L128R, 64, 128, 3, 16448, red=True, c_entry=80)
_case("pooled group 1, one tile", LP, 128, 128, 1, 192, pooled=1)
_case("pooled group 16, one and two tiles", LP, 128, 128, 3, 2880, pooled=16)
_case("pooled group 24 straddles tiles, three and four", LP, 128, 128, 3, 8256, pooled=24)
_case("pooled group 48 straddles tiles, one tile", LP, 128, 128, 1, 192, pooled=48)
_case("pooled group 48 straddles tiles, one and two", LP, 128, 128, 3, 2880, pooled=48)
_case("pooled PG group 32, one tile", LPG, 128, 128, 1, 192, pooled=32)
_case("pooled PG group 64, one and two tiles", LPG, 128, 128, 3, 2880, pooled=64)
_case("pooled PG group 96, three and four tiles", LPG, 128, 128, 3, 8256, pooled=96)
_case("pooled PG group 32, three and four tiles", LPG, 128, 128, 3, 8256, pooled=32)
_case("pooled red group 32, one tile", LPR, 128, 128, 1, 192, pooled=32, red=True)
_case("pooled red group 96, one and two tiles", LPR, 128, 128, 3, 2880, pooled=96, red=True)
_case("pooled red group 64, three and four tiles", LPR, 128, 128, 3, 8256, pooled=64, red=True)
_case("pooled red group 128, two tiles", LPR, 128, 128, 4, 4096, pooled=128, red=True)
_case("pooled gsum group 128, fewer runs than workgroups", LPR, 128, 128, 1, 768, pooled=128, red=True, gsum=True)
_case("pooled gsum group 64, idle workgroups and two clouds", LPR, 128, 128, 3, 2880, pooled=64, red=True, gsum=True)
_case("pooled gsum group 32, three and four runs", LPR, 128, 128, 3, 8256, pooled=32, red=True, gsum=True)
_case("pooled gsum group 96, two workgroups take two runs", LPR, 128, 128, 3, 8256, pooled=96, red=True, gsum=True)
_case("pooled gsum group 128, wider X", LPR, 128, 128, 3, 8448, pooled=128, red=True, gsum=True, x_rows=160)


def layer_case_fixture(name):
    c = LAYER_CASES[name]
    o = c["opt"]
    return layer_fixture(c["cin"], c["cout"], c["nb"], c["P"], pooled=o.get("pooled", 0), red=o.get("red", False),
                         gsum=o.get("gsum", False), ws_rows=o.get("ws", 0), seed=len(name), x_rows=o.get("x_rows", 0),
                         ldw=o.get("ldw", 0), wcol=o.get("wcol", 0))


# ------------------------------------------------------------------------------------------------ narrow_bwd
# P 64: one tile inside a 256-position segment; P 320: two segments, the last one short; (3, 1088): five segments per cloud;
# (2, 49152): 768 (384 at 128 outputs) segments of 256 positions.  (The smallest shape with more than four 64-position tiles per
# segment has 123 000 positions -- narrow_plan gives tps > 4 only beyond 4 slots / nb tiles per cloud --: pinned on the host.)
NARROW_CASES = {}


def _ncase(name, cout, xpro, red, nb, P, **opt):
    assert name not in NARROW_CASES
    seglen, segs = narrow_plan(cout, P, nb)
    NARROW_CASES[name] = dict(name=name, kernel=NK % (cout, str(xpro).lower(), str(red).lower()), cout=cout, xpro=xpro, red=red,
                              nb=nb, P=P, wgs=nb * segs, seglen=seglen, segs=segs, opt=opt)


for _co in (64, 128):
    for _x, _r in ((False, False), (True, False), (True, True)):
        _tag = "narrow %d%s%s" % (_co, " xpro" if _x else "", " red" if _r else "")
        _ncase(_tag + " one tile", _co, _x, _r, 1, 64)
        _ncase(_tag + " short last segment", _co, _x, _r, 2, 320)
        _ncase(_tag + " five segments, wider X and W", _co, _x, _r, 3, 1088, x_rows=96, ldw=128, wcol=64)
        _ncase(_tag + " chip-filling, four tiles per segment", _co, _x, _r, 2, 49152)


def narrow_case_fixture(name):
    c = NARROW_CASES[name]
    o = c["opt"]
    return narrow_fixture(c["cout"], c["xpro"], c["red"], c["nb"], c["P"], seed=len(name), x_rows=o.get("x_rows", 0),
                          ldw=o.get("ldw", 0), wcol=o.get("wcol", 0))


# ------------------------------------------------------------------------------------------------ wsum_finalize
FINALIZE_BLOCKS = (1, 7, 8, 9, 31, 32, 33, 255, 256, 512)
FINALIZE_ROWS = (1, 3, 8)
