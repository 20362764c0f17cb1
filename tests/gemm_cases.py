"""The exact cases of the shared-MLP product family: which fixture of tests/gemm_oracle.py, reached how, must launch which
kernel instantiation with how many workgroups.  Shared by tests/test_gemm_oracle_cpu.py (which asserts every fixture's claims
on the CPU) and the GPU files tests/test_gemm_forms_gpu.py / tests/test_wgrad_forms_gpu.py.  No library import here."""
from gemm_oracle import gemm_fixture, wgrad_fixture, wgrad_plan, wgrad_x3_plan


# ------------------------------------------------------------------------------------------------ the GEMM cases
# One row per exact case of tests/test_gemm_forms_gpu.py; tests/test_gemm_oracle_cpu.py builds every fixture and asserts its
# record first.  `kernel` / `wgs`: the instantiation the launch log must name and its workgroup count.  Options: stats, rb
# (row-bias group), pool (pro 3 group), fork (group), bias; route: knobs {name: value}, narrow (ops.NARROW_FWD), a_trans,
# a_offset (then lda > M), wider (out= rows of a wider tensor), cache (PLANES_CACHE is a dict), walk (statistics: one slot per
# persistent workgroup, the number = the cap of the walk).
GEMM_CASES = {}


def _case(name, mode, form, pro, nb, K, M, P, kernel, wgs, **opt):
    assert name not in GEMM_CASES
    GEMM_CASES[name] = dict(name=name, mode=mode, form=form, pro=pro, nb=nb, K=K, M=M, P=P, kernel=kernel, wgs=wgs, opt=opt)


def _tile(M, P, nb, bm, bn):
    return nb * ((P + bn - 1) // bn) * ((M + bm - 1) // bm)


F32K = "gemm_kernel<%d, %d, 16, %d, %d, %s, %d>"
# fp32 MFMA tile kernel: <1,4,..,1> 32 x 256, <1,4,..,2> 64 x 256, <2,2,..,1> 64 x 128, <2,2,..,2> 128 x 128 (shared_mlp.hip)
_case("f32 32-row pro1 ragged", "f32", "x2h", 1, 3, 17, 31, 333, F32K % (1, 4, 1, 1, "false", 1), 6, stats=True, rb=3)
_case("f32 32-row 1x1x1", "f32", "x2h", 0, 1, 1, 1, 1, F32K % (1, 4, 0, 1, "false", 1), 1, stats=True)
_case("f32 32-row pro2", "f32", "x2h", 2, 1, 16, 31, 64, F32K % (1, 4, 2, 0, "true", 1), 1, bias=False)
_case("f32 32-row pro3", "f32", "x2h", 3, 1, 16, 31, 64, F32K % (1, 4, 3, 0, "true", 1), 1, pool=16)
_case("f32 64-row pro0", "f32", "x2h", 0, 1, 16, 33, 256, F32K % (1, 4, 0, 1, "true", 2), 1, stats=True, rb=4)
_case("f32 64-row pro1 a_trans", "f32", "x2h", 1, 1, 16, 33, 256, F32K % (1, 4, 1, 1, "true", 2), 1, stats=True, a_trans=True,
      a_offset=3)
_case("f32 64-row pro2 P63", "f32", "x2h", 2, 1, 17, 64, 63, F32K % (1, 4, 2, 0, "false", 2), 1)
_case("f32 64-row pro3", "f32", "x2h", 3, 1, 16, 33, 128, F32K % (1, 4, 3, 0, "true", 2), 1, pool=4)
_case("f32 64x128 pro0 P63", "f32", "x3", 0, 3, 16, 129, 63, F32K % (2, 2, 0, 0, "false", 1), 9)
_case("f32 64x128 pro1 wider", "f32", "x2h", 1, 1, 17, 129, 333, F32K % (2, 2, 1, 1, "false", 1), 9, stats=True, rb=1,
      a_offset=5, wider=True)
_case("f32 64x128 pro2", "f32", "x2h", 2, 1, 16, 129, 128, F32K % (2, 2, 2, 0, "true", 1), 3)
_case("f32 64x128 pro3", "f32", "x3", 3, 1, 17, 129, 128, F32K % (2, 2, 3, 0, "true", 1), 3, pool=4)
_case("f32 128x128 many tiles", "f32", "x2h", 0, 1, 16, 656, 11008, F32K % (2, 2, 0, 1, "true", 2), 516, stats=True, rb=32)
# ... and the float4 path (P % 4 == 0) with the statistics epilogue on the two small tiles: the fixture's first and third rows
_case("f32 32-row pro0 float4 stats", "f32", "x2h", 0, 1, 16, 31, 256, F32K % (1, 4, 0, 1, "true", 1), 1, stats=True)
_case("f32 32-row pro1 float4 stats", "f32", "x2h", 1, 1, 17, 31, 256, F32K % (1, 4, 1, 1, "true", 1), 1, stats=True, rb=32)
_case("f32 64x128 pro0 float4 stats", "f32", "x2h", 0, 1, 16, 129, 128, F32K % (2, 2, 0, 1, "true", 1), 3, stats=True)
_case("f32 64x128 pro1 float4 stats", "f32", "x3", 1, 1, 17, 129, 256, F32K % (2, 2, 1, 1, "true", 1), 6, stats=True, rb=4)
# bf16 multiply: class (a) values only
BF = "gemm_bf16_kernel<%d, %d, 16, %d, %d, %d>"
_case("bf16 128x128", "bf16", "a", 0, 1, 16, 128, 128, BF % (2, 2, 0, 1, 1), 1, stats=True)
_case("bf16 64x256 pro1", "bf16", "a", 1, 3, 17, 33, 333, BF % (1, 4, 1, 1, 1), 6, stats=True, rb=3)
_case("bf16 pro2", "bf16", "a", 2, 1, 16, 129, 63, BF % (2, 2, 2, 0, 1), 2)
_case("bf16 pro3", "bf16", "a", 3, 1, 17, 129, 128, BF % (2, 2, 3, 0, 1), 2, pool=4)
_case("bf16 64x256 pro0 K1", "bf16", "a", 0, 1, 1, 33, 63, BF % (1, 4, 0, 1, 1), 1, stats=True)
_case("bf16 64x256 pro1 row bias 4", "bf16", "a", 1, 1, 16, 33, 256, BF % (1, 4, 1, 1, 1), 1, stats=True, rb=4)
_case("bf16 64x256 pro2", "bf16", "a", 2, 1, 16, 64, 128, BF % (1, 4, 2, 0, 1), 1)
_case("bf16 64x256 pro3", "bf16", "a", 3, 1, 17, 33, 128, BF % (1, 4, 3, 0, 1), 1, pool=4)
_case("bf16 128x128 pro1 a_trans", "bf16", "a", 1, 1, 16, 129, 256, BF % (2, 2, 1, 1, 1), 4, stats=True, rb=32, a_trans=True,
      a_offset=3)
_case("bf16 128x128 pro0 wider", "bf16", "a", 0, 3, 17, 129, 333, BF % (2, 2, 0, 0, 1), 18, rb=1, a_offset=5, wider=True)
# f32x3: the kernel that splits both operands itself
S3 = {"gemm_split3": 2}
_case("f32x3 a_trans", "f32x3", "x3", 0, 1, 32, 128, 200, BF % (2, 2, 0, 1, 3), 2, stats=True, a_trans=True, knobs=S3)
_case("f32x3 K656", "f32x3", "x3", 1, 1, 656, 128, 128, BF % (2, 2, 1, 1, 3), 1, stats=True, knobs=S3)
# gemm_x3p_kernel<PRO, EPI, TM, WN, NPL, ASLOTS>
X3 = "gemm_x3p_kernel<%d, %d, %d, %d, %d, %d>"
_case("x3p nk1", "f32x3", "x3", 0, 1, 16, 128, 200, X3 % (0, 1, 2, 2, 3, 3), 2, stats=True, knobs=S3)
_case("x3p nk2", "f32x3", "x3", 1, 1, 32, 129, 200, X3 % (1, 1, 2, 2, 3, 3), 4, stats=True, rb=4, knobs=S3, cache=True)
_case("x3p nk3", "f32x3", "x3", 2, 2, 48, 128, 200, X3 % (2, 0, 2, 2, 3, 3), 4, knobs=S3)
_case("x3p nk4", "f32x3", "x3", 3, 1, 64, 128, 200, X3 % (3, 0, 2, 2, 3, 3), 2, pool=4, knobs=S3)
_case("x3p nk5 ragged K", "f32x3", "x3", 1, 1, 70, 131, 333, X3 % (1, 0, 2, 2, 3, 3), 6, knobs=S3, wider=True)
_case("x3p two-slot ring", "f32x3", "x3", 0, 1, 48, 128, 200, X3 % (0, 1, 2, 2, 3, 2), 2, stats=True,
      knobs={"gemm_split3": 2, "r5_forms": 32})
_case("x3p 8 tiles", "f32x3", "x3", 0, 1, 16, 128, 1024, X3 % (0, 1, 2, 2, 3, 3), 8, stats=True, knobs=S3)
_case("x3p 256x128", "f32x3", "x3", 0, 1, 16, 256, 32768, X3 % (0, 1, 4, 2, 3, 2), 256, stats=True, knobs=S3)
_case("x3p 256x256 knob 4", "f32x3", "x3", 1, 1, 16, 256, 32768, X3 % (1, 0, 4, 4, 3, 2), 128,
      knobs={"gemm_split3": 2, "x3_gemm_tile": 4})
_case("x3p 256x256 knob 5", "f32x3", "x3", 2, 1, 16, 256, 65536, X3 % (2, 0, 4, 4, 3, 2), 256, bias=False,
      knobs={"gemm_split3": 2, "x3_gemm_tile": 5})
# the same kernel with two fp16 planes
_case("x2h 128-row pro1", "f32x2", "x2h", 1, 1, 48, 200, 200, X3 % (1, 1, 2, 2, 2, 3), 4, stats=True, rb=4, knobs=S3)
_case("x2h 128-row at the bound", "f32x2", "x2h", 1, 1, 16, 129, 256, X3 % (1, 1, 2, 2, 2, 3), 4, stats=True, knobs=S3, cache=True)
_case("x2h 128-row pro2", "f32x2", "x2h", 2, 2, 48, 200, 200, X3 % (2, 0, 2, 2, 2, 3), 8, knobs=S3)
_case("x2h 128-row pro3", "f32x2", "x2h", 3, 1, 48, 200, 256, X3 % (3, 0, 2, 2, 2, 3), 4, pool=16, knobs=S3)
_case("x2h 256-row x2_direct 1", "f32x2", "x2h", 1, 1, 16, 256, 32768, X3 % (1, 1, 4, 2, 2, 2), 256, stats=True,
      knobs={"gemm_split3": 2, "x2_direct": 1})
# gemm_x2r_kernel<PRO, EPI, RB>: persistent, one statistics slot per workgroup
XR = "gemm_x2r_kernel<%d, %d, %s>"
_case("x2r pro1", "f32x2", "x2h", 1, 2, 72, 100, 200, XR % (1, 1, "false"), 8, stats=True, walk=512, knobs=S3)
_case("x2r pro1 no stats", "f32x2", "x2h", 1, 1, 16, 128, 1024, XR % (1, 0, "false"), 16, knobs=S3)
_case("x2r row bias 32", "f32x2", "x2h", 1, 1, 16, 128, 1024, XR % (1, 1, "true"), 16, stats=True, walk=512, rb=32, knobs=S3)
_case("x2r row bias 64", "f32x2", "x2h", 1, 2, 64, 128, 256, XR % (1, 1, "true"), 8, stats=True, walk=512, rb=64, knobs=S3)
_case("x2r pro2", "f32x2", "x2h", 2, 1, 128, 128, 200, XR % (2, 0, "false"), 4, knobs=S3)
_case("x2r pro3", "f32x2", "x2h", 3, 1, 64, 100, 256, XR % (3, 0, "false"), 4, pool=16, knobs=S3)
_case("x2r walks several tiles", "f32x2", "x2h", 1, 1, 16, 100, 33288, XR % (1, 1, "false"), 512, stats=True, walk=512, knobs=S3)
# (no ops.mlp_gemm route reaches the kernel at 64 rows -- the split family starts above them: through usip_mlp_gemm_x2r_f32)
_case("x2r M64 through the C entry", "f32x2", "x2h", 1, 2, 72, 64, 200, XR % (1, 1, "false"), 8, stats=True, walk=512, c_entry=True)
# gemm_x2d_kernel<PRO, EPI, KTAIL, STAGES, RED, GENERAL, DIRECT>
XD = "gemm_x2d_kernel<%d, %d, %s, %d, false, %s, %s>"
_case("x2d K tail", "f32x2", "x2h", 1, 1, 24, 256, 32768, XD % (1, 1, "true", 1, "false", "false"), 256, stats=True, knobs=S3)
_case("x2d odd stages", "f32x2", "x2h", 1, 1, 16, 256, 32768, XD % (1, 1, "false", 1, "false", "false"), 256, stats=True,
      knobs=S3, rb=16)
_case("x2d even stages", "f32x2", "x2h", 1, 1, 32, 256, 32768, XD % (1, 1, "false", 2, "false", "false"), 256, stats=True,
      knobs=S3)
_case("x2d general epilogue", "f32x2", "x2h", 1, 2, 16, 300, 8200, XD % (1, 1, "false", 1, "true", "false"), 260, stats=True,
      knobs=S3)
# (the general epilogue's other trigger: P % 4 != 0 leaves Y unaligned, y_vec = 0 -- dense, and as rows of a wider tensor)
_case("x2d general epilogue unaligned Y", "f32x2", "x2h", 1, 1, 16, 256, 32769, XD % (1, 1, "false", 1, "true", "false"), 257,
      stats=True, knobs=S3)
_case("x2d general epilogue pro2 wider", "f32x2", "x2h", 2, 1, 32, 256, 32770, XD % (2, 0, "false", 1, "true", "false"), 257,
      bias=False, knobs=S3, wider=True)
_case("x2d direct pro2", "f32x2", "x2h", 2, 1, 32, 256, 32768, XD % (2, 0, "false", 2, "false", "true"), 256, bias=False, knobs=S3)
_case("x2d direct pro3", "f32x2", "x2h", 3, 1, 32, 256, 32768, XD % (3, 0, "false", 2, "false", "true"), 256, bias=False, pool=16,
      knobs=S3)
_case("x2d pro2 x2_direct 8", "f32x2", "x2h", 2, 1, 32, 256, 32768, XD % (2, 0, "false", 2, "false", "false"), 256, bias=False,
      knobs={"gemm_split3": 2, "x2_direct": 8})
_case("x2d x2_direct 12", "f32x2", "x2h", 1, 1, 64, 256, 32768, XD % (1, 1, "false", 2, "false", "false"), 256, stats=True,
      knobs={"gemm_split3": 2, "x2_direct": 12})
XRED = "gemm_x2d_kernel<%d, 0, false, %d, true, false, false>"
_case("x2d red", "f32x2", "x2h", 2, 1, 32, 256, 32768, XRED % (2, 2), 256, bias=False, red=0, knobs=S3)
_case("x2d red group 16", "f32x2", "x2h", 2, 1, 64, 256, 32768, XRED % (2, 2), 256, bias=False, red=16, knobs=S3)
_case("x2d red group 32 pooled", "f32x2", "x2h", 3, 1, 16, 256, 32768, XRED % (3, 1), 256, bias=False, red=32, pool=16, knobs=S3)
# gemm_x2f_kernel<PRO, EPI, DGRAD> and the fork kernel: whole 256 x 256 tiles, persistent beyond 256 tiles
XF = "gemm_x2f_kernel<%d, %d, %s>"
_case("x2f K64 stats", "f32x2", "x2h", 1, 1, 64, 256, 32768, XF % (1, 1, "false"), 128, stats=True, knobs=S3)
_case("x2f K128 row bias 8", "f32x2", "x2h", 1, 1, 128, 256, 32768, XF % (1, 0, "false"), 128, rb=8, knobs=S3)
_case("x2f K192 row bias 16", "f32x2", "x2h", 1, 1, 192, 256, 32768, XF % (1, 1, "false"), 128, stats=True, rb=16, knobs=S3)
_case("x2f pro2", "f32x2", "x2h", 2, 1, 64, 256, 32768, XF % (2, 0, "true"), 128, bias=False, knobs=S3)
_case("x2f pro3 group 2", "f32x2", "x2h", 3, 1, 64, 256, 32768, XF % (3, 0, "true"), 128, bias=False, pool=2, knobs=S3)
_case("x2f pro3 group 16", "f32x2", "x2h", 3, 1, 128, 256, 32768, XF % (3, 0, "true"), 128, bias=False, pool=16, knobs=S3)
_case("x2f two tiles per workgroup", "f32x2", "x2h", 1, 2, 64, 256, 65536, XF % (1, 1, "false"), 256, stats=True, knobs=S3)
_case("x2f three tiles per workgroup", "f32x2", "x2h", 2, 1, 64, 512, 98304, XF % (2, 0, "true"), 256, bias=False, knobs=S3)
for _g in (16, 32, 64):
    _case("x2f fork %d" % _g, "f32x2", "x2h", 2, 1, 64 if _g != 32 else 128, 256, 32768, "gemm_x2f_fork_kernel", 128,
          bias=False, fork=_g, knobs=S3)
# narrow_fwd_kernel<OTW, PRO, STATS, RB>: its own minimum position counts
NF = "narrow_fwd_kernel<%d, %s, %s, %s>"
_case("narrow_fwd M64", "f32", "x2h", 1, 1, 64, 64, 196608, NF % (1, "true", "true", "false"), 768, stats=True, walk=768)
_case("narrow_fwd M128", "f32", "x2h", 1, 1, 64, 128, 131072, NF % (2, "true", "true", "false"), 512, stats=True, walk=512)
_case("narrow_fwd M64 pro0 wider", "f32", "x2h", 0, 1, 64, 64, 196640, NF % (1, "false", "false", "true"), 768, rb=32, wider=True)


def case_fixture(name):
    c = GEMM_CASES[name]
    o = c["opt"]
    M = c["M"]
    tile = 0
    if o.get("stats") and not o.get("walk"):
        tile = 256 if M <= 64 else 128                         # (usip_mlp_gemm_tiles)
    return gemm_fixture(c["form"], c["pro"], c["nb"], c["K"], M, c["P"], seed=len(name), bias=o.get("bias", True),
                        rb_group=o.get("rb", 0), stats_tile=tile, pool_group=o.get("pool", 0), fork_group=o.get("fork", 0),
                        x2r_stats=o.get("walk", 0) if o.get("stats") else 0, red_group=o.get("red"))


# ------------------------------------------------------------------------------------------------ the weight-gradient cases
WGRAD_CASES = {}


def _wcase(name, mode, form, pro, nb, M, N, P, kernel, big=False, **opt):
    sl, segs, tiles = (wgrad_x3_plan if big else wgrad_plan)(M, N, P, nb)
    WGRAD_CASES[name] = dict(name=name, mode=mode, form=form, pro=pro, nb=nb, M=M, N=N, P=P, kernel=kernel,
                             wgs=tiles * nb * segs, seglen=sl, segs=segs, opt=opt)


WG = "wgrad_kernel<%d, %d, %d, %s, %s>"
WB = "wgrad_bf16_kernel<%d, %d, %d, %s, %s, %d>"
_wcase("f32 128 tiles, many slices, short last segment", "f32", "x2h", 0, 1, 384, 200, 1040, WG % (2, 2, 0, "false", "true"))
_wcase("f32 64 tiles scalar path", "f32", "x2h", 2, 3, 33, 1, 333, WG % (1, 1, 2, "false", "false"))
_wcase("f32 one slice", "f32", "x3", 0, 1, 1, 129, 48, WG % (2, 2, 0, "false", "true"))
_wcase("f32 two slices coloff", "f32", "x2h", 2, 1, 129, 130, 128, WG % (2, 2, 2, "true", "true"), xpro=True, coloff=3)
_wcase("f32 pooled", "f32", "x2h", 3, 2, 129, 64, 512, WG % (2, 2, 3, "true", "true"), xpro=True, pool=16)
_wcase("bf16", "bf16", "a", 0, 1, 129, 130, 256, WB % (2, 2, 0, "false", "true", 1))
_wcase("bf16 pro2 scalar", "bf16", "a", 2, 1, 40, 33, 333, WB % (1, 1, 2, "false", "false", 1))
_wcase("x3 128 tiles", "f32x3", "x3", 0, 1, 129, 100, 1040, WB % (2, 2, 0, "false", "true", 3), knobs=S3)
_wcase("x3 128 tiles pro2", "f32x3", "x3", 2, 2, 100, 129, 240, WB % (2, 2, 2, "true", "true", 3), knobs=S3, xpro=True)
_wcase("x3 256 tiles", "f32x3", "x3", 0, 1, 384, 200, 1040, "wgrad_x3_kernel<0, false, 3>", big=True, knobs=S3, coloff=5)
_wcase("x3 256 tiles xpro pro2", "f32x3", "x3", 2, 2, 200, 384, 528, "wgrad_x3_kernel<2, true, 3>", big=True, knobs=S3, xpro=True)
_wcase("x3 256 tiles pooled", "f32x3", "x3", 3, 1, 200, 129, 512, "wgrad_x3_kernel<3, false, 3>", big=True, knobs=S3, pool=16)
_wcase("x2l pro2", "f32x2", "x2h", 2, 1, 384, 200, 1040, "wgrad_x2l_kernel<2>", big=True, knobs=S3, xpro=True)
_wcase("x2l pooled", "f32x2", "x2h", 3, 2, 200, 129, 512, "wgrad_x2l_kernel<3>", big=True, knobs=S3, xpro=True, pool=16)
_wcase("x2h half-line predecessor", "f32x2", "x2h", 2, 1, 200, 384, 528, "wgrad_x3_kernel<2, true, 2>", big=True,
       knobs={"gemm_split3": 2, "r5_forms": 1}, xpro=True)


def wgrad_case_fixture(name):
    c = WGRAD_CASES[name]
    o = c["opt"]
    return wgrad_fixture(c["form"], c["pro"], c["nb"], c["M"], c["N"], c["P"], seed=len(name), pool_group=o.get("pool", 0),
                         xpro=o.get("xpro", False))
