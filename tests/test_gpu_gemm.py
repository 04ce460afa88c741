"""The general projection GEMMs alone, against a float64 product.

gemm_f32, gemm_bf16 and gemm_x3 run through zasr_selftest_gemm on seeded host operands: one
call of the public entry point per case, weights prepared as the loader prepares them, the
kernel reached by shape as in a decode (no route override).

Edge shapes (M, N, K), every epilogue of every mode over all of them.  The tile pick
(launch_tile / launch_tile_h / launch_x3 / launch_h3) takes BN = 32 for N = 4, 68, 132,
BN = 64 for N = 36, 272 and BN = 128 for N = 128 (gemm_bf16's multiply epilogues: 64 instead of
32 above N = 64); every row count below 16384 and block count below 512 keeps the 64-row tile;
DEEP is the two-slab path (K % 64 == 0 for gemm_bf16 and bf16x3, K % 32 == 0 for the others).

    (  1,   4, 40)  BN 32, partial K slab, one row
    ( 31,  36, 40)  BN 64, partial K slab
    ( 33,  68, 96)  BN 32; DEEP except gemm_bf16 / bf16x3
    ( 65, 128, 64)  BN 128, DEEP; bf16 C: the paired-fragment store (also at (129, 128, 40))
    (127, 132, 64)  BN 32, DEEP
    (129, 272, 96)  BN 64; f16x3: gemm_glds_h3_kernel, 64-wide tile (M >= 128, K % 32 == 0)
    (129, 128, 40)  BN 128, partial slab; f16x3: K % 32 != 0 -> the register-staged gemm_x3_kernel
    (129,  68, 64)  BN 32, DEEP; f16x3: gemm_glds_h3_kernel, 128-wide tile
    ( 65,  36, 64)  BN 64, DEEP

so each mode meets every (BN, DEEP) pair, and every shape but N = 128 has a column tail and
every M a row tail of the 64-row tile.  EPI_GLU writes N / 2 columns with ldc = N / 2, which the
entry points take for N % 8 == 0 only: its shapes use N = 40 (BN 64), 72 (BN 32), 128, 272.

Dispatch branches the edge shapes cannot reach (DISPATCH_CASES):

    fp32   (65537, 128,   64) RESADD           gemm_f32_kernel<128, 128> (512+ blocks: big), DEEP
    bf16   (65537, 128,   64) RESADD + bypass  gemm_bf16_kernel<128, 128>, DEEP
    bf16   (32769, 256,   64) f32 -> bf16      gemm_bf16_kernel<128, 256> on 8 waves, paired store
    bf16x3 / bf16x6 (65537, 128, 64)           gemm_x3_kernel<128, 128>, DEEP
    f16x3  (65537, 128,   40)                  gemm_x3_kernel<128, 128, FMT 1> (K % 32 != 0)
    bf16   (129, 128 | 132, 1024) bf16 A       try_glds -> gemm_glds_kernel<4>
    bf16   (16389, 384,  384) bf16 A, RESADD   kTuned TT_GLDS3 -> gemm_glds_kernel<3>
    bf16   (16389, 192, 2432) bf16 A           kTuned TT_GLDS3_192 -> gemm_glds_kernel<3, BN 192>
    bf16   (16389, 272,  256) f32 -> bf16      kTuned TT_256x128 -> gemm_bf16_kernel<256, 128>, 8 waves

Bound, per output element, derived (not tuned), with u = 2^-24 and S = |A'| |W'|^T + |bias|
(primes: the operands as the kernel sees them; the bf16 mode's reference uses the operands
rounded to bf16, nearest even):

    pre-activation value      (u_op + 2 K u) S    u_op = 0 (fp32, bf16), 2^-15 (bf16x3),
                                                  2^-22 (bf16x6), 2^-21 (f16x3)
    fast SwooshL / SwooshR    + 1e-6             (slope below 1; gemm_f32's libm forms: + 0)
    GELU (gemm_f32, erff)     x 1.13             (its largest slope)
    RESADD                    unchanged
    bypass  o + (x - o) k     x k
    MULAUX                    x |aux|;  MULAUX16 (aux rounded on the host): + 2^-8 |out|
    GLU  a sigmoid(b)         e_a sigmoid(b) + |a| (e_b / 4 + 1e-6)
    bf16 C                    + 2^-8 |out|

2 K u is the worst-case f32 summation bound (K - 1 additions and the bias add), doubled because
the MFMA's inner sum is not step-wise IEEE; u_op follows from the formats (gemm_x3.hip's and
gemm_dev.h's headers: two bf16 pieces leave 2^-17 per operand and drop a 2^-18 product; three
pieces and the fp16 pair keep 22+ bits per operand).  1e-6 is the native exp2 / log / rcp
forms' "~1e-7" (common.h) with margin.  The epilogue's own few f32 roundings get no term: the
base bound is carried through them in float64 and covers them with room (measured on the
kernels before the shared epilogue: every f32-C ratio at most 0.17, the bf16-C ones up to 0.99,
where the bound is the bf16 rounding itself).  Each test prints its worst |got - ref| / bound.
"""
import math
import zlib
from collections import namedtuple

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

EPI = dict(NONE=0, SWOOSHL=1, SWOOSHR=2, RESADD=3, MULAUX=4, MULAUX16=5, RELU=6, GELU=7, GLU=8)
U = 2.0 ** -24
U_OP = {"fp32": 0.0, "bf16": 0.0, "bf16x3": 2.0 ** -15, "bf16x6": 2.0 ** -22, "f16x3": 2.0 ** -21}
ACT_ABS = 1e-6
U_BF16 = 2.0 ** -8

# epi: an EPI name, or "BYPASS" = RESADD with the bypass_mid operands
Case = namedtuple("Case", "mode a16 c16 epi M N K")

SHAPES = [(1, 4, 40), (31, 36, 40), (33, 68, 96), (65, 128, 64), (127, 132, 64), (129, 272, 96),
          (129, 128, 40), (129, 68, 64), (65, 36, 64)]
GLU_SHAPES = [(1, 72, 40), (31, 40, 64), (33, 128, 96), (65, 272, 64), (127, 72, 64),
              (129, 272, 96), (129, 128, 40), (129, 40, 64)]
SPLIT_EPIS = ["NONE", "SWOOSHL", "SWOOSHR", "RESADD", "BYPASS", "MULAUX", "GLU"]
CONFIGS = [
    ("fp32", 0, 0, ["NONE", "SWOOSHL", "SWOOSHR", "RESADD", "RELU", "GELU", "MULAUX"]),
    ("bf16", 0, 0, ["NONE", "SWOOSHL", "SWOOSHR", "RESADD", "BYPASS"]),
    ("bf16", 0, 1, ["NONE", "SWOOSHL", "GLU"]),
    ("bf16", 1, 0, ["NONE", "RESADD", "BYPASS"]),
    ("bf16", 1, 1, ["NONE", "MULAUX", "MULAUX16"]),
    ("bf16x3", 0, 0, SPLIT_EPIS),
    ("bf16x6", 0, 0, SPLIT_EPIS),
    ("f16x3", 0, 0, SPLIT_EPIS),
]
EDGE_GROUPS = [(m, a, c, e) for m, a, c, epis in CONFIGS for e in epis]
DISPATCH_CASES = [
    Case("fp32", 0, 0, "RESADD", 65537, 128, 64),
    Case("bf16", 0, 0, "BYPASS", 65537, 128, 64),
    Case("bf16", 0, 1, "SWOOSHL", 32769, 256, 64),
    Case("bf16x3", 0, 0, "BYPASS", 65537, 128, 64),
    Case("bf16x6", 0, 0, "BYPASS", 65537, 128, 64),
    Case("f16x3", 0, 0, "BYPASS", 65537, 128, 40),
    Case("bf16", 1, 0, "BYPASS", 129, 128, 1024),
    Case("bf16", 1, 0, "NONE", 129, 132, 1024),
    Case("bf16", 1, 0, "RESADD", 16389, 384, 384),
    Case("bf16", 1, 0, "NONE", 16389, 192, 2432),
    Case("bf16", 0, 1, "NONE", 16389, 272, 256),
]


def group_cases(mode, a16, c16, epi):
    return [Case(mode, a16, c16, epi, *s) for s in (GLU_SHAPES if epi == "GLU" else SHAPES)]


def all_cases():
    return [c for g in EDGE_GROUPS for c in group_cases(*g)] + DISPATCH_CASES


def case_id(c):
    t = {(0, 0): "", (0, 1): "_f32bf16", (1, 0): "_bf16f32", (1, 1): "_bf16bf16"}[(c.a16, c.c16)]
    return f"{c.mode}{t if c.mode == 'bf16' else ''}_{c.epi}_M{c.M}_N{c.N}_K{c.K}"


def rne_bf16(x):
    """float32 -> the nearest-even bfloat16, returned as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def operands(c):
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    o = dict(A=f(c.M, c.K), W=f(c.N, c.K) / np.float32(math.sqrt(c.K)), bias=f(c.N) * np.float32(0.1),
             C0=f(c.M, c.N // 2 if c.epi == "GLU" else c.N), aux=None, bo=None, ks=None)
    if c.epi in ("MULAUX", "MULAUX16"):
        o["aux"] = f(c.M, c.N)
    if c.epi == "BYPASS":
        o["bo"] = f(c.M, c.N)
        o["ks"] = rng.uniform(0.3, 0.9, c.N).astype(np.float32)
    return o


def run(c, o, lib_path=None):
    from zasr.binding import selftest_gemm
    epi = EPI["RESADD" if c.epi == "BYPASS" else c.epi]
    return selftest_gemm(c.mode, o["A"], o["W"], o["bias"], o["C0"], epi, bool(c.a16), bool(c.c16),
                         o["aux"], o["bo"], o["ks"], lib_path=lib_path)


_erf = np.vectorize(math.erf, otypes=[np.float64])


def _swoosh(v, e, c, k, fast):
    return np.logaddexp(0.0, v - c) - 0.08 * v - k, e + (ACT_ABS if fast else 0.0)


def reference(c, o):
    """(float64 reference, per-element bound): the module docstring's table."""
    A, W = (rne_bf16(o["A"]), rne_bf16(o["W"])) if c.mode == "bf16" else (o["A"], o["W"])
    A, W, b = A.astype(np.float64), W.astype(np.float64), o["bias"].astype(np.float64)
    v = A @ W.T + b
    e = (U_OP[c.mode] + 2 * c.K * U) * (np.abs(A) @ np.abs(W).T + np.abs(b))
    if c.epi == "SWOOSHL":
        v, e = _swoosh(v, e, 4.0, 0.035, c.mode != "fp32")
    elif c.epi == "SWOOSHR":
        v, e = _swoosh(v, e, 1.0, 0.313261687, c.mode != "fp32")
    elif c.epi == "RELU":
        v = np.maximum(v, 0.0)
    elif c.epi == "GELU":
        v, e = 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0))), 1.13 * e
    elif c.epi in ("MULAUX", "MULAUX16"):
        x = (rne_bf16(o["aux"]) if c.epi == "MULAUX16" else o["aux"]).astype(np.float64)
        v = v * x
        e = e * np.abs(x) + (U_BF16 * np.abs(v) if c.epi == "MULAUX16" else 0.0)
    elif c.epi in ("RESADD", "BYPASS"):
        v = o["C0"].astype(np.float64) + v
        if c.epi == "BYPASS":
            bo, k = o["bo"].astype(np.float64), o["ks"].astype(np.float64)
            v, e = bo + (v - bo) * k, e * k
    elif c.epi == "GLU":
        a, g, ea, eg = v[:, 0::2], v[:, 1::2], e[:, 0::2], e[:, 1::2]
        s = 1.0 / (1.0 + np.exp(-g))
        v = a * s
        e = ea * s + np.abs(a) * (0.25 * eg + ACT_ABS)
    if c.c16:
        e = e + U_BF16 * np.abs(v)
    return v, e


def check(c):
    o = operands(c)
    got = run(c, o)
    ref, bound = reference(c, o)
    assert got.shape == ref.shape
    ratio = float(np.max(np.abs(got.astype(np.float64) - ref) / bound))
    print(f"{case_id(c)}: worst |got - ref| / bound = {ratio:.3f}")
    return ratio


@pytest.fixture(scope="module")
def need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("group", EDGE_GROUPS, ids=["{}_a{}c{}_{}".format(*g) for g in EDGE_GROUPS])
def test_gemm_edge_shapes_match_f64(need_gpu, group):
    bad = [(case_id(c), r) for c in group_cases(*group) for r in [check(c)] if not r <= 1.0]
    assert not bad, bad


@pytest.mark.parametrize("case", DISPATCH_CASES, ids=[case_id(c) for c in DISPATCH_CASES])
def test_gemm_dispatch_branches_match_f64(need_gpu, case):
    r = check(case)
    assert r <= 1.0, (case_id(case), r)


REFUSED = [
    Case("fp32", 0, 0, "GLU", 33, 128, 64),       # gemm_f32 has no GLU epilogue
    Case("fp32", 0, 0, "MULAUX16", 33, 128, 64),  # bf16 aux: gemm_bf16 only
    Case("fp32", 0, 0, "NONE", 33, 128, 42),      # K % 4
    Case("bf16", 0, 0, "MULAUX", 33, 128, 64),    # the multiply epilogues take bf16 A and C
    Case("bf16", 0, 1, "RESADD", 33, 128, 64),    # the residual stream is f32
    Case("bf16", 0, 0, "NONE", 33, 130, 64),      # N % 4
    Case("bf16", 0, 0, "NONE", 33, 128, 36),      # K % 8
    Case("bf16", 0, 1, "GLU", 33, 36, 64),        # ldc = N / 2 must be a multiple of 4
    Case("bf16x3", 0, 0, "RELU", 33, 128, 64),    # gemm_x3 has no RELU epilogue
    Case("bf16x6", 0, 0, "GLU", 33, 68, 64),      # ldc = N / 2 must be a multiple of 4
    Case("f16x3", 0, 0, "NONE", 33, 128, 36),     # K % 8
    Case("f16x3", 0, 1, "NONE", 33, 128, 64),     # bf16 C outside the bf16 mode
]


@pytest.mark.parametrize("case", REFUSED, ids=[case_id(c) for c in REFUSED])
def test_gemm_refused_combinations_report_an_error(need_gpu, case):
    from zasr.binding import ZasrError
    with pytest.raises(ZasrError):
        run(case, operands(case))
    # the refusal is not sticky: a valid problem still runs
    assert check(Case("fp32", 0, 0, "NONE", 1, 4, 40)) <= 1.0
