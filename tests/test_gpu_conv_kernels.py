"""The convolution path's hand-written kernels and BiasNorm alone, against float64.

glu_dwconv1d_kernel<7 | 15 | 31> (f32 with the GLU, f32 and bf16 after it), conv1_kernel (libm,
native, native with bf16 out), convnext_dw_kernel<float, 32> and <__bf16, 64>,
convnext_mlp_kernel, convnext_mlp_h3_kernel and bias_norm_kernel<1 | 2 | 4> run through
zasr_selftest_dwconv1d / _conv1 / _convnext / _bias_norm on seeded host operands: ragged
batches given as per-sequence lengths, offsets and row maps built as a decode builds them, the
launch call a decode makes, one guard row behind every output.  The references are
tests/conv_reference.py (float64, sequence by sequence; held to torch and the oracle by
tests/test_conv_reference.py, which also asserts which block paths the fixtures below meet).

Fixtures (conv_reference.py): the depthwise conv1d over L = [1, 7, 56, 3, 200, 64, 31, 130]
(492 rows: a one-frame sequence, sequences shorter than the half-window, a boundary on a tile
edge and one three rows past it, interior tiles at every compiled K, a 44-row tail), [1] and
[5]; d = 36 / 64 / 96 (a partial channel block, an exact one, a 32-channel tail block);
Kr = 5, 7, 9, 15, 17, 31 (each instantiation exact and zero-padded).  conv.0 over
T = [3, 4, 10, 35, 9] (51 output rows, 4080 elements: a partial last block; every sequence
shifts the two levels by 2).  ConvNeXt over L = [1, 2, 16, 3, 40, 7, 33] (102 rows: interior
tiles 32-47 and 80-95, a 6-row tail, 1938 = 15 * 128 + 18 MLP positions) and [1] (19
positions).  BiasNorm at d = 4 .. 1024 across the three instantiations, 1 .. 9 rows.

Bounds, per output element, derived (not tuned), u = 2^-24:

    depthwise sums          (n + 2) u S     n taps (Kr, 9, 49), S = |b| + sum |w| |x|: the taps
                                            are sequential fmaf's from the bias, so the
                                            step-wise bound (n roundings) holds undoubled
    GLU input g = a sig(s)  e_g = |a| 1e-6 + u |g|, carried through the conv as sum |w| e_g
    SwooshR / SwooshL       slope below 1: the pre-activation bound passes unchanged;
                            native forms + 1e-6 (common.h's "~1e-7" with tests/test_gpu_gemm.py's
                            margin); libm forms + 4 u (softplus(v - c) + 0.08 |v| + k), the
                            magnitudes of their three terms
    bf16 output             + 2^-8 |out|; bf16 inputs are generated bf16-representable and the
                            reference reads the same values
    BiasNorm                the squares are non-negative, so any summation order leaves a
                            relative error of at most (d + 4) u on the sum, (d / 2 + 8) u |r| on
                            the result r with the division, square root and products; through
                            the blend o + (r - o) s: that times s, + 3 u (|o| + |r|)
    convnext_mlp_kernel     the worst case lets every hidden value flip its bf16 rounding and
                            says nothing; the project's bound for the same arithmetic
                            (tests/test_gpu_kernels_bf16.py): 2e-3 max |o| over the MLP output o
                            of the call, + 2^-8 |out| for the bf16 store; the reference reads the
                            device's own y and rounds the weights and the hidden layer to bf16
    convnext_mlp_h3_kernel  3e-6 max |ref| (tests/test_gpu_kernels_h3.py), on the device's own y

The BiasNorm images written by one launch (x, the copy, the copy over orig) are bit-equal, and
so is x whether or not a copy is written.  Each test prints its worst |got - ref| / bound.

Measured on an MI355X, worst ratio over each test's cases (profiles/conv_kernels/README.md has
every line); no bound was changed after the measurement:

    dwconv1d f32 with the GLU    0.066 - 0.106     f32 after the GLU    0.102 - 0.236
    dwconv1d bf16                0.987 - 0.995     (the bound there is the bf16 rounding itself)
    conv1 libm / native / bf16   0.205 / 0.223 / 0.987
    convnext y  f32              0.095 (102 rows), 0.049 (1 row);   bf16   0.993, 0.986
    convnext out  bf16 MLP       0.813, 0.897       f16x3 MLP    0.039, 0.015
    bias_norm                    0.005 - 0.238 plain, 0.158 - 0.219 with the blend
"""
import zlib

import numpy as np
import pytest

import conv_reference as cr
from conftest import gpu_available

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ACT_ABS = 1e-6
U_BF16 = 2.0 ** -8
MLP_BF16_BOUND = 2e-3
MLP_H3_BOUND = 3e-6


@pytest.fixture(scope="module")
def need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def rne_bf16(x):
    """float32 -> the nearest-even bfloat16, returned as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def worst_ratio(got, ref, bound):
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.all(np.isfinite(got))
    return float(np.max(np.abs(got.astype(np.float64) - ref) / bound))


# ---------------- ConvolutionModule: GLU -> depthwise conv1d -> SwooshR ----------------
DW1_VARIANTS = ("f32_glu", "f32_post_glu", "bf16_post_glu")


def dw1_case(variant, L, d, Kr):
    from zasr.binding import selftest_dwconv1d
    rng = rng_for("dw1", variant, tuple(L), d, Kr)
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    rows = sum(L)
    w = f(d, Kr) * np.float32(1.5 / np.sqrt(Kr))  # pre-activations of about [-6, 6]
    b = f(d) * np.float32(0.5)
    glu, h16 = variant == "f32_glu", variant == "bf16_post_glu"
    x = f(rows, 2 * d) * np.float32(1.5) if glu else f(rows, d)
    if h16:
        x = rne_bf16(x)
    got = selftest_dwconv1d(L, x, w, b, glu=glu, bf16=h16)
    w64, b64, x64 = w.astype(np.float64), b.astype(np.float64), x.astype(np.float64)
    g = cr.glu(x64) if glu else x64
    pre = cr.dwconv1d(g, L, w64, b64)
    bound = (Kr + 2) * U * cr.dwconv1d(np.abs(g), L, np.abs(w64), np.abs(b64))
    if glu:
        e_g = np.abs(x64[:, :d]) * ACT_ABS + U * np.abs(g)
        bound = bound + cr.dwconv1d(e_g, L, np.abs(w64), np.zeros(d))
    ref = cr.swoosh_r(pre)
    bound = bound + ACT_ABS
    if h16:
        bound = bound + U_BF16 * np.abs(ref)
    return worst_ratio(got, ref, bound), float(np.max(np.abs(pre)))


@pytest.mark.parametrize("Kr", cr.DW1_KERNEL_SIZES)
@pytest.mark.parametrize("variant", DW1_VARIANTS)
def test_dwconv1d_matches_f64(need_gpu, variant, Kr):
    bad, worst, span = [], 0.0, 0.0
    for L in cr.DW1_LENGTHS:
        for d in cr.DW1_WIDTHS:
            r, m = dw1_case(variant, L, d, Kr)
            worst, span = max(worst, r), max(span, m)
            if not r <= 1.0:
                bad.append((L, d, r))
    print(f"dwconv1d {variant} Kr={Kr} (K={cr.compiled_k(Kr)}): worst |got - ref| / bound = "
          f"{worst:.3f} (max |pre-activation| {span:.1f})")
    assert not bad, bad


def test_dwconv1d_refuses_glu_with_bf16(need_gpu):
    from zasr.binding import ZasrError, selftest_dwconv1d
    z = np.zeros
    with pytest.raises(ZasrError):
        selftest_dwconv1d([5], z((5, 8)), z((4, 7)), z(4), glu=True, bf16=True)
    with pytest.raises(ZasrError):  # an even kernel size
        selftest_dwconv1d([5], z((5, 4)), z((4, 6)), z(4), glu=False)
    assert dw1_case("f32_post_glu", [5], 36, 7)[0] <= 1.0  # not sticky


# ---------------- conv.0 + SwooshR ----------------
CONV1_FORMS = {0: "libm", 1: "native", 2: "native_bf16"}


@pytest.mark.parametrize("form", sorted(CONV1_FORMS), ids=[CONV1_FORMS[k] for k in sorted(CONV1_FORMS)])
def test_conv1_matches_f64(need_gpu, form):
    from zasr.binding import selftest_conv1
    T = cr.CONV1_FRAMES
    rng = rng_for("conv1", form)
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    fb, w, b = f(sum(T), 80) * np.float32(1.5), f(8, 9) / np.float32(3.0), f(8) * np.float32(0.5)
    got = selftest_conv1(T, fb, w, b, form)
    fb64, w64, b64 = (v.astype(np.float64) for v in (fb, w, b))
    pre = cr.conv0(fb64, T, w64, b64)
    bound = (9 + 2) * U * cr.conv0(np.abs(fb64), T, np.abs(w64), np.abs(b64))
    ref = cr.swoosh_r(pre)
    if form == 0:
        bound = bound + 4 * U * (np.logaddexp(0.0, pre - 1.0) + 0.08 * np.abs(pre) + 0.313261687)
    else:
        bound = bound + ACT_ABS
    if form == 2:
        bound = bound + U_BF16 * np.abs(ref)
    r = worst_ratio(got, ref, bound)
    print(f"conv1 {CONV1_FORMS[form]}: worst |got - ref| / bound = {r:.3f} "
          f"(max |pre-activation| {np.max(np.abs(pre)):.1f})")
    assert r <= 1.0, r


# ---------------- ConvNeXt: depthwise 7x7, pointwise MLP + residual ----------------
CNX_FORMS = {0: "dw_f32", 1: "bf16", 2: "f16x3"}


def cnx_operands(L, form):
    rng = rng_for("convnext", tuple(L), form)
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    o = dict(x=f(sum(L), 19, 128), dw_w=f(128, 7, 7) / np.float32(7.0), dw_b=f(128) * np.float32(0.3),
             w1=f(384, 128) * np.float32(2.0 / np.sqrt(128)), b1=f(384) * np.float32(0.5),
             w2=f(128, 384) / np.float32(np.sqrt(384)), b2=f(128) * np.float32(0.1))
    if form == 1:
        o["x"] = rne_bf16(o["x"])
    return o


@pytest.mark.parametrize("L", cr.CNX_LENGTHS, ids=lambda L: f"rows{sum(L)}")
@pytest.mark.parametrize("form", sorted(CNX_FORMS), ids=[CNX_FORMS[k] for k in sorted(CNX_FORMS)])
def test_convnext_matches_f64(need_gpu, form, L):
    from zasr.binding import selftest_convnext
    o = cnx_operands(L, form)
    mlp = {} if form == 0 else {k: o[k] for k in ("w1", "b1", "w2", "b2")}
    y, out = selftest_convnext(L, o["x"], o["dw_w"], o["dw_b"], form=form, **mlp)
    x64, w64, b64 = (o[k].astype(np.float64) for k in ("x", "dw_w", "dw_b"))
    y_ref = cr.dwconv7x7(x64, L, w64, b64)
    y_bound = (49 + 2) * U * cr.dwconv7x7(np.abs(x64), L, np.abs(w64), np.abs(b64))
    if form == 1:
        y_bound = y_bound + U_BF16 * np.abs(y_ref)
    ry = worst_ratio(y, y_ref, y_bound)
    print(f"convnext {CNX_FORMS[form]} rows={sum(L)}: y worst |got - ref| / bound = {ry:.3f}")
    assert ry <= 1.0, ry
    if form == 0:
        assert out is None
        return
    # the MLP on the device's own y, so the two kernels' errors do not compound
    yd = y.astype(np.float64)
    b1, b2 = o["b1"].astype(np.float64), o["b2"].astype(np.float64)
    if form == 1:
        hid = lambda h: rne_bf16(h.astype(np.float32)).astype(np.float64)
        mo = cr.convnext_mlp(yd, rne_bf16(o["w1"]), b1, rne_bf16(o["w2"]), b2, hidden=hid)
        ref = x64 + mo
        bound = MLP_BF16_BOUND * np.max(np.abs(mo)) + U_BF16 * np.abs(ref)
    else:
        ref = x64 + cr.convnext_mlp(yd, o["w1"], b1, o["w2"], b2)
        bound = np.full(ref.shape, MLP_H3_BOUND * np.max(np.abs(ref)))
    ro = worst_ratio(out, ref, bound)
    print(f"convnext {CNX_FORMS[form]} rows={sum(L)}: out worst |got - ref| / bound = {ro:.3f}")
    assert ro <= 1.0, ro


# ---------------- BiasNorm (+ the bypass blend, + the copy for the next layer) ----------------
def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("d", cr.BN_WIDTHS)
def test_bias_norm_matches_f64(need_gpu, d):
    from zasr.binding import selftest_bias_norm
    worst_plain = worst_blend = 0.0
    for rows in cr.BN_ROWS:
        rng = rng_for("bias_norm", d, rows)
        f = lambda *s: rng.standard_normal(s, dtype=np.float32)
        x, bias, orig = f(rows, d) * np.float32(1.5), f(d) * np.float32(0.3), f(rows, d)
        s = rng.uniform(0.3, 0.9, d).astype(np.float32)
        ls = float(np.float32(rng.uniform(-0.5, 0.5)))
        # without the blend (the front end's out_norm), with and without a copy
        plain = selftest_bias_norm(x, bias, ls)
        plain_c = selftest_bias_norm(x, bias, ls, copy_mode=1)
        ref, r = cr.bias_norm(x, bias, ls)
        e_r = (d / 2 + 8) * U * np.abs(r)
        worst_plain = max(worst_plain, worst_ratio(plain["x"], ref, e_r))
        assert plain["orig"] is None and plain["copy"] is None
        assert same_bits(plain_c["x"], plain["x"]) and same_bits(plain_c["copy"], plain["x"])
        # with the blend (a layer's end): no copy, a separate copy, the copy over orig
        m0 = selftest_bias_norm(x, bias, ls, orig, s, copy_mode=0)
        m1 = selftest_bias_norm(x, bias, ls, orig, s, copy_mode=1)
        m2 = selftest_bias_norm(x, bias, ls, orig, s, copy_mode=2)
        ref, r = cr.bias_norm(x, bias, ls, orig, s)
        o64 = orig.astype(np.float64)
        bound = (d / 2 + 8) * U * np.abs(r) * s.astype(np.float64) + 3 * U * (np.abs(o64) + np.abs(r))
        worst_blend = max(worst_blend, worst_ratio(m0["x"], ref, bound))
        assert same_bits(m0["orig"], orig) and same_bits(m1["orig"], orig)  # read only
        assert same_bits(m1["x"], m0["x"]) and same_bits(m2["x"], m0["x"])
        assert same_bits(m1["copy"], m0["x"]) and same_bits(m2["orig"], m0["x"])
        assert m0["copy"] is None and m2["copy"] is None
    print(f"bias_norm d={d} (NQ={cr.bias_norm_nq(d)}): worst |got - ref| / bound = "
          f"{worst_plain:.3f} plain, {worst_blend:.3f} with the blend")
    assert worst_plain <= 1.0 and worst_blend <= 1.0, (worst_plain, worst_blend)
