"""The fused FeedforwardModule kernels out of place (a layer's feed_forward1: read the layer
input, write the layer's X, leave the input as the bypass operand) against the same kernels in
place, through zasr_selftest_ffn_bf16_oop / zasr_selftest_ffn_h3_oop and the in-place entries.

bf16: ffn_fused_kernel (D = 192), ffn_wide_kernel (256, 384, 512) and the opt-in rows form
ffn_rows_kernel (384, form 1).  f16x3: ffn_wide_h3_kernel at D = 128, 192, 256, 384, 512.
R in {1, 63, 64, 65, 130}: one row, either side of the 32- and 64-token tiles, a tail after
two tiles.  With and without the bypass_mid operands; F = 128.

Held: the output buffer equals the in-place result bit for bit (no row of it keeps its
initial contents), and the input buffer is unchanged.
"""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 130)
F = 128


@pytest.fixture(scope="module")
def need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _operands(D, seed):
    rng = np.random.default_rng(seed)
    W1 = (rng.standard_normal((F, D)) / np.sqrt(D)).astype(np.float32)
    W2 = (rng.standard_normal((D, F)) / np.sqrt(F)).astype(np.float32)
    b1 = rng.standard_normal(F).astype(np.float32) * 0.5
    b2 = rng.standard_normal(D).astype(np.float32) * 0.1
    ks = rng.uniform(0.3, 0.9, D).astype(np.float32)
    return rng, W1, b1, W2, b2, ks


def _check(kind, D, byp, form=0):
    from zasr.binding import selftest_ffn_bf16, selftest_ffn_h3, selftest_ffn_oop
    rng, W1, b1, W2, b2, ks = _operands(D, 4200 + D + 3 * byp + 11 * form + (kind == "h3"))
    for R in ROWS:
        X = rng.standard_normal((R, D)).astype(np.float32)
        bo = rng.standard_normal((R, D)).astype(np.float32) if byp else None
        bs = ks if byp else None
        if kind == "bf16":
            want = selftest_ffn_bf16(W1, b1, W2, b2, X, bo, bs, form=form)
        else:
            want = selftest_ffn_h3(X, W1, b1, W2, b2, X, bo, bs)
        out, xin = selftest_ffn_oop(kind, W1, b1, W2, b2, X, bo, bs, form=form)
        what = f"{kind} D={D} R={R} byp={byp} form={form}"
        assert not np.array_equal(_bits(want), _bits(X)), what  # the FFN did something
        np.testing.assert_array_equal(_bits(out), _bits(want), err_msg=what)
        np.testing.assert_array_equal(_bits(xin), _bits(X), err_msg=what)


@pytest.mark.parametrize("byp", [False, True], ids=["plain", "byp"])
@pytest.mark.parametrize("D", [192, 256, 384, 512])
def test_ffn_bf16_out_of_place_equals_in_place(need_gpu, D, byp):
    _check("bf16", D, byp)


@pytest.mark.parametrize("byp", [False, True], ids=["plain", "byp"])
def test_ffn_bf16_rows_form_out_of_place(need_gpu, byp):
    _check("bf16", 384, byp, form=1)


@pytest.mark.parametrize("byp", [False, True], ids=["plain", "byp"])
@pytest.mark.parametrize("D", [128, 192, 256, 384, 512])
def test_ffn_h3_out_of_place_equals_in_place(need_gpu, D, byp):
    _check("h3", D, byp)
