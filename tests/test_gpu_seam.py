"""The fused stack seam (csrc/encoder_kernels.hip seam_kernel) against the three kernels it
replaces -- stack_glue -> downsample(next stack) -> downsample(full-dim output, 2) -- on the same
host operands through zasr_selftest_seam.

One ragged batch with 50 Hz lengths L in {1, 2, 3, 7, 8, 9, 15, 16, 17}: L below the stack's and
the next stack's factor, L no multiple of either, an output pair straddling a sequence's end.
Stack factor ds in {1, 2, 4, 8}, next stack's in {2, 4, 8, none}, widths 64 -> 96 (zero pad),
128 -> 96 (truncate), 64 -> 64, output columns [c0, d) with c0 = 0 and c0 > 0, plus the last
seam (no next stack) and a seam that owns no output columns.

Held: `next`, the next stack's X and the output columns equal the composition's bit for bit,
and output columns outside [c0, d) keep what they held.  (A float64 evaluation of the same
formulas guards against both sides being wrong together.)
"""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

LENS = np.array([1, 2, 3, 7, 8, 9, 15, 16, 17], dtype=np.int32)
FILL = -777.25
LDO = 128


@pytest.fixture(scope="module")
def need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _operands(d, ds, seed):
    rng = np.random.default_rng(seed)
    rows = int(LENS.sum())
    rs = int(((LENS + ds - 1) // ds).sum())
    orig = rng.standard_normal((rows, d)).astype(np.float32)
    xd = rng.standard_normal((rs, d)).astype(np.float32)
    s = rng.uniform(0.1, 0.9, d).astype(np.float32)
    wn = np.zeros(8, np.float32)
    wn[:] = rng.uniform(0.05, 0.4, 8)
    wo = rng.uniform(0.3, 0.7, 2).astype(np.float32)
    return orig, xd, s, wn, wo


def _downsample64(y, lens, f, w):
    out, base = [], 0
    for L in lens:
        for tp in range((L + f - 1) // f):
            idx = [base + min(tp * f + u, L - 1) for u in range(f)]
            out.append(sum(float(w[u]) * y[i] for u, i in enumerate(idx)))
        base += L
    return np.array(out)


def _reference64(orig, xd, s, ds, dn, ds_next, wn, wo):
    """float64: y, next (width dn), the next stack's X, the 25 Hz output (width d)."""
    d = orig.shape[1]
    y = orig.astype(np.float64).copy()
    if ds > 1:
        base = bs = 0
        for L in LENS:
            for t in range(L):
                up = xd[bs + t // ds].astype(np.float64)
                y[base + t] = y[base + t] + (up - y[base + t]) * s
            base += L
            bs += (L + ds - 1) // ds
    nxt = np.zeros((y.shape[0], dn))
    nxt[:, :min(d, dn)] = y[:, :min(d, dn)]
    xn = _downsample64(nxt, LENS, ds_next, wn) if ds_next > 1 and dn else None
    return nxt, xn, _downsample64(y, LENS, 2, wo)


def _check(d, ds, dn, ds_next, c0, seed):
    from zasr.binding import selftest_seam
    orig, xd, s, wn, wo = _operands(d, ds, seed)
    r = selftest_seam(LENS, d, ds, dn, ds_next, c0, LDO, xd if ds > 1 else None, orig,
                      s if ds > 1 else None, wn, wo, fill=FILL)
    what = f"d={d} ds={ds} dn={dn} ds_next={ds_next} c0={c0}"
    np.testing.assert_array_equal(_bits(r["next"]), _bits(r["next_ref"]), err_msg=what)
    np.testing.assert_array_equal(_bits(r["xnext"]), _bits(r["xnext_ref"]), err_msg=what)
    np.testing.assert_array_equal(_bits(r["out"][:, c0:d]), _bits(r["out_ref"][:, c0:d]), err_msg=what)
    # outside [c0, d) the fused kernel writes nothing
    assert np.all(r["out"][:, :c0] == FILL) and np.all(r["out"][:, max(c0, d):] == FILL), what
    nxt, xn, out = _reference64(orig, xd, s, ds, dn, ds_next, wn, wo)
    np.testing.assert_allclose(r["next"], nxt, atol=1e-5, rtol=0, err_msg=what)
    if xn is not None:
        np.testing.assert_allclose(r["xnext"], xn, atol=1e-5, rtol=0, err_msg=what)
    else:
        assert np.all(r["xnext"] == FILL), what
    if c0 < d:
        np.testing.assert_allclose(r["out"][:, c0:d], out[:, c0:d], atol=1e-5, rtol=0, err_msg=what)


@pytest.mark.parametrize("d,dn", [(64, 96), (128, 96), (64, 64)])
def test_seam_equals_glue_then_downsamples(need_gpu, d, dn):
    seed = 0
    for ds in (1, 2, 4, 8):
        for ds_next in (2, 4, 8, 1):
            for c0 in (0, 32):
                seed += 1
                _check(d, ds, dn, ds_next, c0, 1000 * d + seed)


@pytest.mark.parametrize("ds", [1, 2, 4, 8])
def test_last_seam_and_seam_without_output_columns(need_gpu, ds):
    _check(64, ds, 0, 1, 0, 77 + ds)      # the last stack: output columns only
    _check(128, ds, 0, 1, 64, 87 + ds)
    _check(64, ds, 96, 4, 64, 97 + ds)    # c0 >= d: no output columns
    _check(64, ds, 96, 1, 64, 107 + ds)   # ... and no downsample either: `next` only
