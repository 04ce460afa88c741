"""The joiner kernels alone, against a float64 product.

joiner_kernel, joiner_bf16_kernel, joiner_split_kernel (layout 0) and joiner_reg_kernel,
joiner_split_packed_kernel (layout 1) run through zasr_selftest_joiner on seeded host operands:
the launcher a decode uses, W prepared as the loader prepares it, J laid out on the host as its
producers write it.  Cases, inputs, reference and bound: tests/joiner_reference.py (checked
without a GPU by tests/test_joiner_reference.py).  The entry point keeps a guard row behind
`out` and refuses a run that wrote into it.

Each case prints its worst |got - ref| / bound and the zlib.crc32 of the returned bytes; the
CRCs of two builds of the library compare the kernels bit for bit.
"""
import zlib

import numpy as np
import pytest

import joiner_reference as jr
from conftest import gpu_available

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")


def run(c, o, live=(None, None, 0)):
    from zasr.binding import selftest_joiner
    return selftest_joiner(c.mode, o["J"], o["W"], o["bias"], o["out0"], c.layout, *live)


def ratios(c, o, got):
    ref, bound = jr.reference(c, o)
    assert got.shape == ref.shape and got.dtype == np.float32
    return np.abs(got.astype(np.float64) - ref) / bound


def report(c, got, ratio):
    print(f"{jr.case_id(c)}: worst |got - ref| / bound = {ratio:.3f} crc32 = {zlib.crc32(got.tobytes()):08x}")


@pytest.mark.parametrize("group", jr.EDGE_GROUPS, ids=["l{}_{}_D{}".format(*g) for g in jr.EDGE_GROUPS])
def test_joiner_edge_shapes_match_f64(need_gpu, group):
    bad = []
    for c in jr.group_cases(*group):
        o = jr.operands(c)
        got = run(c, o)
        r = float(np.max(ratios(c, o, got)))
        report(c, got, r)
        if not r <= 1.0:
            bad.append((jr.case_id(c), r))
    assert not bad, bad


@pytest.mark.parametrize("group", jr.LIVE_GROUPS, ids=["l{}_{}".format(*g) for g in jr.LIVE_GROUPS])
def test_joiner_live_filter_skips_only_finished_rows(need_gpu, group):
    for c in jr.live_cases(*group):
        o = jr.operands(c)
        live_t, live_len, done = jr.live_arrays(c)
        got = run(c, o, (live_t, live_len, jr.LIVE_F))
        r = ratios(c, o, got)
        row_done = np.repeat(done, jr.LIVE_F)
        inside = np.all(r <= 1.0, axis=1)
        untouched = np.all(got == jr.SENTINEL, axis=1)
        report(c, got, float(np.max(r[inside])))
        assert np.all(inside[~row_done]), (jr.case_id(c), np.flatnonzero(~inside & ~row_done))
        assert np.all(inside | untouched), (jr.case_id(c), np.flatnonzero(~inside & ~untouched))
        if c.live == "s0_15":  # the filter skips at all
            assert np.all(untouched[:64]), (jr.case_id(c), np.flatnonzero(~untouched[:64]))


REFUSED = [("fp32", 1, 256), ("bf16", 1, 128), ("f16x3", 1, 64), ("bf16", 2, 256),
           ("bf16_enc", 0, 256), ("fp32", 0, 96)]


@pytest.mark.parametrize("mode,layout,D", REFUSED, ids=["{}_l{}_D{}".format(*r) for r in REFUSED])
def test_joiner_refused_combinations_report_an_error(need_gpu, mode, layout, D):
    from zasr.binding import ZasrError
    c = jr.Case(layout, mode, D, 33, 68, None)
    with pytest.raises(ZasrError):
        run(c, jr.operands(c))
