"""The joiner tests' bound and reference, checked without a GPU (tests/joiner_reference.py).

For every case of tests/test_gpu_joiner.py a numpy float32 evaluation of the same operands (as
the kernel sees them) must stay inside the bound around the float64 reference: the bound and S
are sane before any kernel is held to them.
"""
import numpy as np

import joiner_reference as jr


def test_u_op_is_the_gemm_tests_table():
    import test_gpu_gemm
    assert jr.U_OP == test_gpu_gemm.U_OP and jr.U == test_gpu_gemm.U


def test_cases_are_the_planned_set():
    cases = jr.all_cases()
    assert len(cases) == len(set(cases)) == 20 * 4 + 8 * 4 + 4 * 3
    assert {(c.layout, c.D) for c in cases if c.layout} == {(1, 256), (1, 512)}
    assert not [c for c in cases if c.layout and c.mode == "fp32"]


def test_float32_product_stays_inside_the_bound():
    worst = 0.0
    for c in jr.all_cases():
        o = jr.operands(c)
        assert np.all(np.abs(o["J"]) < 1.0) and o["J"].dtype == np.float32
        ref, bound = jr.reference(c, o)
        J, W = jr.seen(c, o)
        got = J @ W.T + o["bias"]
        assert got.dtype == np.float32 and got.shape == ref.shape == (c.M, c.V)
        assert np.all(bound > 0.0) and np.all(np.abs(ref) < 100.0)
        ratio = float(np.max(np.abs(got.astype(np.float64) - ref) / bound))
        assert ratio <= 1.0, (jr.case_id(c), ratio)
        worst = max(worst, ratio)
    print(f"float32 numpy product: worst |got - ref| / bound = {worst:.3f}")


def test_live_patterns_mark_the_planned_streams():
    for c in jr.live_cases(0, "bf16"):
        t, n, done = jr.live_arrays(c)
        assert t.dtype == n.dtype == np.int32 and len(t) == len(n) == c.M // jr.LIVE_F
        assert np.array_equal(t >= n, done) and list(np.flatnonzero(done)) == list(jr.LIVE_PATTERNS[c.live])
