"""The community-1 embedding kernels alone on the MI355X (zasr_selftest_emb_*, zasr_emb_fbank),
one launch each on the operands of tests/resnet34_reference.py, against its float64 restatements.

Convolutions: per element ((K + 4) u) sum|w||x| + 2 u |y|, u = 2^-24 -- a priori, the f32 MFMA is
an fmaf chain.  Every case runs on every route that takes it; the output starts as a sentinel
with guard bytes before and behind (the self-test refuses a touched guard).
Pooling: 8 x the float32 restatement's deviation from the float64 one, floor 16 u.
Fbank: the main fbank kernel's bound, 2e-3 absolute on the log-mel (tests/test_gpu_parity.py).
"""
import numpy as np
import pytest

from conftest import gpu_available

import resnet34_reference as R

pytestmark = pytest.mark.gpu
f64 = np.float64


@pytest.fixture(scope="module")
def need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c.name)
def test_conv2d_case(need_gpu, case):
    from zasr.binding import selftest_emb_conv2d
    x, w, b, res = R.conv_operands(case)
    ref, bound = R.conv_case_ref(case)
    _, routes = selftest_emb_conv2d(x, w, b, case.ks, case.stride, res, case.relu, 0)
    assert routes == (1 if case.co < 64 or case.ci == 1 else 2)
    for route in range(0, routes + 1) if case.ci != 1 else (0,):
        got, _ = selftest_emb_conv2d(x, w, b, case.ks, case.stride, res, case.relu, route)
        assert got.shape == ref.shape and got.dtype == np.float32
        assert not np.any(got == R.SENT), "an output element was not written"
        ratio = float(np.max(np.abs(got.astype(f64) - ref) / bound))
        print(f"case {case.name} route {route}: worst |device - float64| / bound = {ratio:.3f}")
        assert ratio <= 1.0


def test_conv2d_refuses_what_it_cannot_take(need_gpu):
    from zasr.binding import ZasrError, selftest_emb_conv2d
    c = R.CONV_CASES[0]
    x, w, b, _ = R.conv_operands(c)
    with pytest.raises(ZasrError):
        selftest_emb_conv2d(x, w, b, c.ks, c.stride, None, True, 2)       # Co = 32 has one route
    with pytest.raises(ZasrError):
        selftest_emb_conv2d(x[..., :16], w[..., :16], b, c.ks, c.stride)  # Ci = 16


def _pool_inputs(T):
    block = R.pool_block(2560, T)                      # [c * 10 + f][t]
    x = np.ascontiguousarray(block.reshape(256, 10, T).transpose(1, 2, 0))[None]   # [1][F][T][C]
    return block, x


@pytest.mark.parametrize("T", [125, 1, 2])
def test_masked_pool(need_gpu, T):
    from zasr.binding import selftest_emb_pool
    block, x = _pool_inputs(T)
    idx = R.feat_idx(T, R.NSEG)
    names = list(R.pool_masks())
    for i in range(0, len(names), 3):                  # three speakers per launch, as the engine
        trio = names[i:i + 3]
        um = np.stack([R.used_mask(*R.pool_masks()[n], R.MIN_SEG_FRAMES) for n in trio])
        got = selftest_emb_pool(x, um.astype(np.uint8)[None])
        assert got.shape == (1, 3, 5120) and not np.any(np.isnan(got))
        for s, name in enumerate(trio):
            r64, bound, dev = R.pool_bound(block, um[s][idx])
            err = float(np.max(np.abs(got[0, s].astype(f64) - r64)))
            print(f"pool T' = {T} {name}: |device - float64| = {err:.3e} (float32 {dev:.3e}, bound {bound:.3e})")
            assert err <= bound, name
            if name == "all_zero":
                assert np.all(got[0, s] == 0.0)


@pytest.mark.parametrize("T", [125, 2, 1])
def test_population_pool(need_gpu, T):
    from zasr.binding import selftest_emb_pool
    block, x = _pool_inputs(T)
    got = selftest_emb_pool(x, None)
    r64, bound, dev = R.pool_bound(block, None)
    err = float(np.max(np.abs(got[0, 0].astype(f64) - r64)))
    print(f"population pool T' = {T}: {err:.3e} (float32 {dev:.3e}, bound {bound:.3e})")
    assert got.shape == (1, 1, 5120) and err <= bound


@pytest.fixture(scope="module")
def sess(need_gpu, tmp_path_factory):
    from zasr.binding import EmbSession
    from zasr.resnet34 import save_model_dir
    cfg, w, _ = R.network()
    d = tmp_path_factory.mktemp("emb_k")
    save_model_dir(str(d), cfg, w)
    s = EmbSession(str(d))
    yield s
    s.close()


@pytest.mark.parametrize("n", [400, 401, 560, 16000])
def test_fbank_with_the_zero_tail(sess, n):
    a = R.speech(1.0, 5)[:n]
    ref = R.fbank(a, R.TAIL)
    got = sess.fbank(a, R.TAIL)
    assert got.shape == ref.shape == (1 + (n + 160000 - 400) // 160, 80) and got.dtype == np.float32
    err = float(np.max(np.abs(got.astype(f64) - ref)))
    print(f"fbank n = {n}: max |device - float64| = {err:.3e} (bound {R.FBANK_ATOL})")
    assert err <= R.FBANK_ATOL
    first_zero = -(-n // 160)
    assert np.all(got[first_zero:] == np.float32(np.log(R.FLT_EPSILON)))
    # the rows that lie inside the signal do not depend on the tail
    assert np.array_equal(sess.fbank(a, 0), got[:R.fbank_rows(n)])


def test_fbank_shorter_than_a_frame(sess):
    assert sess.fbank(np.zeros(399, np.float32)).shape == (0, 80)
    z = sess.fbank(np.zeros(800, np.float32))
    assert z.shape == (3, 80) and np.all(z == np.float32(np.log(R.FLT_EPSILON)))


def test_population_pool_takes_any_number_of_frames(need_gpu):
    """A long segment (compute_single_embedding has no length limit): 1500 encoder frames, past the
    1024 the masked form stages; the masked form refuses them."""
    from zasr.binding import ZasrError, selftest_emb_pool
    T = 1500
    block = R.pool_block(16, T)                                                   # [c * 2 + f][t]
    x = np.ascontiguousarray(block.reshape(8, 2, T).transpose(1, 2, 0))[None]     # [1][F][T][C]
    got = selftest_emb_pool(x, None)
    r64, bound, dev = R.pool_bound(block, None)
    err = float(np.max(np.abs(got[0, 0].astype(f64) - r64)))
    print(f"population pool T' = {T}: {err:.3e} (float32 {dev:.3e}, bound {bound:.3e})")
    assert got.shape == (1, 1, 32) and err <= bound
    with pytest.raises(ZasrError):
        selftest_emb_pool(x, np.ones((1, 3, R.NSEG), np.uint8))
