"""Centroid-linkage AHC on an MI355X (zasr.binding.CluSession over the zasr_clu_* C ABI) against
the float64 restatement (vbx_reference.ahc_centroid) and scipy's linkage + fcluster on the same
rows: the partitions are identical.  The inputs are clu_inputs.cases(); test_vbx_reference.py
shows on the CPU that each non-degenerate one is stable under +-2 ulp of its normalised rows, so
no case is excused here.  Reads no reference path."""
import numpy as np
import pytest

import clu_inputs
import vbx_reference as R
from conftest import gpu_available

pytestmark = pytest.mark.gpu

CASES = clu_inputs.cases()
GUARD = 64            # int32 words before and behind the labels
SENTINEL = 0x5A5A5A5A
EXPECT = {}


@pytest.fixture(scope="module")
def clu():
    if not gpu_available():
        pytest.skip("no GPU")
    from zasr.binding import CluSession
    s = CluSession()
    yield s
    s.close()


def expected(name):
    """(restatement labels, scipy labels) of a case, computed once."""
    if name not in EXPECT:
        from scipy.cluster.hierarchy import fcluster, linkage
        X, thr, _ = CASES[name]
        Xn = R.l2norm32(X)
        EXPECT[name] = (R.ahc_centroid(Xn, thr),
                        fcluster(linkage(Xn, method="centroid", metric="euclidean"), thr,
                                 criterion="distance"))
    return EXPECT[name]


def run_guarded(clu, ptr, on_device, N, D, thr):
    """Labels of one call written between sentinel-filled guards, which must survive."""
    buf = np.full(N + 2 * GUARD, SENTINEL, np.int32)
    rc = clu.ahc_into(ptr, on_device, N, D, thr, buf[GUARD:].ctypes.data)
    assert rc == 0, clu.lib.zasr_last_error().decode()
    assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + N:] == SENTINEL).all()
    lab = buf[GUARD:GUARD + N].copy()
    assert (lab != SENTINEL).all() and lab.min() == 0 and lab.max() < N
    return lab


def host_labels(clu, name, route=0):
    X, thr, _ = CASES[name]
    clu.force_route(route)
    try:
        return run_guarded(clu, X.ctypes.data, False, X.shape[0], X.shape[1], thr)
    finally:
        clu.force_route(0)


@pytest.mark.parametrize("name", list(CASES))
def test_partition(clu, name):
    X, thr, _ = CASES[name]
    ref, sp = expected(name)
    lab = host_labels(clu, name)
    # numbered by lowest member row: canonical already, and equal to the restatement's labels
    assert np.array_equal(lab, R.canonical_labels(lab))
    assert np.array_equal(lab, ref)
    assert R.same_partition(lab, sp)
    merges, rescans = clu.last_stats()
    assert merges == X.shape[0] - (int(ref.max()) + 1) and rescans >= 0


def test_expected_cluster_counts():
    """What the cases are there for (CPU arithmetic; here so that the GPU cases are the ones
    described)."""
    count = {n: int(expected(n)[0].max()) + 1 for n in CASES}
    assert count["two_merged"] == 1 and count["two_apart"] == 2
    assert count["inversion3"] == 1 and count["identical8"] == 1
    assert count["centroid_merges3"] == 1 and count["centroid_splits3"] == 2
    assert count["zero_row4"] == 2
    assert (count["speakers_65"], count["speakers_257"], count["speakers_1025"]) == (3, 5, 8)
    assert count["close_257"] == 3      # four speakers, two of them 0.57 apart


@pytest.mark.parametrize("name", ["inversion3", "identical8", "speakers_257", "loader_d5",
                                  "loader_d511", "close_257", "speakers_1025"])
def test_runs_and_routes_identical(clu, name):
    first = host_labels(clu, name)
    assert clu.n_routes() >= 2
    for route in range(clu.n_routes()):
        for _ in range(2):
            assert np.array_equal(host_labels(clu, name, route), first), route


@pytest.mark.parametrize("name", ["speakers_65", "loader_d5", "loader_d511", "speakers_1025"])
def test_rows_on_device(clu, name):
    import torch
    X, thr, _ = CASES[name]
    dX = torch.from_numpy(X).cuda()
    torch.cuda.synchronize()
    lab = run_guarded(clu, dX.data_ptr(), True, X.shape[0], X.shape[1], thr)
    assert np.array_equal(lab, host_labels(clu, name))
    assert np.array_equal(dX.cpu().numpy(), X)       # the input rows are left alone


def test_error_codes(clu):
    from zasr.binding import ZasrError
    ok = np.ones((4, 8), np.float32)
    for bad, thr in ((np.ones((1, 8), np.float32), 0.6),          # N < 2
                     (np.ones((2, 513), np.float32), 0.6),        # D > 512
                     (ok, float("nan"))):                         # threshold
        with pytest.raises(ZasrError):
            clu.ahc(bad, thr)
    buf = np.full(8, SENTINEL, np.int32)
    for N, D in ((16385, 8), (4, 0), (0, 8), (-3, 8), (4, -1)):
        assert clu.ahc_into(ok.ctypes.data, False, N, D, 0.6, buf.ctypes.data) != 0
        assert clu.lib.zasr_last_error()
    assert clu.ahc_into(0, False, 4, 8, 0.6, buf.ctypes.data) != 0       # null rows
    assert clu.ahc_into(ok.ctypes.data, False, 4, 8, 0.6, 0) != 0         # null labels
    assert (buf == SENTINEL).all()
    assert clu.ahc(ok, 0.6).tolist() == [0, 0, 0, 0]                      # and the handle lives on


def test_stage_profile(clu):
    X, thr, _ = CASES["speakers_257"]
    clu.set_profile(True)
    try:
        clu.ahc(X, thr)
        ms = clu.stage_ms()
    finally:
        clu.set_profile(False)
    assert list(ms) == ["normalise", "pairwise", "nearest", "merge"]
    assert all(v >= 0.0 for v in ms.values()) and ms["merge"] > 0.0
