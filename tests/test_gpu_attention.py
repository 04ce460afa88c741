"""The attention kernels alone, against a float64 evaluation on ragged batches.

attn_flash_kernel (modes 0-3, every operand format), nonlin_prep_t_kernel, and the fp32 mode's
attn_softmax_kernel / attn_sa_kernel run through zasr_selftest_attn_weights / _attn_sa / _nonlin on
seeded host operands: the launchers a decode calls, the offsets a decode derives, the block map in
the decode's order.  Cases, inputs, reference, bound and what each shape is there for:
tests/attention_reference.py (held to the oracle's formulas, to a numpy emulation of every mode and
to single-defect emulations without a GPU by tests/test_attention_reference.py).  The entries keep
a guard region behind every output and refuse a run that wrote into it.

Each case prints its worst |got - ref| / bound per output and the zlib.crc32 of the returned
bytes; the CRCs of two builds of the library compare the kernels bit for bit.
"""
import zlib

import numpy as np
import pytest

import attention_reference as ar
from conftest import gpu_available

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")


def run(c, o):
    """The entry of the case's route: a dict of the returned arrays."""
    from zasr import binding as zb
    if c.route == "weights":
        return {"A0": zb.selftest_attn_weights(c.mode, c.H, c.L, c.pmax, o["qkp"], o["pos"])}
    if c.route == "sa":
        out1, stats, out2 = zb.selftest_attn_sa(c.mode, c.H, c.L, c.pmax, o["qkp"], o["pos"],
                                                o["v1"], o["v2"])
        return {"out1": out1, "stats": stats, "out2": out2}
    t1t, z = zb.selftest_nonlin(c.mode, c.H, c.L, c.pmax, c.hid, o["qkp"], o["pos"], o["h3"])
    return {"t1t": t1t} if z is None else {"t1t": t1t, "z": z}


def crc(got):
    return zlib.crc32(b"".join(np.ascontiguousarray(got[k]).tobytes() for k in sorted(got)))


def ratios(c, o, got):
    """Worst |got - ref| / bound per output (NaN counts as outside), after the structural checks:
    shapes, nothing left at the sentinel, zero padding."""
    if c.route == "weights":
        ref = {"A0": ar.reference_weights(c, o)}
        val = {"A0": got["A0"]}
        assert np.all(got["A0"][ar.padding_mask_weights(c)] == 0), "weight padding columns not zero"
    elif c.route == "sa":
        ref = ar.reference_sa(c, o)
        val = {"out1": got["out1"], "out2": got["out2"], "stats": ar.stats_as_c(c, got["stats"])}
    else:
        ref = ar.reference_nonlin(c, o)
        pad = ar.padding_mask_t1t(c)
        assert got["t1t"].shape == (ar.t1_planes(c.mode),) + pad.shape
        for plane in got["t1t"]:  # +0 in every piece plane, bf16 and fp16 alike (0x8000 is -0.0)
            assert np.all(plane[pad] == 0), "t1^T padding columns not +0"
        val = {"t1t": ar.decode_t1t(c.mode, got["t1t"])}
        if "z" in ref:
            val["z"] = got["z"]
    res = {}
    for k, (r, b) in ref.items():
        assert val[k].shape == r.shape, (k, val[k].shape, r.shape)
        q = ar.ratio(val[k], r, b)
        res[k] = float(np.where(np.isnan(q), np.inf, q).max()) if q.size else 0.0
    return res


def check(c, o=None):
    o = ar.operands(c) if o is None else o
    got = run(c, o)
    r = ratios(c, o, got)
    print(f"{ar.case_id(c)}: worst |got - ref| / bound = "
          + " ".join(f"{k} {v:.3f}" for k, v in r.items()) + f" crc32 = {crc(got):08x}")
    return got, [(ar.case_id(c), k, v) for k, v in r.items() if not v <= 1.0]


GROUPS = [(r, m) for r in ("weights", "sa", "nonlin") for m in ar.ROUTE_MODES[r]]
IDS = ["{}_{}".format(*g) for g in GROUPS]


@pytest.mark.parametrize("route,mode", GROUPS, ids=IDS)
def test_attention_matches_f64(need_gpu, route, mode):
    """Every output element of every case at ratio <= 1; out1 (online statistics) and out2 (stored
    statistics) both, on different values."""
    bad = []
    for c in ar.route_cases(route, mode):
        bad += check(c)[1]
    assert not bad, bad


@pytest.mark.parametrize("route,mode", GROUPS, ids=IDS)
def test_smallest_pmax_is_bit_identical(need_gpu, route, mode):
    """pmax = max(L) (fp32: rounded up to 32): on the flash routes the row clamp serves every
    staged pad row; no live score reads a clamped row, so the bytes equal the default table's."""
    c, cmin = ar.min_pmax_pair(route, mode)
    got, bad = check(c)
    gmin, bad2 = check(cmin)
    assert not bad + bad2, bad + bad2
    for k in got:
        assert got[k].tobytes() == gmin[k].tobytes(), (ar.case_id(cmin), k)


@pytest.mark.parametrize("route,mode", GROUPS, ids=IDS)
def test_sequence_alone_equals_its_rows_in_the_batch(need_gpu, route, mode):
    """The 130-frame sequence run alone gives the bytes of its rows inside the ragged batch:
    placement in the block map changes nothing."""
    c = ar.route_cases(route, mode)[0]
    o = ar.operands(c)
    b = c.L.index(130)
    c1, o1 = ar.alone(c, o, b)
    got, bad = check(c, o)
    one, bad1 = check(c1, o1)
    assert not bad + bad1, bad + bad1
    off = ar.offsets(c.L)
    rows = slice(off[b], off[b + 1])
    if route == "weights":
        a_off = ar.offsets([L * ar.stride(mode, L) for L in c.L])
        assert got["A0"][a_off[b]:a_off[b + 1]].tobytes() == one["A0"].tobytes()
    elif route == "sa":
        for k in got:
            assert np.ascontiguousarray(got[k][rows]).tobytes() == one[k].tobytes(), k
    else:
        o32 = ar.offsets([(L + 31) // 32 * 32 for L in c.L])
        cols = slice(o32[b], o32[b + 1])
        assert np.ascontiguousarray(got["t1t"][:, :, cols]).tobytes() == one["t1t"].tobytes()
        if "z" in got:
            assert np.ascontiguousarray(got["z"][rows]).tobytes() == one["z"].tobytes()


@pytest.mark.parametrize("mode", ar.MODES)
def test_second_self_attention_agrees_with_the_first_on_equal_values(need_gpu, mode):
    """v1 == v2: out1 from online statistics and out2 from the stored ones, both within bound."""
    c = ar.route_cases("sa", mode)[0]
    o = ar.operands(c)
    o = dict(o, v2=o["v1"])
    got, bad = check(c, o)
    assert not bad, bad
    ref, bound = ar.reference_sa(c, o)["out1"]
    assert np.all(np.abs(got["out1"].astype(np.float64) - got["out2"]) <= 2 * bound)


REFUSED = [
    ("sa", "bf16", dict(H=3)), ("sa", "f16x3", dict(H=18)), ("weights", "bf16x3", dict(H=1)),
    ("sa", "bf16x6", dict(pmax=288)), ("sa", "fp32", dict(pmax=289)), ("nonlin", "bf16", dict(pmax=100)),
    ("nonlin", "bf16", dict(hid=146)), ("nonlin", "f16x3", dict(hid=2)),
    ("weights", "bf16", {}), ("weights", "f16x3", {}), ("nonlin", "fp32", {}),
    ("sa", "bf16_enc", {}),
    ("sa", "bf16", dict(L=(5, -1, 7))),
]


@pytest.mark.parametrize("route,mode,change", REFUSED,
                         ids=["{}_{}_{}".format(r, m, "_".join(f"{k}{v}" for k, v in ch.items()) or "route")
                              for r, m, ch in REFUSED])
def test_refused_shapes_report_an_error(need_gpu, route, mode, change):
    """An odd or too large head count, a table shorter than the longest sequence, hid % 4 != 0, a
    mode the route does not have, a negative length: ZasrError, nothing launched."""
    from zasr.binding import ZasrError
    L = change.get("L", ar.RAGGED)
    good = ar.Case(route, "bf16x3" if route != "nonlin" else "bf16x6", change.get("H", 2),
                   tuple(max(n, 0) for n in L), change.get("pmax", ar.pmax_default(ar.RAGGED)),
                   change.get("hid", 144 if route == "nonlin" else 0))
    o = ar.operands(good._replace(hid=max(good.hid, 4) if route == "nonlin" else 144))
    if route == "nonlin":  # (the operands' h3 follows the requested hid where that is usable)
        o["h3"] = np.zeros((sum(good.L), 3 * max(good.hid, 4)), np.float32)
    with pytest.raises(ZasrError):
        run(good._replace(mode=mode, L=tuple(L)), o)
