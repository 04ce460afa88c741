"""The PyanNet and Conv-TasNet kernels other than the GEMMs alone, against tests/segsep_reference.py.

Each test runs one launch function of seg.h / sep.h through its zasr_selftest_* entry on seeded
host operands and compares every output element with the float64 restatement under the a-priori
bound of that module's docstring: max |got - ref| / bound <= 1, printed per case.  Data movement
and single correctly rounded operations (pool3, sep_frames, sep_prelu, the overlap-add, the head's
classes) are compared bit for bit with float32 numpy.  Every output starts as a sentinel and has
guard bytes behind it (in-place and strided ones in front too); the entry raises when a guard
byte changed, so a passing call also says the kernel stayed inside its output.

The separation entries build their region and tile tables with the engine's own builder
(sep_fill_group) from (sig_off, T) per region and run one launch group of the call, so the
second group of a five-region call is a case like any other.  The three grid-stride kernels run
both as the engine launches them and capped at two blocks: several passes per thread, the last
ragged.

Measured on an MI355X: profiles/segsep_kernels/README.md (worst ratio per group, wall time).
"""
import numpy as np
import pytest

import segsep_reference as sr
from conftest import gpu_available

pytestmark = pytest.mark.gpu

SENT = sr.SENT


@pytest.fixture(scope="module")
def need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")


def report(group, name, ratio):
    print(f"{group} {name}: worst |got - ref| / bound = {ratio:.3f}")
    return ratio


def written(a):
    return not (np.asarray(a) == SENT).any()


def call_of(s):
    from zasr.binding import SepCall
    return SepCall(s.sig_off, s.T, s.r0, s.ng, sr.WIN, sr.HOP)


# ---- segmentation ----
def test_seg_chunk_stats_match_f64(need_gpu):
    from zasr.binding import selftest_seg_chunk_stats
    bad = []
    for c in sr.CHUNK_CASES:
        o = sr.chunk_operands(c)
        st = selftest_seg_chunk_stats(o["audio"], o["starts"], c.T, fill=float(SENT))
        ref, bound = sr.chunk_stats(c, o)
        assert st.shape == ref.shape and written(st), c
        if c.kind == "levels":      # the chunk at `total`: all zeros
            assert st[0, 0] == 0.0 and st[0, 1] == np.float32(1.0 / np.sqrt(1e-5))
        r = report("chunk_stats", f"T{c.T}_{c.kind}", sr.worst_ratio(st, ref, bound))
        if not r <= 1.0:
            bad.append((c, r))
    assert not bad, bad


@pytest.mark.parametrize("T", sr.FRONT_T)
def test_seg_front_matches_f64(need_gpu, T):
    from zasr.binding import selftest_seg_front
    o = sr.front_operands(T)
    y = selftest_seg_front(o["audio"], o["starts"], T, o["stats"], sr.IN_W, sr.IN_B, o["w0t"], fill=float(SENT))
    ref, bound = sr.front(T, o)
    assert y.shape == ref.shape and written(y)          # all 80 channels of every frame
    assert report("front", f"T{T}_F1_{sr.front_f1(T)}", sr.worst_ratio(y, ref, bound)) <= 1.0


def test_seg_pool3_is_exact(need_gpu):
    from zasr.binding import selftest_seg_pool3
    for c in sr.POOL_CASES:
        o = sr.pool_operands(c)
        y = selftest_seg_pool3(o["x"], c.Fp, c.cap, fill=float(SENT))
        assert sr.same_bits(y, sr.pool3(c, o)), c


def test_seg_frame_stats_match_f64(need_gpu):
    from zasr.binding import selftest_seg_frame_stats
    bad = []
    for c in sr.FSTAT_CASES:
        o = sr.fstat_operands(c)
        st = selftest_seg_frame_stats(o["x"], fill=float(SENT))
        ref, bound = sr.frame_stats(c, o)
        assert st.shape == ref.shape and written(st), c
        r = report("frame_stats", f"C{c.C}_F{c.F}", sr.worst_ratio(st, ref, bound))
        if not r <= 1.0:
            bad.append((c, r))
    assert not bad, bad


def test_seg_norm_act_matches_f64(need_gpu):
    from zasr.binding import selftest_seg_norm_act
    bad = []
    for c in sr.NORM_CASES:
        o = sr.norm_operands(c)
        y = selftest_seg_norm_act(o["x"], o["stats"], o["w"], o["b"], c.cap)
        ref, bound = sr.norm_act(c, o)
        assert y.shape == ref.shape and not sr.same_bits(y, o["x"])
        r = report("norm_act", f"C{c.C}_F{c.F}_cap{c.cap}", sr.worst_ratio(y, ref, bound))
        if not r <= 1.0:
            bad.append((c, r))
    assert not bad, bad


@pytest.mark.parametrize("F", sr.LSTM_F)
def test_seg_lstm_matches_f64_and_is_the_same_in_every_group_and_slot(need_gpu, F):
    from zasr.binding import selftest_seg_lstm
    o = sr.lstm_operands(F)
    ref, bound, dev = sr.lstm_bound(o)
    print(f"seg_lstm F = {F}: float32 vs float64 deviation {dev:.2e}, bound {bound:.2e}")
    first = selftest_seg_lstm(o["gx"], o["whh"], 1, fill=float(SENT))     # every sequence alone
    bad, worst = [], 0.0
    for B in sr.LSTM_GROUPS:
        for n in sr.lstm_ns(B):
            y = selftest_seg_lstm(o["gx"][:n], o["whh"], B, fill=float(SENT))
            assert y.shape == (n, F, 256) and written(y), (B, n)
            r = sr.worst_ratio(y, ref[:n], bound)
            worst = max(worst, r)
            if not r <= 1.0:
                bad.append((B, n, r))
            assert sr.same_bits(y, first[:n]), (B, n)       # whatever the group and the slot
    report("lstm", f"F{F}", worst)
    assert not bad, bad


def test_seg_head_matches_f64_and_classes_are_the_first_maximum(need_gpu):
    from zasr.binding import selftest_seg_head
    bad = []
    for c in sr.HEAD_CASES:
        o = sr.head_operands(c)
        logits, classes = selftest_seg_head(o["x"], o["w"], o["b"], fill=float(SENT))
        ref, bound = sr.head(c, o)
        assert logits.shape == ref.shape and written(logits) and classes.shape == (c.rows,), c
        assert sr.same_bits(classes, sr.head_classes(logits)), c        # every frame, ties to the lower index
        if c.kind == "tie":
            assert sr.same_bits(logits[:, 2], logits[:, 3]) and (classes == 2).any() and not (classes == 3).any()
        r = report("head", f"rows{c.rows}_{c.kind}", sr.worst_ratio(logits, ref, bound))
        if not r <= 1.0:
            bad.append((c, r))
    assert not bad, bad


# ---- separation ----
@pytest.mark.parametrize("s", sr.SEP_SETS, ids=lambda s: s.name)
def test_sep_frames_are_exact(need_gpu, s):
    from zasr.binding import selftest_sep_frames
    sig = sr.sep_signal(s)
    assert sr.same_bits(selftest_sep_frames(call_of(s), sig, fill=float(SENT)), sr.sep_frames(s, sig))


@pytest.mark.parametrize("s", sr.SEP_SETS, ids=lambda s: s.name)
def test_sep_statistics_match_f64(need_gpu, s):
    from zasr.binding import selftest_sep_region_stats, selftest_sep_tile_sums
    bad = []
    for C in sr.SEP_C:
        x = sr.gln_operands(s, C)["x"]
        p = selftest_sep_tile_sums(call_of(s), x, fill=float(SENT))
        ref, bound = sr.tile_sums(s, x)
        assert p.shape == ref.shape and written(p)
        r1 = report("tile_sums", f"{s.name}_C{C}", sr.worst_ratio(p, ref, bound))
        # the region statistics from exact partial sums, against the two-pass float64 statistics
        st = selftest_sep_region_stats(call_of(s), ref, C, fill=float(SENT))
        sref, sbound = sr.region_stats(s, x)
        inside = np.arange(len(s.T))[s.r0:s.r0 + s.ng]
        assert written(st[inside]) and (np.delete(st, inside, 0) == SENT).all()     # the stats array is call-wide
        r2 = report("region_stats", f"{s.name}_C{C}", sr.worst_ratio(st[inside], sref[inside], sbound[inside]))
        if not max(r1, r2) <= 1.0:
            bad.append((s.name, C, r1, r2))
    assert not bad, bad


@pytest.mark.parametrize("in_place", (False, True), ids=("out_of_place", "in_place"))
@pytest.mark.parametrize("s", sr.SEP_SETS, ids=lambda s: s.name)
def test_sep_gln_apply_matches_f64(need_gpu, s, in_place):
    from zasr.binding import selftest_sep_gln_apply
    bad = []
    for C in sr.SEP_C:
        o = sr.gln_operands(s, C)
        y = selftest_sep_gln_apply(call_of(s), o["x"], o["stats"], o["gamma"], o["beta"], in_place, fill=float(SENT))
        ref, bound = sr.gln_apply(s, o)
        assert y.shape == ref.shape and written(y)
        r = report("gln_apply", f"{s.name}_C{C}_inplace{int(in_place)}", sr.worst_ratio(y, ref, bound))
        if not r <= 1.0:
            bad.append((s.name, C, r))
    assert not bad, bad


MID_GROUPS = {
    "edges": [c for c in sr.MID_CASES if c.set.name.startswith("dil")],
    "shared_sets": [c for c in sr.MID_CASES if c.C == 512 and not c.set.name.startswith("dil")],
    "layouts": [c for c in sr.MID_CASES if c.C != 512],
}


@pytest.mark.parametrize("group", list(MID_GROUPS))
def test_sep_mid_matches_f64_and_its_partial_sums_are_those_of_its_y(need_gpu, group):
    from zasr.binding import selftest_sep_mid
    bad = []
    for c in MID_GROUPS[group]:
        o = sr.mid_operands(c)
        y, p = selftest_sep_mid(call_of(c.set), o["h"], o["stats"], o["gamma"], o["beta"], o["w"], o["bias"],
                                sr.MID_SLOPE, c.dil, fill=float(SENT))
        ref, bound = sr.mid(c, o)
        assert y.shape == ref.shape and written(y) and written(p), sr.mid_id(c)
        r1 = report("mid_" + group, sr.mid_id(c), sr.worst_ratio(y, ref, bound))
        pref, pbound = sr.mid_partials(c, y)        # of the y the kernel itself returned
        r2 = report("mid_partials_" + group, sr.mid_id(c), sr.worst_ratio(p, pref, pbound))
        if not max(r1, r2) <= 1.0:
            bad.append((sr.mid_id(c), r1, r2))
    assert not bad, bad


def test_sep_prelu_is_exact(need_gpu):
    from zasr.binding import selftest_sep_prelu
    for c in sr.PRELU_CASES:
        o = sr.prelu_operands(c)
        y = selftest_sep_prelu(o["x"], sr.PRELU_C, sr.PRELU_COL0, sr.PRELU_SLOPE, c.cap)
        assert sr.same_bits(y, sr.prelu(c, o)), c                      # columns [C, ld) keep their sentinel
        assert (y[:, :sr.PRELU_COL0] == SENT).all() and written(y[:, sr.PRELU_COL0:])


@pytest.mark.parametrize("s", sr.OLA_SETS, ids=lambda s: s.name)
def test_sep_overlap_add_is_exact(need_gpu, s):
    from zasr.binding import selftest_sep_overlap_add
    o = sr.ola_operands(s)
    out = selftest_sep_overlap_add(call_of(s), o["dec0"], o["dec1"], o["out_off"], o["n_out"], fill=float(SENT))
    assert sr.same_bits(out, sr.overlap_add(s, o))        # gaps keep the sentinel, the tails are +0.0


# ---- what the launch functions refuse comes back as an error, not as a launch ----
def test_refused_arguments_report_an_error_and_the_next_call_runs(need_gpu):
    import zasr.binding as b
    z = lambda *s: np.zeros(s, np.float32)
    one = lambda n=1, T=32, **k: b.SepCall(np.zeros(n, np.int64), np.full(n, T, np.int32), 0, n, **k)

    def still_runs():
        c = sr.PRELU_CASES[0]
        o = sr.prelu_operands(c)
        assert sr.same_bits(b.selftest_sep_prelu(o["x"], sr.PRELU_C, sr.PRELU_COL0, sr.PRELU_SLOPE), sr.prelu(c, o))

    refusals = {
        "lstm group 3": lambda: b.selftest_seg_lstm(z(3, 2, 1024), z(2, 512, 128), 3),
        "frame stats C = 132": lambda: b.selftest_seg_frame_stats(z(1, 4, 132)),
        "pool3 with 3 Fp > L": lambda: b.selftest_seg_pool3(z(1, 5, 8), 2),
        "pool3 C = 6": lambda: b.selftest_seg_pool3(z(1, 6, 6), 2),
        "norm_act C = 6": lambda: b.selftest_seg_norm_act(z(1, 2, 6), z(1, 6, 2), z(6), z(6)),
        "tile_sums C = 6": lambda: b.selftest_sep_tile_sums(one(), z(1, 6)),
        "gln_apply C = 6": lambda: b.selftest_sep_gln_apply(one(), z(1, 6), z(1, 2), z(6), z(6), False),
        "mid C = 6": lambda: b.selftest_sep_mid(one(), z(1, 6), z(1, 2), z(6), z(6), z(3, 6), z(6), 0.25, 1),
        "mid C = 12": lambda: b.selftest_sep_mid(one(), z(1, 12), z(1, 2), z(12), z(12), z(3, 12), z(12), 0.25, 1),
        "prelu C = 6": lambda: b.selftest_sep_prelu(z(2, 8), 6, 0, 0.25),
        "prelu ld = 130": lambda: b.selftest_sep_prelu(z(2, 130), 128, 0, 0.25),
        "front n = 65536": lambda: b.selftest_seg_front(z(300), np.zeros(65536, np.int64), 271, z(65536, 2), 1.0, 0.0,
                                                        z(251, 80)),
        "overlap-add n_regions = 65536": lambda: b.selftest_sep_overlap_add(
            one(65536), z(65536, 32), z(65536, 32), np.zeros(65536, np.int64), 64),
        "overlap-add win != 2 hop": lambda: b.selftest_sep_overlap_add(
            one(1, 32, win=32, hop=8), z(1, 32), z(1, 32), np.zeros(1, np.int64), 64),
    }
    for name, call in refusals.items():
        with pytest.raises(b.ZasrError):
            call()
            pytest.fail(name + " was not refused")
        still_runs()        # a refusal is not sticky
