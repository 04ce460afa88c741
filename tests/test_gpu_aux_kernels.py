"""The CAM++, Silero VAD and ViBERT kernels alone, against tests/aux_reference.py.

Each test runs one launch function through its zasr_selftest_* entry on seeded host operands
(weights N(0, 1) / sqrt(fan_in), activations N(0, 1), scale U(0.5, 1.5), shift and residual
0.5 N(0, 1); the exceptions are stated in aux_reference.py beside their cases) and compares every
output element with the float64 restatement under the a-priori bound of that module's docstring:
max |got - ref| / bound <= 1, printed per case.  Data movement (VAD frames, the im2col kernels,
the gathers, the maxabs bits) is compared bit for bit with the float32 restatement.  Every
output starts as a sentinel and has guard bytes behind it on the device; the entry raises when
a guard byte changed, so a passing call also says the kernel stayed inside its output.

The MFMA convolution's cases name the rows per block, so the ring of input rows slides (one
block, several steps), ends on a single row (odd fo) and starts in the middle of the frequency
axis; the entry reports the kernel that ran and its rows per block, and each case asserts both.

Measured on an MI355X: profiles/aux_kernels/README.md (worst ratio per group, wall time).
"""
import numpy as np
import pytest

import aux_reference as ar
from conftest import gpu_available

pytestmark = pytest.mark.gpu

SENT = ar.SENT


@pytest.fixture(scope="module")
def need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")


def report(group, name, ratio):
    print(f"{group} {name}: worst |got - ref| / bound = {ratio:.3f}")
    return ratio


def written(a):
    return not (np.asarray(a) == SENT).any()


# ---- CAM++ conv2d ----
def run_conv(c, o):
    from zasr.binding import selftest_campp_conv2d
    return selftest_campp_conv2d(o["x"], o["w"], o["scale"], o["shift"], o["res"], ks=c.ks, ci=c.ci, fi=c.fi,
                                 sf=c.sf, T=c.T, n=c.n, relu=c.relu, tdnn_out=c.tdnn, in_tf=c.in_tf,
                                 use_mfma=c.mfma, rb=c.rb, fill=float(SENT))


def check_conv(group, c):
    o = ar.conv_operands(c)
    y, route, rb_used = run_conv(c, o)
    ref, bound = ar.conv2d(c, o)
    assert (route, rb_used) == (c.route, c.rb_used), (ar.conv_id(c), route, rb_used)
    assert y.shape == ref.shape and written(y), ar.conv_id(c)
    return ar.conv_id(c), report(group, ar.conv_id(c), ar.worst_ratio(y, ref, bound))


CONV_GROUPS = {
    "mfma_T": ar.MFMA_T_CASES,
    "mfma_rows_T17": [c for c in ar.MFMA_ROW_CASES if c.T == 17],
    "mfma_rows_T81": [c for c in ar.MFMA_ROW_CASES if c.T == 81],
    "mfma_epilogue": ar.MFMA_EPI_CASES,
    "mfma_engine_pick": ar.MFMA_PICK_CASES,
    "direct": ar.DIRECT_CASES,
}


@pytest.mark.parametrize("group", list(CONV_GROUPS))
def test_campp_conv2d_matches_f64(need_gpu, group):
    bad = [(i, r) for c in CONV_GROUPS[group] for i, r in [check_conv("conv2d_" + group, c)] if not r <= 1.0]
    assert not bad, bad


def test_campp_conv2d_both_routes_meet_the_bound(need_gpu):
    """One problem on the direct and on the MFMA kernel: each within its bound of the same
    reference (their summation orders differ, so they are not compared with each other)."""
    direct, mfma = ar.BOTH_ROUTES
    assert ar.conv_operands(direct)["x"].tobytes() == ar.conv_operands(mfma)["x"].tobytes()
    bad = [(i, r) for c in (direct, mfma) for i, r in [check_conv("conv2d_both_routes", c)] if not r <= 1.0]
    assert not bad, bad


# ---- CAM mask, stats, CMVN, gather ----
def test_campp_cam_mask_matches_f64(need_gpu):
    from zasr.binding import selftest_campp_cam_mask
    bad = []
    for c in ar.CAM_CASES:
        o = ar.cam_operands(c)
        m = selftest_campp_cam_mask(o["h"], o["w1"], o["b1"], o["w2"], o["b2"], c.seg, fill=float(SENT))
        ref, bound = ar.cam_mask(c, o)
        assert m.shape == (c.n, c.T, 32) and written(m), c     # every frame's 32 values
        r = report("cam_mask", "n{}_T{}_seg{}".format(*c), ar.worst_ratio(m, ref[:, :c.T], bound))
        if not r <= 1.0:
            bad.append((c, r))
    assert not bad, bad


def test_campp_stats_match_f64(need_gpu):
    from zasr.binding import selftest_campp_stats
    bad = []
    for c in ar.STATS_CASES:
        o = ar.stats_operands(c)
        out = selftest_campp_stats(o["x"], o["s"], o["b"], fill=float(SENT))
        ref, bound = ar.stats_pool(c, o)
        assert written(out), c
        if c.special == "one_frame":
            assert np.isnan(out[:, c.C:]).all() and np.isnan(ref[:, c.C:]).all()
        if c.special == "negative_column":
            assert (out[:, 2] == 0).all() and (out[:, c.C + 2] == 0).all()
        r = report("stats", "N{}_T{}_C{}_{}".format(*c), ar.worst_ratio(out, ref, bound))
        if not r <= 1.0:
            bad.append((c, r))
    assert not bad, bad


def test_campp_cmvn_matches_f64(need_gpu):
    from zasr.binding import selftest_campp_cmvn
    o = ar.cmvn_operands()
    y = selftest_campp_cmvn(o["x"], o["fr_off"])
    ref, bound = ar.cmvn(o)
    a, b = int(o["fr_off"][0]), int(o["fr_off"][-1])
    assert a > 0 and b < y.shape[0]
    assert ar.same_bits(y[:a], o["x"][:a]) and ar.same_bits(y[b:], o["x"][b:])   # outside: unchanged
    assert report("cmvn", "lens" + "_".join(map(str, ar.CMVN_LENS)), ar.worst_ratio(y, ref, bound)) <= 1.0


@pytest.mark.parametrize("c", ar.GATHER_CASES, ids=lambda c: f"wf{c.wf}")
def test_campp_gather_is_exact(need_gpu, c):
    from zasr.binding import selftest_campp_gather
    o = ar.gather_operands(c)
    out = selftest_campp_gather(o["rows"], o["win_row"], o["win_n"], c.wf, fill=float(SENT))
    assert ar.same_bits(out, ar.campp_gather(c, o))


# ---- Silero VAD ----
@pytest.mark.parametrize("peaks", list(ar.VAD_PEAKS))
def test_vad_frames_file_mode_is_exact(need_gpu, peaks):
    from zasr.binding import selftest_vad_frames
    o = ar.vad_file_operands(peaks)
    plain, none = selftest_vad_frames(o["n_windows"], o["audio"], o["off"], o["win_start"], fill=float(SENT))
    assert none is None and ar.same_bits(plain, ar.vad_frames_files(o))
    boosted, mx = selftest_vad_frames(o["n_windows"], o["audio"], o["off"], o["win_start"], o["len"],
                                      fill=float(SENT))
    assert ar.same_bits(mx, ar.vad_maxabs(o)), (mx, ar.vad_maxabs(o))
    assert ar.same_bits(boosted, ar.vad_frames_files(o, ar.vad_maxabs(o)))
    assert not ar.same_bits(boosted, plain)


def test_vad_frames_row_mode_is_exact(need_gpu):
    from zasr.binding import selftest_vad_frames
    rows = np.random.default_rng(11).standard_normal((3, 576), dtype=np.float32)
    fr, _ = selftest_vad_frames(3, rows576=rows, fill=float(SENT))
    assert ar.same_bits(fr, ar.vad_frames_rows(rows))


def test_vad_im2col_kernels_are_exact(need_gpu):
    from zasr.binding import selftest_vad_im2col, selftest_vad_mag_im2col
    rng = np.random.default_rng(12)
    for nw, bins, ldS, Kp in ar.MAG_CASES:
        S = rng.standard_normal((nw * 4, ldS), dtype=np.float32)
        A = selftest_vad_mag_im2col(S, bins, Kp, fill=float(SENT))
        assert ar.same_bits(A, ar.vad_mag_im2col(S, bins, Kp)), (nw, bins, ldS, Kp)
    for N, T, C, stride in ar.IM2COL_CASES:
        Y = rng.standard_normal((N * T, C), dtype=np.float32)
        A = selftest_vad_im2col(Y, N, T, stride, fill=float(SENT))
        assert ar.same_bits(A, ar.vad_im2col(Y, N, T, C, stride)), (N, T, C, stride)


@pytest.fixture(scope="module")
def lstm_one(need_gpu):
    """The 48 windows as one segment from a zero state, and the device states at 15, 20, 21."""
    from zasr.binding import selftest_vad_lstm
    o = ar.lstm_operands()
    run = lambda *a, **k: selftest_vad_lstm(o["gx"], o["whh"], o["bhh"], o["wd"], float(o["bd"]), *a,
                                            fill=float(SENT), **k)
    probs, s_out, e_out = run([0], [ar.LSTM_WINDOWS])
    _, _, states = run([0, 0, 0], [15, 20, 21])
    return dict(o=o, run=run, probs=probs, s_out=s_out, e_out=e_out,
                at={15: states[0], 20: states[1], 21: states[2]})


def test_vad_lstm_one_segment_matches_f64(lstm_one):
    ref, bound, dev = ar.lstm_bound(lstm_one["o"], [0], [ar.LSTM_WINDOWS])
    got = (lstm_one["probs"], lstm_one["s_out"], lstm_one["e_out"])
    assert all(written(g) for g in got)
    print(f"lstm float32 vs float64 deviation: probs {dev[0]:.2e}, e_out {dev[2]:.2e}")
    ratios = [report("lstm", n, ar.worst_ratio(g, r, b)) for n, g, r, b in zip(("probs", "s_out", "e_out"), got, ref, bound)]
    assert max(ratios) <= 1.0, ratios
    assert (lstm_one["s_out"] == 0).all()


def test_vad_lstm_segments_chain_bit_identically(lstm_one):
    at = lstm_one["at"]
    init = np.stack([np.zeros((2, 128), np.float32), at[20], at[21], at[21]])
    probs, s_out, e_out = lstm_one["run"]([0, 20, 21, 21], [20, 1, 0, 27], init=init)
    assert ar.same_bits(probs, lstm_one["probs"])
    assert ar.same_bits(s_out, init)
    assert ar.same_bits(e_out, np.stack([at[20], at[21], at[21], lstm_one["e_out"][0]]))


def test_vad_lstm_warm_up_writes_no_probability(lstm_one):
    at = lstm_one["at"]
    probs, s_out, e_out = lstm_one["run"]([20], [28], seg_warm=[5], init=at[15][None])
    assert ar.same_bits(probs[20:], lstm_one["probs"][20:])
    assert (probs[:20] == SENT).all()
    assert ar.same_bits(s_out[0], at[20]) and ar.same_bits(e_out, lstm_one["e_out"])


def test_vad_lstm_empty_segments(lstm_one):
    at, run = lstm_one["at"], lstm_one["run"]
    probs, s_out, e_out = run([30], [0], seg_warm=[0], init=at[15][None])
    assert (probs == SENT).all() and ar.same_bits(s_out[0], at[15]) and ar.same_bits(e_out[0], at[15])
    # warm 3, count 0 at window 18: windows 15, 16, 17 run from the state at 15, nothing is
    # written, and s_out = e_out = what the 3-window segment [15, 18) from that state ends in
    _, _, e3 = run([15], [3], init=at[15][None])
    probs, s_out, e_out = run([18], [0], seg_warm=[3], init=at[15][None])
    assert (probs == SENT).all() and ar.same_bits(s_out, e3) and ar.same_bits(e_out, e3)
    assert not ar.same_bits(e3[0], at[15])


def test_vad_lstm_null_init_is_zero_init(lstm_one):
    probs, s_out, e_out = lstm_one["run"]([0], [ar.LSTM_WINDOWS], init=np.zeros((1, 2, 128), np.float32))
    assert ar.same_bits(probs, lstm_one["probs"]) and ar.same_bits(e_out, lstm_one["e_out"])
    assert ar.same_bits(s_out, lstm_one["s_out"])


# ---- ViBERT ----
@pytest.mark.parametrize("embed", (0, 1), ids=("plain", "embedding"))
def test_vibert_layer_norm_matches_f64(need_gpu, embed):
    from zasr.binding import selftest_vibert_ln
    bad = []
    for c in (c for c in ar.LN_CASES if c.embed == embed):
        o = ar.ln_operands(c)
        if embed:
            y = selftest_vibert_ln(o["g"], o["b"], ar.LN_EPS, ids=o["ids"], tt=o["tt"], L=o["L"], word=o["word"],
                                   pos=o["pos"], type_=o["type"], fill=float(SENT))
        else:
            y = selftest_vibert_ln(o["g"], o["b"], ar.LN_EPS, x=o["x"])
        ref, bound = ar.layer_norm(c, o)
        assert y.shape == ref.shape and written(y), c
        r = report("layer_norm", "rows{}_H{}_embed{}".format(*c), ar.worst_ratio(y, ref, bound))
        if not r <= 1.0:
            bad.append((c, r))
    assert not bad, bad


@pytest.mark.parametrize("D", (16, 32, 64))
def test_vibert_attention_matches_f64(need_gpu, D):
    from zasr.binding import selftest_vibert_attn
    bad = []
    for c in (c for c in ar.ATTN_CASES if c.D == D):
        for mask in ar.ATTN_MASKS:
            o = ar.attn_operands(c, mask)
            ctx = selftest_vibert_attn(o["qkv"], o["mask"], 2, c.L, c.heads, c.heads * c.D, fill=float(SENT))
            ref, bound = ar.attention(c, o)
            assert ctx.shape == ref.shape and written(ctx), (c, mask)     # padded query rows too
            name = "h{}_D{}_L{}_".format(*c) + "_".join(mask)
            r = report("attention", name, ar.worst_ratio(ctx, ref, bound))
            if not r <= 1.0:
                bad.append((name, r))
    assert not bad, bad


def test_vibert_gather_is_exact(need_gpu):
    from zasr.binding import selftest_vibert_gather
    o = ar.vibert_gather_operands()
    g = selftest_vibert_gather(o["x"], o["off"], o["L"], fill=float(SENT))
    assert ar.same_bits(g, ar.vibert_gather(o))


# ---- what the launch functions refuse comes back as an error, not as a launch ----
def test_refused_arguments_report_an_error(need_gpu):
    from zasr.binding import (ZasrError, selftest_campp_conv2d, selftest_vibert_attn, selftest_vibert_gather,
                              selftest_vibert_ln)
    z = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(ZasrError):     # H > 1024
        selftest_vibert_ln(z(1025), z(1025), ar.LN_EPS, x=z(2, 1025))
    with pytest.raises(ZasrError):     # L > 256
        selftest_vibert_attn(z(2 * 257, 3 * 32), np.ones(2 * 257, np.int64), 2, 257, 2, 32)
    for heads, H in ((1, 8), (1, 128), (2, 48), (3, 64)):     # head dim 8, 128, 24; H % heads != 0
        with pytest.raises(ZasrError):
            selftest_vibert_attn(z(2 * 4, 3 * H), np.ones(8, np.int64), 2, 4, heads, H)
    with pytest.raises(ZasrError):     # Ci > 32
        selftest_campp_conv2d(z(1, 33, 5, 4), z(32, 33, 3, 3), z(32), z(32), ks=3, ci=33, fi=5, sf=1, T=4, n=1,
                              relu=0, tdnn_out=0, in_tf=0, use_mfma=0)
    with pytest.raises(ZasrError):     # an odd rows-per-block override
        selftest_campp_conv2d(z(1, 32, 5, 4), z(32, 32, 3, 3), z(32), z(32), ks=3, ci=32, fi=5, sf=1, T=4, n=1,
                              relu=0, tdnn_out=0, in_tf=0, use_mfma=1, rb=3)
    with pytest.raises(ZasrError):     # an offset outside its sequence
        selftest_vibert_gather(z(2 * 3, 8), np.array([[0, 3], [1, 2]], np.int64), 3)
    # a refusal is not sticky: a valid problem still runs
    o = ar.vibert_gather_operands()
    assert ar.same_bits(selftest_vibert_gather(o["x"], o["off"], o["L"]), ar.vibert_gather(o))
