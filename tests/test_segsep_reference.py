"""CPU checks of tests/segsep_reference.py: every float64 restatement against torch in float64
(and against the model-level restatements' own _inorm / _pool3 / _gln / _dwconv), the float32
ones bit for bit, every listed single defect caught by the case tables the GPU test runs, and
the recurrence's float32 deviation per case, the base of its bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convtasnet_reference as ctr
import pyannet_reference as pyr
import segsep_reference as sr

T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def close(a, b, tol=1e-11):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b))) <= tol * max(1.0, float(np.max(np.abs(b)))) if a.size else True


def caught(ref, bound, bad, exact=False):
    if exact:
        return not sr.same_bits(ref, bad)
    return sr.worst_ratio(bad, ref, bound) > 1.0


def test_case_tables_hold_what_the_issue_lists():
    assert [sr.front_f1(T) for T in sr.FRONT_T] == [1, 63, 64, 65, 129]
    assert {((T - 251) // 10 + 1) % 3 for T in sr.FRONT_T} == {0, 1, 2}
    assert {int(f) for s in sr.SEP_SETS for _, _, f in sr.sep_rows(s)} == {1, 31, 32, 33, 64, 65, 129, 257}
    assert [(s.r0, s.ng, len(s.T)) for s in sr.SEP_SETS] == [(0, 3, 3), (0, 5, 5), (2, 3, 5)]
    a = sr.SEP_SETS[0]
    assert (a.sig_off[1:] == (a.sig_off + a.T)[:-1]).all()                 # adjacent
    r = sr.SEP_SETS[1]
    assert (r.sig_off % 2 == 1).all() and (np.diff(r.sig_off) < 0).any()    # odd, out of order
    assert {c.dil for c in sr.MID_CASES if c.C == 512} == {1, 2, 4, 8, 16, 32, 64, 128}
    for d in (2, 128):
        s = next(c.set for c in sr.MID_CASES if c.set.name == f"dil{d}")
        assert sr.sep_F(s).tolist() == [d - 1, d, d + 1, 2 * d + 1]
    assert {(c.C, c.dil) for c in sr.MID_CASES if c.C != 512} == {(C, d) for C in (4, 256, 1024, 2048) for d in (1, 32)}
    assert sorted({c.F for c in sr.FSTAT_CASES if c.C == 60}) == [1, 2, 3, 4, 5, 589]
    assert [n for B in sr.LSTM_GROUPS for n in sr.lstm_ns(B)][-1] == sr.LSTM_MAX_N
    # the domain of the one-pass variance term: |mean| / std <= 10 on every region of every set
    for s in sr.SEP_SETS:
        x = sr.sep_activation(s, 128, "glnx").astype(np.float64)
        for _, row, Fr in sr.sep_rows(s):
            assert abs(x[row:row + Fr].mean()) / x[row:row + Fr].std() < 10.0


# ---- segmentation ----
@pytest.mark.parametrize("c", sr.CHUNK_CASES, ids=lambda c: f"T{c.T}_{c.kind}")
def test_chunk_stats_match_instance_norm(c):
    o = sr.chunk_operands(c)
    st, e = sr.chunk_stats(c, o)
    x = np.stack([sr._chunk(o["audio"].astype(np.float64), int(s), c.T)[0] for s in o["starts"]])
    t = F.instance_norm(T64(x)[:, None, :], eps=sr.SEG_EPS)[:, 0].numpy()
    assert close((x - st[:, :1]) * st[:, 1:], t, 1e-9)
    assert (e[:, 1] > 0).all() and ((e[:, 0] > 0) | (st[:, 0] == 0)).all()    # an all-zero chunk: mean exactly 0
    assert close((x - st[:, :1]) * st[:, 1:], pyr._inorm(T64(x)[:, :, None], torch.ones(1, dtype=torch.float64),
                                                          torch.zeros(1, dtype=torch.float64))[:, :, 0].numpy(), 1e-9)
    if c.kind == "levels":
        assert st[0, 0] == 0.0 and st[0, 1] == 1.0 / np.sqrt(1e-5)          # all zeros
        assert abs(st[1, 0] - np.float32(0.3)) < 1e-12 and abs(st[1, 1] - 1.0 / np.sqrt(1e-5)) < 1e-6
        assert abs(st[2, 0] - 0.5) < 1e-3 and 1.0 / st[2, 1] < 4e-3
    else:
        assert [sr._chunk(o["audio"], int(s), c.T)[1] for s in o["starts"]] == [c.T, c.T - 1, 1]


@pytest.mark.parametrize("T", sr.FRONT_T)
def test_front_matches_conv1d_abs_max_pool(T):
    o = sr.front_operands(T)
    y, e = sr.front(T, o)
    mean, rstd = (o["stats"].astype(np.float64)[:, i:i + 1] for i in (0, 1))
    x = np.stack([sr._chunk(o["audio"].astype(np.float64), int(s), T)[0] for s in o["starts"]])
    n = ((x - mean) * rstd) * sr.IN_W + sr.IN_B
    t = F.max_pool1d(F.conv1d(T64(n)[:, None], T64(o["w0"])[:, None], stride=10).abs(), 3, 3)
    assert y.shape == (2, sr.front_f1(T), 80) and close(y, t.transpose(1, 2).numpy()) and (e > 0).all()
    assert sr._chunk(o["audio"], int(o["starts"][1]), T)[1] < T           # chunk 1 leaves the signal


@pytest.mark.parametrize("c", sr.POOL_CASES[::2], ids=lambda c: f"L{c.L}_Fp{c.Fp}_C{c.C}")
def test_pool3_matches_max_pool1d(c):
    o = sr.pool_operands(c)
    y = sr.pool3(c, o)
    t = F.max_pool1d(torch.from_numpy(o["x"]).transpose(1, 2), 3, 3).transpose(1, 2)[:, :c.Fp]
    assert (o["x"] < 0).all() and sr.same_bits(y, t.contiguous().numpy())
    if 3 * c.Fp == c.L:
        assert sr.same_bits(y, pyr._pool3(torch.from_numpy(o["x"])).contiguous().numpy())


@pytest.mark.parametrize("c", sr.FSTAT_CASES, ids=lambda c: f"C{c.C}_F{c.F}")
def test_frame_stats_and_norm_act_match_instance_norm(c):
    o = sr.fstat_operands(c)
    st, e = sr.frame_stats(c, o)
    assert st.shape == (sr.FSTAT_N, c.C, 2) and (e > 0).all()
    # the statistics, rounded as the kernel hands them on, through norm_act: instance_norm + leaky
    rng = np.random.default_rng(1)
    w, b = rng.uniform(0.5, 1.5, c.C).astype(np.float32), rng.standard_normal(c.C).astype(np.float32)
    y, _ = sr.norm_act(sr.NormCase(c.C, c.F, 0), dict(x=o["x"][:sr.SEG_N], stats=st[:sr.SEG_N], w=w, b=b))
    if c.F > 1:       # torch refuses to normalise over one frame
        t = F.leaky_relu(F.instance_norm(T64(o["x"][:sr.SEG_N]).transpose(1, 2), weight=T64(w), bias=T64(b),
                                         eps=sr.SEG_EPS), 0.01).transpose(1, 2)
        assert close(y, t.numpy(), 1e-7)        # channel 1: mean 100, spread 0.01
    assert close(y, pyr._leaky(pyr._inorm(T64(o["x"][:sr.SEG_N]), T64(w), T64(b))).numpy(), 1e-7)


def test_norm_act_takes_both_branches():
    for c in sr.NORM_CASES:
        y, e = sr.norm_act(c, sr.norm_operands(c))
        assert (y > 0).any() and (y < 0).any() and (e > 0).all()


@pytest.mark.parametrize("Fr", sr.LSTM_F)
def test_lstm_matches_torch_bidirectional_lstm(Fr):
    o = sr.lstm_operands(Fr)
    n = 5
    pre = []
    y = sr.lstm(o, n, B=2, pre_range=pre)
    net = torch.nn.LSTM(8 * sr.H, sr.H, bidirectional=True, batch_first=True).double()
    eye = torch.eye(4 * sr.H, dtype=torch.float64)
    zero = torch.zeros(4 * sr.H, 4 * sr.H, dtype=torch.float64)
    with torch.no_grad():      # gx is the given x W_ih^T + b: W_ih selects the direction's half
        net.weight_ih_l0.copy_(torch.cat([eye, zero], 1))
        net.weight_ih_l0_reverse.copy_(torch.cat([zero, eye], 1))
        net.weight_hh_l0.copy_(T64(o["whh"][0]))
        net.weight_hh_l0_reverse.copy_(T64(o["whh"][1]))
        for b in (net.bias_ih_l0, net.bias_hh_l0, net.bias_ih_l0_reverse, net.bias_hh_l0_reverse):
            b.zero_()
        t = net(T64(o["gx"][:n]))[0]
    assert close(y, t.numpy())
    for B in (1, 4):
        assert close(sr.lstm(o, n, B=B), y, 1e-13)          # the group does not enter the reference
    lo, hi = min(p[0] for p in pre), max(p[1] for p in pre)
    print(f"lstm F = {Fr}: pre-activations in ({lo:.2f}, {hi:.2f})")
    assert -12.0 < lo < -4.0 and 4.0 < hi < 12.0      # outside the linear region, not saturated in f32


@pytest.mark.parametrize("c", sr.HEAD_CASES, ids=lambda c: f"rows{c.rows}_{c.kind}")
def test_head_matches_log_softmax(c):
    o = sr.head_operands(c)
    y, e = sr.head(c, o)
    t = F.log_softmax(F.linear(T64(o["x"]), T64(o["w"]), T64(o["b"])), -1)
    assert close(y, t.numpy()) and (e > 0).all()
    if c.kind == "tie":
        cls = sr.head_classes(y)
        assert (y[:, 2] == y[:, 3]).all() and (cls == 2).sum() > c.rows // 4 and not (cls == 3).any()
    if c.kind == "large":
        assert np.abs(F.linear(T64(o["x"]), T64(o["w"]), T64(o["b"])).numpy()).max() > 100.0


# ---- separation ----
@pytest.mark.parametrize("s", sr.SEP_SETS, ids=lambda s: s.name)
def test_frames_tiles_and_stats_of_the_shared_sets(s):
    sig = sr.sep_signal(s)
    fr = sr.sep_frames(s, sig)
    assert fr.shape == (sr.sep_M(s), sr.WIN)
    for r, row, Fr in sr.sep_rows(s):
        t = torch.from_numpy(sig[s.sig_off[r]:s.sig_off[r] + s.T[r]].copy()).unfold(0, sr.WIN, sr.HOP)
        assert sr.same_bits(fr[row:row + Fr], t.contiguous().numpy())
    tiles = sr.sep_tiles(s)
    assert all(n <= sr.TILE for _, _, n in tiles) and sum(n for _, _, n in tiles) == sr.sep_M(s)
    for C in sr.SEP_C:
        o = sr.gln_operands(s, C)
        p, e = sr.tile_sums(s, o["x"])
        st, es = sr.region_stats(s, o["x"])
        assert (e > 0).all() and st.shape == (len(s.T), 2)
        for r, row, Fr in sr.sep_rows(s):
            mine = [i for i, (rr, _, _) in enumerate(tiles) if rr == r]
            assert close(p[mine].sum(0), [o["x"][row:row + Fr].astype(np.float64).sum(),
                                          (o["x"][row:row + Fr].astype(np.float64) ** 2).sum()])
            # these statistics through gln_apply: convtasnet_reference._gln on the region
            xr = T64(o["x"][row:row + Fr]).T
            oo = dict(o, stats=np.where(np.arange(len(s.T))[:, None] == r, st, o["stats"]))
            y, eb = sr.gln_apply(s, oo)
            assert close(y[row:row + Fr], ctr._gln(xr, T64(o["gamma"]), T64(o["beta"])).T.numpy(), 1e-8)
            assert (eb > 0).all() and (es[r] > 0).all()
        outside = [r for r in range(len(s.T)) if not s.r0 <= r < s.r0 + s.ng]
        assert (st[outside] == float(sr.SENT)).all()


@pytest.mark.parametrize("c", sr.MID_CASES, ids=sr.mid_id)
def test_mid_matches_depthwise_conv1d(c):
    o = sr.mid_operands(c)
    y, e = sr.mid(c, o)
    assert (e > 0).all() and (o["beta"] != 0).all()
    st, g, be = o["stats"].astype(np.float64), T64(o["gamma"]), T64(o["beta"])
    for r, row, Fr in sr.sep_rows(c.set):
        n = ((T64(o["h"][row:row + Fr]) - st[r, 0]) * (st[r, 1] * g) + be).T          # [C][F]
        w = T64(o["w"]).T[:, None, :]                                                # [C][1][3]
        t = F.prelu(F.conv1d(n[None], w, T64(o["bias"]), padding=c.dil, dilation=c.dil, groups=c.C),
                    torch.tensor([sr.MID_SLOPE], dtype=torch.float64))[0]
        assert close(y[row:row + Fr], t.T.numpy(), 1e-10)
        if c.C <= 256:
            d = ctr._dwconv(n, w, T64(o["bias"]), c.dil)
            assert close(y[row:row + Fr], ctr._prelu(d, torch.tensor(sr.MID_SLOPE, dtype=torch.float64)).T.numpy(), 1e-10)


@pytest.mark.parametrize("c", sr.PRELU_CASES[::2], ids=lambda c: f"rows{c.rows}")
def test_prelu_matches_torch(c):
    o = sr.prelu_operands(c)
    y = sr.prelu(c, o)
    t = F.prelu(torch.from_numpy(o["x"][:, sr.PRELU_COL0:].copy()), torch.tensor([sr.PRELU_SLOPE]))
    assert sr.same_bits(y[:, sr.PRELU_COL0:], t.numpy()) and (y[:, :sr.PRELU_COL0] == sr.SENT).all()


@pytest.mark.parametrize("s", sr.OLA_SETS, ids=lambda s: s.name)
def test_overlap_add_matches_conv_transpose1d(s):
    o = sr.ola_operands(s)
    out = sr.overlap_add(s, o)
    eye = torch.eye(sr.WIN)[:, None, :]
    written = np.zeros(o["n_out"], bool)
    for r, row, Fr in sr.sep_rows(s):
        T, a = int(s.T[r]), int(o["out_off"][r])
        end = (Fr - 1) * sr.HOP + sr.WIN
        for st, dec in enumerate((o["dec0"], o["dec1"])):
            t = F.conv_transpose1d(torch.from_numpy(dec[row:row + Fr].T.copy())[None], eye, stride=sr.HOP)[0, 0]
            assert np.array_equal(out[a + st * T:a + st * T + end], t.numpy())
            assert sr.same_bits(out[a + st * T + end:a + (st + 1) * T], np.zeros(T - end, np.float32))
        written[a:a + 2 * T] = True
    assert (out[~written] == sr.SENT).all() and (~written).sum() >= sum(sr.OLA_GAPS)
    assert not sr.same_bits(o["dec0"], o["dec1"])


# ---- every listed defect is caught by the cases the GPU test runs ----
@pytest.mark.parametrize("defect", sr.DEFECTS["chunk_stats"])
def test_chunk_stats_defects_are_caught(defect):
    assert [c for c in sr.CHUNK_CASES for o in [sr.chunk_operands(c)]
            if caught(*sr.chunk_stats(c, o), sr.chunk_stats(c, o, defect)[0])], defect


@pytest.mark.parametrize("defect", sr.DEFECTS["front"])
def test_front_defects_are_caught(defect):
    assert [T for T in sr.FRONT_T for o in [sr.front_operands(T)]
            if caught(*sr.front(T, o), sr.front(T, o, defect)[0])], defect


@pytest.mark.parametrize("defect", sr.DEFECTS["pool3"])
def test_pool3_defects_are_caught(defect):
    assert [c for c in sr.POOL_CASES for o in [sr.pool_operands(c)]
            if caught(sr.pool3(c, o), None, sr.pool3(c, o, defect), exact=True)], defect


@pytest.mark.parametrize("defect", sr.DEFECTS["frame_stats"])
def test_frame_stats_defects_are_caught(defect):
    assert [c for c in sr.FSTAT_CASES for o in [sr.fstat_operands(c)]
            if caught(*sr.frame_stats(c, o), sr.frame_stats(c, o, defect)[0])], defect


@pytest.mark.parametrize("defect", sr.DEFECTS["norm_act"])
def test_norm_act_defects_are_caught(defect):
    assert [c for c in sr.NORM_CASES for o in [sr.norm_operands(c)]
            if caught(*sr.norm_act(c, o), sr.norm_act(c, o, defect)[0])], defect


@pytest.fixture(scope="module")
def lstm_refs():
    return {Fr: (sr.lstm_operands(Fr),) + sr.lstm_bound(sr.lstm_operands(Fr)) for Fr in sr.LSTM_F}


@pytest.mark.parametrize("defect", sr.DEFECTS["lstm"])
def test_lstm_defects_are_caught(lstm_refs, defect):
    hits = []
    for Fr, (o, ref, bound, _) in lstm_refs.items():
        for B in sr.LSTM_GROUPS:
            for n in sr.lstm_ns(B):
                if sr.worst_ratio(sr.lstm(o, n, B=B, defect=defect), ref[:n], bound) > 1.0:
                    hits.append((Fr, B, n))
    assert hits, defect


def test_lstm_float32_deviation_per_case(lstm_refs):
    for Fr, (_, _, bound, dev) in lstm_refs.items():
        print(f"seg_lstm F = {Fr}, {sr.LSTM_MAX_N} sequences (CPU): float32 vs float64 {dev:.2e}; device bound {bound:.2e}")
        # a float32 restatement cannot be better than a fraction of u nor, on at most 9
        # well-conditioned steps, worse than a few hundred u: outside that the bound means nothing
        assert 2.0 ** -27 < dev < 1e-5 and bound < 1e-4


@pytest.mark.parametrize("defect", sr.DEFECTS["head"])
def test_head_defects_are_caught(defect):
    hits = []
    for c in sr.HEAD_CASES:
        o = sr.head_operands(c)
        ref, e = sr.head(c, o)
        if defect == "tie_to_higher_index":
            lg = ref.astype(np.float32)
            if caught(sr.head_classes(lg), None, sr.head_classes(lg, defect), exact=True):
                hits.append(c)
        elif caught(ref, e, sr.head(c, o, defect)[0]):
            hits.append(c)
    assert hits, defect
    if defect == "no_max_subtraction":
        assert [c.kind for c in hits] == ["large"]


@pytest.mark.parametrize("defect", sr.DEFECTS["region_stats"])
def test_region_stats_defects_are_caught(defect):
    assert [(s.name, C) for s in sr.SEP_SETS for C in sr.SEP_C for x in [sr.gln_operands(s, C)["x"]]
            if caught(*sr.region_stats(s, x), sr.region_stats(s, x, defect)[0])], defect


def test_gln_defect_is_caught_by_the_second_group_alone():
    hits = [s.name for s in sr.SEP_SETS for o in [sr.gln_operands(s, 128)]
            if caught(*sr.gln_apply(s, o), sr.gln_apply(s, o, "region_group_relative")[0])]
    assert hits == ["group2of5"]


@pytest.mark.parametrize("defect", sr.DEFECTS["mid"])
def test_mid_defects_are_caught(defect):
    hits = []
    for c in sr.MID_CASES:
        o = sr.mid_operands(c)
        ref, e = sr.mid(c, o)
        if defect == "partials_before_prelu":
            if caught(*sr.mid_partials(c, ref), sr.mid_partials(c, ref, defect)[0]):
                hits.append(sr.mid_id(c))
        elif caught(ref, e, sr.mid(c, o, defect)[0]):
            hits.append(sr.mid_id(c))
    assert hits, defect
    if defect == "second_channel_pass_skipped":
        assert all("C2048" in h for h in hits)


@pytest.mark.parametrize("defect", sr.DEFECTS["prelu"])
def test_prelu_defects_are_caught(defect):
    assert [c for c in sr.PRELU_CASES for o in [sr.prelu_operands(c)]
            if caught(sr.prelu(c, o), None, sr.prelu(c, o, defect), exact=True)], defect


@pytest.mark.parametrize("defect", sr.DEFECTS["overlap_add"])
def test_overlap_add_defects_are_caught(defect):
    assert [s.name for s in sr.OLA_SETS for o in [sr.ola_operands(s)]
            if caught(sr.overlap_add(s, o), None, sr.overlap_add(s, o, defect), exact=True)], defect
