"""CPU checks of tests/aux_reference.py: every float64 restatement against torch in float64,
the float32 ones against an independent formulation, every listed single defect caught by the
case tables the GPU test runs, the all-masked attention row, and the LSTM's float32 deviation
(written into profiles/aux_kernels/README.md when that file carries the marker line)."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aux_reference as ar

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
README = os.path.join(REPO, "profiles", "aux_kernels", "README.md")
T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
SMALL_CONV = [c for c in ar.CONV_CASES if c.n <= 3]


def close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    return float(np.max(np.abs(a - b))) <= tol * max(1.0, float(np.max(np.abs(b)))) if a.size else True


# ---- the restatements against torch float64 ----
def test_case_tables_hold_what_the_issue_lists():
    ids = [ar.conv_id(c) for c in ar.CONV_CASES]
    assert len(set(ids)) == len(ids)
    have = {(c.fi, c.sf, c.rb, c.T) for c in ar.MFMA_ROW_CASES}
    assert {(9, 1, 4, 81), (10, 2, 6, 81), (9, 1, 10, 17), (5, 1, 6, 17)} <= have
    assert [ar.conv_fo(c) for c in ar.MFMA_PICK_CASES] == [6, 5]
    assert len(ar.MFMA_EPI_CASES) == 8 and all(c.n == 3 for c in ar.MFMA_EPI_CASES)
    assert sum(1 for c in ar.ATTN_CASES if c.D == 64 and c.L == 256) == 1
    # the engine's rows-per-block pick, restated: about 2048 blocks, an even count, at least 2
    for c in ar.MFMA_PICK_CASES + [ar.BOTH_ROUTES[1]]:
        pairs = (ar.conv_fo(c) + 1) // 2
        chunks = max(1, min(pairs, -(-2048 // c.n)))
        assert 2 * -(-pairs // chunks) == c.rb_used


@pytest.mark.parametrize("c", SMALL_CONV, ids=[ar.conv_id(c) for c in SMALL_CONV])
def test_conv2d_matches_torch(c):
    o = ar.conv_operands(c)
    y, e = ar.conv2d(c, o)
    x = T64(o["x"])
    if c.in_tf:
        x = x.transpose(1, 2)[:, None]
    t = F.conv2d(x, T64(o["w"]), stride=(c.sf, 1), padding=c.ks // 2)
    t = t * T64(o["scale"])[None, :, None, None] + T64(o["shift"])[None, :, None, None]
    if c.res:
        t = t + T64(o["res"])
    if c.relu:
        t = torch.relu(t)
    if c.tdnn:   # [n][T][co * fo + f]
        t = t.permute(0, 3, 1, 2).reshape(c.n, c.T, -1)
    assert y.shape == ar.conv_out_shape(c) == tuple(t.shape) and e.shape == y.shape
    assert close(y, t.numpy()) and (e > 0).all()


@pytest.mark.parametrize("c", ar.CAM_CASES, ids=lambda c: "n{}_T{}_seg{}".format(*c))
def test_cam_mask_matches_torch(c):
    o = ar.cam_operands(c)
    m, e = ar.cam_mask(c, o)
    h = T64(o["h"]).transpose(1, 2)                       # [n][128][T]
    seg = F.avg_pool1d(h, kernel_size=c.seg, stride=c.seg, ceil_mode=True)
    nseg = seg.shape[-1]
    seg = seg[..., None].expand(-1, -1, -1, c.seg).reshape(c.n, 128, nseg * c.seg)[..., :c.T]
    ctx = (h.mean(-1, keepdim=True) + seg).transpose(1, 2)
    t = torch.sigmoid(F.linear(torch.relu(F.linear(ctx, T64(o["w1"]), T64(o["b1"]))), T64(o["w2"]), T64(o["b2"])))
    assert close(m[:, :c.T], t.numpy()) and (m[:, c.T] == float(ar.SENT)).all() and (e > 0).all()


@pytest.mark.parametrize("c", ar.STATS_CASES, ids=lambda c: "N{}_T{}_C{}_{}".format(*c))
def test_stats_match_torch(c):
    o = ar.stats_operands(c)
    out, e = ar.stats_pool(c, o)
    v = torch.relu(T64(o["x"]) * T64(o["s"]) + T64(o["b"]))
    with np.errstate(all="ignore"):
        t = torch.cat([v.mean(1), torch.std(v, dim=1, unbiased=True)], 1).numpy()
    assert np.array_equal(np.isnan(out), np.isnan(t))
    assert close(np.nan_to_num(out), np.nan_to_num(t), 1e-11)
    if c.special == "one_frame":
        assert np.isnan(out[:, c.C:]).all() and np.isfinite(out[:, :c.C]).all()
    if c.special == "negative_column":
        assert (out[:, 2] == 0).all() and (out[:, c.C + 2] == 0).all()


def test_cmvn_matches_torch():
    o = ar.cmvn_operands()
    y, e = ar.cmvn(o)
    x, off = T64(o["x"]), o["fr_off"]
    t = x.clone()
    for a, b in zip(off[:-1], off[1:]):
        if b > a:
            t[a:b] = x[a:b] - x[a:b].mean(0, keepdim=True)
    assert close(y, t.numpy())
    assert (e[:off[0]] == 0).all() and (e[off[-1]:] == 0).all() and (y[:off[0]] == o["x"][:off[0]]).all()
    assert sorted(np.diff(off).tolist()) == sorted(ar.CMVN_LENS)


def test_lstm_matches_torch_lstmcell():
    o = ar.lstm_operands()
    p, s_out, e_out = ar.lstm(o, [0], [ar.LSTM_WINDOWS])
    cell = torch.nn.LSTMCell(1, 128, dtype=torch.float64)
    with torch.no_grad():
        cell.weight_ih.zero_()
        cell.bias_ih.zero_()
        cell.weight_hh.copy_(T64(o["whh"]))
        cell.bias_hh.copy_(T64(o["bhh"]))
        h = c = torch.zeros(1, 128, dtype=torch.float64)
        probs = []
        gx = T64(o["gx"])
        for w in range(ar.LSTM_WINDOWS):
            # x W_ih^T + b_ih is the given gx[w]: fed as the input bias of this step
            cell.bias_ih.copy_(gx[w])
            h, c = cell(torch.zeros(1, 1, dtype=torch.float64), (h, c))
            probs.append(torch.sigmoid(torch.relu(h) @ T64(o["wd"]) + float(o["bd"])))
    assert close(p, torch.cat(probs).numpy())
    assert close(e_out[0, 0], h[0].numpy()) and close(e_out[0, 1], c[0].numpy())
    assert (s_out[0] == 0).all()
    # these operands keep every probability away from saturation, so a dropped term moves them
    assert 0.1 < p.min() and p.max() < 0.9


@pytest.mark.parametrize("c", ar.LN_CASES, ids=lambda c: "rows{}_H{}_embed{}".format(*c))
def test_layer_norm_matches_torch(c):
    o = ar.ln_operands(c)
    y, e = ar.layer_norm(c, o)
    if c.embed:
        pos = np.tile(np.arange(o["L"]), ar.LN_EMBED_B)
        v = T64(o["word"])[o["ids"]] + T64(o["pos"])[pos] + T64(o["type"])[o["tt"]]
    else:
        v = T64(o["x"])
    t = F.layer_norm(v, (c.H,), T64(o["g"]), T64(o["b"]), ar.LN_EPS)
    # at H = 1 and on the mean-50 row the f64 rounding of (v - mean) rstd is what is left
    assert close(y, t.numpy(), 1e-9) and (e > 0).all()


@pytest.mark.parametrize("mask", ar.ATTN_MASKS, ids="_".join)
@pytest.mark.parametrize("c", [c for c in ar.ATTN_CASES if c.L <= 65], ids=lambda c: "h{}_D{}_L{}".format(*c))
def test_attention_matches_torch(c, mask):
    o = ar.attn_operands(c, mask)
    ctx, e = ar.attention(c, o)
    heads, D, L = c
    qkv = T64(o["qkv"]).reshape(2, L, 3, heads, D)
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * float(np.float32(1.0 / math.sqrt(D)))
    # the float32 graph's additive mask, its sum rounded to float32
    add = torch.from_numpy(np.where(o["mask"].reshape(2, 1, 1, L) != 0, 0.0, ar.F32_MIN))
    s = torch.where(add == 0, s, (s + add).to(torch.float32).to(torch.float64))
    t = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(2 * L, heads * D)
    assert close(ctx, t.numpy()) and (e > 0).all()


def test_all_masked_row_is_the_mean_of_v_and_an_exact_mask_is_not():
    c = ar.AttnCase(2, 16, 65)
    o = ar.attn_operands(c, ar.ATTN_MASKS[1])       # sequence 0: zeros in the middle; 1: all masked
    ctx, e = ar.attention(c, o)
    v = o["qkv"].astype(np.float64).reshape(2, c.L, 3, 2 * 16)[1, :, 2]
    assert close(ctx[c.L:], np.broadcast_to(v.mean(0), (c.L, 32)))
    other, _ = ar.attention(c, o, mask_exact=True)
    assert ar.worst_ratio(other[:c.L], ctx[:c.L], e[:c.L]) == 0.0        # sequence 0 keeps some keys
    assert ar.worst_ratio(other[c.L:], ctx[c.L:], e[c.L:]) > 100.0       # an exact sum keeps s
    # a literal float64 addition absorbs s as the float32 one does (the offset's ulp is 2^75)
    s = o["qkv"].astype(np.float64)[:, :8] * 7.0
    assert ((s + ar.F32_MIN) == ar.F32_MIN).all()
    assert ((s + ar.F32_MIN).astype(np.float32) == np.float32(ar.F32_MIN)).all()


# ---- the float32 references against independent formulations ----
def test_vad_frames_reference():
    o = ar.vad_file_operands("a")
    fr = ar.vad_frames_files(o)
    assert fr.shape == (o["n_windows"] * 4, 256) and fr.dtype == np.float32
    # window 1 of file 0, as torch: [64 context | 512 | reflect 64], frames of 256 every 128
    x = torch.from_numpy(o["audio"][512 - 64:1024].copy())[None, None]
    padded = F.pad(x, (0, 64), mode="reflect")[0, 0]
    assert ar.same_bits(fr[4:8], padded.unfold(0, 256, 128).numpy())
    assert (fr[0, :64] == 0).all() and ar.same_bits(fr[0, 64:], o["audio"][:192])
    # row mode on the same 576 samples
    assert ar.same_bits(ar.vad_frames_rows(padded[None, :576].numpy()), fr[4:8])
    mx = ar.vad_maxabs(o)
    assert [float(m) for m in mx.view(np.float32)] == [
        float(np.float32(p)) if n else 0.0 for p, n in zip(ar.VAD_PEAKS["a"], o["len"])]
    assert (np.asarray(ar.VAD_WINDOWS) == o["len"] // 512).all() and sorted(o["len"][np.asarray(ar.VAD_WINDOWS) == 0]) == [0, 100, 100, 511]
    boosted = ar.vad_frames_files(o, mx)
    k = np.float32(0.071) / np.float32(0.0709)
    assert ar.same_bits(boosted[:12], fr[:12] * k) and ar.same_bits(boosted[12:], fr[12:])


def test_vad_im2col_references():
    rng = np.random.default_rng(3)
    for N, T, C, stride in ar.IM2COL_CASES:
        Y = rng.standard_normal((N * T, C), dtype=np.float32)
        A = ar.vad_im2col(Y, N, T, C, stride)
        t = F.unfold(torch.from_numpy(Y.reshape(N, T, C)).permute(0, 2, 1)[:, :, :, None], (3, 1),
                     padding=(1, 0), stride=(stride, 1))               # [N][C * 3][Tout]
        t = t.reshape(N, C, 3, -1).permute(0, 3, 2, 1).reshape(A.shape)
        assert ar.same_bits(A, t.contiguous().numpy())
    for nw, bins, ldS, Kp in ar.MAG_CASES:
        S = rng.standard_normal((nw * 4, ldS), dtype=np.float32)
        A = ar.vad_mag_im2col(S, bins, Kp)
        mag = np.sqrt(S[:, :bins] * S[:, :bins] + S[:, bins:2 * bins] * S[:, bins:2 * bins])
        assert ar.same_bits(A[:, 3 * bins:], np.zeros((nw * 4, Kp - 3 * bins), np.float32))
        assert ar.same_bits(A[:, :3 * bins], ar.vad_im2col(mag, nw, 4, bins, 1))


def test_gather_references():
    for c in ar.GATHER_CASES:
        o = ar.gather_operands(c)
        out = ar.campp_gather(c, o)
        assert sorted(set(o["win_n"].tolist())) == sorted({1, c.wf - 1, c.wf})
        for w in range(len(o["win_n"])):
            n, r = o["win_n"][w], o["win_row"][w]
            assert ar.same_bits(out[w, :n], o["rows"][r:r + n]) and (out[w, n:] == 0).all()
    o = ar.vibert_gather_operands()
    g = ar.vibert_gather(o)
    t = torch.from_numpy(o["x"]).reshape(o["B"], o["L"], -1)
    t = torch.gather(t, 1, torch.from_numpy(o["off"])[:, :, None].expand(-1, -1, o["H"]))
    assert ar.same_bits(g, t.reshape(-1, o["H"]).numpy())


# ---- every listed defect is caught by the cases the GPU test runs ----
def caught(ref, bound, bad, exact=False):
    if exact:
        return not ar.same_bits(ref, bad)
    return ar.worst_ratio(bad, ref, bound) > 1.0


@pytest.mark.parametrize("defect", ar.DEFECTS["conv2d"])
def test_conv2d_defects_are_caught(defect):
    hits = [ar.conv_id(c) for c in SMALL_CONV for o in [ar.conv_operands(c)]
            if caught(*ar.conv2d(c, o), ar.conv2d(c, o, defect)[0])]
    assert hits, defect


@pytest.mark.parametrize("defect", ar.DEFECTS["cam_mask"])
def test_cam_mask_defects_are_caught(defect):
    hits = []
    for c in ar.CAM_CASES:
        o = ar.cam_operands(c)
        ref, e = ar.cam_mask(c, o)
        bad, _ = ar.cam_mask(c, o, defect)
        if caught(ref[:, :c.T], e, bad[:, :c.T]) or (bad[:, c.T] != float(ar.SENT)).any():
            hits.append(c)
    assert hits, defect


@pytest.mark.parametrize("defect", ar.DEFECTS["stats"])
def test_stats_defects_are_caught(defect):
    hits = [c for c in ar.STATS_CASES for o in [ar.stats_operands(c)]
            if caught(*ar.stats_pool(c, o), ar.stats_pool(c, o, defect)[0])]
    assert hits, defect
    if defect == "one_pass_variance_f32":
        assert any(c.special == "offset_column" for c in hits)


@pytest.mark.parametrize("defect", ar.DEFECTS["cmvn"])
def test_cmvn_defects_are_caught(defect):
    o = ar.cmvn_operands()
    assert caught(*ar.cmvn(o), ar.cmvn(o, defect)[0]), defect


@pytest.mark.parametrize("defect", ar.DEFECTS["vad_frames"])
def test_vad_frames_defects_are_caught(defect):
    hits = []
    for peaks in ar.VAD_PEAKS:
        o = ar.vad_file_operands(peaks)
        for mx in (None, ar.vad_maxabs(o)):
            if caught(ar.vad_frames_files(o, mx), None, ar.vad_frames_files(o, mx, defect), exact=True):
                hits.append((peaks, mx is not None))
    assert hits, defect


@pytest.mark.parametrize("defect", ar.DEFECTS["vad_im2col"])
def test_vad_im2col_defects_are_caught(defect):
    rng = np.random.default_rng(5)
    hits = []
    for N, T, C, stride in ar.IM2COL_CASES:
        Y = rng.standard_normal((N * T, C), dtype=np.float32)
        if caught(ar.vad_im2col(Y, N, T, C, stride), None, ar.vad_im2col(Y, N, T, C, stride, defect), exact=True):
            hits.append((N, T, C, stride))
    assert hits, defect


def lstm_scenarios(o):
    """(name, seg_start, seg_count, seg_warm, init) of every launch the GPU test compares."""
    one = ar.lstm(o, [0], [48])
    st = lambda w: np.stack(ar.lstm(o, [0], [w])[2][0]) if w else np.zeros((2, 128))
    chain = [st(0), st(20), st(21), st(21)]
    return [
        ("one", [0], [48], None, None),
        ("chain", [0, 20, 21, 21], [20, 1, 0, 27], None, np.stack(chain)),
        ("warm", [20], [28], [5], st(15)[None]),
        ("empty", [7], [0], [0], st(7)[None]),
        ("empty_warm", [10], [0], [3], st(7)[None]),
    ], one


@pytest.mark.parametrize("defect", ar.DEFECTS["lstm"])
def test_lstm_defects_are_caught(defect):
    o = ar.lstm_operands()
    scen, _ = lstm_scenarios(o)
    hits = []
    for name, ss, sc, sw, init in scen:
        ref, bound, _ = ar.lstm_bound(o, ss, sc, sw, init)
        bad = ar.lstm(o, ss, sc, sw, init, defect=defect)
        if any(ar.worst_ratio(b, r, e) > 1.0 for b, r, e in zip(bad, ref, bound)):
            hits.append(name)
    assert hits, defect


@pytest.mark.parametrize("defect", ar.DEFECTS["layer_norm"])
def test_layer_norm_defects_are_caught(defect):
    hits = [c for c in ar.LN_CASES for o in [ar.ln_operands(c)]
            if caught(*ar.layer_norm(c, o), ar.layer_norm(c, o, defect)[0])]
    assert hits, defect


@pytest.mark.parametrize("defect", ar.DEFECTS["attention"])
def test_attention_defects_are_caught(defect):
    hits = []
    for c in ar.ATTN_CASES:
        if c.L > 65 and defect != "keys_past_64_dropped":
            continue
        for mask in ar.ATTN_MASKS:
            o = ar.attn_operands(c, mask)
            if caught(*ar.attention(c, o), ar.attention(c, o, defect)[0]):
                hits.append((c, mask))
                break
    assert hits, defect
    if defect == "keys_past_64_dropped":
        assert any(c.L == 65 for c, _ in hits) and not any(c.L <= 64 for c, _ in hits)


def test_vibert_gather_defect_is_caught():
    o = ar.vibert_gather_operands()
    assert caught(ar.vibert_gather(o), None, ar.vibert_gather(o, "offset_without_batch"), exact=True)


# ---- the LSTM's float32 deviation, the base of its bound ----
def test_lstm_float32_deviation_is_recorded():
    o = ar.lstm_operands()
    _, bound, dev = ar.lstm_bound(o, [0], [ar.LSTM_WINDOWS])
    print(f"LSTM float32 vs float64 over {ar.LSTM_WINDOWS} windows: probs {dev[0]:.2e}, state {dev[2]:.2e}")
    # a float32 restatement cannot be better than a few u nor, on 48 well-conditioned steps,
    # worse than a few hundred: outside that the bound would mean nothing
    assert 2.0 ** -26 < dev[0] < 1e-5 and 2.0 ** -26 < dev[2] < 1e-5
    assert bound[0] < 1e-4 and bound[2] < 1e-4
    line = (f"LSTM float32 restatement against float64, {ar.LSTM_WINDOWS} windows (CPU): probabilities "
            f"{dev[0]:.2e}, state {dev[2]:.2e}; device bound 8 x = {bound[0]:.2e} / {bound[2]:.2e}")
    if os.path.exists(README) and os.access(README, os.W_OK):
        text = open(README).read()
        new = re.sub(r"(?m)^LSTM float32 restatement against float64.*$", line, text)
        if new != text:
            open(README, "w").write(new)
