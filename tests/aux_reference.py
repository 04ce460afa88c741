"""References for the CAM++, Silero VAD and ViBERT kernels run alone (zasr_selftest_campp_*,
_vad_*, _vibert_*): the case tables, the seeded operands, a float64 (or, where the operation is
data movement, float32) restatement of every operation, and the per-element bound.
tests/test_aux_reference.py pins every restatement to torch in float64 on the CPU and shows
that each case table has power; tests/test_gpu_aux_kernels.py compares the kernels with it.

Every restatement takes a `defect` name.  With None it is the reference; with a name it is the
same operation with that single defect, a transcription of how a kernel could be wrong.  The
CPU test demands that every defect in DEFECTS pushes at least one case of its group over the
bound or breaks an exact comparison, so a case table that could not see it fails there.

Bounds are a-priori and elementwise, u = 2^-24, carried through the epilogues in float64:

    conv2d      (K + 4) u sum |x| |w| |scale| for the K = ci ks ks products (K u: the worst
                case of an f32 sum of K terms; 4: the MFMA's four-product inner sum is not
                step-wise IEEE), + u |y| for the fused multiply-add of scale / shift, + u |y|
                for the residual add.  ReLU has slope <= 1.
    CAM mask    the frame sums are float64: the context carries u (|global mean| + |segment
                mean| + |context|) for its two roundings to f32 and their f32 add; each linear
                layer adds (fan_in + 4) u (|w| |in| + |b|) and passes the incoming error through
                |w|; the sigmoid has slope 1/4 and expf gets ACT_ABS.
    stats       relu(fma(x, s, b)) carries u |x s + b| per element; the mean of those plus
                u |mean| (the float64 sum's own error is 2^-29 of that); the std, a 2-norm of
                the centred column over sqrt(T - 1), moves by at most |e|_2 / sqrt(T - 1) plus
                u |std|.
    CMVN        u |mean| + u |x - mean|.
    LayerNorm   the statistics are float64.  y = ((v - (float)mean) rstd) g + b: u |mean| rstd
                |g| for the rounded mean, 6 u |n g| for the subtraction, rstd's two roundings and
                the products, 2 u |y| for the last multiply-add.  The embedding form forms v in
                f32 first: e_v = u (|word + pos| + |v|), which reaches n as rstd (e_v +
                mean e_v + |n| mean(|n| e_v)) (the derivative of the normalisation).
    attention   scores (D + 1) u sum |q| |k| scale + u |s|; p = exp(s - max) relative e_s + max
                e_s, absolute ACT_ABS for __expf; the context is a ratio, so a common factor of
                p cancels: sum dp (|v| + |ctx|) / sum p (>= sum dp |v - ctx| / sum p), plus (L + 4) u sum p |v| / sum p for the
                sequential f32 accumulation and the final product.
    LSTM        no a-priori bound (the error feeds back): 8 x the deviation of a plain float32
                numpy restatement from the float64 one, floor 16 u, measured per case.

Masked attention scores are formed as the model's float32 graph forms them: s scale +
finfo(float32).min rounded to float32.  Every masked key then has the same score, exp(score -
max) is exactly 0 beside an unmasked key, and a row whose keys are all masked is the plain mean
of V.  A restatement that carried the sum exactly would keep s under the offset, the offset
would cancel in the softmax, and that row would come out as a softmax over s: a different
answer (attention(..., mask_exact=True); test_aux_reference.py shows the two differ by far more
than the bound).  A literal float64 addition does not reach that: the offset's ulp is 2^75 in
float64, so s is absorbed there too and the float64 sum agrees with the float32 one; the same
test holds that, so the rounding step below is what is specified, not an accident of the width.

VAD frames, both im2col kernels, the gathers, the maxabs bits and the boost factor 0.071f / m
are data movement plus correctly rounded f32 operations: their reference is float32 numpy and the
comparison is bit for bit.
"""
import math
import zlib
from collections import namedtuple

import numpy as np

from attention_reference import U_TANH  # noqa: F401  (the project's tanhf term; LSTM notes)
from test_gpu_gemm import ACT_ABS

U = 2.0 ** -24
C_DOT = 4                      # the constant c of (K + c) u
SENT = np.float32(-777.25)     # every output element before a call
F32_MIN = float(np.finfo(np.float32).min)
f64 = np.float64


def _rng(tag, c):
    return np.random.default_rng(zlib.crc32((tag + repr(tuple(c))).encode()))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; equal values (0 / 0, NaN beside NaN) count as 0, a NaN or
    infinity on one side only as infinite."""
    got, ref, bound = np.asarray(got, f64), np.asarray(ref, f64), np.asarray(bound, f64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    with np.errstate(all="ignore"):
        r = np.abs(got - ref) / np.broadcast_to(bound, ref.shape)
    r = np.where(same, 0.0, np.where(np.isfinite(r), r, np.inf))
    return float(r.max()) if r.size else 0.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------
# CAM++ conv2d
# ---------------------------------------------------------------------------------------------
# mfma: the entry passes the permuted weights; rb: rows per block (0 = the engine's pick);
# route / rb_used: what the entry must report (route 1 = the MFMA kernel, 0 = the direct one)
ConvCase = namedtuple("ConvCase", "ks ci fi sf T n relu tdnn in_tf res mfma rb route rb_used")


def conv_fo(c):
    return (c.fi - 1) // c.sf + 1


def _mf(fi, sf, T, rb, n=1, relu=1, tdnn=0, res=1, rb_used=None):
    return ConvCase(3, 32, fi, sf, T, n, relu, tdnn, 0, res, 1, rb, 1, rb if rb_used is None else rb_used)


def _even_up(v):
    return v + (v & 1)


MFMA_T_CASES = [_mf(5, 1, T, 2) for T in (1, 15, 16, 17, 79, 80, 81, 160)]
MFMA_ROW_CASES = [
    _mf(fi, sf, T, rb, n=2)
    for fi, sf in ((4, 1), (5, 1), (5, 2), (6, 2), (7, 2), (9, 1), (10, 2))
    for rb in sorted({2, 4, _even_up((fi - 1) // sf + 1)})
    for T in (17, 81)]
MFMA_EPI_CASES = [_mf(9, 1, 81, 4, n=3, relu=relu, tdnn=tdnn, res=res)
                  for res in (0, 1) for relu in (0, 1) for tdnn in (0, 1)]
MFMA_PICK_CASES = [_mf(6, 1, 3, 0, n=1025, rb_used=4), _mf(5, 1, 2, 0, n=2048, rb_used=6)]
MFMA_CASES = MFMA_T_CASES + MFMA_ROW_CASES + MFMA_EPI_CASES + MFMA_PICK_CASES


def _dr(ks, ci, fi, sf, T, n=2, relu=1, tdnn=0, in_tf=0, res=0, mfma=0):
    return ConvCase(ks, ci, fi, sf, T, n, relu, tdnn, in_tf, res, mfma, 0, 0, 0)


DIRECT_CASES = (
    [_dr(3, 1, 5, 1, T, in_tf=1) for T in (1, 63, 64, 65, 130)]
    + [_dr(3, 32, 5, 1, 65, res=1), _dr(3, 32, 5, 1, 161, res=1),
       _dr(3, 32, 5, 1, 161, res=1, mfma=1),       # T > 160: the launcher falls to the direct kernel
       _dr(3, 32, 6, 2, 81, res=1, tdnn=1)]        # also on the MFMA route (BOTH_ROUTES)
    + [_dr(1, 32, fi, 2, T) for fi in (5, 6) for T in (1, 64, 65)]
    + [_dr(3, 3, 5, 1, 17, res=1)])
BOTH_ROUTES = (_dr(3, 32, 6, 2, 81, res=1, tdnn=1),
               ConvCase(3, 32, 6, 2, 81, 2, 1, 1, 0, 1, 1, 0, 1, 2))
CONV_CASES = MFMA_CASES + DIRECT_CASES + [BOTH_ROUTES[1]]


def conv_id(c):
    return "ks{}_ci{}_fi{}_sf{}_T{}_n{}_relu{}_tdnn{}_tf{}_res{}_mfma{}_rb{}".format(*c[:12])


def conv_operands(c):
    rng = _rng("conv", c[:10])     # both routes of a case see the same operands
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    x = f(c.n, c.T, c.fi) if c.in_tf else f(c.n, c.ci, c.fi, c.T)
    w = f(32, c.ci, c.ks, c.ks) / np.float32(math.sqrt(c.ci * c.ks * c.ks))
    scale = rng.uniform(0.5, 1.5, 32).astype(np.float32)
    shift = f(32) * np.float32(0.5)
    res = f(c.n, 32, conv_fo(c), c.T) * np.float32(0.5) if c.res else None
    return dict(x=x, w=w, scale=scale, shift=shift, res=res)


def conv_out_shape(c):
    fo = conv_fo(c)
    return (c.n, c.T, 32 * fo) if c.tdnn else (c.n, 32, fo, c.T)


def conv2d(c, o, defect=None):
    """(y, bound) in the output's layout, float64; unwritten elements hold SENT."""
    fo, pad, T, fi, ks = conv_fo(c), c.ks // 2, c.T, c.fi, c.ks
    x = o["x"].astype(f64)
    if c.in_tf:
        x = (x.reshape(c.n, fi, T) if defect == "in_tf_read_as_ft" else x.transpose(0, 2, 1))[:, None]
    w = o["w"].astype(f64)
    # rows 0 .. fi - 1, row fi (the padding row below), row fi + 1 = zeros; columns likewise
    xe = np.zeros((c.n, c.ci, fi + 2, T + 2))
    xe[:, :, :fi, :T] = x
    if defect == "pad_col_clamped":
        xe[:, :, :fi, T] = x[:, :, :, T - 1]
    if defect == "row_fi_clamped":
        xe[:, :, fi, :T] = x[:, :, fi - 1, :]
    fw = np.arange(fo)
    acc = np.zeros((c.n, 32, fo, T))
    S = np.zeros_like(acc)
    for r in range(ks):
        g = fw * (1 if defect == "stride_ignored" else c.sf) - pad + r
        if defect == "ring_stale" and c.route == 1:
            rows, begin = c.sf + ks, (fw // c.rb_used) * c.rb_used
            late = ((fw - begin) // 2 >= 1) & (g >= begin * c.sf - pad + rows)
            g = np.where(late, g - rows, g)
        g = np.where((g >= 0) & (g <= fi), g, fi + 1)
        for q in range(ks):
            t = np.arange(T) - pad + q
            t = np.where((t >= 0) & (t <= T), t, T + 1)
            xs = xe[:, :, g][:, :, :, t]
            acc += np.einsum("ncft,oc->noft", xs, w[:, :, r, q])
            S += np.einsum("ncft,oc->noft", np.abs(xs), np.abs(w[:, :, r, q]))
    sc, sh = o["scale"].astype(f64), o["shift"].astype(f64)
    if defect == "scale_shift_swapped16":
        sc, sh = sc[np.arange(32) ^ 16], sh[np.arange(32) ^ 16]
    sc, sh = sc[None, :, None, None], sh[None, :, None, None]
    y = acc * sc + sh
    e = (c.ci * ks * ks + C_DOT) * U * S * np.abs(sc) + U * np.abs(y)
    if c.res:
        res = o["res"].astype(f64)
        if defect == "res_row_above":
            res = res[:, :, np.maximum(fw - 1, 0)]
        y = y + res
        e = e + U * np.abs(y)
    if c.relu:
        y = np.maximum(y, 0.0)
    if defect == "odd_last_row_unwritten" and fo % 2 == 1:
        y[:, :, fo - 1] = SENT
    if c.tdnn:
        lay = lambda v: v.transpose(0, 3, 1, 2).reshape(c.n, T, 32 * fo)
        bad = lambda v: v.transpose(0, 3, 2, 1).reshape(c.n, T, 32 * fo)
        return (bad(y) if defect == "tdnn_index_fo_major" else lay(y)), lay(e)
    return y, e


# ---------------------------------------------------------------------------------------------
# CAM mask, statistics pooling, CMVN, window gather
# ---------------------------------------------------------------------------------------------
CamCase = namedtuple("CamCase", "n T seg")
CAM_CASES = [CamCase(n, T, seg) for n in (1, 3)
             for T, seg in ((1, 100), (2, 100), (15, 100), (16, 100), (17, 100), (31, 7), (33, 16),
                            (100, 100), (101, 100), (201, 100))]


def cam_operands(c):
    rng = _rng("cam", c)
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    return dict(h=f(c.n, c.T, 128), w1=f(64, 128) / np.float32(math.sqrt(128)),
                b1=f(64) * np.float32(0.5), w2=f(32, 64) / np.float32(8.0), b2=f(32) * np.float32(0.5))


def cam_mask(c, o, defect=None):
    """(mexp [n][T + 1][32], bound [n][T][32]): frame T is the first frame behind the output,
    SENT unless something wrote there."""
    T, L = c.T, c.seg
    h = o["h"].astype(f64)
    w1, b1, w2, b2 = (o[k].astype(f64) for k in ("w1", "b1", "w2", "b2"))
    hs = h.copy()
    if defect == "tail_frames_left_out":
        hs[:, 16 * (T // 16):] = 0.0
    out = np.full((c.n, T + 1, 32), float(SENT))
    bound = np.zeros((c.n, T, 32))
    late = []
    for g in range((T + L - 1) // L):
        s0, s1 = g * L, min(T, g * L + L)
        seg = hs[:, s0:s1].sum(1)
        gm = seg / (s1 - s0) if defect == "global_mean_over_segment" else hs.sum(1) / T
        sm = seg / (L if defect == "clipped_divided_by_seg_len" else s1 - s0)
        ctx = gm + sm
        e = U * (np.abs(gm) + np.abs(sm) + np.abs(ctx))
        z = ctx @ w1.T + b1
        e = e @ np.abs(w1).T + (128 + C_DOT) * U * (np.abs(ctx) @ np.abs(w1).T + np.abs(b1))
        z = np.maximum(z, 0.0)
        m = z @ w2.T + b2
        e = e @ np.abs(w2).T + (64 + C_DOT) * U * (z @ np.abs(w2).T + np.abs(b2))
        p = 1.0 / (1.0 + np.exp(-m))
        out[:, s0:s1] = p[:, None]
        bound[:, s0:s1] = (0.25 * e + ACT_ABS)[:, None]
        late.append((s1, p))
    if defect == "mask_written_to_s1":
        for s1, p in late:
            out[:, s1] = p
    return out, bound


StatsCase = namedtuple("StatsCase", "N T C special")
STATS_CASES = [StatsCase(*s, "") for s in ((1, 2, 1), (3, 75, 127), (1, 75, 128), (3, 2, 129), (1, 115, 512))] + [
    StatsCase(2, 1, 5, "one_frame"), StatsCase(2, 40, 6, "negative_column"),
    StatsCase(2, 64, 6, "offset_column")]


def stats_operands(c):
    rng = _rng("stats", c)
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    x, s, b = f(c.N, c.T, c.C), rng.uniform(0.5, 1.5, c.C).astype(np.float32), f(c.C) * np.float32(0.5)
    if c.special == "negative_column":   # column 2: every pre-ReLU value negative
        x[:, :, 2] = -np.abs(x[:, :, 2]) - np.float32(1.0)
        b[2] = np.float32(-0.25)
    if c.special == "offset_column":     # column 3: mean 100, spread 0.01, taken as is
        x[:, :, 3] = np.float32(100.0) + np.float32(0.01) * x[:, :, 3]
        s[3], b[3] = np.float32(1.0), np.float32(0.0)
    return dict(x=x, s=s, b=b)


def stats_pool(c, o, defect=None):
    """(out [N][2 C] = mean | unbiased std of relu(x s + b), bound); std is NaN at T = 1."""
    T = c.T
    v = o["x"].astype(f64) * o["s"].astype(f64) + o["b"].astype(f64)
    e = U * np.abs(v)
    if defect != "relu_dropped":
        v = np.maximum(v, 0.0)
    mean = v.mean(1)
    with np.errstate(all="ignore"):
        if defect == "one_pass_variance_f32":
            v32 = v.astype(np.float32)
            s1, s2 = np.zeros((c.N, c.C), np.float32), np.zeros((c.N, c.C), np.float32)
            for t in range(T):
                s1 = s1 + v32[:, t]
                s2 = s2 + v32[:, t] * v32[:, t]
            var = (s2 - s1 * s1 / np.float32(T)) / np.float32(T - 1)
            std = np.sqrt(np.maximum(var, np.float32(0.0))).astype(f64)
        else:
            ss = ((v - mean[:, None]) ** 2).sum(1)
            std = np.sqrt(ss / (T if defect == "variance_divided_by_T" else T - 1)) if T > 1 else np.full_like(mean, np.nan)
        e_std = np.sqrt((e ** 2).sum(1) / max(T - 1, 1)) + U * np.abs(std)
    e_mean = e.mean(1) + U * np.abs(mean)
    return np.concatenate([mean, std], 1), np.concatenate([e_mean, e_std], 1)


CMVN_LENS = [0, 1, 11, 12, 13, 95, 96, 97, 200]
CMVN_BEFORE, CMVN_AFTER = 3, 2    # rows before the first and behind the last sequence


def cmvn_operands():
    rng = _rng("cmvn", CMVN_LENS)
    fr_off = (CMVN_BEFORE + np.concatenate([[0], np.cumsum(CMVN_LENS)])).astype(np.int32)
    rows = int(fr_off[-1]) + CMVN_AFTER
    x = (np.float32(-8.0) + np.float32(3.0) * rng.standard_normal((rows, 80), dtype=np.float32))
    return dict(x=x, fr_off=fr_off)


def cmvn(o, defect=None):
    """(x after per-sequence mean removal [rows][80] float64, bound; rows outside stay, bound 0)."""
    x, off = o["x"].astype(f64), o["fr_off"]
    y, e = x.copy(), np.zeros_like(x)
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        if b <= a:
            continue
        mean = x[a:b + 1].sum(0) / (b - a) if defect == "mean_includes_next_row" else x[a:b].mean(0)
        end = min(b, a + 96) if defect == "rows_past_96_not_centred" else b
        y[a:end] = x[a:end] - mean
        e[a:b] = U * np.abs(mean) + U * np.abs(x[a:b] - mean)
    return y, e


GatherCase = namedtuple("GatherCase", "wf")
GATHER_CASES = [GatherCase(7), GatherCase(150)]


def gather_operands(c):
    rng = _rng("gather", c)
    wf = c.wf
    win_n = np.array([1, wf - 1, wf, wf, wf - 1, 1], np.int32)
    win_row = np.array([0, 1, 2, wf // 2, wf + 1, 2 * wf], np.int32)   # overlapping sources
    nrows = int((win_row + win_n).max()) + 1
    return dict(rows=rng.standard_normal((nrows, 80), dtype=np.float32), win_row=win_row, win_n=win_n)


def campp_gather(c, o):
    out = np.zeros((len(o["win_n"]), c.wf, 80), np.float32)
    for w, (r, n) in enumerate(zip(o["win_row"], o["win_n"])):
        out[w, :n] = o["rows"][r:r + n]
    return out


# ---------------------------------------------------------------------------------------------
# Silero VAD: frames, the two im2col kernels (float32, bit for bit), the LSTM recurrence
# ---------------------------------------------------------------------------------------------
VAD_WINDOWS = [3, 0, 1, 0, 0, 2, 0]
VAD_EXTRA = [37, 100, 5, 0, 511, 301, 100]     # samples behind the last whole window
# per-file peaks; two assignments so that every threshold meets a file that has windows
VAD_PEAKS = {"a": [0.0709, 0.5, 0.071, 0.0, 0.0, 0.5, 1e-7],
             "b": [1e-7, 0.0709, 0.0, 0.0, 0.5, 0.0709, 0.071]}


def vad_file_operands(peaks):
    rng = _rng("vadfiles", peaks)
    lens = np.array([512 * w + x for w, x in zip(VAD_WINDOWS, VAD_EXTRA)], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    win_start = np.concatenate([[0], np.cumsum(VAD_WINDOWS)[:-1]]).astype(np.int64)
    audio = np.zeros(int(lens.sum()), np.float32)
    for f, p in enumerate(VAD_PEAKS[peaks]):
        n = int(lens[f])
        if n == 0:
            continue
        a = (rng.uniform(-0.9, 0.9, n) * p).astype(np.float32)
        a[n // 3] = np.float32(-p if f % 2 else p)
        audio[off[f]:off[f] + n] = a
    return dict(audio=audio, off=off, len=lens, win_start=win_start, n_windows=int(sum(VAD_WINDOWS)))


def vad_maxabs(o):
    mx = np.zeros(len(o["off"]), np.uint32)
    for f, (a, n) in enumerate(zip(o["off"], o["len"])):
        if n > 0:
            mx[f] = np.abs(o["audio"][a:a + n]).max().view(np.uint32)
    return mx


def _vad_rows(src640, scale):
    v = (src640 * scale).astype(np.float32)
    return np.stack([v[128 * fr:128 * fr + 256] for fr in range(4)])


def vad_frames_files(o, maxabs=None, defect=None):
    """frames [windows * 4][256] float32 of the file mode."""
    j = np.arange(640)
    jj = np.where(j >= 576, (2 * 576 - 1 - j) if defect == "reflection_repeats_edge" else (2 * 575 - j), j)
    ap = np.concatenate([np.zeros(64, np.float32), o["audio"], np.zeros(1024, np.float32)])
    ws, out = o["win_start"], []
    for g in range(o["n_windows"]):
        f = int(np.searchsorted(ws, g, "right")) - 1
        if defect == "window_file_first_match":
            k = int(np.searchsorted(ws, g, "left"))
            f = k if k < len(ws) and ws[k] == g else k - 1
        w = g - int(ws[f])
        src = ap[64 + int(o["off"][f]) + w * 512 - 64 + jj].copy()
        if w == 0 and defect != "context_not_zeroed":
            src[jj < 64] = 0.0
        scale = np.float32(1.0)
        if maxabs is not None:
            m = maxabs[f:f + 1].view(np.float32)[0]
            if m > np.float32(1e-6) and (m < np.float32(0.071) or defect == "boost_without_upper_limit"):
                scale = np.float32(0.071) / m
        out.append(_vad_rows(src, scale))
    return np.concatenate(out)


def vad_frames_rows(rows576):
    j = np.arange(640)
    jj = np.where(j >= 576, 2 * 575 - j, j)
    return np.concatenate([_vad_rows(r[jj], np.float32(1.0)) for r in rows576])


MAG_CASES = [(3, 129, 258, 392), (2, 129, 264, 387), (1, 5, 12, 20)]   # windows, bins, ldS, Kp
IM2COL_CASES = [(3, 4, 128, 2), (3, 2, 64, 2), (2, 1, 64, 1), (2, 5, 16, 1)]   # N, T, C, stride


def vad_mag_im2col(S, bins, Kp):
    """A [windows * 4][Kp] from S [windows * 4][ldS] = (re | im) rows."""
    re, im = S[:, :bins], S[:, bins:2 * bins]
    mag = np.sqrt((re * re + im * im).astype(np.float32)).astype(np.float32).reshape(-1, 4, bins)
    A = np.zeros((mag.shape[0], 4, Kp), np.float32)
    for t in range(4):
        for k in range(3):
            if 0 <= t + k - 1 < 4:
                A[:, t, k * bins:(k + 1) * bins] = mag[:, t + k - 1]
    return A.reshape(-1, Kp)


def vad_im2col(Y, N, T, C, stride, defect=None):
    """A [N * Tout][3 C] from Y [N * T][C]."""
    Tout = (T - 1) // stride + 1
    Yn = Y.reshape(N, T, C)
    A = np.zeros((N, Tout, 3, C), np.float32)
    for to in range(Tout):
        for k in range(3):
            t = to * (1 if defect == "stride_ignored" else stride) + k - (0 if defect == "left_pad_dropped" else 1)
            if 0 <= t < T:
                A[:, to, k] = Yn[:, t]
    return A.reshape(N * Tout, 3 * C)


LSTM_WINDOWS = 48


def lstm_operands():
    rng = _rng("lstm", (LSTM_WINDOWS,))
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    return dict(gx=f(LSTM_WINDOWS, 512), whh=f(512, 128) / np.float32(math.sqrt(128)),
                bhh=f(512) * np.float32(0.1), wd=f(128) * np.float32(0.3), bd=np.float32(0.1))


def lstm(o, seg_start, seg_count, seg_warm=None, init=None, dtype=f64, defect=None, probs=None,
         s_out=None, e_out=None):
    """The segment contract of vad_lstm_kernel in `dtype` arithmetic: returns (probs [windows],
    s_out, e_out [segments][2][128]); what a segment does not write keeps its initial value
    (SENT unless given)."""
    dt = dtype
    gx, whh, bhh, wd = (o[k].astype(dt) for k in ("gx", "whh", "bhh", "wd"))
    bd = dt(o["bd"])
    nseg = len(seg_start)
    probs = np.full(gx.shape[0], SENT, dt) if probs is None else probs.astype(dt)
    s_out = np.full((nseg, 2, 128), SENT, dt) if s_out is None else s_out.astype(dt)
    e_out = np.full((nseg, 2, 128), SENT, dt) if e_out is None else e_out.astype(dt)
    sig = lambda v: dt(1) / (dt(1) + np.exp(-v))
    order = (0, 2, 1, 3) if defect == "gate_order_igfo" else (0, 1, 2, 3)
    for s in range(nseg):
        warm = int(seg_warm[s]) if seg_warm is not None else 0
        w0, n = int(seg_start[s]) - warm, int(seg_count[s]) + warm
        h = init[s, 0].astype(dt) if init is not None else np.zeros(128, dt)
        c = init[s, 1].astype(dt) if init is not None else np.zeros(128, dt)
        mark = warm + 1 if defect == "s_out_one_window_late" else warm
        for t in range(n):
            if t == mark:
                s_out[s, 0], s_out[s, 1] = h, c
            pre = gx[w0 + t] + whh @ h
            if defect != "bhh_dropped":
                pre = pre + bhh
            gi, gf, gg, go = (pre[128 * k:128 * k + 128] for k in order)
            c = sig(gf) * c + sig(gi) * np.tanh(gg)
            h = sig(go) * np.tanh(c)
            if t >= warm or defect == "prob_written_in_warmup":
                hr = h if defect == "relu_dropped" else np.maximum(h, dt(0))
                probs[w0 + t] = sig(hr @ wd + bd)
        if n <= mark:
            s_out[s, 0], s_out[s, 1] = h, c
        if not (defect == "e_out_untouched_when_empty" and int(seg_count[s]) == 0):
            e_out[s, 0], e_out[s, 1] = h, c
    return probs, s_out, e_out


def lstm_bound(o, seg_start, seg_count, seg_warm=None, init=None):
    """(reference triple in float64, bound triple): 8 x the float32 restatement's deviation from
    the float64 one on these inputs, floor 16 u, per output; plus the deviations themselves."""
    r64 = lstm(o, seg_start, seg_count, seg_warm, init, f64)
    r32 = lstm(o, seg_start, seg_count, seg_warm, init, np.float32)
    dev = [float(np.max(np.abs(a.astype(f64) - b))) if a.size else 0.0 for a, b in zip(r32, r64)]
    return r64, [max(8.0 * d, 16.0 * U) for d in dev], dev


# ---------------------------------------------------------------------------------------------
# ViBERT: LayerNorm (plain and embedding form), attention, gather
# ---------------------------------------------------------------------------------------------
LN_EPS = 1e-12          # BERT's layer_norm_eps
LnCase = namedtuple("LnCase", "rows H embed")
LN_WIDTHS = (1, 16, 255, 256, 257, 768, 1024)
LN_CASES = [LnCase(r, H, e) for e in (0, 1) for H in LN_WIDTHS for r in (1, 5)]
LN_EMBED_B = 2          # the embedding form runs B sequences of L = `rows` tokens each


def ln_operands(c):
    rng = _rng("ln", c)
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    o = dict(g=rng.uniform(0.5, 1.5, c.H).astype(np.float32), b=f(c.H) * np.float32(0.5))
    if not c.embed:
        x = f(c.rows, c.H)
        x[-1] = np.float32(50.0) + np.float32(0.01) * x[-1]     # one row: mean 50, spread 0.01
        o["x"] = x
        return o
    L, V, TT = c.rows, 11, 2                # B sequences of L = c.rows tokens
    rows = LN_EMBED_B * L
    o.update(L=L, rows=rows, ids=rng.integers(0, V, rows).astype(np.int64),
             tt=rng.integers(0, TT, rows).astype(np.int64), word=f(V, c.H),
             pos=f(rows, c.H), type=f(TT, c.H))     # pos has `rows` rows; the kernel reads L
    return o


def layer_norm(c, o, defect=None, eps=LN_EPS):
    """(y [rows][H] float64, bound)."""
    H = c.H
    if c.embed:
        r = np.arange(o["rows"])
        l = r if defect == "position_not_wrapped" else r % o["L"]
        wp = o["word"].astype(f64)[o["ids"]] + o["pos"].astype(f64)[l]
        v = wp + o["type"].astype(f64)[o["tt"]]
        e_v = U * (np.abs(wp) + np.abs(v))
    else:
        v = o["x"].astype(f64)
        e_v = np.zeros_like(v)
    g, b = o["g"].astype(f64), o["b"].astype(f64)
    vv = v.copy()
    if defect == "columns_past_768_dropped":
        vv[:, 768:] = 0.0
    mean = vv.sum(1, keepdims=True) / H
    d = vv - mean
    if defect == "columns_past_768_dropped":
        d[:, 768:] = 0.0
    with np.errstate(all="ignore"):
        var = (d * d).sum(1, keepdims=True) / ((H - 1) if defect == "variance_over_H_minus_1" else H)
        rstd = 1.0 / np.sqrt(var + eps)
    n = d * rstd
    y = n * g + b
    if defect == "columns_past_768_dropped":
        y[:, 768:] = float(SENT)
    e_n = rstd * (e_v + e_v.mean(1, keepdims=True) + np.abs(n) * (np.abs(n) * e_v).mean(1, keepdims=True))
    bound = (e_n + U * np.abs(mean) * rstd) * np.abs(g) + 6 * U * np.abs(n * g) + 2 * U * np.abs(y)
    return y, bound


AttnCase = namedtuple("AttnCase", "heads D L")
ATTN_CASES = [AttnCase(h, D, L) for h, D in ((2, 16), (3, 32), (2, 64)) for L in (1, 63, 64, 65, 200, 256)
              if not (D == 64 and L == 256)] + [AttnCase(1, 64, 256)]
ATTN_MASKS = (("ones", "tail"), ("middle", "all_masked"))   # B = 2: (sequence 0, sequence 1)


def attn_operands(c, mask):
    rng = _rng("attn", tuple(c) + (mask,))
    H, L = c.heads * c.D, c.L
    qkv = rng.standard_normal((2 * L, 3 * H), dtype=np.float32)
    m = np.ones((2, L), np.int64)
    for b, kind in enumerate(mask):
        if kind == "tail":
            m[b, (2 * L) // 3:] = 0
        elif kind == "middle":
            m[b, L // 4:(L // 4) + max(L // 3, 1)] = 0
        elif kind == "all_masked":
            m[b] = 0
    return dict(qkv=qkv, mask=m.reshape(-1))


def attention(c, o, defect=None, mask_exact=False):
    """(ctx [B L][H] float64, bound); B = 2.  Padded query rows are computed like the others."""
    heads, D, L = c
    H, B = heads * D, 2
    scale = float(np.float32(1.0 / math.sqrt(D)))
    qkv = o["qkv"].astype(f64).reshape(B, L, 3, heads, D)
    q, k, v = (qkv[:, :, i].transpose(0, 2, 1, 3) for i in range(3))      # [B][heads][L][D]
    keep = o["mask"].reshape(B, 1, 1, L).astype(bool)
    if defect == "mask_ignored":
        keep = np.ones_like(keep)
    s = q @ k.transpose(0, 1, 3, 2)
    S = np.abs(q) @ np.abs(k).transpose(0, 1, 3, 2)
    sc = s * (1.0 if defect == "scale_dropped" else scale)
    if mask_exact:   # s + offset carried exactly: the offset cancels where every key has it
        masked = np.where(keep.any(-1, keepdims=True), F32_MIN, sc)
    else:
        masked = (sc + F32_MIN).astype(np.float32).astype(f64)       # the float32 graph's value
    sc = np.where(keep, sc, masked)
    e_s = np.where(keep, (D + 1) * U * S * scale + U * np.abs(sc), 0.0)
    if defect == "keys_past_64_dropped":
        sc, e_s = sc[..., :64], e_s[..., :64]
        v = v[:, :, :64]
    mx = sc.max(-1, keepdims=True)
    p = np.exp(sc - mx)
    den = p.sum(-1, keepdims=True)
    ctx = (p @ v) / den
    if defect == "all_masked_row_zero":
        ctx = np.where(keep.any(-1, keepdims=True), ctx, 0.0)
    dp = p * (e_s + e_s.max(-1, keepdims=True)) + ACT_ABS
    e = (dp @ np.abs(v) + dp.sum(-1, keepdims=True) * np.abs(ctx)) / den + (L + 4) * U * (p @ np.abs(v)) / den
    lay = lambda t: t.transpose(0, 2, 1, 3).reshape(B * L, H)
    return lay(ctx), lay(e)


def vibert_gather_operands():
    rng = _rng("vgather", (2, 9, 5, 48))
    B, L, W, H = 2, 9, 5, 48
    off = np.array([[0, 0, 3, 8, 3], [8, 0, 0, 1, 8]], np.int64)           # repeated and zero
    return dict(B=B, L=L, W=W, H=H, x=rng.standard_normal((B * L, H), dtype=np.float32), off=off)


def vibert_gather(o, defect=None):
    B, L, W = o["B"], o["L"], o["W"]
    src = o["off"] + (0 if defect == "offset_without_batch" else np.arange(B)[:, None] * L)
    return o["x"][src.reshape(-1)]


# every listed single defect, by group (tests/test_aux_reference.py: each must be caught)
DEFECTS = {
    "conv2d": ["stride_ignored", "pad_col_clamped", "row_fi_clamped", "odd_last_row_unwritten",
               "ring_stale", "res_row_above", "scale_shift_swapped16", "tdnn_index_fo_major",
               "in_tf_read_as_ft"],
    "cam_mask": ["clipped_divided_by_seg_len", "global_mean_over_segment", "tail_frames_left_out",
                 "mask_written_to_s1"],
    "stats": ["variance_divided_by_T", "relu_dropped", "one_pass_variance_f32"],
    "cmvn": ["mean_includes_next_row", "rows_past_96_not_centred"],
    "vad_frames": ["reflection_repeats_edge", "context_not_zeroed", "boost_without_upper_limit",
                   "window_file_first_match"],
    "vad_im2col": ["stride_ignored", "left_pad_dropped"],
    "lstm": ["gate_order_igfo", "bhh_dropped", "relu_dropped", "prob_written_in_warmup",
             "s_out_one_window_late", "e_out_untouched_when_empty"],
    "layer_norm": ["variance_over_H_minus_1", "columns_past_768_dropped", "position_not_wrapped"],
    "attention": ["mask_ignored", "scale_dropped", "keys_past_64_dropped", "all_masked_row_zero"],
    "vibert_gather": ["offset_without_batch"],
}
