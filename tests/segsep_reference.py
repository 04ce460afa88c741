"""References for the PyanNet and Conv-TasNet kernels run alone (zasr_selftest_seg_*, _sep_*):
the case tables, the seeded operands, a float64 (or, where the operation is data movement or one
correctly rounded operation, float32) restatement of every operation, and the per-element bound.
tests/test_segsep_reference.py pins every restatement to torch on the CPU and shows that each
case table has power; tests/test_gpu_segsep_kernels.py compares the kernels with it.

Operands follow aux_reference: weights N(0, 1) / sqrt(fan_in), activations N(0, 1), scales
U(0.5, 1.5), shifts 0.5 N(0, 1), every case seeded from its own tuple; exceptions beside the case.
Every restatement takes `defect`: None is the reference, a name is the same operation with that
single defect (DEFECTS, below); the CPU test demands that each is caught by its group's cases.

Bounds are a-priori and elementwise, u = 2^-24, written before the first GPU run:

    chunk_stats, frame_stats
                the sums are float64: mean carries u |mean| for its rounding to f32 plus the
                float64 sum's own error, count 2^-53 sum |x| / count.  rstd = (var + eps)^-1/2
                carries u rstd plus, through d rstd = rstd^3 dvar / 2, the error of the sum of
                centred squares, (count + 3) 2^-53 var, and the float64 sum's own error in the
                mean, dm = count 2^-53 sum |x| / count (sum d = 0, so it moves var by dm^2).  The
                rounding of the returned mean to f32 is a term of the mean alone: the second pass
                centres on the float64 mean.
    region_stats
                as above with the partial sums given; the kernel forms var = q / n - mean^2 in
                float64, whose cancellation adds 2^-52 (q / n) / (2 (var + eps)) relative to rstd.
                Domain: |mean| / std <= 10 (the case tables stay below 3), where that term is
                below 2^-52 * 101 / 2, far under u.
    seg_front   normalised sample n = fma((x - mean) rstd, in_w, in_b), statistics given as f32:
                e_n = u |mean| rstd |in_w| + 3 u |(x - mean) rstd in_w| + u |n|; per conv output
                sum |w| e_n + (251 + 4) u sum |w| |n|; |.| and max are 1-Lipschitz, so a pooled
                value takes the largest bound of its three.
    norm_act, gln_apply
                y = ((x - mean) rstd) g + b with f32 statistics given: 4 u |n g| + 2 u |y|
                (subtraction, the product with rstd or rstd g, the fused multiply-add, the leaky
                product; leaky_relu has slope <= 1).
    sep_mid     each normalised tap n_k as above: e_k = 4 u |(h - mean) rstd g| + 2 u |n_k|
                (a padded tap is exactly 0: e_k = 0); through the taps sum |w_k| e_k +
                (3 + 1) u (sum |w_k n_k| + |bias|) + u |y|; PReLU passes it through
                max(1, |slope|).  The partial sums are compared with the float64 sums of the y the
                kernel itself returned: rows C 2^-53 sum |y| (and sum y^2; a square of an f32
                is exact in float64).
    tile_sums   the same float64-sum bound against the operand.
    seg_head    logits z: (128 + 4) u (sum |w| |x| + |b|) = e_z; log-softmax turns that into at
                most 2 max_k e_z; the seven expf (each <= 1) and their f32 sum add 7 ACT_ABS + 7 u
                to se >= 1, logf one more ACT_ABS, the two subtractions 2 u |o|.
    seg_lstm    no a-priori bound (the error feeds back): 8 x the deviation of a plain float32
                numpy restatement from the float64 one, floor 16 u, measured per F on the CPU
                (never on the device).  gx has std 1.5: the pre-activations span (-6.0, 6.5)
                (observed on the CPU), so gates leave the linear region and do not saturate in f32.

Bit for bit against float32 numpy: seg_pool3, sep_frames, sep_prelu (one f32 product),
sep_overlap_add (one f32 add, +0.0 from (F - 1) hop + win to T), and the head's classes against
the first index of the maximum of the logits row the device returned.
"""
import math
from collections import namedtuple

import numpy as np

from aux_reference import ACT_ABS, SENT, U, U_TANH, _rng, f64, same_bits, worst_ratio  # noqa: F401

U53 = 2.0 ** -53
SEG_EPS, GLN_EPS, LEAKY = 1e-5, 1e-8, 0.01
TAPS, STRIDE0, C0, H, NC = 251, 10, 80, 128, 7
TILE, WIN, HOP = 32, 32, 16
f32 = np.float32


def _f(rng, *s):
    return rng.standard_normal(s, dtype=np.float32)


def _stats64(x, axis, eps, count=None):
    """(mean, rstd, e_mean, e_rstd) of x (float64) over `axis` with the float64-sum bound."""
    n = count if count is not None else x.shape[axis]
    mean = x.sum(axis, keepdims=True) / n
    d = x - mean
    var = (d * d).sum(axis, keepdims=True) / n
    rstd = 1.0 / np.sqrt(var + eps)
    e_sum = n * U53 * np.abs(x).sum(axis, keepdims=True) / n      # the float64 sum's own error
    e_mean = U * np.abs(mean) + e_sum
    # the second pass centres on the float64 mean, so the rounding of the returned mean to f32
    # does not enter the variance: only e_sum does, and since sum d = 0 a mean off by dm moves
    # var by dm^2; the centred squares add (n + 3) 2^-53 var (subtraction, square, the sum)
    e_var = (n + 3) * U53 * var + e_sum ** 2
    e_rstd = U * rstd + 0.5 * rstd ** 3 * e_var
    sq = lambda a: np.squeeze(a, axis)
    return sq(mean), sq(rstd), sq(e_mean), sq(e_rstd)


# ---------------------------------------------------------------------------------------------
# segmentation: chunk statistics
# ---------------------------------------------------------------------------------------------
# audio of 4 T samples: [0, T) constant 0.3, [T, 2 T) 0.5 + 1e-3 N, [2 T, 4 T) N(0, 1)
ChunkCase = namedtuple("ChunkCase", "T kind")
CHUNK_CASES = [ChunkCase(T, k) for T in (1261, 1281, 4000) for k in ("edges", "levels")]


def chunk_operands(c):
    rng, T = _rng("chunk", c), c.T
    audio = np.concatenate([np.full(T, 0.3, f32), f32(0.5) + f32(1e-3) * _f(rng, T), _f(rng, 2 * T)])
    if c.kind == "edges":     # wholly inside, the last sample missing, one sample inside
        starts = [2 * T + 3, 3 * T + 1, 4 * T - 1]
    else:                     # starts at `total` (all zeros), constant, mean 0.5 with std 1e-3
        starts = [4 * T, 0, T]
    return dict(audio=audio, starts=np.array(starts, np.int64))


def _chunk(audio, s0, T):
    x = np.zeros(T)
    a = audio[s0:s0 + T]
    x[:a.size] = a
    return x, a.size


def chunk_stats(c, o, defect=None):
    """(stats [n][2] float64, bound)."""
    out, bound = [], []
    for s0 in o["starts"]:
        x, avail = _chunk(o["audio"].astype(f64), int(s0), c.T)
        m, r, em, er = _stats64(x, 0, SEG_EPS)
        if defect == "divide_by_avail":
            m, r, _, _ = _stats64(x, 0, SEG_EPS, count=max(avail, 1))
        if defect == "eps_omitted":
            with np.errstate(all="ignore"):
                m, r, _, _ = _stats64(x, 0, 0.0)
        if defect == "variance_without_zero_tail":
            r = 1.0 / np.sqrt(((x[:avail] - m) ** 2).sum() / c.T + SEG_EPS)
        out.append([m, r])
        bound.append([em, er])
    return np.array(out, f64), np.array(bound, f64)


# ---------------------------------------------------------------------------------------------
# segmentation: front (gather + normalise + sinc conv + |.| + max-pool 3)
# ---------------------------------------------------------------------------------------------
# T -> F1 = l0 // 3, l0 = (T - 251) // 10 + 1: F1 = 1, 63 (l0 % 3 = 0), 64 (1), 65 (2), 129
FRONT_T = (271, 2131, 2176, 2220, 4111)
IN_W, IN_B = 1.3, -0.2
FRONT_BLOCK = 64


def front_f1(T):
    return ((T - TAPS) // STRIDE0 + 1) // 3


def front_operands(T):
    rng = _rng("front", (T,))
    total = T + T // 2 + 7
    audio = _f(rng, total)
    starts = np.array([5, total - (T // 2 + 3)], np.int64)     # chunk 1 runs past `total`
    st = []
    for s0 in starts:
        x, _ = _chunk(audio.astype(f64), int(s0), T)
        m, r, _, _ = _stats64(x, 0, SEG_EPS)
        st.append([m, r])
    w0 = _f(rng, C0, TAPS) / f32(math.sqrt(TAPS))
    return dict(audio=audio, starts=starts, stats=np.array(st, f32), w0=w0,
                w0t=np.ascontiguousarray(w0.T))


def front(T, o, defect=None):
    """(out [n][F1][80] float64, bound)."""
    F1, n = front_f1(T), len(o["starts"])
    w = o["w0"].astype(f64)
    if defect == "taps_reversed":
        w = w[:, ::-1]
    aw = np.abs(w)
    stride = 9 if defect == "stride_9" else STRIDE0
    blocks = -(-F1 // FRONT_BLOCK)
    nfr = 3 * FRONT_BLOCK * blocks                    # conv frames a launch computes
    need = (nfr - 1) * STRIDE0 + TAPS
    pooled, bounds = [], []
    for k in range(n):
        mean, rstd = (float(v) for v in o["stats"][k])
        x, avail = _chunk(o["audio"].astype(f64), int(o["starts"][k]), T)
        t = (x - mean) * rstd * IN_W
        nrm = t + IN_B
        e = U * abs(mean) * rstd * abs(IN_W) + 3 * U * np.abs(t) + U * np.abs(nrm)
        if defect == "zeros_after_norm":
            nrm[avail:] = 0.0
        pad = lambda v: np.concatenate([v, np.zeros(max(need - T, 0))])   # past the chunk: 0
        nrm, e = pad(nrm), pad(e)
        idx = np.arange(nfr)[:, None] * stride + np.arange(TAPS)[None, :]
        idx = np.minimum(idx, nrm.size - 1)
        y = nrm[idx] @ w.T                                                # [nfr][80]
        b = e[idx] @ aw.T + (TAPS + 4) * U * (np.abs(nrm[idx]) @ aw.T)
        y3, b3 = y.reshape(-1, 3, C0), b.reshape(-1, 3, C0)
        if defect == "pool_2_of_3":
            y3 = y3[:, :2]
        p = np.abs(y3.max(1)) if defect == "max_before_abs" else np.abs(y3).max(1)
        if defect == "chan_pass2_offset_10":          # wave w, pass 2: channels 20 w + 20 .. + 29
            c = np.arange(C0)
            p = p[:, np.where(c % 20 >= 10, (c + 10) % C0, c)]
        pooled.append(p)
        bounds.append(b3.max(1))
    out = np.stack([p[:F1] for p in pooled])
    if defect == "rows_not_clipped" and F1 % FRONT_BLOCK:     # chunk 0's last block runs on
        over = min(FRONT_BLOCK * blocks - F1, F1)
        out[1, :over] = pooled[0][F1:F1 + over]
    return out, np.stack([b[:F1] for b in bounds])


# ---------------------------------------------------------------------------------------------
# segmentation: MaxPool1d(3, 3), frame statistics, normalise + leaky_relu
# ---------------------------------------------------------------------------------------------
PoolCase = namedtuple("PoolCase", "L Fp C cap")
POOL_CASES = [PoolCase(L, Fp, C, cap) for L, Fp in ((3, 1), (4, 1), (5, 1), (587, 195), (197, 65))
              for C in (60, 80) for cap in (0, 2)]
SEG_N = 2


def pool_operands(c):
    rng = _rng("pool", c[:3])
    return dict(x=-np.abs(_f(rng, SEG_N, c.L, c.C)) - f32(0.1))     # all negative


def pool3(c, o, defect=None):
    x = o["x"]
    if defect == "chunk_stride_3Fp":
        flat = np.concatenate([x.reshape(-1, c.C), np.full((3 * c.Fp, c.C), SENT, f32)])
        x = np.stack([flat[n * 3 * c.Fp:n * 3 * c.Fp + 3 * c.Fp] for n in range(SEG_N)])
    y = x[:, :3 * c.Fp].reshape(SEG_N, c.Fp, 3, c.C).max(2)
    if defect == "zero_initialised_max":
        y = np.maximum(y, f32(0.0))
    return np.ascontiguousarray(y, f32)


FstatCase = namedtuple("FstatCase", "C F")
FSTAT_N = 3
FSTAT_CASES = [FstatCase(C, F) for C in (80, 60, 128, 4)
               for F in sorted({1, 2, 256 // C - 1, 256 // C, 256 // C + 1, 589} - {0})]


def fstat_operands(c):
    rng = _rng("fstat", c)
    x = _f(rng, FSTAT_N, c.F, c.C)
    x[:, :, 1] = f32(100.0) + f32(0.01) * x[:, :, 1]        # one channel with a large mean
    return dict(x=x)


def frame_stats(c, o, defect=None):
    """(stats [n][C][2] float64, bound)."""
    x = o["x"].astype(f64)
    m, r, em, er = _stats64(x, 1, SEG_EPS)
    if defect in ("last_slot_dropped", "G_plus_1"):
        G = 256 // c.C + (1 if defect == "G_plus_1" else 0)
        f, ch = np.arange(c.F)[:, None], np.arange(c.C)[None, :]
        keep = (f % G != G - 1) if defect == "last_slot_dropped" else ((f % G) * c.C + ch < 256)
        xm = np.where(keep[None], x, 0.0)
        m = xm.sum(1) / c.F
        r = 1.0 / np.sqrt((np.where(keep[None], (x - m[:, None]) ** 2, 0.0)).sum(1) / c.F + SEG_EPS)
    if defect == "second_pass_on_f32_mean":      # centred on the mean as returned, not the float64 one
        m32 = m.astype(f32).astype(f64)
        r = 1.0 / np.sqrt(((x - m32[:, None]) ** 2).sum(1) / c.F + SEG_EPS)
    if defect == "divide_by_F_minus_1":
        with np.errstate(all="ignore"):
            m, r, _, _ = _stats64(x, 1, SEG_EPS, count=c.F - 1)
    return np.stack([m, r], -1), np.stack([em, er], -1)


NormCase = namedtuple("NormCase", "C F cap")
NORM_CASES = [NormCase(C, F, cap) for C in (60, 80, 128) for F in (1, 7, 195) for cap in (0, 2)]


def norm_operands(c):
    rng = _rng("norm", c[:2])
    x = f32(1.5) * _f(rng, SEG_N, c.F, c.C) + f32(0.3)       # straddles 0 after the affine
    stats = np.stack([f32(0.5) * _f(rng, SEG_N, c.C), rng.uniform(0.5, 1.5, (SEG_N, c.C)).astype(f32)], -1)
    return dict(x=x, stats=stats, w=rng.uniform(0.5, 1.5, c.C).astype(f32), b=f32(0.5) * _f(rng, c.C))


def norm_act(c, o, defect=None):
    """(y [n][F][C] float64, bound)."""
    x, st, w, b = (o[k].astype(f64) for k in ("x", "stats", "w", "b"))
    if defect == "stats_of_chunk_0":
        st = np.broadcast_to(st[:1], st.shape)
    mean, rstd = st[:, None, :, 0], st[:, None, :, 1]
    if defect == "affine_before_norm":
        y = ((x * w + b) - mean) * rstd
        ng = y
    else:
        ng = (x - mean) * rstd * w
        y = ng + b
    bound = 4 * U * np.abs(ng) + 2 * U * np.abs(y)
    return np.where(y > 0, y, (0.1 if defect == "leaky_slope_0.1" else LEAKY) * y), bound


# ---------------------------------------------------------------------------------------------
# segmentation: the recurrence
# ---------------------------------------------------------------------------------------------
LSTM_F = (1, 2, 9)
LSTM_GROUPS = (1, 2, 4, 8, 16)
LSTM_MAX_N = 2 * 16 + 1


def lstm_ns(B):
    return sorted({1, B - 1, B, B + 1, 2 * B + 1} - {0})


def lstm_operands(F):
    """LSTM_MAX_N sequences, each with its own gx (std 1.5); a case of n takes the first n, so a
    sequence's result can be compared across n, group and slot.  The directions' W_hh differ."""
    rng = _rng("seglstm", (F,))
    return dict(gx=f32(1.5) * _f(rng, LSTM_MAX_N, F, 8 * H), whh=_f(rng, 2, 4 * H, H) / f32(math.sqrt(H)))


def lstm(o, n, B=1, dtype=f64, defect=None, pre_range=None):
    """out [n][F][256] in `dtype` arithmetic, group by group as the kernel walks them."""
    dt = dtype
    gx, whh = o["gx"][:n].astype(dt), o["whh"].astype(dt)
    F = gx.shape[1]
    out = np.zeros((n, F, 2 * H), dt)
    sig = lambda v: dt(1) / (dt(1) + np.exp(-v))
    order = (0, 2, 1, 3) if defect == "gate_order_igfo" else (0, 1, 2, 3)
    for d in (0, 1):
        W = whh[0 if defect == "whh_dir0_for_both" else d]
        c_prev = None
        for s0 in range(0, n, B):
            nb = min(B, n - s0)
            h = np.zeros((nb, H), dt)
            c = np.zeros((nb, H), dt)
            if defect == "cell_not_reset" and c_prev is not None:
                c = c_prev[:nb].copy()
            src = np.arange(nb)
            if defect == "tail_fed_slot0_h" and nb < B:
                src = np.zeros(nb, np.int64)
            for t in range(F):
                tt = F - 1 - t if (d == 1 and defect != "backward_not_reversed") else t
                pre = gx[s0:s0 + nb, tt, d * 4 * H:(d + 1) * 4 * H] + h[src] @ W.T
                if pre_range is not None:
                    pre_range.append((float(pre.min()), float(pre.max())))
                gi, gf, gg, go = (pre[:, H * k:H * k + H] for k in order)
                c = sig(gf) * c + sig(gi) * np.tanh(gg)
                h = sig(go) * np.tanh(c)
                to = F - 1 - tt if (d == 1 and defect == "backward_written_mirrored") else tt
                out[s0:s0 + nb, to, d * H:(d + 1) * H] = h
            c_prev = c
    return out


def lstm_bound(o):
    """(float64 reference of all LSTM_MAX_N sequences, bound (a scalar), deviation)."""
    r64 = lstm(o, LSTM_MAX_N)
    r32 = lstm(o, LSTM_MAX_N, dtype=np.float32)
    dev = float(np.max(np.abs(r32.astype(f64) - r64)))
    return r64, max(8.0 * dev, 16.0 * U), dev


# ---------------------------------------------------------------------------------------------
# segmentation: head
# ---------------------------------------------------------------------------------------------
HeadCase = namedtuple("HeadCase", "rows kind")
HEAD_CASES = [HeadCase(r, "plain") for r in (1, 255, 256, 257, 513)] + [
    HeadCase(257, "tie"), HeadCase(513, "large")]


def head_operands(c):
    rng = _rng("head", c)
    w, b = _f(rng, NC, H) / f32(math.sqrt(H)), f32(0.5) * _f(rng, NC)
    if c.kind == "tie":       # classes 2 and 3 identical, and with this bias often the maximum
        b[2] = f32(1.5)
        w[3], b[3] = w[2], b[2]
    if c.kind == "large":     # logits of magnitude ~60
        w *= f32(60.0)
    return dict(x=_f(rng, c.rows, H), w=w, b=b)


def head(c, o, defect=None):
    """(log-probabilities [rows][7] float64, bound)."""
    x, w, b = (o[k].astype(f64) for k in ("x", "w", "b"))
    z = x @ w.T + (0.0 if defect == "bias_omitted" else b)
    e_z = (H + 4) * U * (np.abs(x) @ np.abs(w).T + np.abs(b))
    if defect == "no_max_subtraction":        # float32 expf overflows where float64 does not
        with np.errstate(all="ignore"):
            z32 = z.astype(f32)
            out = (z32 - np.log(np.exp(z32).sum(1, keepdims=True, dtype=f32))).astype(f64)
    else:
        m = z.max(1, keepdims=True)
        out = z - m - np.log(np.exp(z - m).sum(1, keepdims=True))
    bound = 2 * e_z.max(1, keepdims=True) + 8 * ACT_ABS + 7 * U + 2 * U * np.abs(out)
    return out, np.broadcast_to(bound, out.shape)


def head_classes(logits, defect=None):
    """the first index of each row's maximum (uint8)"""
    if defect == "tie_to_higher_index":
        return (NC - 1 - np.argmax(logits[:, ::-1], 1)).astype(np.uint8)
    return np.argmax(logits, 1).astype(np.uint8)


# ---------------------------------------------------------------------------------------------
# separation: the shared region sets
# ---------------------------------------------------------------------------------------------
def _T_of(F, extra=0):
    return HOP * (F - 1) + WIN + extra


def _regions(Fs, extras, adjacent):
    T = [_T_of(F, e) for F, e in zip(Fs, extras)]
    if adjacent:
        off = np.concatenate([[0], np.cumsum(T)[:-1]])
    else:                                       # odd, overlapping, out of signal order
        off = np.array([4001, 17, 1203, 9, 2575][:len(T)])
    return np.asarray(off, np.int64), np.asarray(T, np.int32)


SepSet = namedtuple("SepSet", "name sig_off T r0 ng")
_A = _regions((33, 1, 65), (0, 0, 0), True)
_R = _regions((31, 32, 257, 64, 129), (3, 15, 0, 7, 1), False)
SEP_SETS = [SepSet("adjacent3", *_A, 0, 3), SepSet("ragged5", *_R, 0, 5), SepSet("group2of5", *_R, 2, 3)]


def sep_F(s):
    return (s.T.astype(np.int64) - WIN) // HOP + 1


def sep_rows(s):
    """per region of the group: (call-wide region index, first row in the group, F)"""
    F, out, row = sep_F(s), [], 0
    for r in range(s.r0, s.r0 + s.ng):
        out.append((r, row, int(F[r])))
        row += int(F[r])
    return out


def sep_tiles(s):
    """(region, first row in the group, rows) of every tile of the group, in launch order"""
    return [(r, row + f0, min(TILE, F - f0)) for r, row, F in sep_rows(s) for f0 in range(0, F, TILE)]


def sep_M(s):
    return sum(F for _, _, F in sep_rows(s))


def sep_activation(s, C, tag):
    """x [M][C]: region r at level 0.7 (1 + r) around the DC offset +-2 (1 + r), so a row read
    across a region edge is far outside any bound (|mean| / std < 3)."""
    rng = _rng(tag, (s.name, C))
    x = _f(rng, sep_M(s), C)
    for r, row, F in sep_rows(s):
        x[row:row + F] = x[row:row + F] * f32(0.7 * (1 + r)) + f32((-2.0 if r % 2 else 2.0) * (1 + r))
    return x


def sep_signal(s):
    rng = _rng("sepsig", (s.name,))
    return _f(rng, int((s.sig_off + s.T).max()) + 5)


def sep_frames(s, signal):
    rows = [signal[int(s.sig_off[r]) + HOP * f:int(s.sig_off[r]) + HOP * f + WIN]
            for r, _, F in sep_rows(s) for f in range(F)]
    return np.ascontiguousarray(np.stack(rows), f32)


# ---------------------------------------------------------------------------------------------
# separation: gLN statistics and application
# ---------------------------------------------------------------------------------------------
SEP_C = (512, 128, 4)


def tile_sums(s, x):
    """(partial [nt][2] float64, bound).  The listed defects of the statistics (a dropped tile, the
    count, eps) belong to the per-region sum: region_stats."""
    x = np.asarray(x, f64)
    p = np.array([[x[a:a + n].sum(), (x[a:a + n] ** 2).sum()] for _, a, n in sep_tiles(s)])
    e = np.array([[n * x.shape[1] * U53 * np.abs(x[a:a + n]).sum(), n * x.shape[1] * U53 * (x[a:a + n] ** 2).sum()]
                  for _, a, n in sep_tiles(s)])
    return p, e


def region_stats(s, x, defect=None):
    """(stats [n_regions][2] float64 with SENT outside the group, bound) from the float64 partial
    sums of x's tiles, as the kernel is given them."""
    x = np.asarray(x, f64)
    C = x.shape[1]
    out = np.full((len(s.T), 2), float(SENT))
    bound = np.zeros((len(s.T), 2))
    for r, row, F in sep_rows(s):
        xr = x[row:row + F]
        m, rs, em, er = _stats64(xr.reshape(-1), 0, GLN_EPS)
        var = 1.0 / rs ** 2 - GLN_EPS
        er = er + rs * 2.0 ** -52 * ((xr ** 2).mean()) / (2 * (var + GLN_EPS))
        if defect is not None:
            nt = -(-F // TILE) - (1 if defect == "last_tile_dropped" else 0)
            xs = xr[:nt * TILE]
            n = F if defect == "n_is_F" else F * C
            m = xs.sum() / n
            with np.errstate(all="ignore"):
                v = max((xs ** 2).sum() / n - m * m, 0.0)
                rs = 1.0 / np.sqrt(v + (1e-5 if defect == "eps_1e-5" else GLN_EPS))
        out[r], bound[r] = (m, rs), (em, er)
    return out, bound


def gln_operands(s, C):
    rng = _rng("gln", (s.name, C))
    n = len(s.T)
    stats = np.stack([f32(0.5) * _f(rng, n), rng.uniform(0.5, 1.5, n).astype(f32)], -1)
    for r in range(n):                      # regions outside the group: values no row may see
        if not s.r0 <= r < s.r0 + s.ng:
            stats[r] = (f32(1e6), f32(1e3))
    return dict(x=sep_activation(s, C, "glnx"), stats=stats, gamma=rng.uniform(0.5, 1.5, C).astype(f32),
                beta=f32(0.5) * _f(rng, C))


def gln_apply(s, o, defect=None):
    """(y [M][C] float64, bound)."""
    x, st, g, b = (o[k].astype(f64) for k in ("x", "stats", "gamma", "beta"))
    y, bound = np.zeros_like(x), np.zeros_like(x)
    for r, row, F in sep_rows(s):
        mean, rstd = st[r - s.r0 if defect == "region_group_relative" else r]
        ng = (x[row:row + F] - mean) * rstd * g
        y[row:row + F] = ng + b
        bound[row:row + F] = 4 * U * np.abs(ng) + 2 * U * np.abs(ng + b)
    return y, bound


# ---------------------------------------------------------------------------------------------
# separation: the middle of a TCN block
# ---------------------------------------------------------------------------------------------
MID_SLOPE = 0.25
MidCase = namedtuple("MidCase", "set C dil")


def _dil_set(d):
    Fs = [F for F in (d - 1, d, d + 1, 2 * d + 1) if F >= 1]
    return SepSet(f"dil{d}", *_regions(Fs, [0] * len(Fs), True), 0, len(Fs))


MID_CASES = ([MidCase(_dil_set(d), 512, d) for d in (1, 2, 4, 8, 16, 32, 64, 128)]
             + [MidCase(s, 512, d) for s in SEP_SETS for d in (1, 2, 4, 8, 16, 32, 64, 128)]
             + [MidCase(SEP_SETS[0], C, d) for C in (4, 256, 1024, 2048) for d in (1, 32)])


def mid_id(c):
    return f"{c.set.name}_C{c.C}_d{c.dil}"


def mid_operands(c):
    s, C = c.set, c.C
    rng = _rng("mid", (s.name, C, c.dil))
    h = sep_activation(s, C, "midh")
    stats = np.full((len(s.T), 2), (1e6, 1e3), f32)
    for r, row, F in sep_rows(s):               # the region's own statistics, as the engine's
        m, rs, _, _ = _stats64(h[row:row + F].astype(f64).reshape(-1), 0, GLN_EPS)
        stats[r] = (m, rs)
    return dict(h=h, stats=stats, gamma=rng.uniform(0.5, 1.5, C).astype(f32), beta=f32(0.5) * _f(rng, C),
                w=_f(rng, 3, C) / f32(math.sqrt(3.0)), bias=f32(0.5) * _f(rng, C))


def mid(c, o, defect=None):
    """(y [M][C] float64, bound); SENT where a defect leaves y unwritten."""
    s, C, d = c.set, c.C, c.dil
    h, st, g, be, w, bias = (o[k].astype(f64) for k in ("h", "stats", "gamma", "beta", "w", "bias"))
    if defect == "taps_swapped":
        w = w[::-1]
    dd = d - 1 if defect == "dilation_minus_1" else d
    M = h.shape[0]
    y, bound = np.zeros_like(h), np.zeros_like(h)
    for r, row, F in sep_rows(s):
        mean, rstd = st[r]
        sc = rstd * g

        def tap(off):
            u = np.arange(F) + off                       # frame within the region
            inside = (u >= 0) & ((u <= F) if defect == "edge_u_gt_F" else (u < F))
            if defect == "no_region_edge":
                inside = np.ones(F, bool)
            a = row + u                                  # row of the group's buffer
            have = (a >= 0) & (a < M)
            hv = np.where(have[:, None], h[np.clip(a, 0, M - 1)], 0.0)
            t = (hv - mean) * sc
            n = t + be
            e = 4 * U * np.abs(t) + 2 * U * np.abs(n)
            ok = (inside & have)[:, None]
            if defect == "pad_before_norm":
                return np.where(ok, n, (0.0 - mean) * sc + be), np.where(ok, e, 0.0)
            return np.where(ok, n, 0.0), np.where(ok, e, 0.0)

        taps = [tap(-dd), tap(0), tap(dd)]
        acc = sum(w[k] * taps[k][0] for k in range(3)) + bias
        mag = sum(np.abs(w[k] * taps[k][0]) for k in range(3)) + np.abs(bias)
        e = sum(np.abs(w[k]) * taps[k][1] for k in range(3)) + 4 * U * mag + U * np.abs(acc)
        y[row:row + F] = np.where(acc > 0, acc, MID_SLOPE * acc)
        bound[row:row + F] = e * max(1.0, abs(MID_SLOPE))
    if defect == "second_channel_pass_skipped" and C > 1024:
        y[:, 1024:] = float(SENT)
    return y, bound


def mid_partials(c, y, defect=None):
    """(partial [nt][2] float64 of the given y, bound); the defect sums before the PReLU."""
    y = np.asarray(y, f64)
    if defect == "partials_before_prelu":
        y = np.where(y > 0, y, y / MID_SLOPE)
    return tile_sums(c.set, y)


# ---------------------------------------------------------------------------------------------
# separation: PReLU on a column block, overlap-add
# ---------------------------------------------------------------------------------------------
PreluCase = namedtuple("PreluCase", "rows cap")
PRELU_CASES = [PreluCase(r, cap) for r in (1, 33, 1000) for cap in (0, 2)]
PRELU_C, PRELU_LD, PRELU_COL0, PRELU_SLOPE = 128, 256, 128, 0.25


def prelu_operands(c):
    rng = _rng("prelu", (c.rows,))
    x = np.full((c.rows, PRELU_LD), SENT, f32)      # the kernel's columns [C, ld): sentinels
    x[:, PRELU_COL0:] = _f(rng, c.rows, PRELU_C)
    return dict(x=x)


def prelu(c, o, defect=None):
    x = o["x"].copy()
    if defect == "ld_is_C":         # row r of the kernel starts at col0 + r C of the flat buffer
        flat = x.reshape(-1)
        for r in range(c.rows):
            a = PRELU_COL0 + r * PRELU_C
            v = flat[a:a + PRELU_C]
            flat[a:a + PRELU_C] = np.where(v > 0, v, f32(PRELU_SLOPE) * v)
        return x
    v = x[:, PRELU_COL0:]
    neg = f32(PRELU_SLOPE) * v
    x[:, PRELU_COL0:] = neg if defect == "slope_on_positive" else np.where(v > 0, v, neg)
    return x


OLA_T = np.array([32, 47, 255, 256, 257, 2080], np.int32)
OLA_GAPS = (5, 0, 3, 1, 0, 7, 4)        # before each region's [2][T] and behind the last
OLA_SETS = [SepSet("ola_all", np.zeros(6, np.int64), OLA_T, 0, 6),
            SepSet("ola_group2of6", np.zeros(6, np.int64), OLA_T, 2, 4)]


def ola_operands(s):
    rng = _rng("ola", (s.name,))
    off, pos = [], 0
    for T, gap in zip(s.T, OLA_GAPS):
        pos += gap
        off.append(pos)
        pos += 2 * int(T)
    M = sep_M(s)
    return dict(dec0=_f(rng, M, WIN), dec1=_f(rng, M, WIN), out_off=np.array(off, np.int64),
                n_out=pos + OLA_GAPS[-1])


def overlap_add(s, o, defect=None):
    """out [n_out] float32: SENT wherever the launch does not write."""
    out = np.full(o["n_out"], SENT, f32)
    for r, row, F in sep_rows(s):
        T = int(s.T[r])
        t = np.arange(T)
        f, j = t // HOP, t % HOP
        for st in (0, 1):
            dec = o["dec0" if (st == 0 or defect == "stream1_reads_dec0") else "dec1"][row:row + F]
            v = np.zeros(T, f32)
            a = (f >= 1) & (f - 1 < F)
            fa = f[a] if defect == "second_half_from_frame_f" else f[a] - 1
            v[a] = dec[np.minimum(fa, F - 1), HOP + j[a]]
            b = f < F
            v[b] = v[b] + dec[f[b], j[b]]
            if defect == "tail_not_zeroed":
                v[(F - 1) * HOP + WIN:] = SENT
            out[int(o["out_off"][r]) + st * T:int(o["out_off"][r]) + (st + 1) * T] = v
    return out


# every listed single defect, by group (tests/test_segsep_reference.py: each must be caught)
DEFECTS = {
    "front": ["zeros_after_norm", "taps_reversed", "stride_9", "pool_2_of_3", "max_before_abs",
              "rows_not_clipped", "chan_pass2_offset_10"],
    "chunk_stats": ["divide_by_avail", "eps_omitted", "variance_without_zero_tail"],
    "frame_stats": ["last_slot_dropped", "G_plus_1", "divide_by_F_minus_1", "second_pass_on_f32_mean"],
    "norm_act": ["stats_of_chunk_0", "leaky_slope_0.1", "affine_before_norm"],
    "pool3": ["chunk_stride_3Fp", "zero_initialised_max"],
    "lstm": ["gate_order_igfo", "backward_not_reversed", "backward_written_mirrored", "tail_fed_slot0_h",
             "cell_not_reset", "whh_dir0_for_both"],
    "head": ["tie_to_higher_index", "bias_omitted", "no_max_subtraction"],
    "region_stats": ["last_tile_dropped", "n_is_F", "eps_1e-5"],
    "gln": ["region_group_relative"],
    "mid": ["no_region_edge", "pad_before_norm", "taps_swapped", "dilation_minus_1", "edge_u_gt_F",
            "second_channel_pass_skipped", "partials_before_prelu"],
    "prelu": ["ld_is_C", "slope_on_positive"],
    "overlap_add": ["second_half_from_frame_f", "tail_not_zeroed", "stream1_reads_dec0"],
}
