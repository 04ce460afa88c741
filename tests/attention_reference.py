"""Cases, seeded operands, the float64 reference, its per-element bound and a numpy emulation of
the attention kernel tests (tests/test_gpu_attention.py on the GPU through zasr_selftest_attn_weights
/ _attn_sa / _nonlin; tests/test_attention_reference.py without one).

What the kernels are documented to compute, from the operands AS STORED (csrc/attn_kernels.hip,
csrc/encoder_kernels.hip attn_softmax_kernel / attn_sa_kernel), per sequence of L frames and head h:

    s_ij  = q_i . k_j (32 dims) + p_i . pos_tab[(j - i) + pmax - 1] (4 dims)
    P_ij  = softmax over the keys j < L of s_ij
    out_i = sum_j P_ij v_j                       (12 dims per head)
    c_i   = max_j + log(sum_j exp(s_ij - max_j)) (the row statistic)
    t1    = tanh(s) * x,  z_i = (sum_j P0_ij t1_j) * y_i,  (s, x, y) = chunk(h3, 3), P0 = head 0

Softmax domain.  In the bf16 mode the STORED q and p columns carry log2(e) (the model loader folds
it into attn_in), so the softmax is base 2 over the stored values; operands() multiplies q and p
by log2(e) before rounding them to bf16.  In the split modes (bf16x3, bf16x6, f16x3) q and p are
unscaled, the kernel multiplies the score by log2(e) and takes the base-2 softmax: the natural
softmax of s.  The statistic of every flash mode is in the log2 domain, c = max + log2(sum) of
t = s log2(e) (bf16: t = s).  The fp32 route takes the natural softmax and stores (max, 1 / sum);
the tests turn that pair into c = max - ln(1 / sum) in float64.

Inputs (operands()).  One default_rng seed per (mode, H, L, hid) -- not pmax, and pos_tab is a
smooth function of x = j - i and the column, so tables for different pmax hold equal values at
equal x.  q, k ~ 0.665 N(0, 1) over 30 dims (score std ~2.4 nats), p ~ 0.5 N(0, 1).  Dims 0 and 1
carry the edges: on the RAMP rows (frame % 4 == 1 within its sequence) q[0] = 0.98765 and
k_j[0] = 0.0317 j (one nat up per key block: the row maximum rises at most block boundaries, so
the online rescale runs); on the other rows q[1] = 0.98765 and k_j[1] = -0.01585 j (the maximum
sits in the first blocks and the `__any(mn > m)` branch is mostly skipped).  Neither constant has
a short bit pattern: an exactly representable ramp would add to the bound's sum |q||k| and carry
no split error, and hide a lost piece.  v, h3 ~ N(0, 1).  In the bf16 mode every stored
operand is rounded to bf16 here, so that rounding is the reference's input and no error term.

Bound.  u = 2^-24 (f32), u_b = 2^-8 (bf16, 8 significant bits); U_OP the per-product error of a mode's split
(tests/test_gpu_gemm.py): 0 fp32 / bf16, 2^-15 bf16x3 (the u + v < 2 products
of 2 bf16 pieces), 2^-22 bf16x6, 2^-21 f16x3 (the dropped lo lo term, ~2^-22, and the lo pieces'
own rounding).  With Sq = sum |q||k|, Sp = sum |p||R|, kappa = log2(e) in the split modes else 1,
lnb = ln 2 on the flash routes and 1 in fp32, every named term is one rounding a mode performs:

    ds_ij   = kappa ((U_OP + 34 u) Sq        split products, f32 accumulation of 32 + 2 terms
                   + (u_pos + 6 u) Sp)        u_pos = u_b in the bf16 mode: pos rows rounded in-kernel
              + 2 u |t_ij|                    the score's own rounding and its log2(e) scaling
    D_i     = sum_j P_ij ds_ij                what the score errors do to log(sum)
    dcr_i   = u (2 |c_i| + 2 |log sum_i| + 4) c = max + log(sum) in f32, the log's own ulp
    eta_ij  = 2^-23 + 2 u lnb |t_ij - max_i|  hardware exp2 (1 ulp) and its argument's rounding
    eta_sum = nkb 2^-22 + (nkb + 18) u        the sum over nkb key blocks and its rescales
    relP_ij = expm1(lnb (ds_ij + D_i + dcr_i) + eta_ij + eta_sum)
                                              ln 2 |delta s| p: a score error amplified into a weight

    |A0 - P|      <= P relP + u P + 2^-125
    |c_got - c|   <= D + (eta_sum + 2^-22) / lnb + dcr
    |out - P v|   <= sum_j P |v| relP + (u_pv + (L + 16 + nkb) u + nkb 2^-22) sum_j P |v|
                     + (u_st + 2 u) |out| + floor
                     u_pv = u_b (bf16: P rounded to bf16 for the MFMA) or U_OP; u_st = u_b for a bf16
                     output else u; (L + 16 + nkb) u the f32 accumulation over L keys; nkb 2^-22
                     the online rescales; floor = L 2^-35 max |v| in f16x3 (the fp16 pieces of a
                     weight below 2^-14 are subnormal)
    |t1t - t1|    <= (5 2^-23 + 2 u + u_piece) |t1| + floor
                     tanhf within 5 ulp (the OpenCL bound its library states), the product, the piece
                     split: u_piece = u_b, u_b^2, u_b^3 for 1 / 2 / 3 bf16 pieces, 2^-22 and
                     floor 2^-36 for the fp16 pair
    |z - ref|     <= |y| (the `out` form with v -> t1, u_pv + the t1 terms) + (u_st + 2 u) |z|
"""
import math
import zlib
from collections import namedtuple

import numpy as np

LOG2E = 1.4426950408889634
U = 2.0 ** -24
UB = 2.0 ** -8
U_OP = {"fp32": 0.0, "bf16": 0.0, "bf16x3": 2.0 ** -15, "bf16x6": 2.0 ** -22, "f16x3": 2.0 ** -21}
U_TANH = 5 * 2.0 ** -23
U_PIECE = {"bf16": UB, "bf16x3": UB ** 2, "bf16x6": UB ** 3, "f16x3": 2.0 ** -22}
# the edge dims' values (operands()): no short bit patterns, so every piece of a split carries them
Q_EDGE, K_RAMP = 0.98765, 0.0317
SENTINEL = np.float32(-777.25)
SENTINEL16 = 0x7E7E

MODES = ["fp32", "bf16", "bf16x3", "bf16x6", "f16x3"]
ROUTE_MODES = {"weights": ["fp32", "bf16x3", "bf16x6"],
               "sa": MODES,
               "nonlin": ["bf16", "bf16x3", "bf16x6", "f16x3"]}
RAGGED = (1, 3, 33, 0, 130, 64, 289)
SINGLES = [(1,), (4,), (5,), (32,), (128,), (129,)]
HIDS = [144, 192, 288, 384]

# route: "weights" / "sa" / "nonlin"; L: the per-sequence lengths; pmax: the table's half size
Case = namedtuple("Case", "route mode H L pmax hid")


def pmax_default(L):
    return max(L) + 192  # the engine's guarantee (ensure_pos_tables)


def pmax_min(mode, L):
    """The smallest table the entry takes: max(L); the fp32 kernels read unclamped rows for every
    (query, key) of their 32 x 32 tiles, so max(L) rounded up to 32."""
    return (max(L) + 31) // 32 * 32 if mode == "fp32" else max(L)


def route_cases(route, mode):
    """The GPU cases of one (route, mode): the ragged batch at H = 2 and 8 (nonlin: every hid at
    H = 2), the single-sequence batches, pmax = 2048."""
    hid0 = 144 if route == "nonlin" else 0
    mk = lambda H, L, pmax=None, hid=hid0: Case(route, mode, H, tuple(L), pmax or pmax_default(L), hid)
    cs = [mk(2, RAGGED), mk(8, RAGGED)]
    if route == "nonlin":
        cs += [mk(2, RAGGED, hid=h) for h in HIDS[1:]]
    cs += [mk(2, L) for L in SINGLES]
    cs.append(mk(2, RAGGED, 2048))
    return cs


def min_pmax_pair(route, mode):
    """(the default-pmax ragged case, the same at the smallest pmax): equal bit for bit."""
    c = route_cases(route, mode)[0]
    return c, c._replace(pmax=pmax_min(mode, c.L))


def case_id(c):
    return f"{c.route}_{c.mode}_H{c.H}_L{'-'.join(map(str, c.L))}_p{c.pmax}" + \
        (f"_hid{c.hid}" if c.route == "nonlin" else "")


def rne_bf16(x):
    """float32 -> the nearest-even bfloat16, returned as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def f16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def offsets(L):
    return np.concatenate([[0], np.cumsum(L)]).astype(np.int64)


def stride(mode, L):
    return (L + 3) // 4 * 4 if mode == "fp32" else (L + 31) // 32 * 32


def is_ramp(i):
    return i % 4 == 1


def pos_table(coef, pmax, H):
    x = np.arange(-(pmax - 1), pmax, dtype=np.float64)[:, None]
    amp, w, ph = 0.5 + coef[0], 0.5 + 2.5 * coef[1], 2 * math.pi * coef[2]
    return (amp * np.cos(w * np.arctan(x / 12.0) + ph)).astype(np.float32)


def operands(c):
    """The stored operands of a case (float32 arrays; bf16 mode: bf16-representable)."""
    rng = np.random.default_rng(zlib.crc32(repr((c.mode, c.H, c.L, c.hid)).encode()))
    H, R = c.H, int(sum(c.L))
    coef = rng.uniform(size=(3, 4 * H))
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    q, k, p = f(R, H, 32) * np.float32(0.665), f(R, H, 32) * np.float32(0.665), f(R, H, 4) * np.float32(0.5)
    v1, v2 = f(R, 12 * H), f(R, 12 * H)
    h3 = f(R, 3 * c.hid) if c.hid else None
    j = np.concatenate([np.arange(n) for n in c.L]).astype(np.float32)  # frame within its sequence
    ramp = is_ramp(j.astype(np.int64))
    q[:, :, 0] = np.where(ramp, Q_EDGE, 0.0)[:, None]
    q[:, :, 1] = np.where(ramp, 0.0, Q_EDGE)[:, None]
    k[:, :, 0] = (j * np.float32(K_RAMP))[:, None]
    k[:, :, 1] = (-j * np.float32(K_RAMP / 2))[:, None]
    pos = pos_table(coef, c.pmax, H)
    if c.mode == "bf16":
        q, p = q * np.float32(LOG2E), p * np.float32(LOG2E)
        q, k, p, v1, v2 = (rne_bf16(a) for a in (q, k, p, v1, v2))
        h3 = None if h3 is None else rne_bf16(h3)
    qkp = np.concatenate([q.reshape(R, -1), k.reshape(R, -1), p.reshape(R, -1)], axis=1)
    return dict(qkp=np.ascontiguousarray(qkp), pos=pos, v1=v1, v2=v2, h3=h3)


def alone(c, o, b):
    """Sequence b of a case as a batch of its own, on the same stored operands and table."""
    off = offsets(c.L)
    r = slice(off[b], off[b + 1])
    return c._replace(L=(c.L[b],)), dict(qkp=o["qkp"][r], pos=o["pos"], v1=o["v1"][r], v2=o["v2"][r],
                                         h3=None if o["h3"] is None else o["h3"][r])


def head_operands(c, o, b, h, dt=np.float64):
    off, H = offsets(c.L), c.H
    x = o["qkp"][off[b]:off[b + 1]].astype(dt)
    return (x[:, 32 * h:32 * h + 32], x[:, 32 * H + 32 * h:32 * H + 32 * h + 32],
            x[:, 64 * H + 4 * h:64 * H + 4 * h + 4], o["pos"][:, 4 * h:4 * h + 4].astype(dt))


class Dom:
    """Softmax domain of a mode: t = kappa s; base 2 (flash) or e (fp32)."""

    def __init__(self, mode):
        self.kappa = LOG2E if mode in ("bf16x3", "bf16x6", "f16x3") else 1.0
        self.lnb = 1.0 if mode == "fp32" else math.log(2.0)

    def exp(self, x):
        return np.exp(self.lnb * x)

    def log(self, x):
        return np.log(x) / self.lnb


def head_reference(c, o, b, h):
    """float64 weights and statistic of (sequence b, head h) and the bound's per-element parts."""
    q, k, p, Rh = head_operands(c, o, b, h)
    L, d = c.L[b], Dom(c.mode)
    idx = np.arange(L)[None, :] - np.arange(L)[:, None] + c.pmax - 1
    Rg = Rh[idx]  # [i][j][4]
    t = d.kappa * (q @ k.T + np.einsum("ic,ijc->ij", p, Rg))
    Sq = np.abs(q) @ np.abs(k).T
    Sp = np.einsum("ic,ijc->ij", np.abs(p), np.abs(Rg))
    m = t.max(axis=1, keepdims=True)
    w = d.exp(t - m)
    l = w.sum(axis=1, keepdims=True)
    P, cst = w / l, m + d.log(l)
    nkb = (L + 31) // 32
    u_pos = UB if c.mode == "bf16" else 0.0
    ds = d.kappa * ((U_OP[c.mode] + 34 * U) * Sq + (u_pos + 6 * U) * Sp) + 2 * U * np.abs(t)
    D = (P * ds).sum(axis=1, keepdims=True)
    dcr = U * (2 * np.abs(cst) + 2 * np.abs(d.log(l)) + 4)
    eta = 2.0 ** -23 + 2 * U * d.lnb * np.abs(t - m)
    eta_sum = nkb * 2.0 ** -22 + (nkb + 18) * U
    relP = np.expm1(d.lnb * (ds + D + dcr) + eta + eta_sum)
    return dict(P=P, relP=relP, c=cst[:, 0], bc=(D + (eta_sum + 2.0 ** -22) / d.lnb + dcr)[:, 0],
                L=L, nkb=nkb)


def _pv_bound(c, hr, V, out):
    """Bound of out = P V (V float64 [L][n]) without the storage terms."""
    G = hr["P"] @ np.abs(V)
    Gw = (hr["P"] * hr["relP"]) @ np.abs(V)
    u_pv = UB if c.mode == "bf16" else U_OP[c.mode]
    floor = hr["L"] * 2.0 ** -35 * (np.abs(V).max() if V.size else 0.0) if c.mode == "f16x3" else 0.0
    return Gw + (u_pv + (hr["L"] + 16 + hr["nkb"]) * U + hr["nkb"] * 2.0 ** -22) * G + floor


def u_store(c):
    return UB if c.mode == "bf16" else U


def reference_weights(c, o):
    """(ref, bound): the flat head-0 weight buffer, sequence blocks [L][stride], padding 0 / 0."""
    ref, bnd = [], []
    for b, L in enumerate(c.L):
        if L == 0:
            continue
        hr = head_reference(c, o, b, 0)
        S = stride(c.mode, L)
        r, e = np.zeros((L, S)), np.zeros((L, S))
        r[:, :L] = hr["P"]
        e[:, :L] = hr["P"] * hr["relP"] + U * hr["P"] + 2.0 ** -125
        ref.append(r.ravel())
        bnd.append(e.ravel())
    return np.concatenate(ref), np.concatenate(bnd)


def padding_mask_weights(c):
    """True on the padding columns [L, stride) of the flat weight buffer."""
    out = []
    for L in c.L:
        if L:
            m = np.zeros((L, stride(c.mode, L)), bool)
            m[:, L:] = True
            out.append(m.ravel())
    return np.concatenate(out)


def reference_sa(c, o):
    """dict of (ref, bound) for out1, out2 [R][12 H] and the statistic c [R][H] (log2 domain on
    the flash routes, natural in fp32)."""
    R, H, off = int(sum(c.L)), c.H, offsets(c.L)
    res = {k: (np.zeros(s), np.zeros(s)) for k, s in
           (("out1", (R, 12 * H)), ("out2", (R, 12 * H)), ("stats", (R, H)))}
    for b, L in enumerate(c.L):
        if L == 0:
            continue
        rows = slice(off[b], off[b + 1])
        for h in range(H):
            hr = head_reference(c, o, b, h)
            res["stats"][0][rows, h], res["stats"][1][rows, h] = hr["c"], hr["bc"]
            for key, vk in (("out1", "v1"), ("out2", "v2")):
                V = o[vk][rows, 12 * h:12 * h + 12].astype(np.float64)
                out = hr["P"] @ V
                res[key][0][rows, 12 * h:12 * h + 12] = out
                res[key][1][rows, 12 * h:12 * h + 12] = _pv_bound(c, hr, V, out) + \
                    (u_store(c) + 2 * U) * np.abs(out)
    return res


def t1_planes(mode):
    return {"bf16": 1, "bf16x3": 2, "bf16x6": 3, "f16x3": 2}[mode]


def reference_nonlin(c, o):
    """dict of (ref, bound): t1t [hid][R32] (the image's value, padding 0 / 0) and, where the
    route runs flash mode 3 (bf16, f16x3), z [R][hid]."""
    hid, off = c.hid, offsets(c.L)
    L32 = [(L + 31) // 32 * 32 for L in c.L]
    o32 = offsets(L32)
    h3 = o["h3"].astype(np.float64)
    t1 = np.tanh(h3[:, :hid]) * h3[:, hid:2 * hid]
    y = h3[:, 2 * hid:]
    floor = 2.0 ** -36 if c.mode == "f16x3" else 0.0
    e1 = (U_TANH + 2 * U + U_PIECE[c.mode]) * np.abs(t1) + floor
    img, ebd = np.zeros((hid, int(o32[-1]))), np.zeros((hid, int(o32[-1])))
    for b, L in enumerate(c.L):
        img[:, o32[b]:o32[b] + L] = t1[off[b]:off[b + 1]].T
        ebd[:, o32[b]:o32[b] + L] = e1[off[b]:off[b + 1]].T
    res = {"t1t": (img, ebd)}
    if c.mode in ("bf16", "f16x3"):
        z, bz = np.zeros_like(t1), np.zeros_like(t1)
        for b, L in enumerate(c.L):
            if L == 0:
                continue
            rows = slice(off[b], off[b + 1])
            hr = head_reference(c, o, b, 0)
            inner = hr["P"] @ t1[rows]
            bi = _pv_bound(c, hr, t1[rows], inner) + hr["P"] @ e1[rows]
            z[rows] = inner * y[rows]
            bz[rows] = bi * np.abs(y[rows]) + (u_store(c) + 2 * U) * np.abs(z[rows])
        res["z"] = (z, bz)
    return res


def padding_mask_t1t(c):
    L32 = [(L + 31) // 32 * 32 for L in c.L]
    o32 = offsets(L32)
    m = np.ones((c.hid, int(o32[-1])), bool)
    for b, L in enumerate(c.L):
        m[:, o32[b]:o32[b] + L] = False
    return m


def decode_t1t(mode, img):
    """The value a stored t1^T image holds: uint16 [planes][hid][R32] -> float64 [hid][R32]."""
    img = np.ascontiguousarray(img, np.uint16)
    if mode == "f16x3":
        pl = img.view(np.float16).astype(np.float64)
        return pl[0] + pl[1] / 2048.0
    pl = (img.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return pl.sum(axis=0)


def ratio(got, ref, bound):
    """|got - ref| / bound per element; where the bound is 0 (padding) any difference is inf."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))


def stats_as_c(c, stats):
    """The statistic as c = max + log(sum): fp32 stores (max, 1 / sum)."""
    s = np.asarray(stats, np.float64)
    return s[..., 0] - np.log(s[..., 1]) if c.mode == "fp32" else s


# ---------------------------------------------------------------------------------------------
# numpy emulation: f32 arithmetic, the modes' pieces, key blocks of 32, the online rescale -- the
# roundings the bound names and no others.  `mut` names one defect (tests/test_attention_reference.py).
# The pseudo-mode "bf16x1" is one precision step below bf16x3: a split mode's f32 storage and
# log2(e) scaling with a single bf16 piece per operand (lower_mode()).
# ---------------------------------------------------------------------------------------------
F = np.float32
NEG = F(-np.inf)


def split(mode, x):
    """The MFMA pieces of an f32 operand, as f32 arrays that sum (nearly) to x."""
    x = np.asarray(x, F)
    if mode in ("fp32", "bf16"):
        return [x]
    if mode == "bf16x1":
        return [rne_bf16(x)]
    if mode == "f16x3":
        hi = f16(x)
        return [hi, f16((x - hi) * F(2048)) / F(2048)]
    out = []
    for _ in range(3 if mode == "bf16x6" else 2):
        out.append(rne_bf16(x))
        x = x - out[-1]
    return out


def prod(mode, X, Y):
    """sum over u + v < NP of X_u Y_v^T, smallest terms first, f32 accumulate (fp32 / bf16: one)."""
    n = len(X)
    acc = None
    for s in range(n - 1, -1, -1):
        for u in range(s, -1, -1):
            t = X[u] @ Y[s - u].T
            acc = t if acc is None else acc + t
    return acc.astype(F)


def emu_scores(c, o, b, h, mut=None, mask=True):
    """t^ [L][L32] f32 in the mode's softmax domain, keys >= L at -inf (rows past L - 1 clamped)."""
    q, k, p, Rh = head_operands(c, o, b, h, F)
    L = c.L[b]
    L32 = (L + 31) // 32 * 32
    kc = k[np.minimum(np.arange(L32), L - 1)]
    mode = c.mode
    qk = prod(mode, split(mode, q), split(mode, kc))
    idx = np.arange(L32)[None, :] - np.arange(L)[:, None] + c.pmax - 1 + (1 if mut == "pos_shift" else 0)
    Rg = Rh[np.clip(idx, 0, 2 * c.pmax - 2)]
    if mode == "bf16":
        Rg = rne_bf16(Rg)
    pos = np.zeros((L, L32), F)
    for d in range(4):
        pos = pos + p[:, d:d + 1] * Rg[:, :, d]
    t = qk + pos
    if mode in ("bf16x1", "bf16x3", "bf16x6", "f16x3"):
        t = t * F(LOG2E)
    if not mask:
        return t.astype(F)
    lim = L + (1 if mut == "mask_extra" else -1 if mut == "mask_short" else 0)
    if mut == "mask_short" and L < 2:
        lim = L
    t[:, max(lim, 0):] = NEG
    return t.astype(F)


def _exp(c, x):
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.exp(x) if c.mode == "fp32" else np.exp2(x)).astype(F)


def _log(c, x):
    with np.errstate(divide="ignore"):
        return (np.log(x) if c.mode == "fp32" else np.log2(x)).astype(F)


def _pv(c, V, e):
    """V^T P^T of one key block: e [L][32] the weights (f16x3: scaled by 2^11), V [32][n]."""
    mode = c.mode
    if mode == "f16x3":
        ys = f16(e)
        yl, yh = f16(e - ys), f16(ys / F(2048))
        x0 = f16(V)
        x1 = f16((V - x0) * F(2048))
        with np.errstate(invalid="ignore"):  # (a defect may push e past fp16's range)
            return ((yh @ x1) + (yl @ x0) + (ys @ x0)).astype(F)
    if mode in ("bf16", "bf16x1"):
        return (rne_bf16(e) @ rne_bf16(V)).astype(F)
    return prod(mode, split(mode, e), split(mode, V.T))


def emu_online(c, t, V, mut=None):
    """One online pass (flash modes 1 / 3, attn_sa online): returns (O / l, statistic)."""
    L, kE = t.shape[0], F(11.0 if c.mode == "f16x3" else 0.0)
    m, l, lh = np.full((L, 1), NEG), np.zeros((L, 1), F), np.zeros((L, 1), F)
    O = np.zeros((L, V.shape[1]), F)
    for kb in range(t.shape[1] // 32):
        s = t[:, 32 * kb:32 * kb + 32]
        mn = np.maximum(m, s.max(axis=1, keepdims=True))
        sc = np.where(np.isneginf(m), F(0), _exp(c, m - mn)).astype(F)
        if not (mut == "skip_rescale" and kb >= 1):
            O = O * sc
        l, lh, m = l * sc, lh * sc, mn
        e = _exp(c, s - m + kE)
        l = l + e.sum(axis=1, keepdims=True, dtype=F)
        half0 = ((np.arange(32) >> 2) & 1) == 0  # the keys lane half 0 holds
        lh = lh + e[:, half0].sum(axis=1, keepdims=True, dtype=F)
        rows = np.minimum(np.arange(32 * kb, 32 * kb + 32), V.shape[0] - 1)
        O = O + _pv(c, V[rows], e)
    stat = m + _log(c, lh if mut == "half_stat" else l) - kE
    return (O * (F(1) / l)).astype(F), stat.astype(F)[:, 0]


def emu_stats_pass(c, t, V, stat):
    """Flash mode 2 / attn_sa with stored statistics: P = exp(t - c) directly."""
    kE = F(11.0 if c.mode == "f16x3" else 0.0)
    O = np.zeros((t.shape[0], V.shape[1]), F)
    for kb in range(t.shape[1] // 32):
        e = _exp(c, t[:, 32 * kb:32 * kb + 32] - stat[:, None] + kE)
        rows = np.minimum(np.arange(32 * kb, 32 * kb + 32), V.shape[0] - 1)
        O = O + _pv(c, V[rows], e)
    return (O * F(1.0 / 2048 if c.mode == "f16x3" else 1.0)).astype(F)


def _store(c, x):
    return rne_bf16(x) if c.mode == "bf16" else np.asarray(x, F)


def emulate_weights(c, o, mut=None):
    """The flat head-0 weight buffer (mode 0: statistics, then exp2(t - c); fp32: exp(t - max) / sum)."""
    out = []
    for b, L in enumerate(c.L):
        if L == 0:
            continue
        t = emu_scores(c, o, b, 0, mut)
        m = t.max(axis=1, keepdims=True)
        l = _exp(c, t - m).sum(axis=1, keepdims=True, dtype=F)
        if mut == "pad_nonzero":  # the second pass forgets the mask
            t = emu_scores(c, o, b, 0, mut, mask=False)
        A = _exp(c, t - m) * (F(1) / l) if c.mode == "fp32" else _exp(c, t - (m + _log(c, l)))
        out.append(A[:, :stride(c.mode, L)].astype(F).ravel())
    return np.concatenate(out)


def emulate_sa(c, o, mut=None):
    R, H, off = int(sum(c.L)), c.H, offsets(c.L)
    out1, out2 = np.zeros((R, 12 * H), F), np.zeros((R, 12 * H), F)
    stats = np.zeros((R, H), F)
    for b, L in enumerate(c.L):
        if L == 0:
            continue
        rows = slice(off[b], off[b + 1])
        for h in range(H):
            t = emu_scores(c, o, b, h, mut)
            cols = np.arange(12 * h, 12 * h + 12)
            if mut == "v_dim11" and h + 1 < H:
                cols[11] += 1
            a, st = emu_online(c, t, o["v1"][rows][:, cols], mut)
            out1[rows, 12 * h:12 * h + 12], stats[rows, h] = _store(c, a), st
            out2[rows, 12 * h:12 * h + 12] = _store(c, emu_stats_pass(c, t, o["v2"][rows][:, cols], st))
    return out1, stats, out2


def lower_mode(mode):
    """The mode one precision step down, for the check that a bound is not slack."""
    return {"bf16x6": "bf16x3", "f16x3": "bf16x3", "bf16x3": "bf16x1"}[mode]


def emu_t1_pieces(c, o):
    """t1 = tanhf(s) * x in f32 and its stored pieces [planes][R][hid] (values, f32)."""
    hid = c.hid
    h3 = o["h3"].astype(F)
    t1 = (np.tanh(h3[:, :hid]) * h3[:, hid:2 * hid]).astype(F)
    return [rne_bf16(t1)] if c.mode == "bf16" else split(c.mode, t1)


def emulate_nonlin(c, o, mut=None):
    """(t1t value image [hid][R32] float64 from the stored pieces, z [R][hid] or None)."""
    hid, off = c.hid, offsets(c.L)
    L32 = [(L + 31) // 32 * 32 for L in c.L]
    o32 = offsets(L32)
    pcs = emu_t1_pieces(c, o)
    val = np.sum([p.astype(np.float64) for p in pcs], axis=0)
    img = np.zeros((hid, int(o32[-1])))
    if mut == "pad_nonzero":
        img[:] = 2.0 ** -20
    for b, L in enumerate(c.L):
        img[:, o32[b]:o32[b] + L] = val[off[b]:off[b + 1]].T
    if c.mode not in ("bf16", "f16x3"):
        return img, None
    t1 = np.sum(pcs, axis=0, dtype=F) if c.mode == "bf16" else None
    y = o["h3"][:, 2 * hid:].astype(F)
    z = np.zeros((off[-1], hid), F)
    nf = 3 if c.mode == "f16x3" else (5 if ((hid + 31) // 32 % 5 == 0 or (hid + 31) // 32 == 9) else 6)
    for b, L in enumerate(c.L):
        if L == 0:
            continue
        rows = slice(off[b], off[b + 1])
        t = emu_scores(c, o, b, 0, mut)
        if c.mode == "bf16":
            inner, _ = emu_online(c, t, t1[rows], mut)
        else:  # f16x3: the stored fp16 pair is the V operand's pieces
            inner, _ = emu_online_pieces(c, t, pcs[0][rows], pcs[1][rows], mut)
        yy = y[rows]
        if mut == "z_chunk_shift":  # chunks past the first read y one fragment on
            ch = np.arange(hid)
            yy = yy[:, np.where(ch >= nf * 32, np.minimum(ch + 32, hid - 1), ch)]
        z[rows] = _store(c, inner * yy)
    return img, z


def emu_online_pieces(c, t, x0, x1s, mut=None):
    """emu_online for f16x3 mode 3: V given as its stored pieces hi and lo 2^-11."""
    L, kE = t.shape[0], F(11.0)
    m, l = np.full((L, 1), NEG), np.zeros((L, 1), F)
    O = np.zeros((L, x0.shape[1]), F)
    x1 = x1s * F(2048)
    for kb in range(t.shape[1] // 32):
        s = t[:, 32 * kb:32 * kb + 32]
        mn = np.maximum(m, s.max(axis=1, keepdims=True))
        sc = np.where(np.isneginf(m), F(0), _exp(c, m - mn)).astype(F)
        if not (mut == "skip_rescale" and kb >= 1):
            O = O * sc
        l, m = l * sc, mn
        e = _exp(c, s - m + kE)
        l = l + e.sum(axis=1, keepdims=True, dtype=F)
        rows = np.minimum(np.arange(32 * kb, 32 * kb + 32), x0.shape[0] - 1)
        ys = f16(e)
        yl, yh = f16(e - ys), f16(ys / F(2048))
        O = O + ((yh @ x1[rows]) + (yl @ x0[rows]) + (ys @ x0[rows])).astype(F)
    return (O * (F(1) / l)).astype(F), None
