"""The general GEMMs behind their other operand loaders: cases, seeded operands, float64
references, the per-element bound, and a numpy emulation of every route (test infrastructure).

Two entry points are held to this module by tests/test_gpu_gemm_loaders.py:

    zasr_selftest_conv_gemm   conv.4 / conv.7 of Conv2dSubsampling: gemm_f32 / gemm_bf16 / gemm_x3
                              with ALOAD_CONV2 / ALOAD_CONV3 over one z-slice per sequence
    zasr_selftest_gemm_aload  gemm_f32 with ALOAD_BNRELU / ALOAD_IM2COL1D (the CAM++ projections)

tests/test_gemm_loader_reference.py (no GPU) holds the references to torch's conv2d / conv1d,
the emulations to the bound, and shows that each listed single defect of a loader is visible on
the GPU test's fixture.

References.  Every ragged operator is evaluated sequence by sequence (window by window) on that
sequence's own rows as a strided-slice convolution with explicit zero padding, as in
conv_reference.py; none of them restates a loader's index formula.

    conv.4    3x3, stride (2, 2), no padding, over [T - 2][80] x 8 channels, then SwooshR
    conv.7    3x3, stride (1, 2), no padding, over [l2][39] x 32 channels, then SwooshR
    im2col1d  conv1d with the given stride, dilation and zero padding, channels last
    BN-ReLU   A' = max(a s + b, 0) before the product

Bound, per output element: the derived table of test_gpu_gemm.py's docstring, its constants
imported from there, not tuned.  With u = 2^-24 and S = |A'| |W'|^T + |bias| over the taps
actually summed (a padded tap contributes nothing to S):

    pre-activation value     (u_op + 2 K u) S
    fast SwooshR             + 1e-6   (gemm_bf16, gemm_x3; gemm_f32's libm form: + 0)
    RELU epilogue            unchanged (1-Lipschitz)
    MULAUX                   x |aux|
    bf16 C                   + 2^-8 |out|

In the bf16 mode A and W are rounded to bf16 (nearest even) in the reference.  ALOAD_BNRELU forms
A' in f32 with one fused multiply-add: fl(a s + b) = (a s + b)(1 + d), |d| <= u, and max(., 0)
keeps that relative error, so |A'_kernel - A'| <= u |A'| and the product moves by at most
u |A'| |W|^T <= u S: u_op = u for that loader (0 for ALOAD_IM2COL1D, which only gathers).

Emulation.  emulate_conv / emulate_aload transcribe the loaders' index arithmetic from
csrc/gemm_dev.h (load_a4), csrc/gemm.hip (load_a8, the bf16-A branches) and csrc/gemm_x3.hip
(gemm_glds_h3_kernel's gathered row bases) -- loads clamped into range, zero selected afterwards
-- with f32 products accumulated in f32 and each mode's operand rounding, and store through the
slices' c_off / ldc into an image with guard rows.  `defect` switches one deliberate mistake on.
"""
import math
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

from test_gpu_gemm import ACT_ABS, U, U_BF16, U_OP, rne_bf16

FILL = -777.25
ALOAD_BNRELU, ALOAD_IM2COL1D = 4, 5

# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
ConvCase = namedtuple("ConvCase", "mode a16 c16 which T")

# (mode, a_bf16, c_bf16, layers): what the public entry points accept for these loaders
CONV_COMBOS = [
    ("fp32", 0, 0, (4, 7)),    # decode
    ("bf16", 1, 1, (4, 7)),    # decode
    ("bf16", 0, 0, (4, 7)),
    ("bf16", 0, 1, (7,)),
    ("bf16x3", 0, 0, (4, 7)),  # decode
    ("bf16x6", 0, 0, (4, 7)),  # decode
    ("f16x3", 0, 0, (4, 7)),   # decode
]
EDGE_T = (9, 10, 21, 35, 12, 22)
SINGLE_T = ((9,), (35,))


def conv_rows(which, T):
    """GEMM rows (output positions) per slice."""
    return [((t - 3) // 2) * 39 if which == 4 else ((t - 7) // 2) * 19 for t in T]


def pick_tile(N, max_M, num_slices, no32=False):
    """gemm_dev.h pick_tile: (BN, big); big = the 128-row tile, from 512 blocks of it up, the
    count taken over every slice at the longest slice's rows."""
    cdiv = lambda a, b: (a + b - 1) // b
    pad128, pad64, pad32 = cdiv(N, 128) * 128, cdiv(N, 64) * 64, cdiv(N, 32) * 32
    BN = 128 if pad128 * 100 <= pad32 * 115 else 64 if pad64 * 100 <= pad32 * 115 else 32
    if no32 and BN == 32 and N > 64:
        BN = 64
    return BN, cdiv(max_M, 128) * cdiv(N, BN) * num_slices >= 512


def conv_tile(which, T):
    return pick_tile(32 if which == 4 else 128, max(conv_rows(which, T)), len(T))


def dispatch_T(which, nseq=8):
    """The shortest nseq equal sequences whose launch takes the 128-row tile."""
    t = 9
    while not conv_tile(which, (t,) * nseq)[1]:
        t += 1
    return (t,) * nseq


def conv_cases(Ts, skip=()):
    return [ConvCase(m, a, c, w, tuple(T)) for m, a, c, ws in CONV_COMBOS for w in ws for T in Ts
            if (m, w) not in skip]


EDGE_CASES = conv_cases([EDGE_T] + list(SINGLE_T))
# f16x3 conv.7 is gemm_glds_h3_kernel at every size: its case is the edge batch
DISPATCH_CASES = [c for w in (4, 7) for c in conv_cases([dispatch_T(w)], skip=[("f16x3", 7)])
                  if c.which == w]


def conv_case_id(c):
    t = {(0, 0): "", (0, 1): "_f32bf16", (1, 1): "_bf16bf16"}[(c.a16, c.c16)]
    T = f"{len(c.T)}x{c.T[0]}" if len(set(c.T)) == 1 else "-".join(map(str, c.T))
    return f"{c.mode}{t if c.mode == 'bf16' else ''}_conv{c.which}_T{T}"


# kind "i2c" / "bn"; i2c = (Tin, Tout, C, stride, dil, pad); M = windows x Tout
AloadCase = namedtuple("AloadCase", "name kind M K N lda ldc c_col epi i2c ldaux")


def tdnn_cases():
    out = []
    for C, lda in ((160, 160), (8, 12)):
        for T in (1, 2, 97, 150):
            T2 = (T - 1) // 2 + 1
            out.append(AloadCase(f"tdnn_C{C}_T{T}", "i2c", 3 * T2, 5 * C, 128, lda, 224, 0, "RELU",
                                 (T, T2, C, 2, 1, 2), 0))
    return out


def local_cases():
    out = []
    for dil in (1, 2):
        for T2 in (1, 2, 3, 49, 75, 115):
            out.append(AloadCase(f"local_dil{dil}_T{T2}", "i2c", 3 * T2, 384, 32, 128, 224, 128,
                                 "MULAUX", (T2, T2, 128, 1, dil, dil), 32))
    # the decode's ldaux equals N; these two make an aux row stride of its own visible
    for T2 in (3, 49):
        out.append(AloadCase(f"local_dil2_T{T2}_ldaux48", "i2c", 3 * T2, 384, 32, 128, 224, 128,
                             "MULAUX", (T2, T2, 128, 1, 2, 2), 48))
    return out


def bnrelu_cases():
    return [AloadCase(f"bn_K{K}_lda{lda}_N{N}_M{M}_{epi}_ldc{N + x}", "bn", M, K, N, lda, N + x, 0, epi,
                      None, 0)
            for K, lda in ((128, 224), (160, 224), (36, 40)) for N in (128, 32) for M in (1, 65, 225)
            for epi in ("RELU", "NONE") for x in (0, 32)]


ALOAD_GROUPS = {"tdnn": tdnn_cases(), "local": local_cases(), "bnrelu": bnrelu_cases()}


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------------------------------------
# conv.4 / conv.7: operands, reference, bound
# ---------------------------------------------------------------------------------------------
CONV_GEOM = {4: dict(cin=8, fin=80, fout=39, n=32, st=2, cut=2), 7: dict(cin=32, fin=39, fout=19, n=128, st=1, cut=3)}


def conv_lengths(which, T):
    """(input rows, output rows) per sequence."""
    T = np.asarray(T)
    if which == 4:
        return T - 2, (T - 3) // 2
    return (T - 3) // 2, (T - 7) // 2


@lru_cache(maxsize=4)
def conv_operands(which, T):
    """Seeded by (layer, lengths) only, so every mode meets the same problem.  W4 is
    [N][kt][kf][C]; the kernels' [N][K] is its reshape (tap-major, channel-minor).  A sequence
    of SINGLE_T is that sequence of the edge batch: its rows of the batch's A, the same W and
    bias, so its output can be compared with the batch's byte for byte."""
    g = CONV_GEOM[which]
    rin, _ = conv_lengths(which, T)
    if T in SINGLE_T:
        e = conv_operands(which, EDGE_T)
        ein, _ = conv_lengths(which, EDGE_T)
        q = EDGE_T.index(T[0])
        lo = int(ein[:q].sum())
        o = dict(e, A=e["A"][lo:lo + int(rin[0])])
        o["A"].setflags(write=False)
        return o
    rng = _rng("conv", which, T)
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    K = 9 * g["cin"]
    o = dict(A=f(int(rin.sum()), g["fin"], g["cin"]),
             W4=f(g["n"], 3, 3, g["cin"]) / np.float32(math.sqrt(K)), bias=f(g["n"]) * np.float32(0.1))
    o["W"] = o["W4"].reshape(g["n"], K)
    for v in o.values():
        v.setflags(write=False)
    return o


def conv2d_valid(x, w4, st):
    """x [rows][F][C], w4 [N][3][3][C] -> [nt][nf][N]: the unpadded 3x3 convolution with stride
    (st, 2) over (rows, F), as strided slices of x (float64)."""
    nt, nf = (x.shape[0] - 3) // st + 1, (x.shape[1] - 3) // 2 + 1
    acc = np.zeros((nt, nf, w4.shape[0]))
    for kt in range(3):
        for kf in range(3):
            acc += x[kt:kt + st * (nt - 1) + 1:st, kf:kf + 2 * (nf - 1) + 1:2] @ w4[:, kt, kf].T
    return acc


@lru_cache(maxsize=4)
def _conv_pre(which, T, h16):
    """(pre-activation, S) in float64, sequence by sequence; h16: operands rounded to bf16."""
    g = CONV_GEOM[which]
    o = conv_operands(which, T)
    A, W4 = (rne_bf16(o["A"]).reshape(o["A"].shape), rne_bf16(o["W4"]).reshape(o["W4"].shape)) if h16 \
        else (o["A"], o["W4"])
    A, W4, b = A.astype(np.float64), W4.astype(np.float64), o["bias"].astype(np.float64)
    rin, rout = conv_lengths(which, T)
    off = np.concatenate([[0], np.cumsum(rin)])
    v, s = [], []
    for q in range(len(T)):
        # conv.4 stops at l2 = (T - 3) / 2 rows: an even T - 2 leaves its last input row unused
        x = A[off[q]:off[q + 1]][:g["st"] * (int(rout[q]) - 1) + 3]
        v.append(conv2d_valid(x, W4, g["st"]) + b)
        s.append(conv2d_valid(np.abs(x), np.abs(W4), g["st"]) + np.abs(b))
        assert v[-1].shape == (rout[q], g["fout"], g["n"])
    v, s = np.concatenate(v), np.concatenate(s)
    v.setflags(write=False)
    s.setflags(write=False)
    return v, s


def swoosh_r(v):
    return np.logaddexp(0.0, v - 1.0) - 0.08 * v - 0.313261687


def conv_reference(c):
    """(float64 reference [sum rows][F'][N], bound): the module docstring's table."""
    v, S = _conv_pre(c.which, c.T, c.mode == "bf16")
    K = 9 * CONV_GEOM[c.which]["cin"]
    out = swoosh_r(v)
    e = (U_OP[c.mode] + 2 * K * U) * S + (0.0 if c.mode == "fp32" else ACT_ABS)
    if c.c16:
        e = e + U_BF16 * np.abs(out)
    return out, e


def fill_of(c16):
    """What an untouched output element reads back as."""
    return float(rne_bf16(np.float32([FILL]))[0]) if c16 else FILL


def conv_verdict(c, got):
    """(worst |got - ref| / bound, output rows that kept their initial contents)."""
    ref, bound = conv_reference(c)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    ratio = float(np.max(np.abs(got.astype(np.float64) - ref) / bound))
    kept = int(np.all(got.reshape(got.shape[0], -1) == np.float32(fill_of(c.c16)), axis=1).sum())
    return ratio, kept


# ---------------------------------------------------------------------------------------------
# gemm_f32 behind ALOAD_IM2COL1D / ALOAD_BNRELU: operands, reference, bound
# ---------------------------------------------------------------------------------------------
def aload_rows(c):
    return c.M if c.kind == "bn" else -(-c.M // c.i2c[1]) * c.i2c[0]


def aload_operands(c):
    rng = _rng("aload", c.name)
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    o = dict(A=f(aload_rows(c), c.lda), W=f(c.N, c.K) / np.float32(math.sqrt(c.K)),
             bias=f(c.N) * np.float32(0.1), C0=f(c.M, c.ldc), aux=None, scale=None, shift=None)
    if c.epi == "MULAUX":
        o["aux"] = f(c.M, c.ldaux)
    if c.kind == "bn":
        o["scale"] = rng.uniform(0.5, 1.5, c.K).astype(np.float32)
        o["shift"] = f(c.K) * np.float32(0.5)  # the loader's ReLU cuts about half
    return o


def conv1d_cl(x, w3, stride, dil, pad, Tout):
    """x [Tin][C] channels last, w3 [N][taps][C] -> [Tout][N]: conv1d with zero padding."""
    taps = w3.shape[1]
    need = stride * (Tout - 1) + dil * (taps - 1) + 1
    xp = np.zeros((max(need, pad + x.shape[0]), x.shape[1]))
    xp[pad:pad + x.shape[0]] = x
    acc = np.zeros((Tout, w3.shape[0]))
    for q in range(taps):
        acc += xp[q * dil:q * dil + stride * (Tout - 1) + 1:stride] @ w3[:, q].T
    return acc


def aload_reference(c, o):
    """(float64 reference of the N written columns [M][N], bound)."""
    A, W, b = (o[k].astype(np.float64) for k in ("A", "W", "bias"))
    if c.kind == "bn":
        Ap = np.maximum(A[:, :c.K] * o["scale"].astype(np.float64) + o["shift"].astype(np.float64), 0.0)
        v, S, u_op = Ap @ W.T + b, Ap @ np.abs(W).T + np.abs(b), U
    else:
        Tin, Tout, C, stride, dil, pad = c.i2c
        w3 = W.reshape(c.N, c.K // C, C)
        wins = [A[n * Tin:(n + 1) * Tin, :C] for n in range(c.M // Tout)]
        v = np.concatenate([conv1d_cl(x, w3, stride, dil, pad, Tout) for x in wins]) + b
        S = np.concatenate([conv1d_cl(np.abs(x), np.abs(w3), stride, dil, pad, Tout) for x in wins]) + np.abs(b)
        u_op = 0.0
    e = (u_op + 2 * c.K * U) * S
    if c.epi == "RELU":
        v = np.maximum(v, 0.0)
    elif c.epi == "MULAUX":
        x = o["aux"][:, :c.N].astype(np.float64)
        v, e = v * x, e * np.abs(x)
    return v, e


def aload_verdict(c, o, img):
    """(worst ratio on the written columns, True when every other column kept C0's bytes)."""
    ref, bound = aload_reference(c, o)
    assert img.shape == o["C0"].shape
    got = img[:, c.c_col:c.c_col + c.N].astype(np.float64)
    ratio = float(np.max(np.abs(got - ref) / bound))
    mask = np.ones(c.ldc, bool)
    mask[c.c_col:c.c_col + c.N] = False
    return ratio, bool(np.array_equal(img[:, mask].view(np.uint32), o["C0"][:, mask].view(np.uint32)))


# ---------------------------------------------------------------------------------------------
# emulation: the loaders' index arithmetic, f32 products, each mode's operand rounding
# ---------------------------------------------------------------------------------------------
def _f32(x):
    return np.ascontiguousarray(x, np.float32)


def _rne_f16(x):
    return x.astype(np.float16).astype(np.float32)


def split_product(mode, A, W):
    """A [M][K] W[N][K]^T as the mode forms it, f32 throughout."""
    A, W = _f32(A), _f32(W)
    if mode == "fp32":
        return A @ W.T
    if mode == "bf16":
        return rne_bf16(A).reshape(A.shape) @ rne_bf16(W).reshape(W.shape).T
    if mode == "f16x3":
        ah, wh = _rne_f16(A), _rne_f16(W)
        al, wl = _rne_f16((A - ah) * np.float32(2048)), _rne_f16((W - wh) * np.float32(2048))
        return ah @ wh.T + (al @ wh.T + ah @ wl.T) * np.float32(1 / 2048)
    npc = 2 if mode == "bf16x3" else 3

    def pieces(x):
        out, r = [], x
        for _ in range(npc):
            h = rne_bf16(r).reshape(x.shape)
            out.append(h)
            r = r - h
        return out
    a, w = pieces(A), pieces(W)
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for s in range(npc - 1, -1, -1):  # smallest terms first
        for i in range(s, -1, -1):
            acc += a[i] @ w[s - i].T
    return acc


def swoosh_r_f32(v):
    v = _f32(v)
    return (np.logaddexp(np.float32(0), v - np.float32(1)) - np.float32(0.08) * v - np.float32(0.313261687)).astype(np.float32)


def conv_slices(which, T):
    """engine.h frontend_conv_slices: (a_off, c_off, M) per sequence, offsets in elements."""
    g = CONV_GEOM[which]
    rin, rout = conv_lengths(which, T)
    ai = np.concatenate([[0], np.cumsum(rin)]) * g["fin"] * g["cin"]
    ci = np.concatenate([[0], np.cumsum(rout)]) * g["fout"] * g["n"]
    return [(int(ai[q]), int(ci[q]), int(rout[q]) * g["fout"]) for q in range(len(T))]


def conv_gather(which, variant, M, rows, defect=None):
    """Element offsets [rows][Kpad] from the slice's A and the zero-select mask, for GEMM rows
    0 .. rows - 1 of a slice of M rows.  variant "a4": gemm_dev.h load_a4 (float4 groups);
    "a8": gemm.hip load_a8's bf16-A branch (8-channel groups); "h3": gemm_glds_h3_kernel
    (conv.7, a 32-channel k-tile per tap from a gathered row base; rows clamped, never zeroed)."""
    K = 72 if which == 4 else 288
    Kp = -(-K // 32) * 32
    gm, gk = np.arange(rows)[:, None], np.arange(Kp)[None, :]
    ok = (gm < M) & (gk < K)
    m = np.where(gm < M, gm, M - 1)
    if variant == "h3":
        assert which == 7
        t, f = m // 19, m - (m // 19) * 19
        fs = 1 if defect == "c7_fstride1" else 2
        kt = gk // 32
        a, b = (kt % 3, kt // 3) if defect == "kt_kf_swapped" else (kt // 3, kt % 3)
        idx = (t * 39 + fs * f) * 32 + (a * 39 + b) * 32 + gk % 32
        return np.where(gk < K, idx, 0), np.broadcast_to(gk < K, idx.shape)
    grp = 4 if variant == "a4" else 8
    k = np.where(gk < K, gk, K - grp) // grp * grp  # the group's first k, clamped
    lane = gk % grp
    if which == 4:
        t, f = m // 39, m - (m // 39) * 39
        kk, c = k >> 3, k & 7
        kt, kf = kk // 3, kk - (kk // 3) * 3
        if defect == "kt_kf_swapped":
            kt, kf = kf, kt
        ts = 1 if defect == "c4_tstride1" else 2
        fs = 1 if defect == "c4_fstride1" else 2
        base = ((ts * t + kt) * 80 + fs * f + kf) * 8
        idx = base + (c if variant == "a4" else 0) + lane
    else:
        t, f = m // 19, m - (m // 19) * 19
        kk, c = k >> 5, k & 31
        kt, kf = kk // 3, kk - (kk // 3) * 3
        if defect == "kt_kf_swapped":
            kt, kf = kf, kt
        fs = 1 if defect == "c7_fstride1" else 2
        idx = ((t + kt) * 39 + fs * f + kf) * 32 + c + lane
    return idx, ok


def conv_variant(c):
    if c.mode == "f16x3" and c.which == 7:
        return "h3"
    return "a8" if c.a16 else "a4"


def emulate_conv(c, defect=None):
    """The output image [sum rows][F'][N] as the route leaves it, starting from FILL, and
    whether the guard rows before and behind it are intact."""
    g = CONV_GEOM[c.which]
    o = conv_operands(c.which, c.T)
    row_in = g["fin"] * g["cin"]
    A = np.concatenate([_f32(o["A"]).ravel(), np.ones(row_in, np.float32)])  # + a row a defect may read
    if c.a16:
        A = rne_bf16(A)
    row_out = g["fout"] * g["n"]
    sl = conv_slices(c.which, c.T)
    total = sum(s[2] for s in sl) * g["n"]
    img = np.full(total + 2 * row_out, fill_of(c.c16), np.float32)
    C = img[row_out:]  # guard row before; one behind
    for q, (a_off, c_off, M) in enumerate(sl):
        if defect == "a_off_row":
            a_off += row_in
        if defect == "prev_sequence" and q > 0:
            a_off = sl[q - 1][0]
        rows = M + 1  # one clamped row past the slice, stored by one defect only
        idx, ok = conv_gather(c.which, conv_variant(c), M, rows, defect)
        Ap = np.where(ok, A[np.minimum(a_off + idx, A.size - 1)], np.float32(0))
        v = split_product(c.mode, Ap[:, :idx.shape[1]], np.pad(_f32(o["W"]), ((0, 0), (0, idx.shape[1] - o["W"].shape[1]))))
        v = swoosh_r_f32(v + o["bias"])
        if c.c16:
            v = rne_bf16(v).reshape(v.shape)
        stored = M - 1 if defect == "last_row_unwritten" else M + 1 if defect == "clamped_row_stored" else M
        C[c_off:c_off + stored * g["n"]] = v[:stored].ravel()
    guards_ok = bool(np.all(img[:row_out] == np.float32(fill_of(c.c16))) and
                     np.all(img[row_out + total:] == np.float32(fill_of(c.c16))))
    return img[row_out:row_out + total].reshape(-1, g["fout"], g["n"]).copy(), guards_ok


def emulate_aload(c, o, defect=None):
    """C's image [M][ldc] after gemm_f32 behind the case's loader (gemm_dev.h load_a4's
    ALOAD_BNRELU / ALOAD_IM2COL1D branches; gemm_f32_kernel's epilogue), and whether the guard
    rows around it are intact."""
    A = _f32(o["A"]).ravel()
    Kp = -(-c.K // 16) * 16
    gm, gk = np.arange(c.M)[:, None], np.arange(Kp)[None, :]
    ok = (gm < c.M) & (gk < c.K)
    m = np.where(gm < c.M, gm, c.M - 1)
    k = np.where(gk < c.K, gk, c.K - 4) // 4 * 4
    lane = gk % 4
    if c.kind == "bn":
        v = A[m * c.lda + k + lane]
        ks = np.minimum(k + lane + (1 if defect == "scale_off_by_one" else 0), c.K - 1)
        s, b = o["scale"][ks], o["shift"][np.minimum(k + lane, c.K - 1)]
        if defect == "shift_dropped":
            b = np.zeros_like(b)
        v = (v.astype(np.float64) * s + b).astype(np.float32)  # one rounding: the fma
        Ap = np.where(ok, v if defect == "relu_dropped" else np.maximum(v, np.float32(0)), np.float32(0))
    else:
        Tin, Tout, Cc, stride, dil, pad = c.i2c
        per = Tin if defect == "tin_for_tout" else Tout
        n = m // per
        t = m - n * per
        q = k // Cc
        ch = k - q * Cc
        ts = t * stride + q * (1 if defect == "dilation_ignored" else dil) - pad
        inside = (ts >= 0) & (ts < Tin)
        row = np.clip(ts, 0, Tin - 1) if defect == "padding_clamped" else np.where(inside, ts, 0)
        if defect == "padding_clamped":
            inside = np.ones_like(inside)
        v = A[np.minimum((n * Tin + row) * c.lda + ch + lane, A.size - 1)]
        Ap = np.where(ok & inside, v, np.float32(0))
    acc = _f32(Ap) @ np.pad(_f32(o["W"]), ((0, 0), (0, Kp - c.K))).T + o["bias"]
    if c.epi == "RELU":
        acc = np.maximum(acc, np.float32(0))
    elif c.epi == "MULAUX":
        lx = c.N if defect == "ldaux_is_n" else c.ldaux
        rr, cc = np.arange(c.M)[:, None], np.arange(c.N)[None, :]
        acc = acc * o["aux"].ravel()[rr * lx + cc]
    ldc = c.N if defect == "ldc_is_n" else c.ldc
    img = np.concatenate([np.full(c.ldc, FILL, np.float32), _f32(o["C0"]).ravel(), np.full(c.ldc, FILL, np.float32)])
    rr, cc = np.arange(c.M)[:, None], np.arange(c.N)[None, :]
    img[c.ldc + c.c_col + rr * ldc + cc] = acc.astype(np.float32)
    guards_ok = bool(np.all(img[:c.ldc] == np.float32(FILL)) and np.all(img[-c.ldc:] == np.float32(FILL)))
    return img[c.ldc:-c.ldc].reshape(c.M, c.ldc).copy(), guards_ok


CONV_DEFECTS = ("c4_tstride1", "c4_fstride1", "kt_kf_swapped", "c7_fstride1", "a_off_row",
                "prev_sequence", "last_row_unwritten", "clamped_row_stored")
ALOAD_DEFECTS = ("padding_clamped", "dilation_ignored", "tin_for_tout", "shift_dropped",
                 "relu_dropped", "scale_off_by_one", "ldaux_is_n", "ldc_is_n")
