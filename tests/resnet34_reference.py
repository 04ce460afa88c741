"""Float64 restatements of the community-1 embedding stage, the torch module of the
same network, and the cases, operands and bounds the CPU and GPU tests share.

  fbank(audio, tail)            compute_emb_fbank's option set (core/speaker_diarization_pure_ort.py
                                :271-301) before its CMVN: x 32768, snip_edges, DC removal, knf's
                                in-frame pre-emphasis, Hamming, |rfft 512|^2, the 20 Hz .. Nyquist
                                bank of oracle.campplus.kaldi_mel_bank, floor FLT_EPSILON; `tail`
                                zeros appended (:812)
  chunk_feats(image, start)     rows [start // 160, + 998), zeros past the image, CMVN over all 998
  conv2d_cl / forward           the folded network on channels-last float64 arrays (im2col GEMM)
  torch_forward                 the same network through F.conv2d (float32 or float64, folded), and
                                torch_forward_unfolded with batch_norm in eval on the raw weights
  masked_pool / pop_pool        PureOrtDiarizer._masked_stats_pool and the unmasked pooling of
                                compute_single_embedding, in a chosen dtype
  chunk_embeddings / segment_embedding   the stage end to end from fbank rows

Defects (`defect=`) are single deliberate errors for tests/test_resnet34_reference.py's sweep.

Bounds.  Kernel cases: per element ((K + 4) u) sum|w||x| + 2 u |y|, u = 2^-24 (the MFMA is an
fmaf chain, so this is a priori; C_DOT of tests/aux_reference.py).  Pooling: 8 x the float32
restatement's deviation from the float64 one, floor 16 u.  Whole model: torch float32 on the CPU
deviates from the float64 restatement, relative to the float64 peak, by

  frame features, full depth, n = 2:   T = 40: 4.83e-7    T = 41: 3.40e-7
  embeddings, 12.3 s signal, 4 chunks of 998 frames (float32 network, pooling and projection
  on the float64 rows rounded to float32):  5.79e-7

  single segments (fbank rows -> float32 CMVN, network, pooling, projection, as the reference's
  compute_emb_fbank + compute_single_embedding are float32 throughout):  9 frames: 7.80e-7    250 frames: 5.41e-7

(tests/test_resnet34_reference.py re-measures these).  The device is allowed 8 x the named
constants F32_DEV[T], F32_DEV_EMB and F32_DEV_SEG[frames] below, each case its own.

The end-to-end GPU check also runs against the restatement driven by the float64 fbank.  There
the device's fbank error, which its own test allows up to FBANK_ATOL = 2e-3, is an input
perturbation, so the bound adds FBANK_PROP: the float64 restatement's deviation when its fbank
image is perturbed element-wise by a seeded uniform draw from [-2e-3, 2e-3]: 8.33e-5 of the peak.
"""
from __future__ import annotations

import functools
import math
import zlib
from collections import namedtuple

import numpy as np

from zasr import resnet34 as R

f64 = np.float64
U = 2.0 ** -24
C_DOT = 4
SENT = np.float32(-777.25)
FLT_EPSILON = 1.1920928955078125e-07
FBANK_ATOL = 2e-3            # the main fbank kernel's bound (tests/test_gpu_parity.py)
F32_DEV = {40: 4.83e-7, 41: 3.40e-7}     # measured per T: torch float32 vs float64 frame features
F32_DEV_EMB = 5.79e-7        # measured: float32 vs float64 embeddings of the 12.3 s signal's chunks
F32_DEV_SEG = {9: 7.80e-7, 250: 5.41e-7}         # measured per length: the single-segment path
BOUND = {T: 8 * d for T, d in F32_DEV.items()}
BOUND_EMB = 8 * F32_DEV_EMB
BOUND_SEG = {n: 8 * d for n, d in F32_DEV_SEG.items()}
# what an fbank inside FBANK_ATOL can move the 12.3 s signal's embeddings by: the float64
# restatement's own deviation, relative to its peak, when every element of its fbank image is
# moved by a seeded uniform draw from [-FBANK_ATOL, FBANK_ATOL] (measured; docstring)
FBANK_PROP = 8.33e-5
BOUND_EMB_FULL = BOUND_EMB + FBANK_PROP
NSEG = 589
MIN_SEG_FRAMES = math.ceil(NSEG * 1680 / 160000)     # 7
CHUNK_FRAMES = 998
TAIL = 160000


def _rng(tag, c=()):
    return np.random.default_rng(zlib.crc32((tag + repr(tuple(c))).encode()))


# ---------------------------------------------------------------------------------------------
# fbank and chunk windows
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tables(povey: bool):
    from oracle.campplus import kaldi_mel_bank
    i = np.arange(400)
    if povey:
        win = np.power(0.5 - 0.5 * np.cos(2.0 * np.pi * i / 399), 0.85)
    else:
        win = 0.54 - 0.46 * np.cos(2.0 * np.pi * i / 399)
    return win.astype(np.float32).astype(f64), kaldi_mel_bank().astype(f64)


def fbank_rows(n: int, tail: int = 0) -> int:
    return 1 + (n + tail - 400) // 160 if n + tail >= 400 else 0


def fbank(audio, tail: int = 0, defect: str = "") -> np.ndarray:
    """[rows, 80] float64, no CMVN."""
    win, mel = _tables(defect == "povey_window")
    x = (np.asarray(audio, np.float32) * np.float32(32768.0)).astype(f64)
    if defect != "zero_tail_omitted":
        x = np.concatenate([x, np.zeros(tail)])
    nf = fbank_rows(x.shape[0])
    if nf <= 0:
        return np.empty((0, 80))
    fr = x[160 * np.arange(nf)[:, None] + np.arange(400)[None, :]]
    fr = fr - fr.mean(axis=1, keepdims=True)
    pre = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)     # w[0] -= 0.97 w[0]
    fr = (fr - 0.97 * pre) * win
    pad = np.zeros((nf, 512))
    pad[:, :400] = fr
    spec = np.fft.rfft(pad)
    power = spec.real ** 2 + spec.imag ** 2
    return np.log(np.maximum(power @ mel.T, FLT_EPSILON))


def chunk_feats(image: np.ndarray, start: int, defect: str = "", signal_rows: int = 0) -> np.ndarray:
    """[998, 80]: the chunk's window of the fbank image with CMVN over all 998 rows (:831-839).
    signal_rows: the frames that lie wholly inside the signal (the defect's "valid" rows; the
    rows behind them come from the appended zeros)."""
    r0 = start // 160
    r1 = min(r0 + CHUNK_FRAMES, image.shape[0])
    out = np.zeros((CHUNK_FRAMES, 80), image.dtype)
    n = max(r1 - r0, 0)
    if n > 0:
        out[:n] = image[r0:r1]
    if defect == "cmvn_valid_rows_only":
        v = max(min(n, signal_rows - r0), 1)
        out -= out[:v].mean(axis=0, keepdims=True)
    else:
        out -= out.mean(axis=0, keepdims=True)
    return out


# ---------------------------------------------------------------------------------------------
# the network
# ---------------------------------------------------------------------------------------------
def tap_major(w):
    """torch [co][ci][r][q] -> the kernels' [co][r][q][ci]."""
    return np.ascontiguousarray(np.transpose(w, (0, 2, 3, 1)))


def conv2d_cl(x, w, b, ks, stride, res=None, relu=True, defect=""):
    """x [n, F, T, Ci], w [Co, ks, ks, Ci], b [Co] -> (y [n, Fo, To, Co] float64, its bound)."""
    x, w, b = np.asarray(x, f64), np.asarray(w, f64), np.asarray(b, f64)
    n, F, T, Ci = x.shape
    Co = w.shape[0]
    pad = 1 if ks == 3 else 0
    Fo, To = (F - 1) // stride + 1, (T - 1) // stride + 1
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    if pad and defect == "pad_missing_edge":          # the low-T edge reads the row's first frame
        xp[:, :, 0] = xp[:, :, 1]
    if pad and defect == "neighbour_across_sample":   # F padding reads the next / previous sample
        xp[1:, 0, pad:-pad] = x[:-1, F - 1]
        xp[:-1, F + 1, pad:-pad] = x[1:, 0]
    st = 1 if defect == "stride_one_axis" else stride
    if defect == "rq_swapped":
        w = np.transpose(w, (0, 2, 1, 3))
    cols = [xp[:, r:r + (Fo - 1) * stride + 1:stride, q:q + (To - 1) * st + 1:st]
            for r in range(ks) for q in range(ks)]
    a = np.concatenate(cols, axis=-1)
    wm = w.reshape(Co, -1)
    acc = a @ wm.T
    S = np.abs(a) @ np.abs(wm).T
    y = acc + b
    if res is not None:
        res = np.asarray(res, f64)
        if defect == "res_after_relu":
            y = np.maximum(y, 0.0) + res
        elif defect == "bias_dropped_with_res":
            y = acc + res
        else:
            y = y + res
    bound = (wm.shape[1] + C_DOT) * U * S + 2 * U * np.abs(y)
    if relu and defect != "res_after_relu":
        y = np.maximum(y, 0.0)
    return y, bound


def to_cft(y, defect=""):
    """[n, F, T, C] -> [n, C F, T], channel c * F + f (the reference's (B, 2560, F) tensor)."""
    n, F, T, C = y.shape
    if defect == "f_major_channels":
        return np.transpose(y, (0, 1, 3, 2)).reshape(n, F * C, T)
    return np.transpose(y, (0, 3, 1, 2)).reshape(n, C * F, T)


def forward(cfg, folded, x, defect=""):
    """x [n, T, 80] -> frame features [n, 2560, T'] in float64 on the folded float32 tensors."""
    x = np.asarray(x, f64)
    h = np.transpose(x, (0, 2, 1))[..., None]
    w, b = folded["resnet.conv1"]
    h, _ = conv2d_cl(h, tap_major(w), b, 3, 1, None, True, defect)
    for p, _cin, _c, stride, sc in R.block_plan(cfg):
        w1, b1 = folded[p + "conv1"]
        w2, b2 = folded[p + "conv2"]
        mid, _ = conv2d_cl(h, tap_major(w1), b1, 3, stride, None, True, defect)
        if sc:
            ws, bs = folded[p + "shortcut"]
            short, _ = conv2d_cl(h, tap_major(ws), bs, 1, stride, None, False, defect)
        else:
            short = h
        h, _ = conv2d_cl(mid, tap_major(w2), b2, 3, 1, short, True, defect)
    return to_cft(h, defect)


def torch_forward(cfg, folded, x, dtype=np.float32):
    """The same network through F.conv2d on the folded tensors; x [n, T, 80] -> [n, 2560, T']."""
    import torch
    import torch.nn.functional as F
    td = torch.float32 if dtype == np.float32 else torch.float64
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(td)  # noqa: E731

    def conv(h, name, stride, pad):
        w, b = folded[name]
        return F.conv2d(h, t(w), t(b), stride=stride, padding=pad)
    with torch.no_grad():
        h = t(np.asarray(x, dtype)).permute(0, 2, 1).unsqueeze(1)
        h = F.relu(conv(h, "resnet.conv1", 1, 1))
        for p, _cin, _c, stride, sc in R.block_plan(cfg):
            mid = F.relu(conv(h, p + "conv1", stride, 1))
            y = conv(mid, p + "conv2", 1, 1)
            short = conv(h, p + "shortcut", stride, 0) if sc else h
            h = F.relu(y + short)
        return h.reshape(h.shape[0], -1, h.shape[3]).numpy()


def torch_forward_unfolded(cfg, weights, x):
    """float64, the raw weights, F.conv2d + F.batch_norm in eval: what the fold must equal."""
    import torch
    import torch.nn.functional as F
    W = {k: torch.from_numpy(np.asarray(v, f64)) for k, v in weights.items()}

    def cbn(h, conv, bn, stride, pad):
        h = F.conv2d(h, W[conv + ".weight"], None, stride=stride, padding=pad)
        return F.batch_norm(h, W[bn + ".running_mean"], W[bn + ".running_var"], W[bn + ".weight"],
                            W[bn + ".bias"], False, 0.0, cfg.bn_eps)
    with torch.no_grad():
        h = torch.from_numpy(np.asarray(x, f64)).permute(0, 2, 1).unsqueeze(1)
        h = F.relu(cbn(h, "resnet.conv1", "resnet.bn1", 1, 1))
        for p, _cin, _c, stride, sc in R.block_plan(cfg):
            mid = F.relu(cbn(h, p + "conv1", p + "bn1", stride, 1))
            y = cbn(mid, p + "conv2", p + "bn2", 1, 1)
            short = cbn(h, p + "shortcut.0", p + "shortcut.1", stride, 0) if sc else h
            h = F.relu(y + short)
        return h.reshape(h.shape[0], -1, h.shape[3]).numpy()


# ---------------------------------------------------------------------------------------------
# pooling and the stage end to end
# ---------------------------------------------------------------------------------------------
def feat_idx(n_feat_frames, num_seg_frames, defect=""):
    q = np.arange(n_feat_frames) * num_seg_frames / n_feat_frames
    idx = (np.round(q) if defect == "feat_idx_round" else np.floor(q)).astype(int)
    return np.clip(idx, 0, num_seg_frames - 1)


def used_mask(full, clean, min_seg_frames, defect=""):
    if defect == "clean_rule_ge":
        return clean if clean.sum() >= min_seg_frames else full
    return clean if clean.sum() > min_seg_frames else full


def masked_pool(frame_feat, weights, dtype=f64, defect=""):
    """_masked_stats_pool (:756-767) on features of `dtype`.  The weights are float32 there, so
    v1, v2 and the denominator are float32 scalars under numpy 2 (1 + 1e-8 == 1) in either
    dtype; the sums over frames are `dtype`."""
    x = np.asarray(frame_feat, dtype)
    w32 = np.asarray(weights, np.float32)
    eps = np.float32(1e-8)
    v1 = np.float32(w32.sum()) + eps
    v2 = np.float32((w32 * w32).sum())
    den = v1 if defect == "population_variance" else (v1 - v2 / v1 + eps)
    w = w32.astype(dtype)[np.newaxis, :]
    mean = (x * w).sum(axis=1) / dtype(v1)
    dx2 = (x - mean[:, np.newaxis]) ** 2
    var = (dx2 * w).sum(axis=1) / dtype(den)
    return np.concatenate([mean, np.sqrt(var)])


def pop_pool(frame_feat, dtype=f64):
    """compute_single_embedding's pooling (:701-706)."""
    x = np.asarray(frame_feat, dtype)
    mean = x.mean(axis=1)
    var = ((x - mean[:, np.newaxis]) ** 2).mean(axis=1)
    return np.concatenate([mean, np.sqrt(var)])


def pool_bound(frame_feat, weights):
    """(float64 reference, scalar bound, the float32 deviation): the lstm_bound form."""
    x32 = np.asarray(frame_feat, np.float32)
    if weights is None:
        r64, r32 = pop_pool(x32, f64), pop_pool(x32, np.float32)
    else:
        r64, r32 = masked_pool(x32, weights, f64), masked_pool(x32, weights, np.float32)
    dev = float(np.max(np.abs(r32.astype(f64) - r64)))
    return r64, max(8.0 * dev, 16.0 * U), dev


def network(seed: int = 17):
    cfg = R.ResNet34Config()
    w = R.synth_weights(cfg, seed)
    return cfg, w, R.folded_weights(cfg, w)


def encode64(cfg, folded, feats, impl="numpy"):
    if impl == "torch":
        return torch_forward(cfg, folded, np.asarray(feats, f64), f64)
    return forward(cfg, folded, feats)


def chunk_embeddings(cfg, weights, folded, image, starts, binarized, clean, min_seg_frames=MIN_SEG_FRAMES,
                     dtype=f64, defect="", signal_rows=0):
    """[chunks, 3, 256] from the fbank image [rows, 80] (:820-872).  dtype float32: the float32
    class (torch float32 network, numpy float32 pooling and projection)."""
    feats = np.stack([chunk_feats(np.asarray(image, f64), int(s), defect, signal_rows) for s in starts])
    if dtype == np.float32:
        ff = torch_forward(cfg, folded, feats.astype(np.float32), np.float32)
    else:
        ff = torch_forward(cfg, folded, feats.astype(np.float32).astype(f64), f64)
    W = weights["resnet.seg_1.weight"].astype(dtype)
    b = weights["resnet.seg_1.bias"].astype(dtype)
    nseg = binarized.shape[1]
    idx = feat_idx(ff.shape[2], nseg, defect)
    out = np.empty((len(starts), binarized.shape[2], W.shape[0]), dtype)
    for c in range(len(starts)):
        for s in range(binarized.shape[2]):
            um = used_mask(binarized[c, :, s], clean[c, :, s], min_seg_frames, defect)
            stats = masked_pool(ff[c], um[idx].astype(np.float32), dtype, defect)
            out[c, s] = stats @ W.T + b
    return out


def segment_embedding(cfg, weights, folded, rows, dtype=f64):
    """compute_single_embedding from the segment's fbank rows [T, 80] (before CMVN).  float64: the
    CMVN in float64, then the float32 features the network is given; float32: the CMVN in
    float32 as compute_emb_fbank does it (:303), the float32 class throughout."""
    if dtype == np.float32:
        feats = np.asarray(rows, np.float32)
        feats = feats - feats.mean(axis=0, keepdims=True)
    else:
        feats = np.asarray(rows, f64)
        feats = (feats - feats.mean(axis=0, keepdims=True)).astype(np.float32)
    ff = torch_forward(cfg, folded, feats[None].astype(dtype), dtype)[0]
    stats = pop_pool(ff, dtype)
    return stats @ weights["resnet.seg_1.weight"].astype(dtype).T + weights["resnet.seg_1.bias"].astype(dtype)


def segment_audio(frames: int) -> np.ndarray:
    return speech(3.0, 33)[1000:1000 + 400 + 160 * (frames - 1)]


def perturbed_image(image: np.ndarray) -> np.ndarray:
    """The fbank image moved element-wise by a seeded uniform draw from [-FBANK_ATOL, FBANK_ATOL]."""
    return image + _rng("fbank_prop").uniform(-FBANK_ATOL, FBANK_ATOL, image.shape)


def peak_dev(got, ref):
    ref = np.asarray(ref, f64)
    return float(np.max(np.abs(np.asarray(got, f64) - ref)) / np.max(np.abs(ref)))


def acceptance(got, ref32):
    """(max_abs, rel_l2) of the reference's rule for this stage (core/calibration.py:84, :1279-1286:
    accepted when max_abs <= 2e-3 or rel_l2 <= 2e-4)."""
    d = np.asarray(got, f64) - np.asarray(ref32, f64)
    return float(np.max(np.abs(d))), float(np.linalg.norm(d) / max(np.linalg.norm(np.asarray(ref32, f64)), 1e-30))


# ---------------------------------------------------------------------------------------------
# shared inputs
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def speech(sec: float, seed: int) -> np.ndarray:
    from zasr.synth_audio import synth_speech
    return synth_speech(sec, seed)


@functools.lru_cache(maxsize=None)
def model_feats(T: int) -> np.ndarray:
    """[2, T, 80] float32: CMVN'd fbank windows of synthetic speech, the whole-model inputs."""
    img = fbank(speech(2.0, 40 + T))
    out = np.stack([img[5:5 + T], img[60:60 + T]])
    return (out - out.mean(axis=1, keepdims=True)).astype(np.float32)


MODEL_T = (40, 41)
E2E_SEC, E2E_SEED = 12.3, 91
E2E_STARTS = (0, 16000, 32000, 48000)     # the 1 s step; 12.3 s: the last chunk past the signal


def e2e_masks():
    """(binarized, clean) [4, 589, 3] float32: speaker 0 speaks in blocks with a clean subset,
    speaker 1 switches between clean and full at exactly MIN_SEG_FRAMES, speaker 2 of chunk 1 is
    all zero."""
    rng = _rng("e2e_masks")
    full = (rng.random((4, NSEG, 3)) < 0.5).astype(np.float32)
    for c in range(4):
        full[c, :, 0] = 0.0
        full[c, 40 * c:40 * c + 300, 0] = 1.0
    clean = full * (rng.random((4, NSEG, 3)) < 0.6)
    for c in range(4):      # speaker 1: the clean mask has MIN_SEG_FRAMES + (c % 2) active frames
        clean[c, :, 1] = 0.0
        on = np.flatnonzero(full[c, :, 1])[:MIN_SEG_FRAMES + (c % 2)]
        clean[c, on, 1] = 1.0
    full[1, :, 2] = 0.0
    clean[1, :, 2] = 0.0
    return full.astype(np.float32), clean.astype(np.float32)


# kernel cases of tests/test_gpu_emb_kernels.py: (name, ci, co, ks, stride, F, T, n, res, relu)
ConvCase = namedtuple("ConvCase", "name ci co ks stride F T n res relu")
CONV_CASES = [
    ConvCase("A", 32, 32, 3, 1, 5, 7, 2, False, True),
    ConvCase("B", 32, 64, 3, 2, 5, 7, 2, False, False),
    ConvCase("C", 32, 64, 1, 2, 5, 7, 2, False, False),
    ConvCase("D", 64, 64, 3, 1, 3, 70, 3, True, True),
    ConvCase("E", 128, 256, 3, 2, 4, 9, 1, False, False),
    ConvCase("F", 1, 32, 3, 1, 80, 9, 2, False, True),
]


def conv_operands(c: ConvCase):
    """x (channels-last; the stem's [n][T][80]), w [co][ks][ks][ci], bias, res or None."""
    rng = _rng("emb_conv", c)
    fo, to = (c.F - 1) // c.stride + 1, (c.T - 1) // c.stride + 1
    if c.ci == 1:
        x = rng.normal(0.0, 2.0, (c.n, c.T, c.F))
    else:
        x = np.maximum(rng.normal(0.2, 1.0, (c.n, c.F, c.T, c.ci)), 0.0)     # a ReLU stream
    w = rng.normal(0.0, math.sqrt(2.0 / (c.ci * c.ks * c.ks)), (c.co, c.ks, c.ks, c.ci))
    b = rng.uniform(-0.2, 0.2, c.co)
    res = np.maximum(rng.normal(0.0, 1.0, (c.n, fo, to, c.co)), 0.0) if c.res else None
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)  # noqa: E731
    return f(x), f(w), f(b), f(res)


def conv_case_ref(c: ConvCase, defect=""):
    x, w, b, res = conv_operands(c)
    xin = np.transpose(x, (0, 2, 1))[..., None] if c.ci == 1 else x
    return conv2d_cl(xin, w, b, c.ks, c.stride, res, c.relu, defect)


POOL_MASKS = ("all_zero", "one_frame", "two_frames", "all_ones", "alternating", "clean_switch")


def pool_masks(nseg=NSEG):
    """{name: (full, clean)} float32 [nseg]: the golden's six masks."""
    z, o = np.zeros(nseg, np.float32), np.ones(nseg, np.float32)
    one, two, alt = z.copy(), z.copy(), z.copy()
    # frames feat_idx(125, 589) samples (floor(43 * 4.712) = 202, floor(89 * 4.712) = 419), so the
    # weights have exactly one and two active frames
    one[202] = 1.0
    two[[202, 419]] = 1.0
    alt[::2] = 1.0
    sw = z.copy()
    sw[100:100 + MIN_SEG_FRAMES] = 1.0          # exactly min_seg_frames: the full mask is used
    return {"all_zero": (z, z), "one_frame": (one, one), "two_frames": (two, two),
            "all_ones": (o, o), "alternating": (alt, alt), "clean_switch": (alt, sw)}


def pool_block(rows: int, T: int = 125):
    return _rng("emb_pool", (rows, T)).normal(0.3, 1.0, (rows, T)).astype(np.float32)
