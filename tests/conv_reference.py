"""float64 references of the encoder's convolution path and BiasNorm (test infrastructure).

Every ragged operator is evaluated sequence by sequence on that sequence's own rows, padded
with explicit zeros, so the zero padding at sequence edges holds by construction and not by a
mask.  tests/test_conv_reference.py holds these functions to torch's conv1d / conv2d and the
oracle's activations; tests/test_gpu_conv_kernels.py holds the HIP kernels to them.

Layouts are the kernels': packed rows, sequence after sequence, channels last.

Also here: the kernels' tile constants and the block-level facts that follow from a list of
sequence lengths (which tiles take the masked path), so the tests can state which code paths
their fixtures meet.
"""
import numpy as np

# ---- tile constants of the kernels (csrc/encoder_kernels.hip, csrc/convnext_kernels.hip) ----
DW1_TILE_ROWS = 64        # kDw1T: packed rows per glu_dwconv1d_kernel block
DW1_TILE_CH = 64          # channels per block
DW1_COMPILED_K = (7, 15, 31)
CNX_TILE_ROWS = 16        # kDwT: frames per convnext_dw_kernel block
CNX_HALF = 3
MLP_TILE_POS = 128        # kMlpM: (frame, freq) positions per convnext_mlp*_kernel block
CONV1_BLOCK = 256         # conv1_kernel: one thread per (row, freq)
BIAS_NORM_ROWS = 4        # bias_norm_kernel: one wave per row, four per block


# ---- the ragged fixtures both test modules use ----
DW1_LENGTHS = ([1, 7, 56, 3, 200, 64, 31, 130], [1], [5])
DW1_WIDTHS = (36, 64, 96)
DW1_KERNEL_SIZES = (5, 7, 9, 15, 17, 31)
CONV1_FRAMES = [3, 4, 10, 35, 9]
CNX_LENGTHS = ([1, 2, 16, 3, 40, 7, 33], [1])
BN_WIDTHS = (4, 64, 192, 256, 260, 384, 512, 516, 1024)
BN_ROWS = (1, 3, 4, 5, 9)


def compiled_k(kr):
    """The instantiation launch_glu_dwconv1d_t picks for kernel size kr."""
    return next(k for k in DW1_COMPILED_K if kr <= k)


def bias_norm_nq(d):
    """float4 loads per lane of the bias_norm_kernel instantiation for width d."""
    return 1 if d <= 256 else 2 if d <= 512 else 4


def offsets(L):
    return np.concatenate([[0], np.cumsum(np.asarray(L, dtype=np.int64))])


def masked_tiles(L, tile, half):
    """Per tile of `tile` packed rows: True where the depthwise kernels take the per-row masked
    path -- some row of the tile has a window [r - half, r + half] that leaves its own sequence
    (rows past the last one count as interior, as in the kernels)."""
    off = offsets(L)
    rows = int(off[-1])
    lo = np.repeat(off[:-1], L)
    hi = np.repeat(off[1:], L)
    r = np.arange(rows)
    cut = (r - half < lo) | (r + half > hi - 1)
    ntile = (rows + tile - 1) // tile
    return np.array([bool(cut[t * tile:(t + 1) * tile].any()) for t in range(ntile)])


# ---- activations ----
def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def swoosh_r(v):
    return np.logaddexp(0.0, v - 1.0) - 0.08 * v - 0.313261687


def swoosh_l(v):
    return np.logaddexp(0.0, v - 4.0) - 0.08 * v - 0.035


def glu(x2):
    """[rows][2 d] -> [rows][d]: first half times the sigmoid of the second."""
    x2 = np.asarray(x2, dtype=np.float64)
    d = x2.shape[1] // 2
    return x2[:, :d] * sigmoid(x2[:, d:])


# ---- depthwise conv over time (ConvolutionModule) ----
def dwconv1d(g, L, w, b):
    """g [sum L][d], w [d][K] (K odd), b [d] -> b[c] + sum_k w[c][k] g[t + k - K // 2][c] with
    zeros outside each sequence; [sum L][d] (the pre-activation)."""
    g, w, b = (np.asarray(v, dtype=np.float64) for v in (g, w, b))
    K = w.shape[1]
    half = K // 2
    off = offsets(L)
    out = np.empty_like(g)
    for s in range(len(L)):
        n = int(L[s])
        pad = np.zeros((n + 2 * half, g.shape[1]))
        pad[half:half + n] = g[off[s]:off[s + 1]]
        acc = np.tile(b, (n, 1))
        for k in range(K):
            acc += w[:, k] * pad[k:k + n]
        out[off[s]:off[s + 1]] = acc
    return out


def conv_module_core(x, L, w, b, with_glu):
    """GLU (optional) -> depthwise conv1d -> SwooshR."""
    g = glu(x) if with_glu else np.asarray(x, dtype=np.float64)
    return swoosh_r(dwconv1d(g, L, w, b))


# ---- conv.0 of Conv2dSubsampling: Conv2d(1 -> 8, 3x3, padding (0, 1)) ----
def conv0(fb, T, w, b):
    """fb [sum T][80], w [8][9] (tap kt * 3 + kf), b [8] -> [sum (T - 2)][80][8], the
    pre-activation: no padding in time (each sequence loses two frames), zeros beyond the 80
    mel bins."""
    fb, w, b = (np.asarray(v, dtype=np.float64) for v in (fb, w, b))
    off = offsets(T)
    out = []
    for s in range(len(T)):
        n = int(T[s]) - 2
        pad = np.zeros((int(T[s]), 82))
        pad[:, 1:81] = fb[off[s]:off[s + 1]]
        acc = np.tile(b, (n, 80, 1))
        for kt in range(3):
            for kf in range(3):
                acc += pad[kt:kt + n, kf:kf + 80, None] * w[:, kt * 3 + kf]
        out.append(acc)
    return np.concatenate(out, axis=0)


# ---- ConvNeXt block ----
def dwconv7x7(x, L, w, b):
    """x [sum L][19][128], w [128][7][7] (time tap, freq tap), b [128] -> the depthwise 7x7
    conv over (time, freq) with padding 3, zeros outside each sequence and outside [0, 19)."""
    x, w, b = (np.asarray(v, dtype=np.float64) for v in (x, w, b))
    off = offsets(L)
    out = np.empty_like(x)
    F = x.shape[1]
    for s in range(len(L)):
        n = int(L[s])
        pad = np.zeros((n + 6, F + 6, x.shape[2]))
        pad[3:3 + n, 3:3 + F] = x[off[s]:off[s + 1]]
        acc = np.tile(b, (n, F, 1))
        for kt in range(7):
            for kf in range(7):
                acc += w[:, kt, kf] * pad[kt:kt + n, kf:kf + F]
        out[off[s]:off[s + 1]] = acc
    return out


def convnext_mlp(y, w1, b1, w2, b2, hidden=None):
    """The pointwise MLP per position: pw2(SwooshL(pw1(y) + b1)) + b2, y [...][128] ->
    [...][128] (the residual is the caller's).  hidden: applied to the activated hidden layer
    (a kernel's storage rounding)."""
    y, w1, b1, w2, b2 = (np.asarray(v, dtype=np.float64) for v in (y, w1, b1, w2, b2))
    h = swoosh_l(y @ w1.T + b1)
    if hidden is not None:
        h = hidden(h)
    return h @ w2.T + b2


# ---- BiasNorm (+ the layer's bypass blend) ----
def bias_norm(x, bias, log_scale, orig=None, bscale=None):
    """x exp(log_scale) / sqrt(mean((x - bias)^2)) over channels; with orig and bscale then
    orig + (. - orig) bscale.  Returns (result, the normalised value before the blend)."""
    x, bias = np.asarray(x, dtype=np.float64), np.asarray(bias, dtype=np.float64)
    r = x * np.exp(np.float64(log_scale)) / np.sqrt(np.mean((x - bias) ** 2, axis=-1, keepdims=True))
    if orig is None:
        return r, r
    o, s = np.asarray(orig, dtype=np.float64), np.asarray(bscale, dtype=np.float64)
    return o + (r - o) * s, r
