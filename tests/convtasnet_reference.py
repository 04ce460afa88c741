"""Float64 restatement of the Conv-TasNet separation network (zasr/convtasnet.py)
in plain torch ops: unfold + matmul for the filter banks and the 1x1 convolutions, explicit
sums for the global layer norm, explicit shifted adds for the dilated depthwise convolution and
for the decoder's overlap-add.  No F.conv1d and no conv_transpose1d here; forward_modules is
the same network through torch's own modules, which tests/test_convtasnet_reference.py holds
this restatement to and evaluates in float32 to set the device tolerance."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from zasr.convtasnet import ConvTasNetConfig

EPS = 1e-8


def _t(w: Dict[str, np.ndarray], name: str, dtype=torch.float64) -> torch.Tensor:
    return torch.from_numpy(np.asarray(w[name])).to(dtype)


def _gln(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """x [C, F]: one mean and one biased variance over all C x F values."""
    n = x.shape[0] * x.shape[1]
    mean = x.sum() / n
    var = ((x - mean) ** 2).sum() / n
    return gamma.reshape(-1, 1) * ((x - mean) / torch.sqrt(var + EPS)) + beta.reshape(-1, 1)


def _prelu(x: torch.Tensor, slope: torch.Tensor) -> torch.Tensor:
    return torch.where(x > 0, x, slope.reshape(()) * x)


def _dwconv(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, d: int) -> torch.Tensor:
    """x [C, F], w [C, 1, 3]: out[t] = w0 x[t - d] + w1 x[t] + w2 x[t + d] + b, zeros outside."""
    C, F = x.shape
    out = w[:, 0, 1:2] * x + b.reshape(-1, 1)
    if d < F:
        out[:, d:] += w[:, 0, 0:1] * x[:, :F - d]
        out[:, :F - d] += w[:, 0, 2:3] * x[:, d:]
    return out


def forward(cfg: ConvTasNetConfig, w: Dict[str, np.ndarray], mixture: np.ndarray,
            return_masks: bool = False):
    """mixture [T] -> sources [2, T] (float64 numpy), the raw network output."""
    x = torch.from_numpy(np.asarray(mixture, np.float64))
    T = x.shape[0]
    K, S = cfg.kernel_size, cfg.stride
    frames = x.unfold(0, K, S)                                         # [F, K]
    F = frames.shape[0]
    tf = _t(w, "encoder.filterbank._filters")[:, 0, :] @ frames.T      # [N, F]
    o = _t(w, "masker.bottleneck.1.weight")[:, :, 0] @ _gln(
        tf, _t(w, "masker.bottleneck.0.gamma"), _t(w, "masker.bottleneck.0.beta")) \
        + _t(w, "masker.bottleneck.1.bias").reshape(-1, 1)
    skip = torch.zeros((cfg.skip_chan, F), dtype=torch.float64)
    for i in range(cfg.n_blocks * cfg.n_repeats):
        p = f"masker.TCN.{i}."
        d = 2 ** (i % cfg.n_blocks)
        y = _t(w, p + "shared_block.0.weight")[:, :, 0] @ o + _t(w, p + "shared_block.0.bias").reshape(-1, 1)
        y = _gln(_prelu(y, _t(w, p + "shared_block.1.weight")),
                 _t(w, p + "shared_block.2.gamma"), _t(w, p + "shared_block.2.beta"))
        y = _dwconv(y, _t(w, p + "shared_block.3.weight"), _t(w, p + "shared_block.3.bias"), d)
        y = _gln(_prelu(y, _t(w, p + "shared_block.4.weight")),
                 _t(w, p + "shared_block.5.gamma"), _t(w, p + "shared_block.5.beta"))
        o = o + _t(w, p + "res_conv.weight")[:, :, 0] @ y + _t(w, p + "res_conv.bias").reshape(-1, 1)
        skip = skip + _t(w, p + "skip_conv.weight")[:, :, 0] @ y + _t(w, p + "skip_conv.bias").reshape(-1, 1)
    m = _t(w, "masker.mask_net.1.weight")[:, :, 0] @ _prelu(skip, _t(w, "masker.mask_net.0.weight")) \
        + _t(w, "masker.mask_net.1.bias").reshape(-1, 1)
    mask = torch.clamp(m, min=0.0).reshape(cfg.n_src, cfg.n_filters, F)
    masked = mask * tf.unsqueeze(0)
    dec = _t(w, "decoder.filterbank._filters")[:, 0, :]                # [N, K]
    out = torch.zeros((cfg.n_src, T), dtype=torch.float64)
    for s in range(cfg.n_src):
        rows = masked[s].T @ dec                                       # [F, K]
        for f in range(F):
            out[s, f * S:f * S + K] += rows[f]
    if return_masks:
        return out.numpy(), mask.numpy()
    return out.numpy()


def forward_modules(cfg: ConvTasNetConfig, w: Dict[str, np.ndarray], mixture: np.ndarray,
                    dtype=torch.float64) -> np.ndarray:
    """The same network through F.conv1d / F.prelu / F.conv_transpose1d in `dtype`."""
    import torch.nn.functional as Fn

    def t(name):
        return _t(w, name, dtype)

    def gln(x, gamma, beta):
        mean = x.mean(dim=(1, 2), keepdim=True)
        var = ((x - mean) ** 2).mean(dim=(1, 2), keepdim=True)
        return gamma * ((x - mean) / (var + EPS).sqrt()) + beta

    x = torch.from_numpy(np.array(mixture)).to(dtype).reshape(1, 1, -1)
    T = x.shape[-1]
    with torch.no_grad():
        tf = Fn.conv1d(x, t("encoder.filterbank._filters"), stride=cfg.stride)
        o = Fn.conv1d(gln(tf, t("masker.bottleneck.0.gamma"), t("masker.bottleneck.0.beta")),
                      t("masker.bottleneck.1.weight"), t("masker.bottleneck.1.bias"))
        skip = 0.0
        for i in range(cfg.n_blocks * cfg.n_repeats):
            p = f"masker.TCN.{i}."
            d = 2 ** (i % cfg.n_blocks)
            y = Fn.conv1d(o, t(p + "shared_block.0.weight"), t(p + "shared_block.0.bias"))
            y = gln(Fn.prelu(y, t(p + "shared_block.1.weight")), t(p + "shared_block.2.gamma"),
                    t(p + "shared_block.2.beta"))
            y = Fn.conv1d(y, t(p + "shared_block.3.weight"), t(p + "shared_block.3.bias"),
                          padding=d, dilation=d, groups=cfg.hid_chan)
            y = gln(Fn.prelu(y, t(p + "shared_block.4.weight")), t(p + "shared_block.5.gamma"),
                    t(p + "shared_block.5.beta"))
            o = o + Fn.conv1d(y, t(p + "res_conv.weight"), t(p + "res_conv.bias"))
            skip = skip + Fn.conv1d(y, t(p + "skip_conv.weight"), t(p + "skip_conv.bias"))
        m = Fn.conv1d(Fn.prelu(skip, t("masker.mask_net.0.weight")), t("masker.mask_net.1.weight"),
                      t("masker.mask_net.1.bias"))
        mask = torch.relu(m).reshape(1, cfg.n_src, cfg.n_filters, -1)
        masked = mask * tf.unsqueeze(1)
        dec = Fn.conv_transpose1d(masked.reshape(cfg.n_src, cfg.n_filters, -1),
                                  t("decoder.filterbank._filters"), stride=cfg.stride)[:, 0, :]
        out = torch.zeros((cfg.n_src, T), dtype=dtype)
        out[:, :dec.shape[-1]] = dec
    return out.numpy()
