"""Float64 restatement of the PyanNet segmentation network (zasr/pyannet.py) in plain torch
ops: no nn.InstanceNorm1d, no nn.LSTM, no F.conv1d -- sums, unfolds and matmuls written out, so
it is an independent statement of the network the device kernels are held to
(tests/test_gpu_seg.py).  tests/test_pyannet_reference.py shows it is the same network as the
torch modules compute (forward_modules, below), which is also the float32 evaluation "in
another summation order" that sets the device tolerance.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

EPS = 1e-5
LEAKY = 0.01


def _t(w: Dict[str, np.ndarray], name: str, dtype) -> torch.Tensor:
    return torch.from_numpy(np.asarray(w[name])).to(dtype)


def _leaky(x: torch.Tensor) -> torch.Tensor:
    return torch.where(x > 0, x, LEAKY * x)


def _inorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """x [n, frames, C]: normalise over frames (biased variance), affine per channel."""
    mean = x.sum(1, keepdim=True) / x.shape[1]
    d = x - mean
    var = (d * d).sum(1, keepdim=True) / x.shape[1]
    return d / torch.sqrt(var + EPS) * weight + bias


def _pool3(x: torch.Tensor) -> torch.Tensor:
    n, L, C = x.shape
    F = L // 3
    return x[:, :3 * F].reshape(n, F, 3, C).max(2).values


def _lstm_dir(x, w_ih, w_hh, b_ih, b_hh, reverse: bool) -> torch.Tensor:
    n, F, _ = x.shape
    H = w_hh.shape[1]
    gx = x @ w_ih.T + b_ih + b_hh
    h = torch.zeros(n, H, dtype=x.dtype)
    c = torch.zeros(n, H, dtype=x.dtype)
    out = torch.empty(n, F, H, dtype=x.dtype)
    for t in (range(F - 1, -1, -1) if reverse else range(F)):
        g = gx[:, t] + h @ w_hh.T
        i, f, gg, o = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        out[:, t] = h
    return out


def forward(w: Dict[str, np.ndarray], x: np.ndarray, dtype=torch.float64,
            layers: int = 4) -> np.ndarray:
    """x [n, T] -> log-probabilities [n, F, 7]."""
    with torch.no_grad():
        x = torch.from_numpy(np.asarray(x)).to(dtype)
        x = _inorm(x[:, :, None], _t(w, "sincnet.wav_norm1d.weight", dtype),
                   _t(w, "sincnet.wav_norm1d.bias", dtype))[:, :, 0]
        w0 = _t(w, "sincnet.conv1d.0.weight", dtype)[:, 0]          # [80, 251]
        y = x.unfold(1, w0.shape[1], 10) @ w0.T                       # [n, L0, 80]
        y = _leaky(_inorm(_pool3(y.abs()), _t(w, "sincnet.norm1d.0.weight", dtype),
                          _t(w, "sincnet.norm1d.0.bias", dtype)))
        for i in (1, 2):
            wc = _t(w, f"sincnet.conv1d.{i}.weight", dtype)           # [co, ci, 5]
            win = y.unfold(1, wc.shape[2], 1)                         # [n, L, ci, 5]
            y = torch.einsum("nlcq,ocq->nlo", win, wc) + _t(w, f"sincnet.conv1d.{i}.bias", dtype)
            y = _leaky(_inorm(_pool3(y), _t(w, f"sincnet.norm1d.{i}.weight", dtype),
                              _t(w, f"sincnet.norm1d.{i}.bias", dtype)))
        for l in range(layers):
            dirs = []
            for sfx, rev in (("", False), ("_reverse", True)):
                dirs.append(_lstm_dir(y, _t(w, f"lstm.weight_ih_l{l}{sfx}", dtype),
                                      _t(w, f"lstm.weight_hh_l{l}{sfx}", dtype),
                                      _t(w, f"lstm.bias_ih_l{l}{sfx}", dtype),
                                      _t(w, f"lstm.bias_hh_l{l}{sfx}", dtype), rev))
            y = torch.cat(dirs, -1)
        for i in (0, 1):
            y = _leaky(y @ _t(w, f"linear.{i}.weight", dtype).T + _t(w, f"linear.{i}.bias", dtype))
        z = y @ _t(w, "classifier.weight", dtype).T + _t(w, "classifier.bias", dtype)
        m = z.max(-1, keepdim=True).values
        z = z - m
        return (z - torch.log(torch.exp(z).sum(-1, keepdim=True))).numpy()


def forward_modules(w: Dict[str, np.ndarray], x: np.ndarray, dtype=torch.float32) -> np.ndarray:
    """The same network through torch's own modules (F.instance_norm, F.conv1d, F.max_pool1d,
    nn.LSTM, F.linear, F.log_softmax) on the CPU in `dtype`."""
    import torch.nn.functional as Fn
    with torch.no_grad():
        y = torch.from_numpy(np.asarray(x)).to(dtype)[:, None, :]
        y = Fn.instance_norm(y, weight=_t(w, "sincnet.wav_norm1d.weight", dtype),
                             bias=_t(w, "sincnet.wav_norm1d.bias", dtype), eps=EPS)
        for i in range(3):
            if i == 0:
                y = Fn.conv1d(y, _t(w, "sincnet.conv1d.0.weight", dtype), stride=10).abs()
            else:
                y = Fn.conv1d(y, _t(w, f"sincnet.conv1d.{i}.weight", dtype),
                              _t(w, f"sincnet.conv1d.{i}.bias", dtype))
            y = Fn.max_pool1d(y, 3, 3)
            y = Fn.leaky_relu(Fn.instance_norm(y, weight=_t(w, f"sincnet.norm1d.{i}.weight", dtype),
                                               bias=_t(w, f"sincnet.norm1d.{i}.bias", dtype), eps=EPS),
                              LEAKY)
        H = w["lstm.weight_hh_l0"].shape[1]
        lstm = torch.nn.LSTM(y.shape[1], H, num_layers=4, bidirectional=True, batch_first=True).to(dtype)
        lstm.load_state_dict({k[len("lstm."):]: _t(w, k, dtype) for k in w if k.startswith("lstm.")})
        lstm.eval()
        y = lstm(y.transpose(1, 2))[0]
        for i in (0, 1):
            y = Fn.leaky_relu(Fn.linear(y, _t(w, f"linear.{i}.weight", dtype),
                                        _t(w, f"linear.{i}.bias", dtype)), LEAKY)
        return Fn.log_softmax(Fn.linear(y, _t(w, "classifier.weight", dtype),
                                        _t(w, "classifier.bias", dtype)), -1).numpy()
