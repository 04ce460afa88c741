"""Conv-TasNet separation model description, synthetic weights and on-disk format.

The reference separates every two-speaker overlap region with asteroid's
ConvTasNet_Libri2Mix_sepclean_16k, exported by convert_onnx/export_convtasnet_onnx.py and run
through onnxruntime on the CPU, one region per call (core/overlap_separator.py:45-60, :281-296).
Neither the .onnx nor onnx / onnxruntime / asteroid ship with the reference tree or this image,
so the network is restated from asteroid's published ConvTasNet (free filter-bank encoder /
decoder, TDConvNet masker):

  mixture [T],  F = (T - kernel_size) // stride + 1
  tf   = Conv1d(1, n_filters, kernel_size, stride, no bias)(x)                   (no activation)
  o    = Conv1d(n_filters, bn_chan, 1)(gLN(tf));  skip = 0
  for i in range(n_repeats * n_blocks), dilation d = 2 ** (i % n_blocks):
      y    = gLN(PReLU(Conv1d(bn_chan, hid_chan, 1)(o)))
      y    = gLN(PReLU(depthwise Conv1d(hid_chan, hid_chan, 3, dilation d, padding d)(y)))
      o    = o + res_conv(y);  skip = skip + skip_conv(y)     (the last res_conv is unused)
  mask = relu(Conv1d(skip_chan, n_src * n_filters, 1)(PReLU(skip))) as [n_src, n_filters, F]
  out  = ConvTranspose1d(n_filters, 1, kernel_size, stride, no bias)(mask * tf), zero-padded to T

gLN is one mean and one biased variance over all channels x frames of a sample (eps 1e-8) with
an affine gamma / beta per channel; every PReLU has a single slope.

UNPINNED: the real file and its hyper-parameters.  The defaults below are the issue's; every
size is carried in config.json, and reading the .onnx is a follow-up.  Weights are SYNTHETIC
(seeded numpy PCG64) under asteroid's state-dict names.
"""
from __future__ import annotations

import dataclasses
import json
import math
import os
from collections import OrderedDict
from typing import Dict, Tuple

import numpy as np

SR = 16000


@dataclasses.dataclass
class ConvTasNetConfig:
    sample_rate: int = SR
    n_src: int = 2
    n_filters: int = 512
    kernel_size: int = 32
    stride: int = 16
    bn_chan: int = 128
    hid_chan: int = 512
    skip_chan: int = 128
    conv_kernel_size: int = 3
    n_blocks: int = 8
    n_repeats: int = 3
    norm_type: str = "gLN"
    mask_act: str = "relu"

    def to_json(self) -> str:
        return json.dumps(dataclasses.asdict(self), indent=1)

    @staticmethod
    def from_json(text: str) -> "ConvTasNetConfig":
        return ConvTasNetConfig(**json.loads(text))

    def num_frames(self, T: int) -> int:
        return (T - self.kernel_size) // self.stride + 1 if T >= self.kernel_size else 0

    def decoded_samples(self, T: int) -> int:
        """Samples the decoder produces; the rest up to T is zero padding."""
        F = self.num_frames(T)
        return (F - 1) * self.stride + self.kernel_size if F > 0 else 0

    @property
    def min_samples(self) -> int:
        return self.kernel_size


def param_shapes(cfg: ConvTasNetConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    s["encoder.filterbank._filters"] = (cfg.n_filters, 1, cfg.kernel_size)
    s["masker.bottleneck.0.gamma"] = (1, cfg.n_filters, 1)
    s["masker.bottleneck.0.beta"] = (1, cfg.n_filters, 1)
    s["masker.bottleneck.1.weight"] = (cfg.bn_chan, cfg.n_filters, 1)
    s["masker.bottleneck.1.bias"] = (cfg.bn_chan,)
    for i in range(cfg.n_blocks * cfg.n_repeats):
        p = f"masker.TCN.{i}."
        s[p + "shared_block.0.weight"] = (cfg.hid_chan, cfg.bn_chan, 1)
        s[p + "shared_block.0.bias"] = (cfg.hid_chan,)
        s[p + "shared_block.1.weight"] = (1,)
        s[p + "shared_block.2.gamma"] = (1, cfg.hid_chan, 1)
        s[p + "shared_block.2.beta"] = (1, cfg.hid_chan, 1)
        s[p + "shared_block.3.weight"] = (cfg.hid_chan, 1, cfg.conv_kernel_size)
        s[p + "shared_block.3.bias"] = (cfg.hid_chan,)
        s[p + "shared_block.4.weight"] = (1,)
        s[p + "shared_block.5.gamma"] = (1, cfg.hid_chan, 1)
        s[p + "shared_block.5.beta"] = (1, cfg.hid_chan, 1)
        s[p + "res_conv.weight"] = (cfg.bn_chan, cfg.hid_chan, 1)
        s[p + "res_conv.bias"] = (cfg.bn_chan,)
        s[p + "skip_conv.weight"] = (cfg.skip_chan, cfg.hid_chan, 1)
        s[p + "skip_conv.bias"] = (cfg.skip_chan,)
    s["masker.mask_net.0.weight"] = (1,)
    s["masker.mask_net.1.weight"] = (cfg.n_src * cfg.n_filters, cfg.skip_chan, 1)
    s["masker.mask_net.1.bias"] = (cfg.n_src * cfg.n_filters,)
    s["decoder.filterbank._filters"] = (cfg.n_filters, 1, cfg.kernel_size)
    return s


def num_params(cfg: ConvTasNetConfig) -> int:
    return int(sum(int(np.prod(s)) for s in param_shapes(cfg).values()))


def synth_weights(cfg: ConvTasNetConfig, seed: int = 11) -> Dict[str, np.ndarray]:
    """Seeded weights.  The encoder is a unit-norm random filter bank and the decoder its scaled
    transpose, so an all-ones mask would return the mixture's scale; the 1x1 convolutions have
    fan-in gain about 1 (the gLN after each re-centres the stream); the mask projection has
    zero-mean weights and a positive bias, so that on synthetic speech roughly half of each
    source's relu mask is open and both streams carry signal (asserted in
    tests/test_convtasnet_reference.py: a dead mask would make every tolerance vacuous)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out: Dict[str, np.ndarray] = {}
    for name, shape in param_shapes(cfg).items():
        if name == "encoder.filterbank._filters":
            w = rng.normal(size=shape)
            w /= np.sqrt((w ** 2).sum(axis=2, keepdims=True))
        elif name == "decoder.filterbank._filters":
            w = rng.normal(size=shape) / math.sqrt(cfg.n_filters)
        elif name.endswith("gamma"):
            w = 1.0 + 0.1 * rng.normal(size=shape)
        elif name.endswith("beta"):
            w = 0.1 * rng.normal(size=shape)
        elif name.endswith("shared_block.1.weight") or name.endswith("shared_block.4.weight") \
                or name == "masker.mask_net.0.weight":
            w = np.full(shape, 0.25) + 0.05 * rng.normal(size=shape)   # torch's PReLU init +- a bit
        elif name.endswith("shared_block.3.weight"):
            w = rng.normal(0.0, 1.0, size=shape) / math.sqrt(shape[2])
        elif name == "masker.mask_net.1.weight":
            w = rng.normal(0.0, 1.0, size=shape) / math.sqrt(shape[1])
        elif name == "masker.mask_net.1.bias":
            w = 0.1 + 0.1 * rng.normal(size=shape)
        elif name.endswith("res_conv.weight") or name.endswith("skip_conv.weight"):
            w = rng.normal(0.0, 0.5, size=shape) / math.sqrt(shape[1])
        elif name.endswith("weight"):
            w = rng.normal(0.0, 1.0, size=shape) / math.sqrt(shape[1])
        else:  # conv biases
            w = rng.normal(0.0, 0.1, size=shape)
        out[name] = np.ascontiguousarray(w, dtype=np.float32)
    return out


def save_model_dir(path: str, cfg: ConvTasNetConfig, weights: Dict[str, np.ndarray]) -> str:
    """config.json + model.safetensors (the engine's separation format)."""
    from safetensors.numpy import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        f.write(cfg.to_json())
    save_file({k: np.ascontiguousarray(v, dtype=np.float32) for k, v in weights.items()},
              os.path.join(path, "model.safetensors"))
    return path


def region_flops(cfg: ConvTasNetConfig, T: int) -> Dict[str, float]:
    """Multiply-adds x 2 of one region of T samples by stage."""
    F = cfg.num_frames(T)
    nb = cfg.n_blocks * cfg.n_repeats
    return {
        "encoder": 2.0 * F * cfg.n_filters * cfg.kernel_size,
        "gemms": 2.0 * F * (cfg.n_filters * cfg.bn_chan
                            + nb * cfg.hid_chan * (2 * cfg.bn_chan + cfg.skip_chan)),
        "norms_depthwise": 2.0 * F * (2 * cfg.n_filters
                                      + nb * cfg.hid_chan * (cfg.conv_kernel_size + 4)),
        "mask_decoder": 2.0 * F * cfg.n_src * cfg.n_filters * (cfg.skip_chan + cfg.kernel_size),
    }


def region_bytes(cfg: ConvTasNetConfig, T: int) -> float:
    """Activation bytes the engine's kernels read and write for one region (weights, which stay
    in cache, not counted): per TCN block the 1x1 GEMM (read o, write h), the statistics pass
    over h, the fused middle (read h, write y), the second norm in place (read + write y) and
    the res | skip GEMM (read y, read + write o | skip)."""
    F = cfg.num_frames(T)
    nb = cfg.n_blocks * cfg.n_repeats
    os_ = cfg.bn_chan + cfg.skip_chan
    block = os_ + cfg.hid_chan * 7 + 2 * os_
    head = cfg.kernel_size * 2 + cfg.n_filters * 4 + os_ * 2
    tail = cfg.n_src * (cfg.skip_chan + cfg.n_filters * 3 + cfg.kernel_size * 2)
    return 4.0 * F * (head + nb * block + tail)
