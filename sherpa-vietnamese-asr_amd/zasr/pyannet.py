"""PyanNet segmentation model description, synthetic weights and on-disk format.

The reference's diarizer runs models/pyannote-onnx/segmentation-community-1.onnx with
onnxruntime on the CPU as its first stage (core/speaker_diarization_senko_campp_optimized.py
:383-396, :411-437): 10 s chunks of 16 kHz audio in, 589 frames x 7 powerset classes of
log-probabilities out.  Neither the .onnx nor onnx / onnxruntime ship with the reference tree
or this image, so the network is restated from pyannote's published PyanNet architecture, with
which everything the reference tree does hold about the file agrees (589 frames, 991-sample
receptive field, 270-sample frame step, 5.9 MB):

  input [N, 1, T]
  InstanceNorm1d(1, affine) over the T samples
  3 x (conv -> |.| (stage 0 only) -> MaxPool1d(3, 3) -> InstanceNorm1d(C, affine) -> leaky_relu):
      conv_0 80 filters x 251 taps, stride 10, no bias (the sinc filter bank, taken as a plain
      weight tensor [80, 1, 251]); conv_1 Conv1d(80, 60, 5); conv_2 Conv1d(60, 60, 5)
  LSTM(60, 128, num_layers 4, bidirectional), zero initial state
  leaky_relu(Linear(256, 128)) -> leaky_relu(Linear(128, 128)) -> Linear(128, 7) -> log_softmax
  output [N, F(T), 7]

Weights are SYNTHETIC (seeded numpy PCG64) under pyannote's state-dict names; how the real
export expresses the sinc parametrisation is not pinned (reading the .onnx is a follow-up).
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
CHUNK = 160000        # core/speaker_diarization_senko_campp_optimized.py:413
STEP = 80000          # :415
MIN_SAMPLES = 1261    # fewest samples that give 2 frames


@dataclasses.dataclass
class PyanNetConfig:
    sample_rate: int = SR
    sinc_filters: int = 80
    sinc_taps: int = 251
    sinc_stride: int = 10
    conv_channels: Tuple[int, ...] = (60, 60)
    conv_kernel: int = 5
    lstm_hidden: int = 128
    lstm_layers: int = 4
    linear: Tuple[int, ...] = (128, 128)
    classes: int = 7

    def to_json(self) -> str:
        return json.dumps(dataclasses.asdict(self), indent=1)

    @staticmethod
    def from_json(text: str) -> "PyanNetConfig":
        d = json.loads(text)
        d["conv_channels"] = tuple(d["conv_channels"])
        d["linear"] = tuple(d["linear"])
        return PyanNetConfig(**d)

    def stage_frames(self, T: int) -> Tuple[int, ...]:
        """Frames after conv_0, pool, conv_1, pool, conv_2, pool (0s once a stage is empty)."""
        out = []
        n = (T - self.sinc_taps) // self.sinc_stride + 1 if T >= self.sinc_taps else 0
        for i in range(3):
            if i > 0:
                n = n - self.conv_kernel + 1 if n >= self.conv_kernel else 0
            out.append(n)
            n //= 3
            out.append(n)
        return tuple(out)

    def num_frames(self, T: int) -> int:
        """F(T): 589 at T = 160000 (core/speaker_diarization_pure_ort.py:114)."""
        return self.stage_frames(T)[-1]


def param_shapes(cfg: PyanNetConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    s["sincnet.wav_norm1d.weight"] = (1,)
    s["sincnet.wav_norm1d.bias"] = (1,)
    s["sincnet.conv1d.0.weight"] = (cfg.sinc_filters, 1, cfg.sinc_taps)
    cin = cfg.sinc_filters
    s["sincnet.norm1d.0.weight"] = (cin,)
    s["sincnet.norm1d.0.bias"] = (cin,)
    for i, co in enumerate(cfg.conv_channels):
        s[f"sincnet.conv1d.{i + 1}.weight"] = (co, cin, cfg.conv_kernel)
        s[f"sincnet.conv1d.{i + 1}.bias"] = (co,)
        s[f"sincnet.norm1d.{i + 1}.weight"] = (co,)
        s[f"sincnet.norm1d.{i + 1}.bias"] = (co,)
        cin = co
    H = cfg.lstm_hidden
    for l in range(cfg.lstm_layers):
        k = cin if l == 0 else 2 * H
        for sfx in ("", "_reverse"):
            s[f"lstm.weight_ih_l{l}{sfx}"] = (4 * H, k)
            s[f"lstm.weight_hh_l{l}{sfx}"] = (4 * H, H)
            s[f"lstm.bias_ih_l{l}{sfx}"] = (4 * H,)
            s[f"lstm.bias_hh_l{l}{sfx}"] = (4 * H,)
    k = 2 * H
    for i, w in enumerate(cfg.linear):
        s[f"linear.{i}.weight"] = (w, k)
        s[f"linear.{i}.bias"] = (w,)
        k = w
    s["classifier.weight"] = (cfg.classes, k)
    s["classifier.bias"] = (cfg.classes,)
    return s


def num_params(cfg: PyanNetConfig) -> int:
    return int(sum(int(np.prod(s)) for s in param_shapes(cfg).values()))


def sinc_bank(cfg: PyanNetConfig) -> np.ndarray:
    """A mel-spaced band-pass bank in the sinc layer's shape: 40 band-pass filters (difference of
    two windowed sincs) and, as in pyannote's ParamSincFB, their quadrature twins -> [80, 1, 251]."""
    n = cfg.sinc_taps
    half = cfg.sinc_filters // 2
    t = (np.arange(n) - (n - 1) / 2) / cfg.sample_rate
    win = np.hamming(n)
    mel = np.linspace(2595 * np.log10(1 + 30 / 700), 2595 * np.log10(1 + (cfg.sample_rate / 2 - 100) / 700),
                      half + 1)
    hz = 700 * (10 ** (mel / 2595) - 1)
    bank = np.zeros((cfg.sinc_filters, 1, n))
    for i in range(half):
        lo, hi = hz[i], hz[i + 1]
        fc, bw = 0.5 * (lo + hi), hi - lo
        env = np.sinc(bw * t) * win
        c = env * np.cos(2 * np.pi * fc * t)
        s_ = env * np.sin(2 * np.pi * fc * t)
        bank[i, 0] = c / np.sqrt((c ** 2).sum())
        bank[half + i, 0] = s_ / np.sqrt((s_ ** 2).sum())
    return bank.astype(np.float32)


def synth_weights(cfg: PyanNetConfig, seed: int = 7) -> Dict[str, np.ndarray]:
    """Seeded weights.  A strong input gain and a weak recurrent gain in the LSTM make the
    hidden state follow the signal, the linears carry no bias (a bias gives every frame the
    same class), and the classifier gain spreads the log-probabilities over several units, so
    that with the default seed all 7 classes occur on synthetic speech (asserted in
    tests/test_pyannet_reference.py)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out: Dict[str, np.ndarray] = {}
    for name, shape in param_shapes(cfg).items():
        if name == "sincnet.conv1d.0.weight":
            w = sinc_bank(cfg)
        elif name.startswith("sincnet.wav_norm1d") or name.startswith("sincnet.norm1d"):
            w = (1.0 + 0.1 * rng.normal(size=shape)) if name.endswith("weight") \
                else 0.1 * rng.normal(size=shape)
        elif name.startswith("sincnet.conv1d") and name.endswith("weight"):
            w = rng.normal(0.0, 1.0, size=shape) / math.sqrt(shape[1] * shape[2])
        elif name.startswith("lstm.weight_ih"):
            w = rng.normal(0.0, 4.0, size=shape) / math.sqrt(shape[1])
        elif name.startswith("lstm.weight_hh"):
            w = rng.normal(0.0, 0.5, size=shape) / math.sqrt(shape[1])
        elif name.startswith("linear") and name.endswith("weight"):
            w = rng.normal(0.0, 1.5, size=shape) / math.sqrt(shape[1])
        elif name == "classifier.weight":
            w = rng.normal(0.0, 8.0, size=shape) / math.sqrt(shape[1])
        elif name == "classifier.bias" or name.startswith("linear"):
            w = np.zeros(shape)
        else:  # conv / lstm biases
            w = rng.normal(0.0, 0.1, size=shape)
        out[name] = np.ascontiguousarray(w, dtype=np.float32)
    return out


def save_model_dir(path: str, cfg: PyanNetConfig, weights: Dict[str, np.ndarray]) -> str:
    """config.json + model.safetensors (the engine's segmentation format)."""
    from safetensors.numpy import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        f.write(cfg.to_json())
    save_file({k: np.ascontiguousarray(v, dtype=np.float32) for k, v in weights.items()},
              os.path.join(path, "model.safetensors"))
    return path


def chunk_flops(cfg: PyanNetConfig, T: int = CHUNK) -> Dict[str, float]:
    """Multiply-adds x 2 of one chunk by stage."""
    l0, f1, l1, f2, l2, F = cfg.stage_frames(T)
    H = cfg.lstm_hidden
    c1, c2 = cfg.conv_channels
    out = {"front": 2.0 * l0 * cfg.sinc_filters * cfg.sinc_taps,
           "convs": 2.0 * cfg.conv_kernel * (l1 * cfg.sinc_filters * c1 + l2 * c1 * c2)}
    proj = rec = 0.0
    for l in range(cfg.lstm_layers):
        k = c2 if l == 0 else 2 * H
        proj += 2.0 * F * 2 * 4 * H * k
        rec += 2.0 * F * 2 * 4 * H * H
    out["projections"] = proj
    out["recurrence"] = rec
    k, head = 2 * H, 0.0
    for w in cfg.linear:
        head += 2.0 * F * k * w
        k = w
    out["head"] = head + 2.0 * F * k * cfg.classes
    return out
