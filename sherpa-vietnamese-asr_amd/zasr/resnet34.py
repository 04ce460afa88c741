"""WeSpeaker ResNet34 speaker-embedding model description, synthetic weights and on-disk format
(DESIGN §4i).

The reference's production diarizer (core/speaker_diarization_pure_ort.py) runs pyannote's
community-1 embedding model split in two (convert_onnx/split_pyannote_embedding.py): an encoder
whose output tensor /resnet/pool/Reshape_output_0 has shape (B, 2560, F), and the projection
resnet.seg_1.weight (256, 5120) / resnet.seg_1.bias applied on the host after the masked
statistics pooling.  Neither embedding_encoder.onnx nor onnx / onnxruntime / wespeaker ship with
the reference tree or this image, so the network is restated from WeSpeaker's published ResNet34
(wespeaker/models/resnet.py, BasicBlock, two-dimensional convolutions over frequency x time):

  x [B, T, 80] -> [B, 1, 80, T]                                   (H = frequency, W = time)
  relu(bn1(Conv2d(1, 32, 3, stride 1, pad 1, no bias)))
  layer1: 3 x BasicBlock(32 -> 32,  stride 1)      layer2: 4 x BasicBlock(32 -> 64,  first stride 2)
  layer3: 6 x BasicBlock(64 -> 128, first stride 2) layer4: 3 x BasicBlock(128 -> 256, first stride 2)
  BasicBlock: y = bn2(conv3x3(relu(bn1(conv3x3(x, stride s))), stride 1)); out = relu(y + sc(x)),
              sc = identity, or bn(Conv2d 1x1, stride s, no bias) when s != 1 or the width changes
  [B, 256, 10, T'] -> reshape [B, 2560, T'], channel index c * 10 + f

Each strided stage maps n -> (n - 1) // 2 + 1: 998 -> 499 -> 250 -> 125 frames, 80 -> 10 bins.
Every BatchNorm is folded into the convolution before it once, in float64, at load
(fold_batchnorm); the engine, the tests' torch module and their float64 restatement all use the
folded float32 tensors.

UNPINNED: the real file.  Only the output tensor's shape and seg_1's names are pinned by the
reference; reading the .onnx is a follow-up.  Weights are SYNTHETIC (seeded numpy PCG64) under
WeSpeaker's state-dict names.
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
CHUNK_SAMPLES = 160000       # core/speaker_diarization_pure_ort.py CHUNK_SAMPLES
CHUNK_FRAMES = 998           # :801
MAX_SPEAKERS_PER_CHUNK = 3


@dataclasses.dataclass
class ResNet34Config:
    feat_dim: int = 80
    m_channels: int = 32
    num_blocks: Tuple[int, int, int, int] = (3, 4, 6, 3)
    embed_dim: int = 256
    bn_eps: float = 1e-5

    def to_json(self) -> str:
        d = dataclasses.asdict(self)
        d["num_blocks"] = list(self.num_blocks)
        return json.dumps(d, indent=1)

    @staticmethod
    def from_json(text: str) -> "ResNet34Config":
        d = json.loads(text)
        d["num_blocks"] = tuple(d["num_blocks"])
        return ResNet34Config(**d)

    @staticmethod
    def down(n: int, times: int = 3) -> int:
        for _ in range(times):
            n = (n - 1) // 2 + 1
        return n

    @property
    def out_bins(self) -> int:
        return self.down(self.feat_dim)

    @property
    def out_channels(self) -> int:
        return 8 * self.m_channels

    @property
    def feat_width(self) -> int:
        """Rows of the frame-feature matrix (2560)."""
        return self.out_channels * self.out_bins

    @property
    def stats_dim(self) -> int:
        return 2 * self.feat_width

    def num_feat_frames(self, T: int) -> int:
        return self.down(T) if T >= 1 else 0


def block_plan(cfg: ResNet34Config):
    """(prefix, in_planes, planes, stride, has_shortcut) of every BasicBlock in order."""
    out, in_planes = [], cfg.m_channels
    for li, nb in enumerate(cfg.num_blocks):
        planes = cfg.m_channels << li
        for bi in range(nb):
            stride = 2 if (bi == 0 and li > 0) else 1
            out.append((f"resnet.layer{li + 1}.{bi}.", in_planes, planes, stride,
                        stride != 1 or in_planes != planes))
            in_planes = planes
    return out


def _bn(s, p, c):
    for k in ("weight", "bias", "running_mean", "running_var"):
        s[p + "." + k] = (c,)


def param_shapes(cfg: ResNet34Config) -> "OrderedDict[str, Tuple[int, ...]]":
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    s["resnet.conv1.weight"] = (cfg.m_channels, 1, 3, 3)
    _bn(s, "resnet.bn1", cfg.m_channels)
    for p, cin, c, _stride, sc in block_plan(cfg):
        s[p + "conv1.weight"] = (c, cin, 3, 3)
        _bn(s, p + "bn1", c)
        s[p + "conv2.weight"] = (c, c, 3, 3)
        _bn(s, p + "bn2", c)
        if sc:
            s[p + "shortcut.0.weight"] = (c, cin, 1, 1)
            _bn(s, p + "shortcut.1", c)
    s["resnet.seg_1.weight"] = (cfg.embed_dim, cfg.stats_dim)
    s["resnet.seg_1.bias"] = (cfg.embed_dim,)
    return s


def num_params(cfg: ResNet34Config) -> int:
    return int(sum(int(np.prod(s)) for s in param_shapes(cfg).values()))


# Every BasicBlock adds its branch to its input, so with He weights throughout the stream's
# variance doubles per block: 16 blocks take CMVN'd fbank rows (rms 2-3) to frame features of rms
# ~800, where an absolute tolerance means nothing.  The branch's closing convolution (conv2) is
# therefore drawn at RESIDUAL_GAIN x the He deviation (the role zero-initialised last BatchNorms
# play in trained residual networks); frame features then have rms ~3.
RESIDUAL_GAIN = 0.25


def synth_weights(cfg: ResNet34Config, seed: int = 17) -> Dict[str, np.ndarray]:
    """Seeded weights: convolutions N(0, 2 / fan_in) (He; conv2 of every block x RESIDUAL_GAIN,
    see above: tests/test_resnet34_reference.py asserts frame features with rms in [0.1, 10]),
    BatchNorm gamma and running_var in [0.8, 1.2], beta and running_mean in [-0.1, 0.1], seg_1
    N(0, 1 / 5120)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out: Dict[str, np.ndarray] = {}
    for name, shape in param_shapes(cfg).items():
        if name.startswith("resnet.seg_1"):
            w = rng.normal(0.0, math.sqrt(1.0 / cfg.stats_dim), size=shape)
        elif len(shape) == 4:
            w = rng.normal(0.0, math.sqrt(2.0 / (shape[1] * shape[2] * shape[3])), size=shape)
            if name.endswith(".conv2.weight"):
                w *= RESIDUAL_GAIN
        elif name.endswith("running_var") or name.endswith(".weight"):
            w = rng.uniform(0.8, 1.2, size=shape)
        else:
            w = rng.uniform(-0.1, 0.1, size=shape)
        out[name] = np.ascontiguousarray(w, dtype=np.float32)
    return out


def fold_batchnorm(w: np.ndarray, gamma, beta, mean, var, eps: float, dtype=np.float32):
    """(w', b'): w' = w gamma / sqrt(var + eps), b' = beta - mean gamma / sqrt(var + eps),
    computed in float64 and rounded once to `dtype` (float32: what the engine holds)."""
    sc = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + eps)
    wf = (w.astype(np.float64) * sc[:, None, None, None]).astype(dtype)
    bf = (beta.astype(np.float64) - mean.astype(np.float64) * sc).astype(dtype)
    return wf, bf


def folded_weights(cfg: ResNet34Config, weights: Dict[str, np.ndarray], dtype=np.float32):
    """{conv name: (w' [co][ci][r][q], b' [co])} for every convolution."""
    def fold(conv, bn):
        return fold_batchnorm(weights[conv + ".weight"], weights[bn + ".weight"], weights[bn + ".bias"],
                              weights[bn + ".running_mean"], weights[bn + ".running_var"], cfg.bn_eps,
                              dtype)
    out = {"resnet.conv1": fold("resnet.conv1", "resnet.bn1")}
    for p, _cin, _c, _stride, sc in block_plan(cfg):
        out[p + "conv1"] = fold(p + "conv1", p + "bn1")
        out[p + "conv2"] = fold(p + "conv2", p + "bn2")
        if sc:
            out[p + "shortcut"] = fold(p + "shortcut.0", p + "shortcut.1")
    return out


def save_model_dir(path: str, cfg: ResNet34Config, weights: Dict[str, np.ndarray]) -> str:
    """config.json + model.safetensors (the engine's embedding format)."""
    from safetensors.numpy import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        f.write(cfg.to_json())
    save_file({k: np.ascontiguousarray(v, dtype=np.float32) for k, v in weights.items()},
              os.path.join(path, "model.safetensors"))
    return path


def encoder_flops(cfg: ResNet34Config, T: int) -> float:
    """Multiply-adds x 2 of the encoder on one input of T fbank frames."""
    fl = 2.0 * 9 * cfg.m_channels * cfg.feat_dim * T
    F = cfg.feat_dim
    for _p, cin, c, stride, sc in block_plan(cfg):
        F, T = (F - 1) // stride + 1, (T - 1) // stride + 1
        fl += 2.0 * F * T * (9 * cin * c + 9 * c * c + (cin * c if sc else 0))
    return fl


def layer_flops(cfg: ResNet34Config, T: int) -> Dict[str, float]:
    """Multiply-adds x 2 of one input of T frames by stage: stem, layer1 .. layer4."""
    out = {"stem": 2.0 * 9 * cfg.m_channels * cfg.feat_dim * T}
    F = cfg.feat_dim
    for p, cin, c, stride, sc in block_plan(cfg):
        F, T = (F - 1) // stride + 1, (T - 1) // stride + 1
        k = p.split(".")[1]
        out[k] = out.get(k, 0.0) + 2.0 * F * T * (9 * cin * c + 9 * c * c + (cin * c if sc else 0))
    return out


def chunk_flops(cfg: ResNet34Config, T: int = CHUNK_FRAMES) -> Dict[str, float]:
    """Multiply-adds x 2 of one chunk by stage (the pooling counted as 6 per element and speaker)."""
    Tq = cfg.num_feat_frames(T)
    return {
        "encoder": encoder_flops(cfg, T),
        "pooling": 6.0 * MAX_SPEAKERS_PER_CHUNK * cfg.feat_width * Tq,
        "projection": 2.0 * MAX_SPEAKERS_PER_CHUNK * cfg.stats_dim * cfg.embed_dim,
    }


def group_bytes(cfg: ResNet34Config, T: int = CHUNK_FRAMES) -> int:
    """Activation bytes of one input in a launch group: three layer1-sized buffers and the rows."""
    return 4 * (3 * cfg.feat_dim * T * cfg.m_channels + cfg.feat_dim * T)
