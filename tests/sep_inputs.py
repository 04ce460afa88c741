"""Inputs and cached references shared by the separation tests (tests/test_convtasnet_reference.py
on the CPU, tests/test_gpu_sep.py on the device): the seeded network, the issue's region lengths
and ragged batch, and for each mixture the float64 restatement and torch's float32 evaluation,
computed once per process."""
from __future__ import annotations

import functools
from typing import Dict, Tuple

import numpy as np

from zasr.convtasnet import ConvTasNetConfig, synth_weights
from zasr.synth_audio import synth_speech

WEIGHT_SEED = 11
# T of the single-region cases: F = 1; F = 1 with a 15-sample zero tail; F = 128 (at dilation 128
# only the centre tap lands inside); F = 129 (all three taps of the dilation-128 blocks live);
# the reference's shortest region (0.4 s); one long region (3 s)
SINGLE_CASES: Tuple[int, ...] = (32, 47, 2064, 2080, 6400, 48000)
RAGGED: Tuple[int, ...] = (6400, 32, 2080, 16000, 47)
ALL_LENGTHS: Tuple[int, ...] = tuple(sorted(set(SINGLE_CASES) | set(RAGGED)))


@functools.lru_cache(maxsize=None)
def network() -> Tuple[ConvTasNetConfig, Dict[str, np.ndarray]]:
    cfg = ConvTasNetConfig()
    return cfg, synth_weights(cfg, WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def speech(seconds: float, seed: int) -> np.ndarray:
    a = synth_speech(seconds, seed).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def mixture(T: int) -> np.ndarray:
    """A two-voice mixture of T samples: two cuts of different synthetic speakers."""
    a, b = speech(12.0, 21), speech(12.0, 22)
    m = (0.6 * a[5000:5000 + T] + 0.5 * b[20000:20000 + T]).astype(np.float32)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def ref64(T: int) -> np.ndarray:
    from convtasnet_reference import forward
    cfg, w = network()
    r = forward(cfg, w, mixture(T))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def ref_f32(T: int) -> np.ndarray:
    import torch
    from convtasnet_reference import forward_modules
    cfg, w = network()
    r = forward_modules(cfg, w, mixture(T), torch.float32)
    r.setflags(write=False)
    return r


def peak_dev(got: np.ndarray, ref: np.ndarray) -> float:
    """Largest per-stream deviation divided by that stream's float64 peak."""
    return float(max(np.abs(got[s] - ref[s]).max() / np.abs(ref[s]).max() for s in range(2)))
