"""Inputs and cached references shared by the segmentation tests (tests/test_pyannet_reference.py
on the CPU, tests/test_gpu_seg.py on the device): the seeded network, the four logits cases of
the issue, and for each the float64 restatement and torch's float32 evaluation, computed once
per process."""
from __future__ import annotations

import functools
from typing import Dict, Tuple

import numpy as np

from zasr.pyannet import CHUNK, PyanNetConfig, synth_weights
from zasr.synth_audio import synth_speech

WEIGHT_SEED = 7
# (n, T) of the logits cases: F = 2; three tiny chunks; one full chunk; five full chunks, the
# last 70 % zero padding
LOGIT_CASES: Tuple[Tuple[int, int], ...] = ((1, 1261), (3, 1531), (1, CHUNK), (5, CHUNK))


@functools.lru_cache(maxsize=None)
def network() -> Tuple[PyanNetConfig, Dict[str, np.ndarray]]:
    cfg = PyanNetConfig()
    return cfg, synth_weights(cfg, WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def speech(seconds: float, seed: int) -> np.ndarray:
    a = synth_speech(seconds, seed).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case_batch(n: int, T: int) -> np.ndarray:
    """Batch [n, T] of one logits case: consecutive half-overlapping cuts of synthetic speech."""
    a = speech(35.0, 11)
    step = T // 2
    b = np.zeros((n, T), np.float32)
    for i in range(n):
        b[i] = a[4000 + i * step:4000 + i * step + T]
    if (n, T) == (5, CHUNK):
        b[4, int(0.3 * T):] = 0.0
    return b


@functools.lru_cache(maxsize=None)
def case_ref64(n: int, T: int) -> np.ndarray:
    from pyannet_reference import forward
    r = forward(network()[1], case_batch(n, T))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def case_f32(n: int, T: int) -> np.ndarray:
    import torch
    from pyannet_reference import forward_modules
    r = forward_modules(network()[1], case_batch(n, T), torch.float32)
    r.setflags(write=False)
    return r


def top2_margin(logits: np.ndarray) -> np.ndarray:
    s = np.sort(logits, -1)
    return s[..., -1] - s[..., -2]
