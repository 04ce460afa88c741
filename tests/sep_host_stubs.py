"""Deterministic inputs and stubs shared by tests/golden/make_golden_sep.py (which runs the
reference's OverlapSeparator on them) and tests/test_overlap_host.py (which runs zasr.overlap
on them): a synthetic file, segment / overlap layouts, a stand-in for the separation network
and a stand-in for the speaker embedding.  Everything is exact integer or elementwise float32
arithmetic, so both sides see the same bits on any machine."""
from __future__ import annotations

import hashlib
from typing import Dict, List, Optional

import numpy as np

SR = 16000


def make_audio(seconds: float, silent=()) -> np.ndarray:
    """A sawtooth-like float32 signal with exactly representable steps; zero in `silent` spans."""
    n = int(seconds * SR)
    i = np.arange(n, dtype=np.int64)
    a = (((i * 7919 + (i // 613) * 104729) % 2001) - 1000).astype(np.float32) / np.float32(1024.0)
    a *= np.float32(0.25)
    for s, e in silent:
        a[int(s * SR):int(e * SR)] = 0.0
    return a


def seg(start, end, speaker):
    return {"start": start, "end": end, "speaker": speaker}


# speakers 0 and 1 alternate with overlaps; 2 joins late; 3 only ever speaks inside overlaps (no
# centroid); one unlabelled segment (-1); clean segments that touch an overlap's edge; a clean
# segment of 160 samples (shorter than the 240-sample fade)
SEGMENTS: List[Dict] = [
    seg(0.0, 5.0, 0), seg(4.0, 8.0, 1), seg(8.0, 10.0, 0), seg(10.0, 11.5, -1),
    seg(10.5, 14.0, 1), seg(13.2, 13.9, 0), seg(14.0, 15.0, 0), seg(15.0, 18.0, 2),
    seg(16.0, 19.0, 0), seg(17.0, 17.6, 1), seg(19.0, 19.8, 1), seg(20.0, 24.0, 1),
    seg(22.0, 23.5, 3), seg(24.0, 27.5, 0), seg(26.0, 30.0, 1), seg(30.0, 30.5, 0),
    seg(31.0, 36.0, 0), seg(33.0, 33.01, 1), seg(34.5, 35.7, 1), seg(36.0, 40.0, 1),
]
# (4, 5): 0 + 1.  (13.2, 13.9): under 1 s.  (16, 18): three participants.  (22, 23.5): speaker 3
# has no centroid.  (26, 27.5): 0 + 1, silent audio.  (34.5, 35.7): 0 + 1 near the end
OVERLAPS = [(4.0, 5.0), (13.2, 13.9), (16.0, 18.0), (22.0, 23.5), (26.0, 27.5), (34.5, 35.7)]
FILE_SEC = 38.0          # shorter than the last segment: slices clamp to the file
SILENT = ((26.0, 27.5),)


class SegObj:
    """Segments as objects with attributes (the reference accepts both forms)."""

    def __init__(self, d):
        self.start, self.end, self.speaker = d["start"], d["end"], d["speaker"]


def fake_separation(x: np.ndarray) -> np.ndarray:
    """[T] -> [2, T + 3]: two complementary slowly varying gains, padded by three samples as
    an exported network may (the caller crops)."""
    x = np.asarray(x, np.float32)
    T = x.shape[0]
    g = ((np.arange(T, dtype=np.int64) % 97).astype(np.float32) / np.float32(128.0))
    out = np.zeros((2, T + 3), np.float32)
    out[0, :T] = x * g * np.float32(3.0)
    out[1, :T] = x * (np.float32(1.0) - g) * np.float32(0.5)
    out[:, T:] = np.float32(0.125)
    return out


def fake_embedding(audio: np.ndarray) -> Optional[np.ndarray]:
    """A 4-dim unit vector from exact integer statistics; None under 0.3 s, as the real one."""
    if len(audio) < int(0.3 * SR):
        return None
    q = np.round(np.asarray(audio, np.float64) * 4096.0).astype(np.int64)
    k = np.arange(q.shape[0], dtype=np.int64)
    v = np.array([int(np.abs(q).sum()) + 1, int(q[::2].sum()), int((q * q).sum() // 1000),
                  int((q * (k % 5)).sum())], np.float64)
    v = v / np.sqrt((v * v).sum())
    return v.astype(np.float32)


def digest(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def describe(a: np.ndarray) -> Dict:
    """What the golden file keeps of an audio array: length, digest and a few samples."""
    a = np.asarray(a, np.float32)
    idx = sorted({0, 1, 239, 240, 241, len(a) // 2, len(a) - 241, len(a) - 240, len(a) - 1} & set(range(len(a))))
    return {"n": int(len(a)), "sha256": digest(a), "idx": idx, "val": [float(a[i]) for i in idx]}
