"""Speech and overlap regions from the PyanNet segmentation: the host logic of the
reference's _pyannote_vad (core/speaker_diarization_senko_campp_optimized.py:411-517) around
the network, which runs on the device (zasr.binding.SegSession).

The chunking (:413-424), the powerset decode (:439-445), the per-frame vote of overlapping
chunks (:448-470) and the two region builders (:472-517) are reproduced exactly -- the same
IEEE operations in the same precision -- but vectorised with numpy: O(frames) array work
instead of a Python loop over every (chunk, frame).  tests/test_segmentation_host.py pins them
to lists the reference itself produced (tests/golden/seg_cases.json).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

SR = 16000
CHUNK_SECONDS = 10.0    # :413, and the numerator of frame_dur (:445)
STEP_SECONDS = 5.0      # :415
SPEECH_CLASSES_FROM = 1     # powerset classes 1-6 have a speaker active (:440-442, :460)
OVERLAP_CLASSES_FROM = 4    # classes 4-6 have two (:462)
MIN_OVERLAP = 0.3           # :482


class Regions(list):
    """The merged speech regions [(start_s, end_s)] as _pyannote_vad returns them, carrying the
    overlap regions the reference keeps in _last_overlap_regions (:489)."""
    overlap_regions: List[Tuple[float, float]] = []


def chunk_starts(total: int, sr: int = SR) -> List[int]:
    """First sample of every chunk (:413-424)."""
    chunk, step = int(CHUNK_SECONDS * sr), int(STEP_SECONDS * sr)
    if total <= 0:
        return []
    # 0, step, ... up to and including the first start with start + chunk >= total
    last = 0 if total <= chunk else -(-(total - chunk) // step) * step
    return list(range(0, last + 1, step))


def _runs(active: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Runs of True: (first frame, frame after the last, whether the run ends inside the array)."""
    a = np.concatenate([[False], active, [False]]).astype(np.int8)
    d = np.diff(a)
    start = np.flatnonzero(d == 1)
    end = np.flatnonzero(d == -1)
    return start, end, end < active.shape[0]


def output_frames(starts: Sequence[int], n_seg_frames: int, total: int, sr: int = SR
                  ) -> Tuple[np.ndarray, int]:
    """(out_f [n_chunks, F], n_out): the output frame every chunk frame votes in, out_f =
    int((t0 + f * frame_dur) / frame_dur) evaluated in doubles as the reference does (:450,
    :455-457; not round(t0 / frame_dur) + f in floating point), and the number of output
    frames; votes with out_f >= n_out are dropped."""
    frame_dur = CHUNK_SECONDS / n_seg_frames
    n_out = int((total / sr) / frame_dur) + 1
    t0 = np.asarray(starts, np.int64).astype(np.float64) / np.float64(sr)
    f = np.arange(n_seg_frames, dtype=np.float64)
    return ((t0[:, None] + f[None, :] * frame_dur) / frame_dur).astype(np.int64), n_out


def aggregate(classes: np.ndarray, starts: Sequence[int], total: int, min_speech: float = 0.25,
              min_silence: float = 0.1, sr: int = SR
              ) -> Tuple[List[Tuple[float, float]], List[Tuple[float, float]]]:
    """(speech_regions, overlap_regions) of the class maps [n_chunks, F] of the chunks at
    `starts` of a file of `total` samples (:444-517)."""
    classes = np.asarray(classes)
    n_seg_frames = classes.shape[1]
    frame_dur = CHUNK_SECONDS / n_seg_frames
    total_dur = total / sr
    out_f, n_out = output_frames(starts, n_seg_frames, total, sr)
    keep = (out_f >= 0) & (out_f < n_out)
    idx = out_f[keep]
    cls = classes[keep]
    total_count = np.bincount(idx, minlength=n_out).astype(np.float32)
    speech_count = np.bincount(idx[cls >= SPEECH_CLASSES_FROM], minlength=n_out).astype(np.float32)
    overlap_count = np.bincount(idx[cls >= OVERLAP_CLASSES_FROM], minlength=n_out).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        speech_prob = np.where(total_count > 0, speech_count / total_count, 0)
        overlap_prob = np.where(total_count > 0, overlap_count / total_count, 0)
    is_speech = speech_prob > 0.5
    is_overlap = overlap_prob > 0.5

    overlap: List[Tuple[float, float]] = []
    a, b, _ = _runs(is_overlap)
    ta, tb = a.astype(np.float64) * frame_dur, b.astype(np.float64) * frame_dur
    for s, e in zip(ta[tb - ta >= MIN_OVERLAP].tolist(), tb[tb - ta >= MIN_OVERLAP].tolist()):
        overlap.append((s, min(e, total_dur)))

    regions: List[Tuple[float, float]] = []
    a, b, closed = _runs(is_speech)
    ta, tb = a.astype(np.float64) * frame_dur, b.astype(np.float64) * frame_dur
    ok = tb - ta >= min_speech
    for s, e, c in zip(ta[ok].tolist(), tb[ok].tolist(), closed[ok].tolist()):
        regions.append((s, e) if c else (s, min(e, total_dur)))   # :502 / :507

    if not regions:
        return [(0.0, total_dur)], overlap
    merged = [regions[0]]
    for s, e in regions[1:]:
        if s - merged[-1][1] < min_silence:
            merged[-1] = (merged[-1][0], e)
        else:
            merged.append((s, e))
    return merged, overlap


def classes_of(audio, session, sr: int = SR) -> Tuple[np.ndarray, List[int], int]:
    """Class maps of every chunk of `audio`: a host array (batched through session.run as the
    reference does, :426-443) or a 1-D float32 torch tensor already on the device (one
    classes_device call on the HBM signal, no host batch)."""
    chunk, step = int(CHUNK_SECONDS * sr), int(STEP_SECONDS * sr)
    if hasattr(audio, "data_ptr") and getattr(audio, "is_cuda", False):
        import torch
        if audio.dtype != torch.float32 or audio.dim() != 1 or not audio.is_contiguous():
            raise ValueError("pyannote_vad: the device signal must be contiguous 1-D float32")
        total = int(audio.shape[0])
        starts = chunk_starts(total, sr)
        stream = torch.cuda.current_stream(audio.device).cuda_stream
        classes = session.classes_device(audio.data_ptr(), total, chunk, step, stream=stream)
        return classes, starts, total
    audio = np.asarray(audio, np.float32)
    total = int(audio.shape[0])
    starts = chunk_starts(total, sr)
    maps = []
    for b in range(0, len(starts), 32):
        be = min(b + 32, len(starts))
        batch = np.zeros((be - b, 1, chunk), np.float32)
        for i, cs in enumerate(starts[b:be]):
            ce = min(cs + chunk, total)
            batch[i, 0, :ce - cs] = audio[cs:ce]
        maps.append(np.argmax(session.run(None, {"input_values": batch})[0], axis=-1))
    n_frames = session.num_frames(chunk) if hasattr(session, "num_frames") else 0
    classes = np.concatenate(maps, 0) if maps else np.zeros((0, n_frames), np.int64)
    return classes.astype(np.uint8), starts, total


def pyannote_vad(audio, session, sr: int = SR, min_speech: float = 0.25,
                 min_silence: float = 0.1) -> Regions:
    """What the reference's _pyannote_vad(audio, sr, min_speech, min_silence) returns, with the
    overlap regions as `.overlap_regions`."""
    classes, starts, total = classes_of(audio, session, sr)
    if not starts:   # an empty file: the reference's loops run over nothing
        out = Regions([(0.0, total / sr)])
        out.overlap_regions = []
        return out
    speech, overlap = aggregate(classes, starts, total, min_speech, min_silence, sr)
    out = Regions(speech)
    out.overlap_regions = overlap
    return out
