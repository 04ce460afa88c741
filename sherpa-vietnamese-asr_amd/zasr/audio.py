"""Device audio front end: raw PCM to the 16 kHz mono float32 signal in HBM, and the
reference's level conditioning on that signal (zasr.binding.AudioFrontEnd over the
zasr_audio_* C ABI of include/zasr.h).

What it stands in for:

  core/asr_engine.py:492-508   load_audio's decode side: soundfile's float32 read (int16 ->
                               x * 2^-15), audio.mean(axis=1), the resample to 16 kHz (ffmpeg /
                               soxr there; here the Hann-windowed sinc of sherpa-onnx's
                               LinearResample, DESIGN.md "Audio front end")     -> to_16k
  core/asr_engine.py:512-516   the quiet-file boost audio / peak * 0.95         -> boost_quiet
  core/audio_preprocessing.py  compute_segment_rms, per_segment_rms_normalize,
                               adaptive_peak_limit, preprocess_audio (:39-140, :226-293), same
                               names and signatures
  core/audio_preprocessing.py  apply_wpe_dereverberation (:157-216), same name and signature:
                               the per-frequency WPE of DESIGN.md §4k (the documented
                               algorithm; the reference's own call stacks the 257 bins as
                               channels and is not reproduced, so installing it is opt-in);
                               apply_wpe_batch runs every chunk of a file in one device call

Every function takes a numpy array and returns numpy float32, or takes a torch CUDA tensor
and returns one (nothing then leaves the device but the per-segment sums and the peak).  The
sums of squares, the gain application and the peaks run on the GPU; the gain plan between them
is host logic with the reference's numpy calls, kept sparse: one constant per segment plus the
5 ms ramps.  There is no CPU fallback: without libzasr.so or a GPU these raise.
"""
from __future__ import annotations

import bisect
import logging
import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np

from zasr.binding import AudioFrontEnd, WpeEngine, ZasrError, audio_out_len

logger = logging.getLogger("zasr")

_fronts: dict = {}
_wpes: dict = {}
_lock = threading.Lock()


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise ZasrError("the audio front end runs on the GPU: no HIP device is visible")
    return torch


def front_end(device_id: Optional[int] = None) -> AudioFrontEnd:
    """The process-wide front end of one device (its tables and staging buffers are cached)."""
    torch = _torch()
    dev = torch.cuda.current_device() if device_id is None else int(device_id)
    with _lock:
        fe = _fronts.get(dev)
        if fe is None or not fe.handle:
            fe = _fronts[dev] = AudioFrontEnd(dev)
        return fe


def wpe_engine(device_id: Optional[int] = None) -> WpeEngine:
    """The process-wide WPE engine of one device (its tables and workspace are cached)."""
    torch = _torch()
    dev = torch.cuda.current_device() if device_id is None else int(device_id)
    with _lock:
        we = _wpes.get(dev)
        if we is None or not we.handle:
            we = _wpes[dev] = WpeEngine(dev)
        return we


def close() -> None:
    with _lock:
        for fe in _fronts.values():
            fe.close()
        _fronts.clear()
        for we in _wpes.values():
            we.close()
        _wpes.clear()


def _stream() -> int:
    return int(_torch().cuda.current_stream().cuda_stream)


def _is_tensor(x) -> bool:
    return type(x).__module__.startswith("torch")


def _to_device(audio):
    """(float32 CUDA tensor holding a copy of audio, whether audio was a tensor)."""
    torch = _torch()
    if _is_tensor(audio):
        if not audio.is_cuda:
            raise ValueError("a torch input must be a CUDA tensor")
        return audio.to(torch.float32).contiguous().clone(), True
    a = np.ascontiguousarray(audio, np.float32)
    if a.ndim != 1:
        raise ValueError("audio must be mono: shape [n]")
    return torch.from_numpy(a).cuda(), False


def _back(d, was_tensor: bool):
    return d if was_tensor else d.cpu().numpy()


def to_16k(samples, sample_rate: int, device_out: bool = False):
    """samples [n] or [n, C] (C <= 8), float32 or int16, numpy or a torch CUDA tensor, at
    sample_rate Hz (4000..384000) -> the 16 kHz mono float32 signal, as numpy or (device_out, or
    a tensor input) a torch CUDA tensor."""
    torch = _torch()
    fe = front_end()
    tensor_in = _is_tensor(samples)
    if tensor_in:
        if not samples.is_cuda or samples.dtype not in (torch.float32, torch.int16):
            raise ValueError("a torch input must be a float32 or int16 CUDA tensor")
        src = samples.contiguous()
        fmt = "float32" if src.dtype == torch.float32 else "int16"
    else:
        src = np.asarray(samples)
        if src.dtype not in (np.float32, np.int16):
            raise ValueError("samples must be float32 or int16")
        src = np.ascontiguousarray(src)
    if src.ndim not in (1, 2):
        raise ValueError("samples must be shaped [n] or [n, channels]")
    n = int(src.shape[0])
    ch = int(src.shape[1]) if src.ndim == 2 else 1
    n_out = audio_out_len(sample_rate, n)
    out = torch.empty(max(n_out, 1), dtype=torch.float32, device="cuda")
    if tensor_in:
        got = fe.to_16k(src.data_ptr(), sample_rate, out.data_ptr(), n_out, channels=ch,
                        n_frames=n, fmt=fmt, stream=_stream())
    else:
        got = fe.to_16k(src, sample_rate, out.data_ptr(), n_out, stream=_stream())
    assert got == n_out, (got, n_out)
    out = out[:n_out]
    return out if (device_out or tensor_in) else out.cpu().numpy()


# ---- level conditioning on a device-resident signal, in place --------------------------------

def _boost_quiet_device(fe: AudioFrontEnd, d_ptr: int, n: int, stream: int) -> bool:
    peak = fe.peak(d_ptr, n, stream)
    if peak > 0 and peak < 0.5:
        fe.scale(d_ptr, n, peak, np.float32(0.95), stream)
        return True
    return False


def _rms_of(sumsq: float, count: int) -> float:
    """float(np.sqrt(np.mean(x ** 2))) of a float32 x from its sum of squares: numpy's mean is
    a float32 sum divided by the count in float32, its sqrt a float32 one."""
    return float(np.sqrt(np.float32(sumsq) / np.float32(count)))


class _SparseGain:
    """The reference's gain_map (core/audio_preprocessing.py:102) as sorted disjoint pieces
    over a background of 1.0: a piece is a float32 constant or a float32 array.  set() and
    get() behave as slice assignment and indexing of the dense array do, so the plan keeps the
    order dependence of the reference's writes (a ramp reads its neighbour's current gain)."""

    def __init__(self):
        self.b: List[int] = []
        self.e: List[int] = []
        self.v: list = []

    def get(self, i: int) -> np.float32:
        k = bisect.bisect_right(self.b, i) - 1
        if k >= 0 and i < self.e[k]:
            v = self.v[k]
            return v[i - self.b[k]] if isinstance(v, np.ndarray) else v
        return np.float32(1.0)

    @staticmethod
    def _cut(v, lo: int, hi: int):
        return v[lo:hi] if isinstance(v, np.ndarray) else v

    def set(self, s: int, e: int, val) -> None:
        if e <= s:
            return
        k0 = bisect.bisect_right(self.e, s)  # first piece ending after s
        k1 = bisect.bisect_left(self.b, e)   # first piece starting at or after e
        new = []
        if k0 < k1:
            b0, v0 = self.b[k0], self.v[k0]
            if b0 < s:
                new.append((b0, s, self._cut(v0, 0, s - b0)))
            b1, e1, v1 = self.b[k1 - 1], self.e[k1 - 1], self.v[k1 - 1]
            new.append((s, e, val))
            if e1 > e:
                new.append((e, e1, self._cut(v1, e - b1, e1 - b1)))
        else:
            new.append((s, e, val))
        self.b[k0:k1] = [p[0] for p in new]
        self.e[k0:k1] = [p[1] for p in new]
        self.v[k0:k1] = [p[2] for p in new]


def build_gain_plan(n: int, segment_rms: Sequence[Tuple[int, int, float]],
                    sample_rate: int = 16000, max_gain_db: float = 20.0,
                    crossfade_ms: float = 5) -> Optional[dict]:
    """The gain map of per_segment_rms_normalize (core/audio_preprocessing.py:88-126) for a
    signal of n samples, from the (start, end, rms) of the segments that passed its length and
    rms > 1e-8 filters, in sparse form: {"begin", "end" int64, "gain" float32, "ramp" int64
    (offset into "values", -1 for a constant piece), "values" float32}; pieces ascending and
    disjoint, gain 1 elsewhere.  None when the reference returns the audio unchanged."""
    if len(segment_rms) == 0:
        return None
    all_rms = np.array([r for _, _, r in segment_rms])
    target_rms = float(np.median(all_rms))
    if target_rms < 1e-8:
        return None
    max_gain_linear = 10 ** (max_gain_db / 20.0)
    crossfade_samples = int(crossfade_ms * sample_rate / 1000)
    g = _SparseGain()
    for s, e, rms in segment_rms:
        gain = max(min(target_rms / rms, max_gain_linear), 1.0 / max_gain_linear)
        g.set(max(s, 0), min(e, n), np.float32(gain))
    if crossfade_samples > 0:
        for s, e, _ in segment_rms:
            fade_len = min(crossfade_samples, (e - s) // 4)
            if fade_len <= 0:
                continue
            if s > 0:
                fade = np.linspace(g.get(s - 1), g.get(s), fade_len, dtype=np.float32)
                g.set(s, s + fade_len, fade)
            if e < n:
                fade = np.linspace(g.get(e - 1), g.get(e), fade_len, dtype=np.float32)
                g.set(e - fade_len, e, fade)
    ramp, vals, off = [], [], 0
    for b, e, v in zip(g.b, g.e, g.v):
        if isinstance(v, np.ndarray):
            ramp.append(off)
            vals.append(v)
            off += e - b
        else:
            ramp.append(-1)
    return {"begin": np.array(g.b, np.int64), "end": np.array(g.e, np.int64),
            "gain": np.array([np.float32(1.0) if isinstance(v, np.ndarray) else v for v in g.v],
                             np.float32),
            "ramp": np.array(ramp, np.int64),
            "values": np.concatenate(vals) if vals else np.zeros(0, np.float32),
            "target_rms": target_rms}


def _check_segments(vad_segments, n: int) -> List[Tuple[int, int]]:
    segs = [(int(s), int(e)) for s, e in vad_segments]
    for s, e in segs:
        if s < 0 or e < s or e > n:
            raise ValueError(f"VAD segment ({s}, {e}) outside the signal of {n} samples")
    return segs


def _normalize_device(fe: AudioFrontEnd, d_ptr: int, n: int, vad_segments, sample_rate: int,
                      min_segment_ms: float, max_gain_db: float, crossfade_ms: float,
                      stream: int) -> Optional[np.float32]:
    """per_segment_rms_normalize in place on the device signal; returns the peak of the result
    when a gain was applied (the same pass takes it), None when the signal is unchanged."""
    segs = _check_segments(vad_segments, n)
    min_samples = int(min_segment_ms * sample_rate / 1000)
    long_enough = [(s, e) for s, e in segs if e - s >= min_samples and e > s]
    if not long_enough:
        return None
    sums = fe.segment_sumsq(d_ptr, n, [s for s, _ in long_enough], [e for _, e in long_enough],
                            stream)
    seg_rms = []
    for (s, e), ss in zip(long_enough, sums):
        rms = _rms_of(ss, e - s)
        if rms > 1e-8:
            seg_rms.append((s, e, rms))
    plan = build_gain_plan(n, seg_rms, sample_rate, max_gain_db, crossfade_ms)
    if plan is None:
        return None
    r = [x[2] for x in seg_rms]
    logger.info("[Preprocess] RMS normalize: %d segments, target_rms=%.6f (min=%.6f, max=%.6f)",
                len(seg_rms), plan["target_rms"], min(r), max(r))
    return fe.apply_gain(d_ptr, n, plan["begin"], plan["end"], plan["gain"], plan["ramp"],
                         plan["values"], stream)


def _limit_device(fe: AudioFrontEnd, d_ptr: int, n: int, peak, target_peak, stream: int) -> None:
    if peak > target_peak:
        # audio * (target_peak / peak): a float32 quotient (peak is float32, target_peak a
        # Python float), then a float32 product
        fe.scale(d_ptr, n, np.float32(1.0), np.float32(target_peak) / np.float32(peak), stream)
        logger.info("[Preprocess] Peak limited: %.4f -> %s", float(peak), target_peak)


def condition_device(d_ptr: int, n: int, vad_segments=(), sample_rate: int = 16000,
                     boost: bool = True, enable_rms_normalize: bool = True,
                     stream: Optional[int] = None) -> None:
    """load_audio's quiet-file boost (when `boost`) and preprocess_audio, in place on n float32
    samples at device pointer d_ptr (zasr.pipeline.FullPipe.prepare)."""
    fe = front_end()
    st = _stream() if stream is None else int(stream)
    if n <= 0:
        return
    if boost:
        _boost_quiet_device(fe, d_ptr, n, st)
    peak = None
    if enable_rms_normalize and len(vad_segments) > 0:
        peak = _normalize_device(fe, d_ptr, n, vad_segments, sample_rate, 100, 20.0, 5, st)
    if peak is None:
        peak = fe.peak(d_ptr, n, st)
    _limit_device(fe, d_ptr, n, peak, 0.95, st)


# ---- the reference's names --------------------------------------------------------------------

def boost_quiet(audio):
    """core/asr_engine.py:512-516: a signal whose peak is in (0, 0.5) becomes
    audio / peak * 0.95 (numpy's two float32 roundings); any other comes back unchanged."""
    d, was_tensor = _to_device(audio)
    if d.numel():
        _boost_quiet_device(front_end(), d.data_ptr(), d.numel(), _stream())
    return _back(d, was_tensor)


def compute_segment_rms(audio_segment) -> float:
    """core/audio_preprocessing.py:39-43, the sum of squares taken on the GPU in float64."""
    if len(audio_segment) == 0:
        return 0.0
    d, _ = _to_device(audio_segment)
    n = d.numel()
    return _rms_of(front_end().segment_sumsq(d.data_ptr(), n, [0], [n], _stream())[0], n)


def per_segment_rms_normalize(audio, vad_segments, sample_rate=16000, min_segment_ms=100,
                              max_gain_db=20.0, crossfade_ms=5):
    """core/audio_preprocessing.py:46-140."""
    if len(vad_segments) == 0:
        return audio
    d, was_tensor = _to_device(audio)
    done = _normalize_device(front_end(), d.data_ptr(), d.numel(), vad_segments, sample_rate,
                             min_segment_ms, max_gain_db, crossfade_ms, _stream())
    return audio if done is None else _back(d, was_tensor)


def adaptive_peak_limit(audio, target_peak=0.95):
    """core/audio_preprocessing.py:226-243."""
    d, was_tensor = _to_device(audio)
    n = d.numel()
    if n == 0:
        return audio
    fe, st = front_end(), _stream()
    peak = fe.peak(d.data_ptr(), n, st)
    if not peak > target_peak:
        return audio
    _limit_device(fe, d.data_ptr(), n, peak, target_peak, st)
    return _back(d, was_tensor)


def preprocess_audio(audio, vad_segments, sample_rate=16000, enable_rms_normalize=True,
                     progress_callback=None):
    """core/audio_preprocessing.py:250-293: per-segment RMS normalisation (when enabled and
    there are segments), then the peak limiter; always a new array, as the reference's copy."""
    def emit(msg):
        if progress_callback:
            progress_callback(msg)

    d, was_tensor = _to_device(audio)
    if enable_rms_normalize and len(vad_segments) > 0:
        emit("PHASE:Preprocess|Đang chuẩn hóa âm lượng từng đoạn|50")
    condition_device(d.data_ptr(), d.numel(), vad_segments, sample_rate, boost=False,
                     enable_rms_normalize=enable_rms_normalize)
    emit("PHASE:Preprocess|Preprocessing hoàn tất|100")
    return _back(d, was_tensor)


# ---- WPE dereverberation (core/audio_preprocessing.py:157-216) -----------------

WPE_FFT, WPE_HOP, WPE_MAX_SAMPLES = 512, 128, 60 * 16000


def _check_wpe(sample_rate, fft_size, hop_size, taps, delay, iterations) -> None:
    if int(fft_size) != WPE_FFT or int(hop_size) != WPE_HOP:
        raise ValueError("the device WPE supports fft_size=512, hop_size=128 only")
    if int(sample_rate) != 16000:
        raise ValueError("the device WPE runs on the 16 kHz signal")
    if not 1 <= int(taps) <= 16:
        raise ValueError("taps must be in 1..16")
    if not 1 <= int(delay) <= 16:
        raise ValueError("delay must be in 1..16")
    if not 1 <= int(iterations) <= 8:
        raise ValueError("iterations must be in 1..8")


def apply_wpe_batch(signal, spans, sample_rate=16000, fft_size=512, hop_size=128, taps=10, delay=3,
                    iterations=3, peak_limit: bool = False, device_out: bool = False,
                    target_peak=0.95):
    """apply_wpe_dereverberation on signal[start:end] for every (start, end) of spans, all in
    one device call; signal is numpy or a torch CUDA tensor (float32, mono).  A chunk's result
    is bit-identical to running it alone.  peak_limit applies adaptive_peak_limit
    (core/audio_preprocessing.py:226-243) to every chunk afterwards, on the device, bit-identical
    to zasr.audio.adaptive_peak_limit on that chunk.  Returns the list of float32 arrays (CUDA
    tensors for a tensor input), or with device_out (packed float32 CUDA tensor, int64 offsets
    [len(spans) + 1]): chunk c is packed[offsets[c]:offsets[c + 1]]."""
    torch = _torch()
    _check_wpe(sample_rate, fft_size, hop_size, taps, delay, iterations)
    tensor_in = _is_tensor(signal)
    if tensor_in:
        if not signal.is_cuda:
            raise ValueError("a torch input must be a CUDA tensor")
        d = signal.to(torch.float32).contiguous()
    else:
        a = np.ascontiguousarray(signal, np.float32)
        if a.ndim != 1:
            raise ValueError("audio must be mono: shape [n]")
        d = torch.from_numpy(a).cuda()
    if d.ndim != 1:
        raise ValueError("audio must be mono: shape [n]")
    total = int(d.numel())
    spans = [(int(s), int(e)) for s, e in spans]
    for s, e in spans:
        if s < 0 or e < s or e > total:
            raise ValueError(f"span ({s}, {e}) outside the signal of {total} samples")
        if e - s > WPE_MAX_SAMPLES:
            raise ValueError("a chunk is at most 60 s (960000 samples)")
    lens = np.array([e - s for s, e in spans], np.int64)
    offsets = np.zeros(len(spans) + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    packed = torch.empty(max(int(offsets[-1]), 1), dtype=torch.float32, device=d.device)
    st = _stream()
    if spans:
        wpe_engine().run_device(d.data_ptr(), total, [s for s, _ in spans], lens, packed.data_ptr(),
                                offsets[:-1], taps, delay, iterations, st)
        if peak_limit:
            fe = front_end()
            for c in range(len(spans)):
                n = int(lens[c])
                if n == 0:
                    continue
                ptr = packed.data_ptr() + 4 * int(offsets[c])
                peak = fe.peak(ptr, n, st)
                if peak > target_peak:
                    _limit_device(fe, ptr, n, peak, target_peak, st)
    packed = packed[:int(offsets[-1])]
    if device_out:
        return packed, offsets
    chunks = [packed[int(offsets[c]):int(offsets[c + 1])] for c in range(len(spans))]
    if tensor_in:
        return [c.clone() for c in chunks]
    host = packed.cpu().numpy()
    return [host[int(offsets[c]):int(offsets[c + 1])].copy() for c in range(len(spans))]


def apply_wpe_dereverberation(audio, sample_rate=16000, fft_size=512, hop_size=128, taps=10,
                              delay=3, iterations=3):
    """core/audio_preprocessing.py:157-216, per frequency bin.  numpy in, numpy
    float32 out; a torch CUDA tensor in, one out.  A signal under 2 * fft_size samples comes
    back as the same object (:188-189)."""
    _check_wpe(sample_rate, fft_size, hop_size, taps, delay, iterations)
    n = int(audio.shape[0]) if hasattr(audio, "shape") else len(audio)
    if n < 2 * int(fft_size):
        return audio
    return apply_wpe_batch(audio, [(0, n)], sample_rate, fft_size, hop_size, taps, delay,
                           iterations)[0]


AUDIO_NAMES = ("compute_segment_rms", "per_segment_rms_normalize", "adaptive_peak_limit",
               "preprocess_audio")
