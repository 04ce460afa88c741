"""Overlap speaker separation host logic: the behaviour of the reference's
OverlapSeparator (core/overlap_separator.py) restated on arrays, with the Conv-TasNet forward
pass on the MI355X (zasr.binding.SepSession) and the CAM++ embeddings from the session the
diarizer already holds (zasr.binding.CamppEmbedder).

Structure.  A file's diarization segments are read once into a `SegmentTable` (start, end and
speaker columns); one interval test, `SegmentTable.touching`, answers every "does this segment
meet one of these regions" question of the stage -- who takes part in a region, which segments
are clean enough for a centroid, which clean segment lies next to a region -- as a mask over the
table.  Sample bounds come from one helper (`sample_span`), the context audio from a span
plan (`context_spans`) and a join (`join_with_fades`).  `OverlapSeparator` keeps the reference's
constants, method names and return shapes on top of these, so it is a drop-in; what its methods
return is pinned to lists recorded from the reference (tests/golden/sep_cases.json).

`process` collects every eligible region and separates them in ONE device call, where the
reference makes one onnxruntime call per region (:470).

Differences from the reference, stated once:
  * compute_embedding uses the embedder's own front end (the diarizer's fbank, which snips
    edges: 1 + (n - 400) // 160 frames) where the reference uses kaldi-native-fbank with
    snip_edges=False (:90-98, about n / 160 frames); the < 0.3 s and < 10 frames -> None rules
    (:129, :135) are kept.
  * the 2 x 2 stream-to-speaker assignment is scipy.optimize.linear_sum_assignment (:323)
    followed by hand into a closed form, ties included, so scipy is not needed.
"""
from __future__ import annotations

from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

SAMPLE_RATE = 16000
CONTEXT_SEC_DEFAULT = 3.0
MIN_REGION_SEC = 0.4     # core/overlap_separator.py:34
MIN_REF_SEC = 1.0        # :35
MIN_OVERLAP_SEC = 1.0    # :36
FADE_MS = 15             # :40

Region = Tuple[float, float]


# ---------------------------------------------------------------------------- tables and spans
class SegmentTable:
    """Columns of a segment list: dicts with 'start' / 'end' / 'speaker' or objects with those
    attributes; a missing start is 0, a missing end the start, a missing speaker -1."""

    def __init__(self, segments: Iterable[Any]):
        rows = [self._row(s) for s in segments]
        self.start = np.array([r[0] for r in rows], np.float64)
        self.end = np.array([r[1] for r in rows], np.float64)
        self.speaker = np.array([r[2] for r in rows], np.int64)

    @staticmethod
    def _row(seg) -> Tuple[float, float, int]:
        read = seg.get if isinstance(seg, dict) else (lambda k, d=None: getattr(seg, k, d))
        start = float(read("start", 0))
        return start, float(read("end", start)), int(read("speaker", -1))

    @classmethod
    def of(cls, segments) -> "SegmentTable":
        return segments if isinstance(segments, cls) else cls(segments)

    def touching(self, regions: Sequence[Region]) -> np.ndarray:
        """Mask of the segments that share more than a point with at least one region:
        max(start, r0) < min(end, r1).  Touching edges do not count."""
        if len(self.start) == 0 or len(regions) == 0:
            return np.zeros(len(self.start), bool)
        r = np.asarray(regions, np.float64).reshape(-1, 2)
        lo = np.maximum(self.start[:, None], r[None, :, 0])
        hi = np.minimum(self.end[:, None], r[None, :, 1])
        return (lo < hi).any(axis=1)

    def clean(self, regions: Sequence[Region]) -> np.ndarray:
        return ~self.touching(regions)


def sample_span(t0: float, t1: float, n_samples: int) -> Tuple[int, int]:
    """[t0, t1) seconds as sample indices, the end clamped to the file."""
    return int(t0 * SAMPLE_RATE), min(int(t1 * SAMPLE_RATE), n_samples)


def assign_2x2(cost: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """linear_sum_assignment of a 2 x 2 cost matrix in closed form: rows (0, 1) and their
    columns.  scipy's shortest-augmenting-path solver, followed by hand for two rows: row 0 first
    takes its cheaper column a (column 0 on a tie); row 1 takes the other column b when that is
    no dearer for it than a; otherwise row 1 gets a and row 0 moves to b only if that is
    strictly cheaper in the solver's own arithmetic, (c1a + c0b) - c0a < c1b.  So on a tie of
    the two permutations row 0 keeps its cheaper column, which need not be the identity."""
    c = np.asarray(cost, dtype=np.float64)
    if c.shape != (2, 2):
        raise ValueError("cost must be 2 x 2")
    a = 1 if c[0, 1] < c[0, 0] else 0
    b = 1 - a
    if c[1, b] > c[1, a] and (c[1, a] + c[0, b]) - c[0, a] < c[1, b]:
        a, b = b, a
    return np.array([0, 1]), np.array([a, b])


def neighbour_segment(table: SegmentTable, regions: Sequence[Region], spk: int, t: float,
                      direction: str) -> Optional[Region]:
    """The speaker's clean segment next to time t: ending at or before t with the latest end
    ('before'), or starting at or after t with the earliest start ('after'); the first such
    segment in list order when several tie."""
    ok = (table.speaker == spk) & table.clean(regions)
    if direction == "before":
        ok &= table.end <= t
        key = table.end
    elif direction == "after":
        ok &= table.start >= t
        key = -table.start
    else:
        return None
    idx = np.flatnonzero(ok)
    if idx.size == 0:
        return None
    i = idx[np.argmax(key[idx])]
    return float(table.start[i]), float(table.end[i])


def context_spans(table: SegmentTable, regions: Sequence[Region], region: Region, spk: int,
                  context_sec: float, n_samples: int) -> Tuple[Optional[Tuple[int, int]],
                                                               Optional[Tuple[int, int]]]:
    """Sample spans of the speaker's clean audio to put before and after a separated region:
    the last context_sec of the clean segment before it, the first context_sec of the one
    after; None where there is no such segment or nothing of it lies inside the file."""
    spans: List[Optional[Tuple[int, int]]] = []
    before = neighbour_segment(table, regions, spk, region[0], "before")
    after = neighbour_segment(table, regions, spk, region[1], "after")
    if before is not None:
        before = (max(before[0], before[1] - context_sec), before[1])
    if after is not None:
        after = (after[0], min(after[1], after[0] + context_sec))
    for seg in (before, after):
        span = None if seg is None else sample_span(seg[0], seg[1], n_samples)
        spans.append(span if span is not None and span[1] > span[0] else None)
    return spans[0], spans[1]


def join_with_fades(pieces: Sequence[np.ndarray], fade_n: int) -> np.ndarray:
    """Concatenation with linear ramps at the inner joints: a piece longer than fade_n samples
    fades in over its first fade_n samples unless it is the first piece, and out over its last
    fade_n unless it is the last.  Shorter pieces are joined as they are."""
    if len(pieces) == 0:
        return np.zeros(0, np.float32)
    out = np.concatenate([np.asarray(p).astype(np.float32) for p in pieces])
    if len(pieces) == 1:
        return out
    up = np.linspace(0, 1, fade_n, dtype=np.float32)
    down = np.linspace(1, 0, fade_n, dtype=np.float32)
    edges = np.cumsum([0] + [len(p) for p in pieces])
    last = len(pieces) - 1
    for k, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        if hi - lo <= fade_n:
            continue
        if k > 0:
            out[lo:lo + fade_n] *= up
        if k < last:
            out[hi - fade_n:hi] *= down
    return out


def scale_to_mixture(ests: np.ndarray, mixture: np.ndarray) -> Optional[np.ndarray]:
    """The network's streams cropped to the mixture's length and each brought to 0.9 of the
    mixture's peak (its output scale is arbitrary); None for a silent mixture (peak < 1e-6).
    A stream that is all zeros stays as it is."""
    streams = np.array(ests, np.float32)[..., :len(mixture)]
    mix_peak = float(np.abs(mixture).max())
    if mix_peak < 1e-6:
        return None
    for row in streams:
        peak = float(np.abs(row).max())
        if peak > 0:
            row *= np.float32(mix_peak * 0.9 / peak)
    return streams


# ---------------------------------------------------------------------------- the separator
class OverlapSeparator:
    """Per-region separation of two-speaker overlaps (core/overlap_separator.py:43).

    sep: a zasr.binding.SepSession (or any object with separate(list of arrays) -> list of
    [2, T]); embedder: a zasr.binding.CamppEmbedder (fbank(audio) -> [frames, 80],
    embed(feats [N, T, 80]) -> [N, dim])."""

    def __init__(self, sep, embedder, context_sec: float = CONTEXT_SEC_DEFAULT):
        self.sep = sep
        self.embedder = embedder
        # (device pointer, samples) of the same 16 kHz signal in HBM, when the caller has one:
        # process() then cuts the regions there (SepSession.separate_device; same bits)
        self.device_audio: Optional[Tuple[int, int]] = None
        self.context_sec = context_sec
        self.context_samples = int(context_sec * SAMPLE_RATE)
        self.fade_n = int(FADE_MS / 1000.0 * SAMPLE_RATE)

    # ---- embeddings ----
    def compute_embedding(self, audio: np.ndarray) -> Optional[np.ndarray]:
        """Unit-norm CAM++ embedding of a stretch of audio; None under 0.3 s or 10 frames."""
        if len(audio) < int(0.3 * SAMPLE_RATE):
            return None
        feats = np.asarray(self.embedder.fbank(np.asarray(audio, np.float32)), np.float32)
        if feats.shape[0] < 10:
            return None
        feats = feats - feats.mean(axis=0, keepdims=True)
        emb = np.asarray(self.embedder.embed(feats[None, :, :])[0])
        norm = np.linalg.norm(emb)
        return (emb / norm if norm > 1e-10 else emb).astype(np.float32)

    def compute_centroids(self, audio: np.ndarray, segments: Sequence[Any],
                          overlap_regions: Sequence[Region]) -> Dict[int, np.ndarray]:
        """Per speaker, the normalised mean embedding of its labelled segments of at least
        MIN_REF_SEC that meet no overlap region."""
        table = SegmentTable.of(segments)
        usable = ((table.speaker >= 0) & ~((table.end - table.start) < MIN_REF_SEC)
                  & table.clean(overlap_regions))
        per_speaker: Dict[int, List[np.ndarray]] = {}
        for i in np.flatnonzero(usable):
            lo, hi = sample_span(table.start[i], table.end[i], len(audio))
            emb = self.compute_embedding(audio[lo:hi])
            if emb is not None:
                per_speaker.setdefault(int(table.speaker[i]), []).append(emb)
        centroids: Dict[int, np.ndarray] = {}
        for spk, embs in per_speaker.items():
            mean = np.stack(embs).mean(axis=0)
            norm = np.linalg.norm(mean)
            centroids[spk] = (mean / norm if norm > 1e-10 else mean).astype(np.float32)
        return centroids

    # ---- who and where ----
    @staticmethod
    def participants_in_region(region: Region, segments: Sequence[Any]) -> List[int]:
        table = SegmentTable.of(segments)
        inside = table.touching([region]) & (table.speaker >= 0)
        return np.unique(table.speaker[inside]).tolist()

    @staticmethod
    def _closest_clean_segment(audio_len_sec: float, segments: Sequence[Any],
                               overlap_regions: Sequence[Region], spk: int, target_t: float,
                               direction: str) -> Optional[Region]:
        return neighbour_segment(SegmentTable.of(segments), overlap_regions, spk, target_t,
                                 direction)

    # ---- one region ----
    @staticmethod
    def _mixture(audio: np.ndarray, region: Region, participants: Sequence[int],
                 centroids: Dict[int, np.ndarray]) -> Optional[Tuple[int, np.ndarray]]:
        """(first sample, samples) of a region that can be separated: exactly two
        participants, both with a centroid, at least MIN_REGION_SEC long in seconds and in
        samples inside the file; else None."""
        if len(participants) != 2 or any(p not in centroids for p in participants):
            return None
        if region[1] - region[0] < MIN_REGION_SEC:
            return None
        lo, hi = sample_span(region[0], region[1], len(audio))
        mix = audio[lo:hi]
        return None if len(mix) < int(MIN_REGION_SEC * SAMPLE_RATE) else (lo, mix)

    @staticmethod
    def assignment_cost(e0, e1, centroids, ps) -> np.ndarray:
        """Cosine distance of stream (row) to participant centroid (column)."""
        return np.array([[1.0 - float(e @ centroids[p]) for p in ps] for e in (e0, e1)])

    def _streams_by_speaker(self, mix: np.ndarray, ests: np.ndarray, participants: Sequence[int],
                            centroids: Dict[int, np.ndarray]) -> Optional[Dict[int, np.ndarray]]:
        """Raw network output -> {speaker: stream}: rescaled to the mixture, then given to the
        participants by embedding distance (in stream order when a stream is too short to embed)."""
        streams = scale_to_mixture(ests, mix)
        if streams is None:
            return None
        ps = list(participants)
        embs = [self.compute_embedding(s) for s in streams]
        if any(e is None for e in embs):
            return dict(zip(ps, streams))
        rows, cols = assign_2x2(self.assignment_cost(embs[0], embs[1], centroids, ps))
        return {ps[int(c)]: streams[int(r)] for r, c in zip(rows, cols)}

    def separate_region(self, audio: np.ndarray, region: Region, participants: Sequence[int],
                        centroids: Dict[int, np.ndarray]) -> Optional[Dict[int, np.ndarray]]:
        found = self._mixture(audio, region, participants, centroids)
        if found is None:
            return None
        mix = found[1]
        ests = self.sep.separate([mix.astype(np.float32)])[0]
        return self._streams_by_speaker(mix, ests, participants, centroids)

    # ---- context audio for the second decode ----
    def build_context_audio(self, audio: np.ndarray, audio_len_sec: float, segments: Sequence[Any],
                            overlap_regions: Sequence[Region], region: Region, spk: int,
                            separated: np.ndarray) -> Tuple[np.ndarray, float, float]:
        """(clean context + separated + clean context, and where the separated part starts and
        ends in it, in seconds)."""
        before, after = context_spans(SegmentTable.of(segments), overlap_regions, region, spk,
                                      self.context_sec, len(audio))
        pieces = [audio[s[0]:s[1]] for s in (before,) if s is not None]
        pieces.append(separated.astype(np.float32))
        pieces += [audio[s[0]:s[1]] for s in (after,) if s is not None]
        real_start = 0.0 if before is None else (before[1] - before[0]) / SAMPLE_RATE
        real_end = real_start + len(separated) / SAMPLE_RATE
        return self._concat_with_fade(pieces), real_start, real_end

    def _concat_with_fade(self, chunks: List[np.ndarray]) -> np.ndarray:
        return join_with_fades(chunks, self.fade_n)

    # ---- all regions of a file ----
    def _separate_all(self, audio: np.ndarray, jobs: Sequence[Tuple[int, np.ndarray]]):
        if not jobs:
            return []
        if self.device_audio is not None and len(audio) == self.device_audio[1]:
            ptr, total = self.device_audio
            return self.sep.separate_device(ptr, total, [lo for lo, _ in jobs],
                                            [len(mix) for _, mix in jobs])
        return self.sep.separate([mix.astype(np.float32) for _, mix in jobs])

    def process(self, audio: np.ndarray, segments: Sequence[Any],
                overlap_regions: Sequence[Region], progress_callback=None) -> List[Dict]:
        """Per separated region: {'start', 'end', 'participants', 'audio_per_speaker',
        'real_start_per_speaker', 'real_end_per_speaker'}.  Regions under MIN_OVERLAP_SEC
        (backchannels) are dropped first and count as clean audio from then on."""
        def report(pct):
            if progress_callback is not None:
                try:
                    progress_callback(pct)
                except Exception:
                    pass

        regions = [r for r in (overlap_regions or []) if (r[1] - r[0]) >= MIN_OVERLAP_SEC]
        if not regions:
            return []
        table = SegmentTable.of(segments)
        centroids = self.compute_centroids(audio, table, regions)
        picked = []
        for region in regions:
            who = self.participants_in_region(region, table)
            found = self._mixture(audio, region, who, centroids)
            if found is not None:
                picked.append((region, who, found))
        report(0)
        outputs = self._separate_all(audio, [found for _, _, found in picked])
        results: List[Dict] = []
        for k, ((region, who, (_, mix)), ests) in enumerate(zip(picked, outputs)):
            report(int(k / max(1, len(picked)) * 100))
            streams = self._streams_by_speaker(mix, ests, who, centroids)
            if streams is None:
                continue
            built = {spk: self.build_context_audio(audio, len(audio) / SAMPLE_RATE, table, regions,
                                                   region, spk, s) for spk, s in streams.items()}
            results.append({
                "start": region[0], "end": region[1], "participants": who,
                "audio_per_speaker": {spk: b[0] for spk, b in built.items()},
                "real_start_per_speaker": {spk: b[1] for spk, b in built.items()},
                "real_end_per_speaker": {spk: b[2] for spk, b in built.items()},
            })
        report(100)
        return results

    # ---- words of the second decode inside the overlap window ----
    @staticmethod
    def filter_words_in_window(words: Sequence[Dict], real_start: float, real_end: float,
                               real_offset: float = 0.0) -> List[Dict]:
        """Copies of the words whose midpoint lies in [real_start, real_end], shifted by
        real_offset (a missing start is 0, a missing end the start)."""
        def times(w):
            t0 = float(w.get("start", 0))
            return t0, float(w.get("end", t0))
        spans = [times(w) for w in words]
        return [{**w, "start": t0 + real_offset, "end": t1 + real_offset}
                for w, (t0, t1) in zip(words, spans) if real_start <= (t0 + t1) / 2.0 <= real_end]


def overlap_segments(results: Sequence[Dict], decode_fn: Callable[[np.ndarray], Sequence[Dict]],
                     speaker_name: Callable[[int], str] = lambda spk: f"Người nói {spk + 1}"
                     ) -> List[Dict]:
    """The parallel segments of core/asr_engine.py:2789-2830 from process()'s results: each
    per-speaker audio is decoded with decode_fn(audio float32) -> words ({'word' | 'text',
    'start', 'end'} in seconds of that audio); the words whose midpoint lies in the separated
    part are kept and moved to file time.  A decode that raises, or leaves no word or no text,
    gives no segment for that speaker."""
    def text_of(words):
        tokens = [(w.get("word") or w.get("text") or "") for w in words]
        return " ".join(t.strip() for t in tokens if t).strip()

    out: List[Dict] = []
    for reg in results:
        for spk, spk_audio in reg["audio_per_speaker"].items():
            window = reg["real_start_per_speaker"][spk], reg["real_end_per_speaker"][spk]
            try:
                words = decode_fn(spk_audio.astype(np.float32))
            except Exception:
                continue
            kept = OverlapSeparator.filter_words_in_window(words, window[0], window[1],
                                                           reg["start"] - window[0])
            text = text_of(kept) if kept else ""
            if text:
                out.append({"speaker": speaker_name(int(spk)), "speaker_id": int(spk),
                            "start": reg["start"], "end": reg["end"], "text": text,
                            "raw_words": kept, "overlap": True})
    return out
