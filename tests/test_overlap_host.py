"""zasr.overlap reproduces the reference's OverlapSeparator host logic exactly: every list and
audio array tests/golden/make_golden_sep.py recorded from core/overlap_separator.py on the
layouts of tests/sep_host_stubs.py (tests/golden/sep_cases.json), the 2 x 2 assignment against
scipy, and the overlap-segment builder of core/asr_engine.py:2789-2830 on a stub decoder.
No GPU."""
import json
import os

import numpy as np
import pytest

import sep_host_stubs as H
from zasr import overlap as O
from zasr.overlap import OverlapSeparator, assign_2x2, overlap_segments

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "sep_cases.json")))


class _Sep:
    """Stand-in for SepSession: counts the device calls."""

    def __init__(self):
        self.calls = []

    def separate(self, mixtures):
        self.calls.append([len(m) for m in mixtures])
        return [H.fake_separation(m) for m in mixtures]


class _Separator(OverlapSeparator):
    def compute_embedding(self, audio):
        return H.fake_embedding(audio)


@pytest.fixture()
def sep():
    return _Separator(_Sep(), None)


def test_constants():
    assert (O.SAMPLE_RATE, O.CONTEXT_SEC_DEFAULT, O.MIN_REGION_SEC, O.MIN_REF_SEC,
            O.MIN_OVERLAP_SEC, O.FADE_MS) == (16000, 3.0, 0.4, 1.0, 1.0, 15)
    s = OverlapSeparator(None, None)
    assert GOLD["constants"] == {"fade_n": s.fade_n, "context_samples": s.context_samples}
    assert OverlapSeparator(None, None, context_sec=1.5).context_samples == 24000


def test_participants_in_region():
    objs = [H.SegObj(s) for s in H.SEGMENTS]
    for c in GOLD["participants"]:
        r = tuple(c["region"])
        assert OverlapSeparator.participants_in_region(r, H.SEGMENTS) == c["dicts"], r
        assert OverlapSeparator.participants_in_region(r, objs) == c["objects"], r
    got = {tuple(c["region"]): c["dicts"] for c in GOLD["participants"]}
    assert got[(16.0, 18.0)] == [0, 1, 2] and got[(22.0, 23.5)] == [1, 3] and got[(5.0, 5.0)] == []


def test_closest_clean_segment():
    for c in GOLD["closest"]:
        r = OverlapSeparator._closest_clean_segment(
            H.FILE_SEC, H.SEGMENTS, H.OVERLAPS if c["with_overlaps"] else [], c["spk"], c["t"],
            c["direction"])
        assert (None if r is None else list(r)) == c["result"], c


def test_concat_with_fade(sep):
    base = H.make_audio(40.0)
    for c in GOLD["concat_with_fade"]:
        chunks = [base[1000 * (i + 1):1000 * (i + 1) + n] for i, n in enumerate(c["lens"])]
        out = sep._concat_with_fade(chunks)
        assert out.dtype == np.float32 and H.describe(out) == c["out"], c["lens"]


def test_build_context_audio(sep):
    audio = H.make_audio(H.FILE_SEC, H.SILENT)
    for c in GOLD["build_context_audio"]:
        region = tuple(c["region"])
        a_s, a_e = int(region[0] * H.SR), int(region[1] * H.SR)
        separated = (audio[a_s:a_e] * np.float32(0.5)).astype(np.float32)
        out, rs, re = sep.build_context_audio(audio, H.FILE_SEC, H.SEGMENTS, H.OVERLAPS, region,
                                              c["spk"], separated)
        assert (rs, re) == (c["real_start"], c["real_end"]), c
        assert H.describe(out) == c["out"], (c["region"], c["spk"])


def test_filter_words_in_window():
    words = GOLD["filter_words"]["words"]
    for c in GOLD["filter_words"]["cases"]:
        assert OverlapSeparator.filter_words_in_window(words, *c["args"]) == c["result"], c["args"]


@pytest.mark.parametrize("name", ["dicts", "objects", "none", "all_short", "reversed"])
def test_process(sep, name):
    audio = H.make_audio(H.FILE_SEC, H.SILENT)
    segments = [H.SegObj(s) for s in H.SEGMENTS] if name == "objects" else H.SEGMENTS
    regions = {"none": [], "all_short": [(13.2, 13.9), (17.0, 17.6)],
               "reversed": list(reversed(H.OVERLAPS))}.get(name, H.OVERLAPS)
    seen = []
    res = sep.process(audio, segments, regions, progress_callback=seen.append)
    gold = GOLD["process"][name]
    assert len(res) == len(gold)
    for r, g in zip(res, gold):
        assert (r["start"], r["end"], r["participants"]) == (g["start"], g["end"], g["participants"])
        assert [int(k) for k in r["audio_per_speaker"]] == g["speakers"]     # dict order too
        for k, v in r["audio_per_speaker"].items():
            assert v.dtype == np.float32 and H.describe(v) == g["audio"][str(k)]
            assert r["real_start_per_speaker"][k] == g["real_start"][str(k)]
            assert r["real_end_per_speaker"][k] == g["real_end"][str(k)]
    # every eligible region went to the device in ONE call (none when nothing is eligible)
    if gold:
        assert len(sep.sep.calls) == 1 and len(sep.sep.calls[0]) == 3   # two results + the silent region
        assert seen[-1] == 100
    else:
        assert sep.sep.calls == []


def test_separate_region_equals_process(sep):
    """The per-region entry (the reference's own call path) gives what the batched one gives."""
    audio = H.make_audio(H.FILE_SEC, H.SILENT)
    regions = [r for r in H.OVERLAPS if r[1] - r[0] >= O.MIN_OVERLAP_SEC]
    cent = sep.compute_centroids(audio, H.SEGMENTS, regions)
    assert sorted(cent) == [0, 1]
    res = {(r["start"], r["end"]): r for r in sep.process(audio, H.SEGMENTS, H.OVERLAPS)}
    for region in regions:
        parts = sep.participants_in_region(region, H.SEGMENTS)
        one = sep.separate_region(audio, region, parts, cent)
        if region in res:
            for spk, a in one.items():
                ctx, _, _ = sep.build_context_audio(audio, H.FILE_SEC, H.SEGMENTS, regions, region,
                                                    spk, a)
                assert np.array_equal(ctx, res[region]["audio_per_speaker"][spk])
        else:
            assert one is None
    assert sep.separate_region(audio, (4.0, 4.3), [0, 1], cent) is None      # under 0.4 s
    assert sep.separate_region(audio, (4.0, 5.0), [0, 1], {0: cent[0]}) is None


def test_compute_embedding_rules():
    """< 0.3 s and < 10 frames give None; the segment's mean is subtracted, the embedding is
    made at the segment's own frame count and normalised."""
    class Emb:
        def __init__(self, frames=None):
            self.frames, self.seen = frames, None

        def fbank(self, a):
            n = (1 + (len(a) - 400) // 160) if self.frames is None else self.frames
            return np.arange(n * 80, dtype=np.float32).reshape(n, 80)

        def embed(self, feats):
            self.seen = feats
            return np.array([[3.0, 4.0, 0.0]], np.float32)

    e = Emb()
    s = OverlapSeparator(None, e)
    assert s.compute_embedding(np.zeros(4799, np.float32)) is None and e.seen is None
    out = s.compute_embedding(np.zeros(4800, np.float32))
    assert e.seen.shape == (1, 28, 80) and np.allclose(e.seen.mean(axis=1), 0.0, atol=1e-3)
    assert out.dtype == np.float32 and np.allclose(out, [0.6, 0.8, 0.0])
    assert OverlapSeparator(None, Emb(9)).compute_embedding(np.zeros(8000, np.float32)) is None
    assert OverlapSeparator(None, Emb(10)).compute_embedding(np.zeros(8000, np.float32)) is not None


def test_assignment_equals_scipy():
    from scipy.optimize import linear_sum_assignment
    rng = np.random.Generator(np.random.PCG64(5))
    costs = [rng.uniform(0.0, 2.0, size=(2, 2)) for _ in range(500)]
    costs += [np.round(rng.uniform(0.0, 2.0, size=(2, 2)), 1) for _ in range(500)]   # many ties
    costs += [np.array(c, float) for c in ([[0, 0], [0, 0]], [[1, 1], [1, 1]], [[0, 1], [1, 0]],
                                           [[1, 0], [0, 1]], [[0.5, 0.25], [0.75, 0.5]],
                                           [[0.25, 0.5], [0.5, 0.75]], [[2, 1], [1, 0]])]
    ties = 0
    for c in costs:
        r, k = linear_sum_assignment(c)
        r2, k2 = assign_2x2(c)
        assert list(r) == list(r2) and list(k) == list(k2), c
        ties += c[0, 0] + c[1, 1] == c[0, 1] + c[1, 0]
    assert ties >= 20
    with pytest.raises(ValueError):
        assign_2x2(np.zeros((2, 3)))


def test_overlap_segments_on_a_stub_decoder():
    a0, a1 = np.zeros(16000 * 6, np.float32), np.ones(16000 * 4, np.float32)
    results = [{"start": 10.0, "end": 12.0, "participants": [0, 2],
                "audio_per_speaker": {2: a0, 0: a1},
                "real_start_per_speaker": {2: 3.0, 0: 0.0},
                "real_end_per_speaker": {2: 5.0, 0: 2.0}},
               {"start": 30.0, "end": 31.5, "participants": [1, 2],
                "audio_per_speaker": {1: a0[:100], 2: a1[:50]},
                "real_start_per_speaker": {1: 0.0, 2: 0.0},
                "real_end_per_speaker": {1: 1.5, 2: 1.5}}]

    def decode(audio):
        assert audio.dtype == np.float32
        if len(audio) == 100:
            raise RuntimeError("decode failed")          # that speaker's segment is dropped
        if len(audio) == 50:
            return [{"word": "  ", "start": 0.1, "end": 0.2}]          # no text: dropped
        if audio[0] == 0.0:     # speaker 2: context before (3 s) and after
            return [{"word": "ctx", "start": 1.0, "end": 1.5}, {"word": "xin", "start": 2.9, "end": 3.1},
                    {"text": "chào", "start": 4.0, "end": 4.4}, {"word": "after", "start": 5.0, "end": 5.2}]
        return [{"word": "dạ", "start": 0.5, "end": 0.9, "conf": 0.7}, {"word": "late", "start": 2.0, "end": 2.2}]

    segs = overlap_segments(results, decode)
    assert [(s["speaker_id"], s["text"]) for s in segs] == [(2, "xin chào"), (0, "dạ")]
    s2, s0 = segs
    assert set(s2) == {"speaker", "speaker_id", "start", "end", "text", "raw_words", "overlap"}
    assert s2["overlap"] is True and (s2["start"], s2["end"]) == (10.0, 12.0)
    assert s2["speaker"] == "Người nói 3" and s0["speaker"] == "Người nói 1"
    assert [(w["start"], w["end"]) for w in s2["raw_words"]] == [(2.9 + 7.0, 3.1 + 7.0), (4.0 + 7.0, 4.4 + 7.0)]
    assert s0["raw_words"] == [{"word": "dạ", "start": 10.5, "end": 10.9, "conf": 0.7}]
    assert overlap_segments([], decode) == []
    assert overlap_segments(results, decode, speaker_name=lambda k: f"S{k}")[0]["speaker"] == "S2"
