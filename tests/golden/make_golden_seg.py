"""Writes tests/golden/seg_cases.json: the reference's own _pyannote_vad
(core/speaker_diarization_senko_campp_optimized.py:411-517) run on hand-made class maps, for
tests/test_segmentation_host.py.

    python tests/golden/make_golden_seg.py /path/to/reference

The reference is imported here only.  _pyannote_vad is called unbound on a stub `self` whose
seg_sess.run returns one-hot logits of the case's class maps, so the chunking, the powerset
decode, the vote of overlapping chunks and both region builders that run are the reference's own
text.  Per case the JSON holds the total sample count, the chunk starts (its loop restated; the
number of chunks it asked for is checked), the class maps (one string of digits per chunk), the returned
regions and the overlap regions it left in _last_overlap_regions.

A case is a timeline on the OUTPUT frames: spans (first frame, frame after the last, class),
silence elsewhere; every chunk's map is that timeline read at the output frame the reference
assigns to each of its frames (computed here in Python doubles, as it does), so overlapping
chunks agree unless the case flips frames of one chunk on purpose.

Asserted here, so that the cases are what they claim: the run shorter than 0.25 s is dropped;
the gaps of 5 and 6 frames lie on either side of 0.1 s; the overlap runs of 17 and 18 frames
lie on either side of 0.3 s; the disagreement frames have exactly two votes; some frame of a
padded last chunk maps past the last output frame.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SR, CHUNK, STEP, F = 16000, 160000, 80000, 589
D = 10.0 / F

SP = [(40, 160, 1), (300, 420, 2)]
CASES = {
    # totals around one chunk, and longer files; speech / overlap spans on the output timeline
    "t10s_minus1": dict(total=159999, spans=SP),
    "t10s": dict(total=160000, spans=SP),
    "t10s_plus1": dict(total=160001, spans=SP + [(600, 700, 3)]),
    "t15s": dict(total=240000, spans=SP + [(500, 640, 4), (700, 760, 1)]),
    "t17_3s": dict(total=276800, spans=SP + [(600, 900, 5)]),
    "t61s": dict(total=976000, spans=[(10, 200, 1), (250, 900, 6), (1200, 1800, 2), (1800, 2400, 4),
                                      (3000, 3550, 3)]),
    # 14 frames = 0.238 s: dropped; 15 frames = 0.255 s: kept
    "short_run": dict(total=240000, spans=[(100, 114, 1), (300, 315, 1)]),
    # gaps of 5 frames (0.085 s: merged) and 6 frames (0.102 s: not merged)
    "gaps": dict(total=320000, spans=[(100, 200, 1), (205, 300, 2), (500, 600, 1), (606, 700, 3)]),
    # overlap runs of 17 frames (0.289 s: dropped) and 18 frames (0.306 s: kept), inside speech
    "overlap_edge": dict(total=320000, spans=[(100, 200, 1), (200, 217, 4), (217, 400, 2),
                                              (400, 418, 5), (418, 500, 1)]),
    # speech and overlap still open at the end of the file
    "open_end": dict(total=276800, spans=[(50, 150, 1), (900, 2000, 6)]),
    "open_end_exact": dict(total=160000, spans=[(500, 2000, 4)]),
    "open_end_long": dict(total=976000, spans=[(3300, 6000, 5)]),
    "silence": dict(total=400000, spans=[]),
    # frames 330-360 (seen by chunks 0 and 1): chunk 1 says silence -> 1 : 1, ratio 0.5, not speech
    "disagree": dict(total=320000, spans=[(300, 400, 1)], flip=dict(chunk=1, lo=330, hi=360, to=0)),
}


def out_frame(cs, f):
    return int((cs / SR + f * D) / D)


def starts_of(total):
    s, out = 0, []
    while s < total:
        out.append(s)
        if s + CHUNK >= total:
            break
        s += STEP
    return out


def class_maps(case):
    total = case["total"]
    n_out = int((total / SR) / D) + 1
    line = np.zeros(n_out + 2 * F, np.int64)
    for a, b, c in case["spans"]:
        line[a:b] = c
    starts = starts_of(total)
    maps = np.zeros((len(starts), F), np.int64)
    votes = np.zeros(line.shape[0], np.int64)
    past = 0
    for k, cs in enumerate(starts):
        for f in range(F):
            o = out_frame(cs, f)
            maps[k, f] = line[o]
            votes[o] += 1
            past += o >= n_out
    flip = case.get("flip")
    if flip:
        cs = starts[flip["chunk"]]
        for f in range(F):
            o = out_frame(cs, f)
            if flip["lo"] <= o < flip["hi"]:
                assert votes[o] == 2, ("disagreement frame without exactly two votes", o, votes[o])
                maps[flip["chunk"], f] = flip["to"]
    return maps, starts, past


class StubSession:
    def __init__(self, maps):
        self.maps, self.pos = maps, 0

    def run(self, names, feeds):
        x = feeds["input_values"]
        assert x.dtype == np.float32 and x.shape[1:] == (1, CHUNK), x.shape
        n = x.shape[0]
        m = self.maps[self.pos:self.pos + n]
        self.pos += n
        logits = np.full((n, F, 7), -20.0, np.float32)
        np.put_along_axis(logits, m[..., None], 0.0, axis=-1)
        return [logits]


def main(ref_root):
    sys.path.insert(0, ref_root)
    from core import speaker_diarization_senko_campp_optimized as ref
    assert 14 * D < 0.25 <= 15 * D and 5 * D < 0.1 <= 6 * D and 17 * D < 0.3 <= 18 * D
    doc, any_past = {}, False
    for name, case in CASES.items():
        maps, starts, past = class_maps(case)
        any_past = any_past or past > 0
        stub = types.SimpleNamespace(seg_sess=StubSession(maps), _last_overlap_regions=[])
        audio = np.zeros(case["total"], np.float32)
        regions = ref.SenkoCamppDiarizerOptimized._pyannote_vad(stub, audio, SR)
        assert stub.seg_sess.pos == len(starts), name
        doc[name] = dict(total=case["total"], starts=starts,
                         classes=["".join(map(str, row)) for row in maps.tolist()],
                         regions=[list(map(float, r)) for r in regions],
                         overlap_regions=[list(map(float, r)) for r in stub._last_overlap_regions],
                         frames_past_end=int(past))
        print(name, "chunks", len(starts), "regions", regions, "overlap", stub._last_overlap_regions,
              "past", past)
    assert any_past, "no frame maps past the last output frame"
    r = doc["short_run"]["regions"]
    assert len(r) == 1 and r[0][0] == 300 * D, r
    assert len(doc["gaps"]["regions"]) == 3, doc["gaps"]["regions"]
    assert len(doc["overlap_edge"]["overlap_regions"]) == 1, doc["overlap_edge"]["overlap_regions"]
    assert doc["silence"]["regions"] == [[0.0, 25.0]], doc["silence"]["regions"]
    for k in ("open_end_exact", "open_end_long"):   # runs open at the end are clipped to the file
        assert doc[k]["regions"][-1][1] == doc[k]["total"] / SR, (k, doc[k]["regions"])
        assert doc[k]["overlap_regions"][-1][1] == doc[k]["total"] / SR, (k, doc[k]["overlap_regions"])
    d = doc["disagree"]["regions"]
    assert len(d) == 2 and d[0][1] == 330 * D and d[1][0] == 360 * D, d
    with open(os.path.join(HERE, "seg_cases.json"), "w") as f:
        json.dump(doc, f, indent=0)


if __name__ == "__main__":
    main(sys.argv[1])
