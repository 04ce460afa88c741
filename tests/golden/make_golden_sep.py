"""Writes tests/golden/sep_cases.json: the reference's own OverlapSeparator host methods
(core/overlap_separator.py) run on the synthetic layouts of tests/sep_host_stubs.py, for
tests/test_overlap_host.py.

    python tests/golden/make_golden_sep.py /path/to/reference

The reference is imported here only (its module imports numpy alone at module level).  The
static methods and the audio builders run as they are.  process() runs with the two things that
need a model replaced on the instance: compute_embedding by sep_host_stubs.fake_embedding, and
the onnxruntime session by an object whose run() returns sep_host_stubs.fake_separation -- so
separate_region's own crop, peak rescale, skip rules and scipy assignment are the reference's
text.  Only data is recorded: lists, floats, and per audio array its length, sha256 and a few
samples.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sep_host_stubs as H  # noqa: E402


class _Session:
    def run(self, names, feeds):
        x = feeds["mixture"]
        assert x.ndim == 2 and x.shape[0] == 1 and x.dtype == np.float32
        return [H.fake_separation(x[0])[None]]


def main(ref_root: str) -> None:
    sys.path.insert(0, ref_root)
    from core.overlap_separator import OverlapSeparator

    sep = OverlapSeparator(campp_onnx_path="unused", convtasnet_onnx_path="unused")
    sep.compute_embedding = H.fake_embedding
    sep._init_convtasnet = lambda: None
    sep._convtasnet = _Session()
    audio = H.make_audio(H.FILE_SEC, H.SILENT)
    out = {"constants": {"fade_n": sep.fade_n, "context_samples": sep.context_samples}}

    probes = list(H.OVERLAPS) + [(0.0, 4.0), (5.0, 5.0), (10.0, 10.5), (19.8, 20.0), (39.0, 45.0)]
    out["participants"] = [
        {"region": list(r), "dicts": OverlapSeparator.participants_in_region(r, H.SEGMENTS),
         "objects": OverlapSeparator.participants_in_region(r, [H.SegObj(s) for s in H.SEGMENTS])}
        for r in probes]

    closest = []
    for spk in (0, 1, 2, 3, 7):
        for t in (0.0, 4.0, 5.0, 8.0, 10.0, 14.0, 19.0, 19.8, 30.0, 33.0, 34.5, 35.7, 36.0, 50.0):
            for direction in ("before", "after"):
                for regions in (H.OVERLAPS, []):
                    r = OverlapSeparator._closest_clean_segment(H.FILE_SEC, H.SEGMENTS, regions, spk,
                                                                t, direction)
                    closest.append({"spk": spk, "t": t, "direction": direction,
                                    "with_overlaps": bool(regions),
                                    "result": None if r is None else list(r)})
    assert any(c["result"] is None for c in closest) and any(c["result"] for c in closest)
    out["closest"] = closest

    fades = []
    for lens in ([], [1000], [100, 500], [1000, 240, 1000], [1000, 241, 1000], [500, 100, 239, 700],
                 [241, 241], [240, 240]):
        chunks = [H.make_audio(40.0)[1000 * (i + 1):1000 * (i + 1) + n] for i, n in enumerate(lens)]
        fades.append({"lens": lens, "out": H.describe(sep._concat_with_fade(chunks))})
    out["concat_with_fade"] = fades

    ctx = []
    for region in ((4.0, 5.0), (34.5, 35.7), (16.0, 18.0), (22.0, 23.5)):
        for spk in (0, 1, 2, 3):
            a_s, a_e = int(region[0] * H.SR), int(region[1] * H.SR)
            separated = (audio[a_s:a_e] * np.float32(0.5)).astype(np.float32)
            res, rs, re = sep.build_context_audio(audio, H.FILE_SEC, H.SEGMENTS, H.OVERLAPS, region,
                                                  spk, separated)
            ctx.append({"region": list(region), "spk": spk, "real_start": rs, "real_end": re,
                        "out": H.describe(res)})
    assert any(c["real_start"] == 0.0 for c in ctx) and any(c["real_start"] > 0.0 for c in ctx)
    assert any(0.0 < c["real_start"] < 0.015 for c in ctx)   # the 160-sample context (< fade)
    out["build_context_audio"] = ctx

    words = [{"word": "a", "start": 0.0, "end": 0.4}, {"word": "b", "start": 0.9, "end": 1.1},
             {"text": "c", "start": 1.0, "end": 1.0}, {"word": "d", "start": 2.9, "end": 3.1},
             {"word": "e", "start": 3.0, "end": 3.2, "conf": 0.5}, {"word": "f", "start": 5.0},
             {"word": "g", "end": 2.0}]
    out["filter_words"] = {"words": words, "cases": [
        {"args": list(a), "result": OverlapSeparator.filter_words_in_window(words, *a)}
        for a in ((1.0, 3.0), (1.0, 3.0, 12.5), (0.0, 10.0, -1.0), (4.0, 4.5), (5.0, 5.0, 2.0))]}

    runs = {}
    for name, segments, regions in (
            ("dicts", H.SEGMENTS, H.OVERLAPS),
            ("objects", [H.SegObj(s) for s in H.SEGMENTS], H.OVERLAPS),
            ("none", H.SEGMENTS, []),
            ("all_short", H.SEGMENTS, [(13.2, 13.9), (17.0, 17.6)]),
            ("reversed", H.SEGMENTS, list(reversed(H.OVERLAPS)))):
        seen = []
        res = sep.process(audio, segments, regions, progress_callback=seen.append)
        runs[name] = [{
            "start": r["start"], "end": r["end"], "participants": r["participants"],
            "speakers": [int(k) for k in r["audio_per_speaker"]],
            "audio": {str(k): H.describe(v) for k, v in r["audio_per_speaker"].items()},
            "real_start": {str(k): v for k, v in r["real_start_per_speaker"].items()},
            "real_end": {str(k): v for k, v in r["real_end_per_speaker"].items()},
        } for r in res]
    # of the six regions: one under 1 s, one with three participants, one without a centroid,
    # one silent -> two results
    assert len(runs["dicts"]) == 2 and runs["none"] == [] and runs["all_short"] == []
    out["process"] = runs

    path = os.path.join(HERE, "sep_cases.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, ensure_ascii=False)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
