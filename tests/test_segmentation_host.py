"""Host logic of the segmentation stage (zasr/segmentation.py) against lists the reference's own
_pyannote_vad produced on hand-made class maps (tests/golden/seg_cases.json, written by
tests/golden/make_golden_seg.py), F(T), and the binding's argument checks.  No GPU."""
import json
import os

import numpy as np
import pytest

from zasr.pyannet import PyanNetConfig
from zasr.segmentation import Regions, aggregate, chunk_starts, pyannote_vad

TOTALS = (159999, 160000, 160001, 240000, 276800, 976000)


@pytest.fixture(scope="module")
def cases(golden_dir):
    with open(os.path.join(golden_dir, "seg_cases.json")) as f:
        return json.load(f)


def _maps(case):
    return np.array([[int(ch) for ch in row] for row in case["classes"]], np.uint8)


def test_golden_covers_the_cases(cases):
    assert {c["total"] for c in cases.values()} >= set(TOTALS)
    assert any(c["frames_past_end"] > 0 for c in cases.values())
    assert cases["silence"]["regions"] == [[0.0, 25.0]]
    assert len(cases["gaps"]["regions"]) == 3 and len(cases["overlap_edge"]["overlap_regions"]) == 1
    assert cases["open_end_long"]["regions"][-1][1] == 61.0


def test_aggregate_equals_reference(cases):
    for name, c in cases.items():
        speech, overlap = aggregate(_maps(c), c["starts"], c["total"])
        assert [list(r) for r in speech] == c["regions"], name            # floats compared with ==
        assert [list(r) for r in overlap] == c["overlap_regions"], name
        assert all(type(v) is float for r in speech + overlap for v in r), name


def test_chunk_starts_equal_reference_loop(cases):
    def loop(total, chunk=160000, step=80000):   # :418-424
        starts, s = [], 0
        while s < total:
            starts.append(s)
            if s + chunk >= total:
                break
            s += step
        return starts
    for c in cases.values():
        assert chunk_starts(c["total"]) == c["starts"]
    for total in TOTALS + (1, 79999, 80000, 80001, 239999, 240001, 320000, 57600000):
        assert chunk_starts(total) == loop(total), total
    assert chunk_starts(0) == []


def test_pyannote_vad_through_a_session_stub(cases):
    """pyannote_vad on host audio asks the session for the reference's batches ([n <= 32, 1,
    160000] float32, zero padded) and returns its regions with the overlap regions attached."""
    c = cases["t61s"]
    maps = _maps(c)

    class Stub:
        pos = 0

        def run(self, names, feeds):
            x = feeds["input_values"]
            assert names is None and x.dtype == np.float32 and x.shape[1:] == (1, 160000)
            m = maps[self.pos:self.pos + x.shape[0]]
            self.pos += x.shape[0]
            out = np.full(m.shape + (7,), -20.0, np.float32)
            np.put_along_axis(out, m[..., None].astype(np.int64), 0.0, axis=-1)
            return [out]
    got = pyannote_vad(np.zeros(c["total"], np.float32), Stub())
    assert isinstance(got, Regions) and isinstance(got, list)
    assert [list(r) for r in got] == c["regions"]
    assert [list(r) for r in got.overlap_regions] == c["overlap_regions"]


def test_argmax_ties_take_the_lowest_class():
    """Two chunks, every frame tied between classes 0 and 1 -> class 0 (numpy's argmax, :443):
    all silence, the fall-back region."""
    class Tied:
        def run(self, names, feeds):
            out = np.full((feeds["input_values"].shape[0], 589, 7), -5.0, np.float32)
            out[..., :2] = -1.0
            return [out]
    got = pyannote_vad(np.zeros(200000, np.float32), Tied())
    assert list(got) == [(0.0, 12.5)] and got.overlap_regions == []


@pytest.mark.parametrize("T,stages", [
    (1261, (102, 34, 30, 10, 6, 2)),
    (1530, (128, 42, 38, 12, 8, 2)),
    (1531, (129, 43, 39, 13, 9, 3)),
    (160000, (15975, 5325, 5321, 1773, 1769, 589)),
    (1391, (115, 38, 34, 11, 7, 2)),     # every pool's floor drops 1 frame
    (1521, (128, 42, 38, 12, 8, 2)),     # every pool's floor drops 2 frames
])
def test_num_frames(T, stages):
    """F(T) through the conv chain (frames after conv_0, pool, conv_1, pool, conv_2, pool).  At
    1261 no pool drops a frame, at 1391 each drops 1, at 1521 and 1530 each drops 2."""
    cfg = PyanNetConfig()
    assert cfg.stage_frames(T) == stages
    assert cfg.num_frames(T) == stages[-1]
    assert cfg.num_frames(1260) == 1 and cfg.num_frames(250) == 0


def test_library_num_frames_and_bad_arguments():
    """The C ABI's host-only entries and argument checks need no device."""
    import ctypes as C
    from zasr.binding import load_library
    lib = load_library()
    cfg = PyanNetConfig()
    for T in (0, 250, 251, 1260, 1261, 1530, 1531, 1281, 2461, 160000, 480000):
        assert lib.zasr_seg_num_frames(None, T) == cfg.num_frames(T), T
    for total in (1, 159999, 160000, 160001, 976000, 57600000):
        assert lib.zasr_seg_num_chunks(total, 160000, 80000) == len(chunk_starts(total))
    assert lib.zasr_seg_num_chunks(0, 160000, 80000) == 0
    fp = C.POINTER(C.c_float)
    x = np.zeros(4000, np.float32)
    # shapes are checked before anything touches the device: T < 1261, n <= 0, null pointers
    assert lib.zasr_seg_logits(None, x.ctypes.data_as(fp), 1, 1260, x.ctypes.data_as(fp)) == 1
    assert b"1261" in lib.zasr_last_error()
    assert lib.zasr_seg_logits(None, x.ctypes.data_as(fp), 0, 4000, x.ctypes.data_as(fp)) == 1
    assert b"positive" in lib.zasr_last_error()
    assert lib.zasr_seg_logits(None, x.ctypes.data_as(fp), 1, 4000, x.ctypes.data_as(fp)) == 1
    assert lib.zasr_seg_classes_device(None, None, 10, 1260, 80000, None, None, None) == 1
    assert b"1261" in lib.zasr_last_error()
    assert lib.zasr_seg_classes_device(None, None, 10, 160000, 80000, None, None, None) == 1
    h = C.c_void_p()
    assert lib.zasr_seg_create(None, 0, C.byref(h)) == 1
    assert lib.zasr_seg_set_group(None, 4) == 1
    assert lib.zasr_seg_trim(None) == 1


def test_missing_model_files_are_not_found(tmp_path):
    import ctypes as C
    from zasr.binding import load_library
    lib = load_library()
    h = C.c_void_p()
    assert lib.zasr_seg_create(str(tmp_path / "absent").encode(), 0, C.byref(h)) == 2
    assert b"config.json" in lib.zasr_last_error() and not h.value
