"""zasr.diarize (host logic of the speaker diarization) against the reference's own answers
(tests/golden/diar_cases.*, written by tests/golden/make_golden_diar.py from
core/speaker_diarization_senko_campp_optimized.py).  No GPU: the spectral embedding handed to
the module is numpy.linalg.eigh (tests/diar_inputs.lapack_embed), not the code under test; the
device's embedding goes through the same cases in tests/test_gpu_diar.py."""
import json
import os

import numpy as np
import pytest

from diar_inputs import canonical, case_embeddings, lapack_embed, window_plan

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    doc = json.load(open(os.path.join(GOLD, "diar_cases.json")))
    arr = np.load(os.path.join(GOLD, "diar_cases.npz"))
    return doc, arr


def cluster_kw(case):
    kw = dict(case["kw"])
    kw.pop("cluster_type")
    return kw


CLUSTER = ["c10", "c24", "c33", "c130", "c257", "c1000", "c2048", "minor", "merge", "forced"]
PROCESS = ["s_general", "s_forced", "s_two", "s_seven"]


@pytest.mark.parametrize("name", CLUSTER)
def test_senko_cluster_matches_reference(gold, name):
    """The partition equals the reference's (labels renumbered by first occurrence on both
    sides: k-means numbers its clusters differently), and so does the speaker count."""
    from zasr.diarize import senko_cluster
    doc, arr = gold
    case = doc[name]
    labels = senko_cluster(case_embeddings(case), embed=lapack_embed, **cluster_kw(case))
    want = arr[f"{name}/labels"]
    assert labels.dtype == np.int32 and labels.shape == want.shape
    assert len(np.unique(labels)) == case["speakers"]
    assert canonical(labels) == canonical(want)
    # the relabel leaves 0 .. S-1
    assert sorted(np.unique(labels).tolist()) == list(range(case["speakers"]))


def test_special_cases_reach_their_branch(gold):
    """`minor`: the spectral step leaves a cluster of fewer than 4 windows, which
    filter_minor_cluster reassigns; `merge`: two spectral clusters whose centres merge."""
    from zasr.diarize import senko_cluster, senko_spectral
    doc, _ = gold
    kw = {k: v for k, v in doc["minor"]["kw"].items()
          if k in ("min_num_spks", "max_num_spks", "pval", "oracle_num")}
    sp = senko_spectral(case_embeddings(doc["minor"]), embed=lapack_embed, **kw)
    assert np.bincount(sp).min() < 4
    out = senko_cluster(case_embeddings(doc["minor"]), embed=lapack_embed, **cluster_kw(doc["minor"]))
    assert np.bincount(out).min() >= 4
    kw = {k: v for k, v in doc["merge"]["kw"].items()
          if k in ("min_num_spks", "max_num_spks", "pval", "oracle_num")}
    sp = senko_spectral(case_embeddings(doc["merge"]), embed=lapack_embed, **kw)
    assert len(np.unique(sp)) == 2
    # without the merge the two stay apart
    out = senko_cluster(case_embeddings(doc["merge"]), embed=lapack_embed,
                        **dict(cluster_kw(doc["merge"]), mer_cos=None))
    assert len(np.unique(out)) == 2


@pytest.mark.parametrize("name", PROCESS)
def test_diarize_matches_reference_segments(gold, name):
    """diarize() on the pipe-shaped plan = the reference's process() segment list, exactly
    (window times from the (region, first frame, frames) rows, n_embs <= 2, N < 10, a forced
    speaker count, the midpoint split and 7a-7d)."""
    from zasr.diarize import diarize
    doc, arr = gold
    case = doc[name]
    off, length, rows, duration = window_plan(case["n"], case["seed"])
    assert duration == case["duration"]
    segs, labels = diarize(case_embeddings(case), rows, off, length, duration,
                           num_speakers=case["num_speakers"], embed=lapack_embed,
                           return_labels=True)
    assert segs == case["segments"]
    assert canonical(labels) == canonical(arr[f"{name}/labels"])


def test_segments_from_windows_steps():
    """Each step of the segment logic on hand-made windows (the reference's rules, :622-654,
    :769-819): same-label windows closer than 10 ms join; overlapping neighbours split at the
    midpoint; 7a joins one speaker's segments up to 4 s apart; 7b drops a segment of at most
    0.78 s and bridges it when the same speaker is on both sides; 7c joins what 7b made
    adjacent; 7d ranks speakers by speaking time."""
    from zasr.diarize import segments_from_labels, segments_from_windows
    t = [(0.0, 1.5), (0.6, 2.1), (1.2, 2.7), (1.8, 3.3)]
    assert segments_from_labels(t, [5, 5, 7, 7]) == [
        {"start": 0.0, "end": 2.1, "speaker": 5}, {"start": 1.2, "end": 3.3, "speaker": 7}]
    # midpoint split, then 7d: speaker 7 (1.65 s .. 3.3) and 5 (0 .. 1.65) tie-free by 7's gap
    out = segments_from_windows(t + [(3.31, 4.0)], [5, 5, 7, 7, 7])
    assert out == [{"start": 0.0, "end": 1.65, "speaker": 1},
                   {"start": 1.65, "end": 4.0, "speaker": 0}]
    # 7a joins a gap of 4.0 s; the 4.5 s gap it leaves is joined by 7c, which has no limit
    out = segments_from_windows([(0.0, 1.0), (5.0, 6.0), (10.5, 12.0)], [1, 1, 1])
    assert out == [{"start": 0.0, "end": 12.0, "speaker": 0}]
    # 7b + 7c: the 0.5 s segment of speaker 2 between speaker 1's goes, and 1's become one
    out = segments_from_windows([(0.0, 2.0), (2.0, 2.5), (2.5, 6.0), (6.0, 7.0)], [1, 2, 1, 3])
    assert out == [{"start": 0.0, "end": 6.0, "speaker": 0}, {"start": 6.0, "end": 7.0, "speaker": 1}]
    # 7b without the same speaker on both sides: dropped, nothing bridged
    out = segments_from_windows([(0.0, 2.0), (2.0, 2.5), (2.5, 6.0)], [1, 2, 3])
    assert out == [{"start": 0.0, "end": 2.0, "speaker": 1}, {"start": 2.5, "end": 6.0, "speaker": 0}]
    assert segments_from_windows([], []) == []


def test_window_times():
    from zasr.diarize import window_times
    rows = np.array([[0, 0, 150], [0, 60, 150], [1, 0, 117], [2, 37, 150]])
    off, length = [8000, 100000, 200000], [40000, 19200, 30000]
    got = window_times(rows, off, length)
    assert got == [(0.5, 2.0), (0.5 + 60 * 10.0 / 1000.0, 0.5 + 60 * 10.0 / 1000.0 + 1.5),
                   (6.25, 7.45), (12.5 + 37 * 10.0 / 1000.0, 12.5 + 37 * 10.0 / 1000.0 + 1.5)]


def test_small_and_refused_inputs():
    from zasr.diarize import diarize, kmeans, senko_cluster, senko_spectral
    x = case_embeddings(dict(seed=1, n=12, spk=2, spread=0.3))
    assert senko_spectral(x[:1], embed=lapack_embed).tolist() == [0]
    assert senko_spectral(x[:0], embed=lapack_embed).tolist() == []
    # an empty gap list (min_num_spks - 1 past the eigenvalues) is one speaker
    assert senko_spectral(x, min_num_spks=13, max_num_spks=15, embed=lapack_embed).tolist() == [0] * 12
    assert senko_cluster(x[:9], embed=lapack_embed).tolist() == [1] * 9
    with pytest.raises(ValueError, match="reproducible"):
        senko_cluster(x, cluster_type="umap_hdbscan", embed=lapack_embed)
    with pytest.raises(ValueError):
        senko_spectral(np.zeros((40, 8), np.float32), max_num_spks=20, embed=lapack_embed)
    assert diarize(x, np.zeros((12, 3), np.int64), [0], [16000], 0.3, embed=lapack_embed) == []
    assert diarize(x[:0], np.zeros((0, 3), np.int64), [], [], 9.0, embed=lapack_embed) == []
    # k-means: deterministic, every cluster non-empty, well-separated groups recovered
    p = np.concatenate([np.zeros((5, 2)), np.ones((4, 2)) * 3, np.array([[9.0, 9.0]])])
    a, b = kmeans(p, 3), kmeans(p, 3)
    assert a.tolist() == b.tolist() and canonical(a) == [0] * 5 + [1] * 4 + [2]
    assert sorted(np.unique(kmeans(np.zeros((4, 2)), 3)).tolist()) == [0, 1, 2]
