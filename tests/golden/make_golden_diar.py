"""Writes tests/golden/diar_cases.npz and diar_cases.json: the reference's own clustering and
segment logic (core/speaker_diarization_senko_campp_optimized.py) run on the CPU over seeded
window embeddings, for tests/test_diarize_host.py and tests/test_gpu_diar.py.

    python tests/golden/make_golden_diar.py /path/to/reference

The reference is imported here only; the tests read the two files and regenerate the inputs
from each case's parameters (tests/diar_inputs.py).  diar_cases.json holds, per case, the
parameters, the keyword arguments, and for the `process` cases the reference's segment list;
diar_cases.npz holds `<case>/labels` (the reference's labels), `<case>/lambdas` (the 16
smallest eigenvalues of its Laplacian in float64) and `<case>/ambiguous` (the share of rows
whose prune threshold is closer than 1e-5 to the next entry).

`cluster` cases call _senko_cluster with process()'s arguments (:738-746) plus the case's
own; `process` cases call SenkoCamppDiarizerOptimized.process() with its two model methods
(_pyannote_vad, _sliding_window_embeddings) replaced by stubs returning the case's regions,
embeddings and window times and emb_sess set to a placeholder, so the clustering call, the
segment logic and the post-processing that run are the reference's own text.

A case whose seeded input misses a condition below is redrawn with seed + 100, + 200, ...; the
seed that held is the one written to the JSON.

Asserted here, so that a test cannot pass or fail by luck:
  a. no row of any case has an exact tie at its prune threshold;
  b. at most 2 % of a case's rows have their threshold within 1e-5 of the next entry;
  c. natural cases: the reference's largest eigengap is at least 3x its second largest;
  d. sklearn's KMeans gives one partition for random_state 0-4 on the reference's rows;
  e. a case at N <= 32 has two speakers in the reference's answer;
  f. the segment cases' speakers have untied total speaking times;
and the special cases reach their branch: `minor` has a spectral cluster below 4 windows,
`merge` has two spectral clusters and one after merge_by_cos.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from diar_inputs import canonical, case_embeddings, pruned_similarity, window_plan  # noqa: E402

PROCESS_KW = dict(cluster_type="spectral", cluster_line=10, mer_cos=0.875, min_cluster_size=4,
                  min_num_spks=1, max_num_spks=15, pval=0.012)

CASES = {
    # N >= cluster_line, one turn per speaker
    "c10": dict(kind="cluster", seed=11, n=10, spk=2, spread=0.3, turns=[[0, 5], [1, 5]]),
    "c24": dict(kind="cluster", seed=12, n=24, spk=2, spread=0.3, turns=[[0, 12], [1, 12]],
                natural=True),
    "c33": dict(kind="cluster", seed=113, n=33, spk=2, spread=0.3, turns=[[0, 16], [1, 17]],
                natural=True),
    "c130": dict(kind="cluster", seed=14, n=130, spk=3, spread=0.4, natural=True),
    "c257": dict(kind="cluster", seed=15, n=257, spk=4, spread=0.5, natural=True),
    "c1000": dict(kind="cluster", seed=16, n=1000, spk=5, spread=0.6, natural=True),
    "c2048": dict(kind="cluster", seed=317, n=2048, spk=6, spread=0.9, natural=True),
    # a speaker of 3 windows: its own cluster with the count forced, then filter_minor_cluster
    "minor": dict(kind="cluster", seed=21, n=60, spk=3, spread=0.3,
                  turns=[[0, 28], [2, 3], [1, 29]], kw=dict(oracle_num=3)),
    # two centres at cosine 0.92: two spectral clusters, one after merge_by_cos
    "merge": dict(kind="cluster", seed=22, n=80, spk=2, spread=0.15, centre_cos=0.92,
                  kw=dict(oracle_num=2)),
    "forced": dict(kind="cluster", seed=23, n=50, spk=2, spread=0.4, kw=dict(oracle_num=2)),
    # process(): segments
    "s_general": dict(kind="process", seed=31, n=130, spk=3, spread=0.4, natural=True,
                      turns=[[0, 20], [1, 1], [0, 14], [2, 18], [1, 25], [2, 1], [1, 9], [0, 22],
                             [2, 20]]),
    "s_forced": dict(kind="process", seed=32, n=60, spk=2, spread=0.4, num_speakers=2),
    "s_two": dict(kind="process", seed=33, n=2, spk=1, spread=0.3),
    "s_seven": dict(kind="process", seed=34, n=7, spk=2, spread=0.3, turns=[[0, 4], [1, 3]]),
}


def reference_times(off, length, rows):
    """What _sliding_window_embeddings returns for the plan (:561-580), in its arithmetic."""
    out = []
    for r, first, frames in rows:
        region_start = off[r] / 16000.0
        if frames < 150:
            out.append((region_start, (off[r] + length[r]) / 16000.0))
        else:
            ws = region_start + int(first) * 10.0 / 1000.0
            out.append((ws, ws + 1.5))
    return out


def check_inputs(name, case, X, kw, ref):
    """Conditions a-d on one case; returns (lambdas, ambiguous share)."""
    from sklearn.cluster import KMeans
    N = X.shape[0]
    pval, min_pnum = kw.get("pval", 0.02), kw.get("min_pnum", 6)
    xn = X / (np.linalg.norm(X, axis=1, keepdims=True) + np.float32(1e-10))
    S = np.sort(xn @ xn.T, axis=1)
    n_elems = max(min(int((1 - pval) * N), N - min_pnum), 0)
    amb = 0.0
    if 0 < n_elems < N:
        gap = S[:, n_elems] - S[:, n_elems - 1]
        assert (gap > 0).all(), (name, "exact tie at the prune threshold")
        amb = float((gap < 1e-5).mean())
        assert amb <= 0.02, (name, amb)
    M = pruned_similarity(X, pval, min_pnum).astype(np.float64)
    w, v = np.linalg.eigh(np.diag(np.abs(M).sum(1)) - M)
    lo, hi = kw.get("min_num_spks", 1), kw.get("max_num_spks", 10)
    if kw.get("oracle_num") is not None:
        nspk = kw["oracle_num"]
    else:
        gaps = np.diff(w[lo - 1:hi + 1])
        nspk = int(np.argmax(gaps)) + lo if len(gaps) else 1
        if case.get("natural") and len(gaps) > 1:
            g = np.sort(gaps)[::-1]
            assert g[0] >= 3 * g[1], (name, "eigengap margin", g[:3])
    nspk = max(1, min(nspk, N))
    parts = {tuple(canonical(KMeans(n_clusters=nspk, random_state=s).fit_predict(v[:, :nspk])))
             for s in range(5)}
    assert len(parts) == 1, (name, "KMeans partition depends on random_state")
    lam = np.zeros(16)
    lam[:min(16, N)] = w[:16]
    return lam, amb


def main(ref_root):
    sys.path.insert(0, ref_root)
    from core import speaker_diarization_senko_campp_optimized as ref
    arrays, doc = {}, {}
    small_multi = False
    for name, case0 in CASES.items():
        # the first seed (seed, seed + 100, ...) whose inputs meet every condition below
        for attempt in range(40):
            case = dict(case0, seed=case0["seed"] + 100 * attempt)
            try:
                entry, labels, lam, amb, multi = run_case(name, case, ref)
                break
            except AssertionError as e:
                print(name, "seed", case["seed"], "rejected:", e)
        else:
            raise SystemExit(f"{name}: no seed met the conditions")
        small_multi = small_multi or multi
        doc[name] = entry
        arrays[f"{name}/labels"] = np.asarray(labels, np.int32)
        arrays[f"{name}/lambdas"] = lam
        arrays[f"{name}/ambiguous"] = np.float64(amb)
        print(name, "N", case["n"], "seed", case["seed"], "speakers", entry["speakers"], "ambiguous",
                amb, "segments", len(entry.get("segments", [])))
    assert small_multi, "no case at N <= 32 with two speakers"
    np.savez_compressed(os.path.join(HERE, "diar_cases.npz"), **arrays)
    with open(os.path.join(HERE, "diar_cases.json"), "w") as f:
        json.dump(doc, f, indent=1)


def run_case(name, case, ref):
    """One case through the reference: (json entry, labels, lambdas, ambiguous share, whether
    it is a case at N <= 32 with two speakers)."""
    small_multi = False
    entry = {k: v for k, v in case.items()}
    if case["kind"] == "cluster":
        X = case_embeddings(case)
        kw = dict(PROCESS_KW, **case.get("kw", {}))
        skw = {k: v for k, v in kw.items()
               if k in ("min_num_spks", "max_num_spks", "pval", "min_pnum", "oracle_num")}
        lam, amb = check_inputs(name, case, X, skw, ref)
        labels = ref._senko_cluster(X.copy(), **kw)
        spectral = ref._senko_spectral(X.copy(), **skw)
        if name == "minor":
            assert np.bincount(spectral).min() < 4 and np.bincount(labels).min() >= 4, name
        if name == "merge":
            assert len(np.unique(spectral)) == 2 and len(np.unique(labels)) == 1, name
        if case["n"] <= 32 and len(np.unique(labels)) >= 2:
            small_multi = True
        entry["kw"] = kw
    else:
        off, length, rows, duration = window_plan(case["n"], case["seed"])
        case = dict(case, n=len(rows))
        X = case_embeddings(case)
        times = reference_times(off, length, rows)
        num_speakers = case.get("num_speakers", -1)
        skw = dict(min_num_spks=num_speakers if num_speakers > 0 else 1, max_num_spks=15,
                   pval=0.012)
        lam, amb = (np.zeros(16), 0.0) if case["n"] <= 2 else check_inputs(name, case, X, skw, ref)
        seen = {}
        orig = ref._senko_cluster

        def spy(emb, **kw):
            seen["labels"] = orig(emb, **kw)
            return seen["labels"]
        ref._senko_cluster = spy
        try:
            d = ref.SenkoCamppDiarizerOptimized(num_speakers=num_speakers)
            d.emb_sess = "placeholder"
            d._pyannote_vad = lambda audio, sr: [(o / 16000.0, (o + m) / 16000.0)
                                                for o, m in zip(off, length)]
            d._sliding_window_embeddings = lambda audio, regions, cb=None: (X.copy(), list(times))
            segments = d.process(audio_data=np.zeros(int(duration * 16000), np.float32),
                                 audio_sample_rate=16000)
        finally:
            ref._senko_cluster = orig
        labels = seen.get("labels", np.zeros(case["n"], np.int32))
        dur = {}
        for s in segments:
            dur[s["speaker"]] = dur.get(s["speaker"], 0.0) + s["end"] - s["start"]
        v = sorted(dur.values())
        assert all(b - a > 1e-6 for a, b in zip(v, v[1:])), (name, "tied speaking times")
        entry.update(segments=segments, duration=duration, num_speakers=num_speakers)
    entry["speakers"] = int(len(np.unique(labels)))
    return entry, labels, lam, amb, small_multi


if __name__ == "__main__":
    main(sys.argv[1])
