"""Writes tests/golden/community1_cluster_cases.json and .npz: the reference's own back-end
functions (core/speaker_diarization_pure_ort.py) on the seeded files of
tests/community1_cases.py, for tests/test_vbx_reference.py.

    python tests/golden/make_golden_community1_cluster.py /path/to/reference

The reference is imported here only (numpy and scipy at import; no model is loaded: the object
is made without __init__ and the segmenter / embedder are the stubs of community1_cases).  Only
data is recorded.  The PLDA parameters are synthetic (community1_cases.synthetic_plda_files): no
real PLDA file is at hand.  No case forces max_clusters (that branch needs sklearn and is a
stated deviation), and every case has at most 16 clusters.
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), REPO, os.path.join(REPO, "sherpa-vietnamese-asr_amd")):
    sys.path.insert(0, p)
import community1_cases as CC  # noqa: E402


def main(ref_root: str) -> None:
    sys.path.insert(0, ref_root)
    import core.speaker_diarization_pure_ort as M

    xv, pl = CC.synthetic_plda_files()
    arrays, meta = {}, {"numpy": np.__version__, "cases": {}}
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "plda"))
        np.savez(os.path.join(d, "plda", "xvec_transform.npz"), **xv)
        np.savez(os.path.join(d, "plda", "plda.npz"), **pl)
        raw = M.load_plda(d)
        np.savez(os.path.join(d, "plda", "plda_prepared.npz"), mean1=raw["mean1"],
                 mean2=raw["mean2"], lda=raw["lda"], mu=raw["plda_mu"], plda_tr=raw["plda_tr"],
                 plda_psi=raw["plda_psi"])
        prepared = M.load_plda(d)
    for k in ("plda_tr", "plda_psi"):
        assert np.array_equal(raw[k], prepared[k])
        arrays["plda_" + k] = np.asarray(raw[k])

    def diarizer(min_duration_off=0.0):
        z = object.__new__(M.PureOrtDiarizer)
        z.threshold, z.Fa, z.Fb = M.DEFAULT_THRESHOLD, M.DEFAULT_FA, M.DEFAULT_FB
        z.min_duration_off, z.num_speakers, z.max_speakers = min_duration_off, -1, None
        z.segmentation_batch_size, z.plda_data = None, raw
        z.speaker_centroids, z._last_overlap_regions = None, []
        return z

    # the stages on one 25-chunk file
    name, seed, samples, n_spk = CC.CLUSTER_CASE
    sc = CC.scenario(seed, samples, n_spk)
    binarized = M.POWERSET_MAP[sc["classes"]]
    emb = sc["embeddings"]
    C = binarized.shape[0]
    z = diarizer()
    single = (binarized.sum(axis=2, keepdims=True) == 1).astype(np.float32)
    train_mask = ((binarized * single).sum(axis=1) >= 0.2 * CC.F) & ~np.isnan(emb[:, :, 0])
    hard = z._cluster(emb, train_mask, binarized, max_clusters=None)
    arrays[name + "_train_mask"] = train_mask
    arrays[name + "_hard"] = hard.copy()
    arrays[name + "_centroids"] = z.speaker_centroids.copy()
    assert z.speaker_centroids.shape[0] <= 16
    hard2 = hard.copy()
    hard2[np.sum(binarized, axis=1) == 0] = -2
    canon, remap = z._canonicalize_clusters(hard2, binarized)
    arrays[name + "_canonical"] = canon
    count = z._speaker_count(binarized, C, CC.F)
    arrays[name + "_count"] = count.data.copy()
    count.data = np.minimum(np.minimum(count.data, int(canon.max()) + 1).astype(np.int8), 1).astype(np.int8)
    duration = samples / CC.SR
    stage = {"remap": {str(k): int(v) for k, v in remap.items()}}
    for mdo in (0.0, 0.5):
        z.min_duration_off = mdo
        z.speaker_centroids = arrays[name + "_centroids"].copy()
        stage[f"segments_mdo{mdo}"] = z._reconstruct_and_diarize(binarized, canon, count, C, CC.F,
                                                                 duration)
    arrays[name + "_centroids_reindexed"] = z.speaker_centroids.copy()
    stage["overlap_regions"] = z._extract_overlap_regions(binarized, sc["starts"], CC.F, duration)
    meta["cases"][name] = stage

    # process() end to end, stub segmenter and embedder
    for fname, (seed, samples, n_spk) in CC.FILES.items():
        sc = CC.scenario(seed, samples, n_spk)
        for mdo in (0.0, 0.5):
            z = diarizer(mdo)
            z.seg_sess = CC.StubSegmenter(sc["classes"])
            z._extract_embeddings = lambda *a, **k: sc["embeddings"].copy()
            segs = z.process(None, audio_data=CC.staircase(samples), audio_sample_rate=CC.SR)
            meta["cases"][f"{fname}_mdo{mdo}"] = {
                "segments": segs, "overlap_regions": z.overlap_regions,
                "chunks": len(sc["starts"]),
                "centroids": None if z.speaker_centroids is None else f"{fname}_mdo{mdo}_centroids"}
            if z.speaker_centroids is not None:
                arrays[f"{fname}_mdo{mdo}_centroids"] = np.asarray(z.speaker_centroids)
    with open(os.path.join(HERE, "community1_cluster_cases.json"), "w") as f:
        json.dump(meta, f, indent=1)
    np.savez_compressed(os.path.join(HERE, "community1_cluster_cases.npz"), **arrays)
    for fn in ("community1_cluster_cases.json", "community1_cluster_cases.npz"):
        print("wrote", fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
