"""CPU checks of the community-1 back end:

  - the restated centroid AHC (vbx_reference.ahc_centroid) equals scipy's linkage + fcluster as
    a partition on every GPU-test input, and every non-degenerate input keeps its partition
    under +-2 ulp (float32) of its normalised rows over 8 seeds -- the condition under which
    test_gpu_clu.py may ask the device for exact equality;
  - the restated assignment equals scipy.optimize.linear_sum_assignment on active rows;
  - zasr.vbx's host functions equal the restatement, and both equal goldens of the reference's
    own functions (tests/golden/make_golden_community1_cluster.py);
  - single planted defects each change a result on these inputs.
"""
import json
import os

import numpy as np
import pytest

import clu_inputs
import community1_cases as CC
import vbx_reference as R
from zasr import community1, vbx

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = clu_inputs.cases()
MEMO = {}


class RefClu:
    """CluSession's ahc() served by the restatement (no device here)."""

    def ahc(self, X, threshold):
        return R.ahc_centroid(R.l2norm32(X), threshold).astype(np.int32)


def ref_labels(name):
    if name not in MEMO:
        X, thr, _ = CASES[name]
        MEMO[name] = R.ahc_centroid(R.l2norm32(X), thr)
    return MEMO[name]


@pytest.fixture(scope="module")
def gold():
    return (json.load(open(os.path.join(GOLD, "community1_cluster_cases.json"))),
            np.load(os.path.join(GOLD, "community1_cluster_cases.npz")))


@pytest.fixture(scope="module")
def plda():
    xv, pl = CC.synthetic_plda_files()
    if "plda" not in MEMO:
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            os.makedirs(os.path.join(d, "plda"))
            np.savez(os.path.join(d, "plda", "xvec_transform.npz"), **xv)
            np.savez(os.path.join(d, "plda", "plda.npz"), **pl)
            raw = vbx.load_plda(d)
            np.savez(os.path.join(d, "plda", "plda_prepared.npz"), mean1=raw["mean1"],
                     mean2=raw["mean2"], lda=raw["lda"], mu=raw["plda_mu"],
                     plda_tr=raw["plda_tr"], plda_psi=raw["plda_psi"])
            MEMO["plda"] = (raw, vbx.load_plda(d))
    return MEMO["plda"][0]


@pytest.fixture(scope="module")
def stage():
    name, seed, samples, n_spk = CC.CLUSTER_CASE
    sc = CC.scenario(seed, samples, n_spk)
    sc["binarized"] = vbx.POWERSET_MAP[sc["classes"]]
    sc["name"], sc["duration"] = name, samples / CC.SR
    return sc


# ---- the AHC restatement ----
@pytest.mark.parametrize("name", list(CASES))
def test_ahc_equals_scipy(name):
    from scipy.cluster.hierarchy import fcluster, linkage
    X, thr, _ = CASES[name]
    sp = fcluster(linkage(R.l2norm32(X), method="centroid", metric="euclidean"), thr,
                  criterion="distance")
    assert R.same_partition(ref_labels(name), sp)


@pytest.mark.parametrize("name", [n for n in CASES if not CASES[n][2]])
def test_ahc_inputs_away_from_ties(name):
    X, thr, _ = CASES[name]
    Xn = R.l2norm32(X)
    for seed in range(8):
        assert R.same_partition(R.ahc_centroid(clu_inputs.perturb_ulp(Xn, seed), thr),
                                ref_labels(name)), seed


def test_ahc_inversions_are_exercised():
    X, thr, _ = CASES["inversion3"]
    h = []
    R.ahc_centroid(R.l2norm32(X), thr, heights=h)
    assert len(h) == 2 and h[1] < h[0]
    X, thr, _ = CASES["speakers_257"]
    h = []
    R.ahc_centroid(R.l2norm32(X), thr, heights=h)
    assert sum(b < a for a, b in zip(h, h[1:])) > len(h) // 8


def test_ahc_threshold_is_inclusive():
    from scipy.cluster.hierarchy import fcluster, linkage
    X, d = clu_inputs.threshold_case()
    Xn = R.l2norm32(X)
    assert R.pairwise64(Xn)[0, 1] == d
    assert fcluster(linkage(Xn, "centroid", "euclidean"), d, "distance").tolist() == [1, 1]
    assert R.ahc_centroid(Xn, d).tolist() == [0, 0]
    assert R.ahc_centroid(Xn, d, defect="stop_ge").tolist() == [0, 1]          # the defect


def test_ahc_defects_change_a_result():
    def labels(name, defect=None, norm_defect=None):
        X, thr, _ = CASES[name]
        return R.ahc_centroid(R.l2norm32(X, norm_defect), thr, defect=defect)
    assert not R.same_partition(labels("centroid_splits3", "squared"), ref_labels("centroid_splits3"))
    assert not R.same_partition(labels("centroid_merges3", "average"), ref_labels("centroid_merges3"))
    assert not R.same_partition(labels("zero_row4", None, "no_eps"), ref_labels("zero_row4"))


# ---- the assignment ----
def test_assignment_equals_scipy_and_brute_force():
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(4)
    for K in (1, 2, 3, 4, 7, 16):
        soft = 2.0 - rng.uniform(0.0, 1.0, (200, 3, K))
        # close calls: two rows prefer one column by a small margin
        soft[::3, 1] = soft[::3, 0] + 1e-3 * rng.standard_normal((len(soft[::3]), K))
        inactive = rng.random((200, 3)) < 0.25
        soft[inactive] = soft.min() - 1.0
        got = vbx.constrained_assignment(soft.copy())
        for c in range(soft.shape[0]):
            want = np.full(3, -2)
            r, k = linear_sum_assignment(soft[c], maximize=True)
            want[r] = k
            brute = R.assign_brute(soft[c])
            act = ~inactive[c]
            assert np.array_equal(brute[act], want[act]), (K, c)
            assert np.array_equal(got[c][act], want[act]), (K, c)
            used = got[c][got[c] >= 0]
            assert len(set(used.tolist())) == len(used) == min(3, K)


# ---- PLDA ----
def test_load_plda_both_routes(gold, plda):
    _, arrays = gold
    raw, prepared = MEMO["plda"]
    for k in raw:
        assert np.array_equal(raw[k], prepared[k]), k
    np.testing.assert_allclose(raw["plda_psi"], arrays["plda_plda_psi"], rtol=1e-9)
    want = arrays["plda_plda_tr"]
    sign = np.sign((raw["plda_tr"] * want).sum(axis=1, keepdims=True))      # free per eigenvector
    assert (sign != 0).all()
    np.testing.assert_allclose(raw["plda_tr"] * sign, want, atol=1e-9 * np.abs(want).max())


def test_vbx_equals_restatement(plda, stage):
    emb = stage["embeddings"].reshape(-1, CC.DIM)
    labels = np.arange(len(emb)) % 5
    fea = vbx.plda_transform(vbx.xvec_transform(emb, plda), plda)
    np.testing.assert_allclose(fea, R.plda_features(emb, plda), rtol=1e-12, atol=1e-12)
    g, p = vbx.vbx_cluster(fea, plda["plda_psi"], labels, 0.07, 0.8)
    g2, p2 = R.vbx(fea, plda["plda_psi"], labels, 0.07, 0.8)
    np.testing.assert_allclose(g, g2, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(p, p2, rtol=1e-9, atol=1e-12)


# ---- the stages against the restatement and the reference's goldens ----
def match_clusters(hard, want):
    """The relabelling old -> new that turns `hard` into `want` (ids are arbitrary before the
    canonicalisation), checked to be a bijection."""
    m = {}
    for a, b in zip(hard.ravel().tolist(), want.ravel().tolist()):
        assert m.setdefault(a, b) == b
    assert len(set(m.values())) == len(m) and m.get(-2, -2) == -2
    return m


def test_cluster(gold, plda, stage):
    _, arrays = gold
    n = stage["name"]
    b, emb = stage["binarized"], stage["embeddings"]
    mask = vbx.filter_mask(b, emb)
    assert np.array_equal(mask, arrays[n + "_train_mask"])
    assert np.array_equal(mask, R.filter_mask(b, emb))
    hard, cent = vbx.cluster(emb, mask, b, RefClu(), plda)
    hard_r, cent_r = R.cluster(emb, mask, b, plda)
    assert hard.dtype == np.int8 and np.array_equal(hard, hard_r)
    np.testing.assert_allclose(cent, cent_r, rtol=1e-9)
    want = arrays[n + "_hard"]
    active = b.sum(axis=1) > 0
    m = match_clusters(hard[active], want[active])
    assert cent.shape == arrays[n + "_centroids"].shape and 2 <= cent.shape[0] <= 16
    for old, new in m.items():
        np.testing.assert_allclose(cent[old], arrays[n + "_centroids"][new], rtol=1e-9)


def test_cluster_few_train_rows(plda, stage):
    b, emb = stage["binarized"][:2], stage["embeddings"][:2]
    mask = np.zeros((2, 3), bool)
    mask[0, 0] = True
    hard, cent = vbx.cluster(emb, mask, b, RefClu(), plda)
    assert cent is None and hard.dtype == np.int8 and not hard.any()


def test_cluster_max_clusters_uses_kmeans(plda, stage):
    b, emb = stage["binarized"], stage["embeddings"]
    hard, cent = vbx.cluster(emb, vbx.filter_mask(b, emb), b, RefClu(), plda, max_clusters=2)
    assert cent.shape[0] == 2 and set(np.unique(hard).tolist()) <= {0, 1, -2}


def canonical_input(arrays, stage):
    hard = arrays[stage["name"] + "_hard"].copy()
    hard[stage["binarized"].sum(axis=1) == 0] = -2
    return hard


def test_canonicalize(gold, stage):
    meta, arrays = gold
    hard = canonical_input(arrays, stage)
    out, remap = vbx.canonicalize_clusters(hard, stage["binarized"])
    out_r, remap_r = R.canonicalize(hard, stage["binarized"])
    assert np.array_equal(out, arrays[stage["name"] + "_canonical"])
    assert np.array_equal(out, out_r) and remap == remap_r
    assert {str(k): v for k, v in remap.items()} == meta["cases"][stage["name"]]["remap"]
    # a permutation of the ids comes back to the same canonical form
    perm = np.where(hard >= 0, (hard + 1) % (hard.max() + 1), hard)
    assert np.array_equal(vbx.canonicalize_clusters(perm, stage["binarized"])[0], out)


def test_speaker_count(gold, stage):
    _, arrays = gold
    got = vbx.speaker_count(stage["binarized"])
    assert got.dtype == np.uint8 and np.array_equal(got, arrays[stage["name"] + "_count"])
    assert np.array_equal(got, R.speaker_count(stage["binarized"]))
    assert got.max() >= 2      # overlap is present
    bad = R.speaker_count(stage["binarized"], defect="floor")
    assert bad.shape != got.shape or not np.array_equal(bad, got)            # the defect


def test_aggregate_sums_in_chunk_order():
    """Non-integer float32 scores with gaps: the vectorised overlap-add equals the loop over
    (chunk, frame) to the bit, so its float32 additions run in chunk order."""
    rng = np.random.default_rng(9)
    data = rng.uniform(0.0, 1.0, (23, CC.F, 4)).astype(np.float32)
    data[rng.random(data.shape) < 0.3] = np.nan
    data[5] = np.nan
    for skip in (True, False):
        got = vbx.aggregate(data.copy(), skip_average=skip, missing=0.0)
        want = R.aggregate(data.copy(), skip, 0.0)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got, want)


def capped_count(arrays, stage):
    canon = arrays[stage["name"] + "_canonical"]
    count = arrays[stage["name"] + "_count"]
    return canon, np.minimum(np.minimum(count, int(canon.max()) + 1).astype(np.int8), 1).astype(np.int8)


@pytest.mark.parametrize("mdo", [0.0, 0.5])
def test_reconstruct(gold, stage, mdo):
    meta, arrays = gold
    n = stage["name"]
    canon, count = capped_count(arrays, stage)
    cent = arrays[n + "_centroids"]
    segs, re = vbx.reconstruct_and_diarize(stage["binarized"], canon, count, mdo, cent)
    assert segs == meta["cases"][n][f"segments_mdo{mdo}"] and len(segs) > 4
    segs_r, re_r = R.reconstruct(stage["binarized"], canon, count, mdo, cent)
    assert segs == segs_r and np.array_equal(re, re_r)
    assert re.dtype == np.float32 and np.array_equal(re, arrays[n + "_centroids_reindexed"])


def test_reconstruct_defects_change_a_result(gold, stage):
    _, arrays = gold
    canon, count = capped_count(arrays, stage)
    good, _ = R.reconstruct(stage["binarized"], canon, count)
    assert R.reconstruct(stage["binarized"], canon, count, defect="floor")[0] != good
    assert R.reconstruct(stage["binarized"], canon, count, defect="tie_high")[0] != good


def test_overlap_regions(gold, stage):
    meta, _ = gold
    want = [tuple(r) for r in meta["cases"][stage["name"]]["overlap_regions"]]
    got = vbx.overlap_regions(stage["binarized"], stage["starts"], CC.F, stage["duration"])
    assert got == want and len(got) >= 1
    assert R.overlap_regions(stage["binarized"], stage["starts"], CC.F, stage["duration"]) == want


# ---- process ----
def test_chunk_starts():
    for total in (1, 116800, 159999, 160000, 160001, 176000, 416000, 3 * 160000):
        assert vbx.chunk_starts_1s(total) == R.chunk_starts_1s(total) == CC.chunk_starts(total)
    assert vbx.chunk_starts_1s(159999) == [0]
    assert vbx.chunk_starts_1s(160000) == [0, 16000]       # the extra chunk of :720-722
    assert vbx.chunk_starts_1s(160001) == [0, 16000]


@pytest.mark.parametrize("fname", list(CC.FILES))
@pytest.mark.parametrize("mdo", [0.0, 0.5])
def test_process(gold, plda, fname, mdo):
    meta, arrays = gold
    seed, samples, n_spk = CC.FILES[fname]
    sc = CC.scenario(seed, samples, n_spk)
    want = meta["cases"][f"{fname}_mdo{mdo}"]
    assert len(sc["starts"]) == want["chunks"]
    out = community1.process(CC.staircase(samples), CC.StubSegmenter(sc["classes"]),
                             CC.StubEmbedder(sc["embeddings"]), RefClu(), plda,
                             min_duration_off=mdo)
    assert list(out) == want["segments"]
    assert out.overlap_regions == [tuple(r) for r in want["overlap_regions"]]
    if want["centroids"] is None:
        assert out.speaker_centroids is None
    else:
        assert out.speaker_centroids.dtype == np.float32
        np.testing.assert_allclose(out.speaker_centroids, arrays[want["centroids"]], rtol=1e-6)
    b = vbx.POWERSET_MAP[sc["classes"]]
    segs_r, cent_r, _ = R.diarize(b, sc["embeddings"], plda, min_duration_off=mdo)
    assert list(out) == segs_r


def test_attach_rebinds_cluster(plda, stage):
    class Obj:
        threshold, Fa, Fb = 0.6, 0.07, 0.8
        speaker_centroids = None

    class Sess:
        model_dir = None

    o = Obj()
    o.plda_data = plda
    community1.attach(o, Sess(), emb_W=np.zeros((1, 1)), emb_b=np.zeros(1), clu_session=RefClu())
    b, emb = stage["binarized"], stage["embeddings"]
    mask = vbx.filter_mask(b, emb)
    hard = o._cluster(emb, mask, b, max_clusters=None)
    want, cent = vbx.cluster(emb, mask, b, RefClu(), plda)
    assert np.array_equal(hard, want) and np.array_equal(o.speaker_centroids, cent)
