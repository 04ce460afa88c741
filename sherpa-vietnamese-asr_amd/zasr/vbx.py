"""Host back end of the community-1 diarizer: everything between the speaker
embeddings and the speaker segments of core/speaker_diarization_pure_ort.py -- PLDA (:317-350),
VBx (:353-378), _cluster (:904-967) with its AHC on a binding.CluSession, _canonicalize_clusters
(:881-902), _speaker_count (:742-754), _reconstruct_and_diarize (:969-1052) with
_pyannote_aggregate (:144-196) and _binarize (:211-262), _extract_overlap_regions (:512-552).

numpy only (no scipy, no sklearn), float64 where the reference is, vectorised over chunks and
frames.  Written from the mathematics; a `:line` citation names the reference lines a function
answers to, and tests/golden/community1_cluster_cases.* (made by the reference's own functions)
hold it to them."""
from __future__ import annotations

import itertools
import os
import time
from typing import Optional

import numpy as np

SAMPLE_RATE = 16000
CHUNK_DURATION = 10.0
CHUNK_STEP = 1.0
CHUNK_SAMPLES = 160000
STEP_SAMPLES = 16000
MAX_SPEAKERS_PER_CHUNK = 3
RF_START = 0.0
RF_DURATION = 0.0619375
RF_STEP = 0.016875
LDA_DIM = 128

POWERSET_MAP = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1],
                         [1, 1, 0], [1, 0, 1], [0, 1, 1]], np.float32)   # :124-132


# ---- chunking ----
def chunk_starts_1s(total: int) -> list:
    """Starts of _segment (:714-726): every second up to and including the first chunk that
    ends AFTER the signal.  One chunk more than zasr_seg_classes_device's rule when
    total - 160000 is a non-negative multiple of 16000."""
    starts, s = [], 0
    while True:
        starts.append(s)
        if s + CHUNK_SAMPLES > total:     # (s + CHUNK) / SR > total / SR: exact in float64 here
            break
        s += STEP_SAMPLES
    return starts


# ---- PLDA (:311-350) ----
def _unit(x):
    """Rows (or one vector) scaled to unit length, the length floored by + 1e-10 (:311-314)."""
    x = np.asarray(x)
    return x / (np.sqrt(np.sum(x * x, axis=-1, keepdims=True)) + 1e-10)


def generalized_eigh(B, W):
    """scipy.linalg.eigh(B, W) for symmetric B and positive definite W, by numpy: eigenvalues
    ascending, eigenvectors in columns with v^T W v = 1.  Signs are free."""
    L = np.linalg.cholesky(W)
    Li = np.linalg.inv(L)
    Cm = Li @ B @ Li.T
    w, y = np.linalg.eigh(0.5 * (Cm + Cm.T))
    return w, Li.T @ y


PLDA_KEYS = ("mean1", "mean2", "lda", "plda_mu", "plda_tr", "plda_psi")   # the reference's dict


def load_plda(model_dir: str) -> dict:
    """The PLDA of a model directory as the reference's dict (:317-339).  plda/plda_prepared.npz
    holds it ready made.  Otherwise plda.npz holds a transform T and a diagonal psi: the
    within-class covariance is (T^T T)^-1, the between-class one (T^T diag(1 / psi) T)^-1, and
    the prepared transform simultaneously diagonalises the two -- the generalised eigenvectors
    as rows, largest eigenvalue first, the eigenvalues being the new psi."""
    folder = os.path.join(model_dir, "plda")
    ready = os.path.join(folder, "plda_prepared.npz")
    if os.path.exists(ready):
        z = np.load(ready)
        stored = ("mean1", "mean2", "lda", "mu", "plda_tr", "plda_psi")
        return {key: z[name] for key, name in zip(PLDA_KEYS, stored)}
    xvec = np.load(os.path.join(folder, "xvec_transform.npz"))
    raw = np.load(os.path.join(folder, "plda.npz"))
    T, psi = raw["tr"], raw["psi"]
    within = np.linalg.inv(T.T @ T)
    between = np.linalg.inv(T.T @ (T / np.asarray(psi)[:, None]))
    lam, vec = generalized_eigh(between, within)
    descending = np.argsort(lam, kind="stable")[::-1]
    return dict(zip(PLDA_KEYS, (xvec["mean1"], xvec["mean2"], xvec["lda"], raw["mu"],
                                vec[:, descending].T, lam[descending])))


def synthetic_plda(seed: int = 1, dim: int = 256, lda_dim: int = LDA_DIM) -> dict:
    """Seeded PLDA parameters of the right shapes, for benchmarks and tests (no real PLDA files
    are needed to run the code)."""
    rng = np.random.default_rng(seed)
    return {"mean1": 0.05 * rng.standard_normal(dim), "mean2": 0.05 * rng.standard_normal(lda_dim),
            "lda": rng.standard_normal((dim, lda_dim)) / np.sqrt(dim),
            "plda_mu": 0.05 * rng.standard_normal(lda_dim),
            "plda_tr": np.linalg.qr(rng.standard_normal((lda_dim, lda_dim)))[0],
            "plda_psi": np.sort(rng.uniform(0.05, 8.0, lda_dim))[::-1].copy()}


def xvec_transform(embeddings, plda):
    """x-vector whitening (:342-346): centre, project to the sphere of radius sqrt(dim), apply
    the LDA, centre again, project to the sphere of radius sqrt(lda dim)."""
    dim_in, dim_out = plda["lda"].shape
    sphere = _unit(np.asarray(embeddings) - plda["mean1"]) * np.sqrt(dim_in)
    return _unit(sphere @ plda["lda"] - plda["mean2"]) * np.sqrt(dim_out)


def plda_transform(embeddings, plda, lda_dim: int = LDA_DIM):
    """Into the PLDA's diagonalising basis, its first lda_dim directions (:349-350)."""
    basis = plda["plda_tr"][:lda_dim]
    return (np.asarray(embeddings) - plda["plda_mu"]) @ basis.T


# ---- VBx (:353-378) ----
def _softmax_rows(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _logsumexp_rows(a):
    top = a.max(axis=1)
    top = np.where(np.isfinite(top), top, 0.0)
    return top + np.log(np.exp(a - top[:, None]).sum(axis=1))


def vbx_cluster(fea, plda_psi, ahc_labels, Fa, Fb, max_iters: int = 20):
    """Variational Bayes clustering of PLDA features [N][D] without the HMM (VBx with loop
    probability 0): (responsibilities [N][K], speaker priors [K]).

    Model: speaker k has a latent y_k ~ N(0, I) and emits x ~ N(sqrt(psi) * y_k, I) in the
    basis where the PLDA is diagonal.  With responsibilities r the posterior of y_k is Gaussian,
    precision 1 + (Fa / Fb) n_k psi with n_k = sum_i r_ik, mean (Fa / Fb) var_k sum_i r_ik
    sqrt(psi) x_i.  The expected log-likelihood of x_i under speaker k, scaled by Fa, and the
    log priors give the new responsibilities; the priors are their normalised column sums.
    Starts from softmax(7 * one-hot(AHC labels)) and uniform priors; stops after max_iters or
    when the evidence lower bound gains less than 1e-4."""
    x = np.asarray(fea, np.float64)
    psi = np.asarray(plda_psi, np.float64)
    n_rows, dim = x.shape
    labels = np.asarray(ahc_labels).astype(np.int64)
    n_spk = int(labels.max()) + 1
    resp = _softmax_rows(7.0 * (labels[:, None] == np.arange(n_spk)[None, :]))
    prior = np.full(n_spk, 1.0 / n_spk)
    scaled = x * np.sqrt(psi)                                         # sqrt(psi) x_i
    gauss_const = -0.5 * ((x * x).sum(axis=1) + dim * np.log(2.0 * np.pi))
    ratio = Fa / Fb
    bound_before = -np.inf
    for it in range(max_iters):
        var = 1.0 / (1.0 + ratio * resp.sum(axis=0)[:, None] * psi)   # [K][D] posterior variances
        mean = ratio * var * (resp.T @ scaled)                        # [K][D] posterior means
        expected = scaled @ mean.T - 0.5 * ((var + mean * mean) @ psi) + gauss_const[:, None]
        joint = Fa * expected + np.log(prior + 1e-8)
        evidence = _logsumexp_rows(joint)
        resp = np.exp(joint - evidence[:, None])
        prior = resp.sum(axis=0)
        prior = prior / prior.sum()
        # sum of log evidences minus Fb * KL(posterior of y || N(0, I))
        bound = evidence.sum() + 0.5 * Fb * np.sum(np.log(var) - var - mean * mean + 1.0)
        if it > 0 and bound - bound_before < 1e-4:
            break
        bound_before = bound
    return resp, prior


# ---- _cluster (:904-967) ----
def cosine_scores(flat_emb, centroids):
    """2 - cdist(flat_emb, centroids, "cosine") in float64 (:951-953)."""
    u = np.asarray(flat_emb, np.float64)
    v = np.asarray(centroids, np.float64)
    nu = np.sqrt((u * u).sum(axis=1))
    nv = np.sqrt((v * v).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = (u @ v.T) / (nu[:, None] * nv[None, :])
    cos = np.where(np.abs(cos) > 1.0, np.copysign(1.0, cos), cos)
    return 2.0 - (1.0 - cos)


def constrained_assignment(soft):
    """linear_sum_assignment(cost, maximize=True) of every chunk's 3 x K matrix (:961-965),
    vectorised over chunks: int8 [chunks][3], -2 for a row left without a column (K < 3).  A
    maximum assignment of three rows only ever uses each row's best three columns, so 27
    candidates per chunk decide it; among equal totals the first candidate wins (the reference's
    choice among exact ties is scipy's and is not pinned)."""
    C, S, K = soft.shape
    hard = np.full((C, S), -2, np.int8)
    if C == 0 or K == 0:
        return hard
    if K >= S:
        top = np.argsort(-soft, axis=2, kind="stable")[:, :, :S]            # [C][3][3]
        val = np.take_along_axis(soft, top, axis=2)
        best_total = np.full(C, -np.inf)
        best = np.zeros((C, S), np.int64)
        for pick in itertools.product(range(S), repeat=S):
            cols = np.stack([top[:, s, pick[s]] for s in range(S)], axis=1)
            total = sum(val[:, s, pick[s]] for s in range(S))
            distinct = np.ones(C, bool)
            for a, b in itertools.combinations(range(S), 2):
                distinct &= cols[:, a] != cols[:, b]
            better = distinct & (total > best_total)
            best_total = np.where(better, total, best_total)
            best[better] = cols[better]
        return best.astype(np.int8)
    # K < 3: K of the three rows get the K columns
    best_total = np.full(C, -np.inf)
    for sub in itertools.permutations(range(S), K):         # sub[k] = the row of column k
        total = sum(soft[:, sub[k], k] for k in range(K))
        better = total > best_total
        best_total = np.where(better, total, best_total)
        cand = np.full((C, S), -2, np.int8)
        for k in range(K):
            cand[:, sub[k]] = k
        hard[better] = cand[better]
    return hard


def cluster(embeddings, train_mask, binarized, clu_session, plda, threshold: float = 0.6,
            Fa: float = 0.07, Fb: float = 0.8, max_clusters: Optional[int] = None):
    """_cluster (:904-967): (hard_clusters int8 [chunks][3], centroids [K][dim] or None).
    clu_session has ahc(X float32 [N][D], threshold) -> labels, a binding.CluSession.

    The train rows are clustered by AHC (device) and refined by VBx in the PLDA space; a
    speaker's centroid is the responsibility-weighted mean of the train rows, for the speakers
    whose prior survives (> 1e-7).  Every (chunk, local speaker) embedding is then scored
    against the centroids (2 - cosine distance) and each chunk's three rows are assigned to
    distinct centroids with the largest total score."""
    emb = np.asarray(embeddings)
    n_chunks, n_local, dim = emb.shape
    train = emb[np.asarray(train_mask, bool)]
    if train.shape[0] < 2:                                                   # :914
        return np.zeros((n_chunks, n_local), np.int8), None
    start = clu_session.ahc(np.ascontiguousarray(train, np.float32), float(threshold))  # :918-921
    start = np.unique(np.asarray(start), return_inverse=True)[1]
    resp, prior = vbx_cluster(plda_transform(xvec_transform(train, plda), plda), plda["plda_psi"],
                              start, Fa, Fb)
    alive = np.flatnonzero(prior > 1e-7)
    if alive.size == 0:
        alive = np.zeros(1, np.int64)
    weight = resp[:, alive]                                                  # [N][K]
    centroids = (weight.T @ train) / (weight.sum(axis=0)[:, None] + 1e-8)
    if max_clusters and centroids.shape[0] > max_clusters:
        # :940-945 with the deterministic Lloyd k-means of zasr/diarize.py standing in for
        # sklearn's seeded KMeans (deviations): cluster the unit rows, average the
        # raw ones
        from .diarize import kmeans
        member = kmeans(_unit(train), max_clusters)
        centroids = np.stack([train[member == k].mean(axis=0) for k in range(max_clusters)])
    score = cosine_scores(emb.reshape(n_chunks * n_local, dim), centroids)
    score = score.reshape(n_chunks, n_local, centroids.shape[0])
    silent = np.asarray(binarized).sum(axis=1) == 0                          # :956-958
    # an embedding with NaN makes the reference's scipy call raise; here it counts as silent
    broken = np.isnan(score).any(axis=2)
    floor = np.nanmin(score) - 1.0 if not broken.all() else -1.0
    score[silent | broken] = floor
    return constrained_assignment(score), centroids


# ---- post-clustering (:613-619, :881-902) ----
def filter_mask(binarized, embeddings):
    """Which (chunk, local speaker) embeddings train the clustering (:613-619): the speaker is
    alone for at least a fifth of the chunk's frames, and the embedding is a number."""
    b = np.asarray(binarized)
    alone = b.sum(axis=2) == 1                                               # [C][F]
    frames_alone = (b * alone[:, :, None]).sum(axis=1)                       # [C][S]
    return (frames_alone >= 0.2 * b.shape[1]) & ~np.isnan(np.asarray(embeddings)[:, :, 0])


def canonicalize_clusters(hard_clusters, activities):
    """Relabel by the first active (chunk, frame, local speaker) of every cluster: (output,
    remap old -> new)."""
    hard = np.asarray(hard_clusters)
    act = np.asarray(activities) > 0                                         # [C][F][S]
    has = act.any(axis=1)
    first = act.argmax(axis=1)
    output = np.full_like(hard, -2)
    keys = []
    big = 10 ** 9
    for cid in sorted(int(k) for k in np.unique(hard) if k >= 0):
        c, s = np.nonzero((hard == cid) & has)
        if c.size:
            f = first[c, s]
            o = np.lexsort((s, f, c))[0]
            key = (int(c[o]), int(f[o]), int(s[o]))
        else:
            key = (big, big, big)
        keys.append((key, cid))
    remap = {old: new for new, (_, old) in enumerate(sorted(keys))}
    for old, new in remap.items():
        output[hard == old] = new
    return output, remap


# ---- aggregation (:144-196) ----
def closest_frame(t, start=RF_START, duration=RF_DURATION, step=RF_STEP):
    return np.rint((t - start - 0.5 * duration) / step).astype(np.int64)


def _extent(n):
    """(start, end) in seconds of n frames on the receptive-field grid from frame 0: the grid's
    start, and half a field past the centre line of frame n."""
    return RF_START, RF_START + (n - 0.5) * RF_STEP + 0.5 * RF_DURATION


def _ordered_sum(slots, first):
    """sum over axis 0 of slots [m][frames][K], per frame in the cyclic order that starts at
    slot first[frame]: float32 additions one slot at a time, every frame at once."""
    m, frames = slots.shape[:2]
    total = np.zeros(slots.shape[1:], np.float32)
    cols = np.arange(frames)
    for step in range(m):
        total += slots[(first + step) % m, cols]
    return total


def aggregate(data, skip_average: bool, missing: float = 0.0):
    """Overlap-add of chunk scores [chunks][frames][classes] (NaN = no score) onto the file's
    frame grid, float32 [num_frames][classes]: the per-frame sum of the scores, divided by the
    number of scores unless skip_average, `missing` where no chunk scored.  What
    _pyannote_aggregate computes with hamming=False and warm_up=(0, 0) for the 10 s / 1 s chunk
    window and the model's receptive field.

    No loop over chunks or frames: chunk c lands at frame closest_frame(c + rf / 2), chunks m
    apart do not overlap (m = 10 here), so chunk c is scattered into slot c % m of an
    [m][num_frames] buffer, and the slots of a frame are summed starting from its earliest
    chunk's -- the float32 additions happen in chunk order, as the reference's do."""
    data = np.asarray(data, np.float32)
    C, F, K = data.shape
    last_end = np.float64(0.0 + CHUNK_DURATION + (C - 1) * CHUNK_STEP)
    num_frames = int(closest_frame(last_end + 0.5 * RF_DURATION)) + 1
    first_frame = closest_frame(0.0 + np.arange(C, dtype=np.float64) * CHUNK_STEP + 0.5 * RF_DURATION)
    length = np.clip(num_frames - first_frame, 0, F)                 # frames of a chunk that fit
    m = 1
    while m < C and np.any(first_frame[m:] - first_frame[:-m] < F):
        m += 1
    scored = ~np.isnan(data)
    value = np.zeros((m, num_frames, K), np.float32)
    present = np.zeros((m, num_frames, K), bool)
    offs = np.arange(F)
    for slot in range(m):
        chunks = np.arange(slot, C, m)
        rows = first_frame[chunks, None] + offs[None, :]
        fits = offs[None, :] < length[chunks, None]
        value[slot][rows[fits]] = np.where(scored[chunks], data[chunks], np.float32(0.0))[fits]
        present[slot][rows[fits]] = scored[chunks][fits]
    # the earliest chunk over every frame: the first one whose end lies beyond it
    frames = np.arange(num_frames)
    earliest = np.searchsorted(first_frame + length, frames, side="right")
    total = _ordered_sum(value, earliest % m)
    n_scores = present.sum(axis=0).astype(np.float32)
    if not skip_average:
        total = total / np.maximum(n_scores, np.float32(1e-12))
    total[n_scores == 0] = missing
    return total


def speaker_count(binarized):
    """_speaker_count (:742-754): uint8 [num_frames][1]."""
    count = np.asarray(binarized).sum(axis=-1, keepdims=True)
    return np.rint(aggregate(count, skip_average=False, missing=0.0)).astype(np.uint8)


def _crop(n, sw_start, focus):
    """_SWF.crop(focus, return_data=False) of n frames on the receptive-field window: (i, j,
    start of the cropped window)."""
    i = int(np.ceil((focus[0] - RF_DURATION - sw_start) / RF_STEP))
    j = int(np.floor((focus[1] - sw_start) / RF_STEP)) + 1
    i, j = max(i, 0), min(j, n)
    return i, j, sw_start + i * RF_STEP


def binarize_segments(binary, sw_start, min_duration_off: float = 0.0):
    """_binarize(binary, sliding_window, 0.5, 0.5, 0.0, min_duration_off) (:211-262) for a 0 / 1
    input: [(start, end, k)] sorted by start (stable over k)."""
    T, K = binary.shape
    if T == 0:
        return []
    s = sw_start + np.arange(T, dtype=np.float64) * RF_STEP
    timestamps = 0.5 * (s + (s + RF_DURATION))
    out = []
    for k in range(K):
        a = binary[:, k] > 0.5
        prev = np.concatenate(([False], a[:-1]))
        on = np.flatnonzero(a & ~prev)
        off = np.flatnonzero(~a & prev)
        if a[-1]:
            off = np.concatenate((off, [T - 1]))
        if min_duration_off > 0.0 and on.size > 1:                           # :245-252
            # a pause of at most min_duration_off joins its two neighbours
            keep = timestamps[on[1:]] - timestamps[off[:-1]] > min_duration_off
            on, off = on[np.concatenate(([True], keep))], off[np.concatenate((keep, [True]))]
        out.extend((float(timestamps[i]), float(timestamps[j]), k) for i, j in zip(on, off))
    out.sort(key=lambda x: x[0])
    return out


def reconstruct_and_diarize(activities, hard_clusters, count, min_duration_off: float = 0.0,
                            speaker_centroids=None):
    """_reconstruct_and_diarize (:969-1052): (segments, centroids reindexed by :1041-1050).
    `count` is speaker_count's array after the caps of :649-653."""
    act = np.asarray(activities, np.float32)
    hard = np.asarray(hard_clusters)
    C, F, S = act.shape
    num_clusters = int(hard.max()) + 1
    if num_clusters <= 0:
        return [], speaker_centroids
    clustered = np.full((C, F, num_clusters), np.nan, np.float32)
    for s in range(S):
        idx = np.flatnonzero(hard[:, s] >= 0)
        ks = hard[idx, s].astype(np.int64)
        clustered[idx, :, ks] = np.fmax(clustered[idx, :, ks], act[idx, :, s])
    activations = aggregate(clustered, skip_average=True, missing=0.0)
    count = np.asarray(count)
    max_spk = int(count.max()) if count.size else 0
    if activations.shape[1] < max_spk:
        activations = np.pad(activations, ((0, 0), (0, max_spk - activations.shape[1])))
    ea, ec = _extent(len(activations)), _extent(len(count))
    extent = (max(ea[0], ec[0]), min(ea[1], ec[1]))
    i, j, sw_start = _crop(len(activations), RF_START, extent)
    activations = activations[i:j] if i < j else activations[:0]
    ci, cj, _ = _crop(len(count), RF_START, extent)
    count_c = count[ci:cj] if ci < cj else count[:0]
    T = min(len(activations), len(count_c))
    binary = np.zeros_like(activations)
    if T:
        a = activations[:T]
        # argsort(-a)[0]: the first maximum, the lowest cluster id among equals
        top = np.argmax(a, axis=1)
        on = np.flatnonzero(np.minimum(count_c[:T].reshape(T, -1)[:, 0].astype(np.int64), 1) >= 1)
        binary[on, top[on]] = 1.0
    raw = binarize_segments(binary, sw_start, min_duration_off)
    if not raw:
        return [], speaker_centroids
    # speakers are numbered in the order of their first segment (:1026-1037)
    cluster_of = np.array([k for _, _, k in raw], np.int64)
    clusters, first_seen = np.unique(cluster_of, return_index=True)
    clusters = clusters[np.argsort(first_seen, kind="stable")]       # cluster id of speaker 0, 1, ..
    speaker_of = np.empty(int(clusters.max()) + 1, np.int64)
    speaker_of[clusters] = np.arange(clusters.size)
    segments = [{"start": round(st, 4), "end": round(en, 4), "speaker": int(speaker_of[k])}
                for st, en, k in raw]
    order = np.argsort([seg["start"] for seg in segments], kind="stable")
    segments = [segments[i] for i in order]
    if speaker_centroids is not None:                                        # :1041-1050
        speaker_centroids = _move_rows(speaker_centroids, clusters, np.arange(clusters.size),
                                       clusters.size, np.float32)
    return segments, speaker_centroids


def _move_rows(rows, src, dst, n_out, dtype):
    """out [n_out][dim] of zeros with out[dst[i]] = rows[src[i]] wherever both rows exist."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    out = np.zeros((n_out, rows.shape[1]), dtype)
    ok = (src < rows.shape[0]) & (dst < n_out)
    out[dst[ok]] = rows[src[ok]]
    return out


def merge_min_duration_off(segments, min_duration_off: float):
    """Consecutive segments of one speaker no more than min_duration_off apart become one
    (:663-671): a run of such links keeps its first start and its last end."""
    if not (min_duration_off > 0 and len(segments) > 1):
        return segments
    start = np.array([seg["start"] for seg in segments])
    end = np.array([seg["end"] for seg in segments])
    spk = np.array([seg["speaker"] for seg in segments])
    linked = (spk[1:] == spk[:-1]) & (start[1:] - end[:-1] <= min_duration_off)
    heads = np.flatnonzero(np.concatenate(([True], ~linked)))
    tails = np.concatenate((heads[1:] - 1, [len(segments) - 1]))
    return [{"start": segments[h]["start"], "end": segments[t]["end"],
             "speaker": segments[h]["speaker"]} for h, t in zip(heads, tails)]


# ---- overlap regions (:512-552) ----
def overlap_regions(binarized, chunk_starts, num_seg_frames: int, duration: float,
                    min_duration: float = 0.3):
    b = np.asarray(binarized)
    frame_dur = CHUNK_DURATION / num_seg_frames
    n_out = int(duration / frame_dur) + 1
    t0 = np.asarray(chunk_starts, np.float64) / SAMPLE_RATE
    out_f = ((t0[:, None] + np.arange(num_seg_frames) * frame_dur) / frame_dur).astype(np.int64)
    ok = (out_f >= 0) & (out_f < n_out)
    two = b.sum(axis=-1) >= 2
    total = np.bincount(out_f[ok], minlength=n_out).astype(np.float32)
    over = np.bincount(out_f[ok & two], minlength=n_out).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        prob = np.where(total > 0, over / total, 0.0)
    a = prob > 0.5
    prev = np.concatenate(([False], a[:-1]))
    on = np.flatnonzero(a & ~prev)
    off = np.flatnonzero(~a & prev)
    if a.size and a[-1]:
        off = np.concatenate((off, [a.size]))
    regions = []
    for i, j in zip(on, off):
        start_t, t = i * frame_dur, j * frame_dur
        if t - start_t >= min_duration:
            regions.append((start_t, min(t, duration)))
    return regions


# ---- steps 4 to 8 of process (:591-671) ----
def diarize_from_embeddings(binarized, embeddings, clu_session, plda, num_speakers: int = 0,
                            max_speakers: Optional[int] = None, threshold: float = 0.6,
                            Fa: float = 0.07, Fb: float = 0.8, min_duration_off: float = 0.0):
    """(segments, info): the speaker count, the train filter, _cluster, the canonical ids and
    the reconstruction.  info holds speaker_centroids, hard_clusters, train_rows and times."""
    b = np.asarray(binarized, np.float32)
    times = {}
    t0 = time.perf_counter()
    count = speaker_count(b)
    times["count"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    train_mask = filter_mask(b, embeddings)
    max_cl = num_speakers if num_speakers and num_speakers > 0 else max_speakers
    hard, centroids = cluster(embeddings, train_mask, b, clu_session, plda, threshold, Fa, Fb,
                              max_cl)
    times["cluster"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    hard = hard.copy()
    hard[b.sum(axis=1) == 0] = -2                                            # :638-639
    hard, remap = canonicalize_clusters(hard, b)
    if centroids is not None and remap:                                      # :641-646
        centroids = _move_rows(centroids, list(remap), list(remap.values()), centroids.shape[0],
                               centroids.dtype)
    num_detected = int(hard.max()) + 1
    count = np.minimum(count, num_detected).astype(np.int8)                  # :649-653
    count = np.minimum(count, 1).astype(np.int8)
    segments, centroids = reconstruct_and_diarize(b, hard, count, min_duration_off, centroids)
    segments = merge_min_duration_off(segments, min_duration_off)
    times["reconstruct"] = time.perf_counter() - t0
    return segments, {"speaker_centroids": centroids, "hard_clusters": hard,
                      "train_rows": int(train_mask.sum()), "times": times}
