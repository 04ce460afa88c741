"""A float64 restatement of the community-1 diarizer's back end, written for reading: primitive
centroid AHC (the global minimum of the whole matrix each step), VBx, the 3 x K assignment by
brute force and the frame aggregation with explicit loops.  Test infrastructure: zasr/vbx.py and
the device AHC are held to it, and it is held to scipy and to goldens of the reference's own
functions in test_vbx_reference.py.  Switches named `defect` plant one single defect each."""
import itertools
import math

import numpy as np

SAMPLE_RATE = 16000
CHUNK_DURATION = 10.0
CHUNK_STEP = 1.0
CHUNK_SAMPLES = 160000
STEP_SAMPLES = 16000
RF_START = 0.0
RF_DURATION = 0.0619375
RF_STEP = 0.016875


# ---- centroid AHC ----
def l2norm32(X, defect=None):
    """x / (|x|_2 + 1e-10) in float32, the reference's own expression (:918)."""
    X = np.asarray(X, np.float32)
    n = np.linalg.norm(X, axis=1, keepdims=True)
    if defect == "no_eps":
        with np.errstate(invalid="ignore", divide="ignore"):
            return X / n
    return X / (n + 1e-10)


def pairwise64(Xn):
    """Euclidean distances from float64 differences, +inf on the diagonal."""
    x = np.asarray(Xn, np.float64)
    N = x.shape[0]
    Dm = np.empty((N, N))
    for i in range(N):
        d = x - x[i]
        Dm[i] = np.sqrt((d * d).sum(axis=1))
    Dm[np.arange(N), np.arange(N)] = np.inf
    return Dm


def canonical_labels(labels):
    """Number the clusters by their lowest member row."""
    labels = np.asarray(labels)
    out = np.full(labels.shape, -1, np.int64)
    seen = {}
    for r, l in enumerate(labels.tolist()):
        if l not in seen:
            seen[l] = len(seen)
        out[r] = seen[l]
    return out


def ahc_centroid(Xn, threshold, defect=None, heights=None):
    """Flat clusters of fcluster(linkage(Xn, "centroid"), threshold, "distance"): merge the
    globally closest pair by scipy's Lance-Williams centroid update on plain distances until the
    first minimum above the threshold.  Labels numbered by lowest member row.
    defects: "squared" (the update on squared distances without the roots), "stop_ge",
    "average" (average linkage)."""
    Dm = pairwise64(Xn)
    N = Dm.shape[0]
    size = np.ones(N)
    root = np.arange(N)
    alive = np.ones(N, bool)
    for _ in range(N - 1):
        flat = int(np.argmin(Dm))
        i, j = divmod(flat, N)
        d = Dm[i, j]
        if not np.isfinite(d):
            break
        if d >= threshold if defect == "stop_ge" else d > threshold:
            break
        if heights is not None:
            heights.append(float(d))
        if i > j:
            i, j = j, i
        ni, nj = size[i], size[j]
        ks = np.flatnonzero(alive)
        ks = ks[(ks != i) & (ks != j)]
        dki, dkj = Dm[i, ks], Dm[j, ks]
        if defect == "average":
            new = (ni * dki + nj * dkj) / (ni + nj)
        elif defect == "squared":
            new = (((ni * dki) + (nj * dkj)) - (ni * nj * d) / (ni + nj)) / (ni + nj)
        else:
            v = (((ni * dki * dki) + (nj * dkj * dkj)) - (ni * nj * d * d) / (ni + nj)) / (ni + nj)
            new = np.sqrt(np.maximum(v, 0.0))
        Dm[i, ks] = new
        Dm[ks, i] = new
        Dm[j, :] = np.inf
        Dm[:, j] = np.inf
        alive[j] = False
        size[i] = ni + nj
        root[root == j] = i
    return canonical_labels(root)


def same_partition(a, b):
    return np.array_equal(canonical_labels(a), canonical_labels(b))


# ---- PLDA and VBx ----
def l2n(x):
    return x / (np.linalg.norm(x, axis=-1, keepdims=True) + 1e-10)


def plda_features(emb, pd, lda_dim=128):
    """xvec_transform then plda_transform (:342-350)."""
    x = l2n(np.asarray(emb) - pd["mean1"]) * math.sqrt(pd["lda"].shape[0])
    x = l2n(x @ pd["lda"] - pd["mean2"]) * math.sqrt(pd["lda"].shape[1])
    return (x - pd["plda_mu"]) @ pd["plda_tr"].T[:, :lda_dim]


def vbx(fea, psi, labels, Fa, Fb, max_iters=20):
    """VBx (:353-378) with the cluster loop written out: (gamma [T][K], pi [K])."""
    T, D = fea.shape
    K = int(np.max(labels)) + 1
    q = np.zeros((T, K))
    q[np.arange(T), np.asarray(labels, int)] = 7.0
    gamma = np.exp(q - q.max(axis=1, keepdims=True))
    gamma /= gamma.sum(axis=1, keepdims=True)
    pi = np.full(K, 1.0 / K)
    G = -0.5 * ((fea ** 2).sum(axis=1) + D * math.log(2 * math.pi))
    rho = fea * np.sqrt(psi)
    prev = -np.inf
    for it in range(max_iters):
        logp = np.empty((T, K))
        reg = 0.0
        for k in range(K):
            invL = 1.0 / (1.0 + Fa / Fb * gamma[:, k].sum() * psi)
            alpha = Fa / Fb * invL * (gamma[:, k] @ rho)
            logp[:, k] = Fa * (rho @ alpha - 0.5 * ((invL + alpha ** 2) @ psi) + G)
            reg += np.sum(np.log(invL) - invL - alpha ** 2 + 1.0)
        a = logp + np.log(pi + 1e-8)
        m = a.max(axis=1)
        lpx = m + np.log(np.exp(a - m[:, None]).sum(axis=1))
        gamma = np.exp(a - lpx[:, None])
        pi = gamma.sum(axis=0)
        pi = pi / pi.sum()
        elbo = lpx.sum() + Fb * 0.5 * reg
        if it > 0 and elbo - prev < 1e-4:
            break
        prev = elbo
    return gamma, pi


# ---- the constrained assignment, by brute force ----
def assign_brute(cost):
    """The maximum assignment of one [S][K] matrix over every injective map of min(S, K) rows
    to columns: int [S], -2 for a row without a column."""
    S, K = cost.shape
    best, best_total = None, -np.inf
    if K >= S:
        for cols in itertools.permutations(range(K), S):
            total = sum(cost[s, cols[s]] for s in range(S))
            if total > best_total:
                best, best_total = list(cols), total
        return np.array(best)
    for rows in itertools.permutations(range(S), K):
        total = sum(cost[rows[k], k] for k in range(K))
        if total > best_total:
            best_total = total
            best = [-2] * S
            for k in range(K):
                best[rows[k]] = k
    return np.array(best)


def cosine_scores(emb, centroids):
    u = np.asarray(emb, np.float64)
    v = np.asarray(centroids, np.float64)
    out = np.empty((u.shape[0], v.shape[0]))
    for a in range(u.shape[0]):
        for b in range(v.shape[0]):
            out[a, b] = 2.0 - (1.0 - (u[a] @ v[b]) / (math.sqrt(u[a] @ u[a]) * math.sqrt(v[b] @ v[b])))
    return out


def cluster(embeddings, train_mask, binarized, plda, threshold=0.6, Fa=0.07, Fb=0.8):
    """_cluster (:904-967) without the max_clusters branch: (hard [C][3], centroids)."""
    emb = np.asarray(embeddings)
    C, S, dim = emb.shape
    train = emb[np.asarray(train_mask, bool)]
    if len(train) < 2:
        return np.zeros((C, S), np.int8), None
    labels = ahc_centroid(l2norm32(train), threshold)
    gamma, pi = vbx(plda_features(train, plda), plda["plda_psi"], labels, Fa, Fb)
    keep = np.flatnonzero(pi > 1e-7)
    if keep.size == 0:
        keep = np.array([0])
    W = gamma[:, keep]
    centroids = (W.T @ train) / (W.sum(axis=0)[:, None] + 1e-8)
    soft = cosine_scores(emb.reshape(-1, dim), centroids).reshape(C, S, -1)
    const = soft.min() - 1.0
    inactive = np.asarray(binarized).sum(axis=1) == 0
    soft[inactive] = const
    hard = np.full((C, S), -2, np.int8)
    for c in range(C):
        hard[c] = assign_brute(soft[c])
    return hard, centroids


# ---- the frame arithmetic, with explicit loops ----
def closest_frame(t, defect=None):
    x = (t - RF_START - 0.5 * RF_DURATION) / RF_STEP
    return int(math.floor(x)) if defect == "floor" else int(np.rint(x))


def aggregate(data, skip_average, missing=0.0, defect=None):
    """_pyannote_aggregate (:144-196), hamming=False, warm_up=(0, 0), one (chunk, frame) at a
    time in float32."""
    data = np.asarray(data, np.float32)
    C, F, K = data.shape
    num_frames = closest_frame(0.0 + CHUNK_DURATION + (C - 1) * CHUNK_STEP + 0.5 * RF_DURATION,
                               defect) + 1
    out = np.zeros((num_frames, K), np.float32)
    weight = np.zeros((num_frames, K), np.float32)
    seen = np.zeros((num_frames, K), bool)
    for c in range(C):
        sf = closest_frame((0.0 + c * CHUNK_STEP) + 0.5 * RF_DURATION, defect)
        for f in range(min(F, num_frames - sf)):
            for k in range(K):
                v = data[c, f, k]
                if not np.isnan(v):
                    out[sf + f, k] = np.float32(out[sf + f, k] + v)
                    weight[sf + f, k] = np.float32(weight[sf + f, k] + np.float32(1.0))
                    seen[sf + f, k] = True
    if not skip_average:
        out = out / np.maximum(weight, np.float32(1e-12))
    out[~seen] = missing
    return out


def speaker_count(binarized, defect=None):
    b = np.asarray(binarized, np.float32)
    return np.rint(aggregate(b.sum(axis=-1, keepdims=True), False, 0.0, defect)).astype(np.uint8)


def canonicalize(hard, activities):
    hard = np.asarray(hard)
    keys = []
    for cid in sorted(set(int(k) for k in hard.ravel() if k >= 0)):
        first = (10 ** 9,) * 3
        for c in range(hard.shape[0]):
            for s in range(hard.shape[1]):
                if hard[c, s] == cid:
                    on = np.flatnonzero(activities[c, :, s] > 0)
                    if on.size:
                        first = min(first, (c, int(on[0]), s))
        keys.append((first, cid))
    remap = {old: new for new, (_, old) in enumerate(sorted(keys))}
    out = np.full_like(hard, -2)
    for old, new in remap.items():
        out[hard == old] = new
    return out, remap


def join_close(spans, collar, alike):
    """Time-ordered spans [start, end, ...]: while the next span is `alike` the current one and
    begins no later than `collar` after its end, the current one swallows it (it takes the
    swallowed span's end).  Used for both min_duration_off rules (:245-252, :663-671)."""
    out, i = [], 0
    while i < len(spans):
        cur = list(spans[i])
        i += 1
        while i < len(spans) and alike(cur, spans[i]) and spans[i][0] - cur[1] <= collar:
            cur[1] = spans[i][1]
            i += 1
        out.append(cur)
    return out


def reconstruct(activities, hard, count, min_duration_off=0.0, centroids=None, defect=None):
    """_reconstruct_and_diarize (:969-1052): (segments, reindexed centroids)."""
    act = np.asarray(activities, np.float32)
    C, F, S = act.shape
    K = int(np.max(hard)) + 1
    if K <= 0:
        return [], centroids
    clustered = np.full((C, F, K), np.nan, np.float32)
    for c in range(C):
        for s in range(S):
            k = int(hard[c, s])
            if k >= 0:
                for f in range(F):
                    if np.isnan(clustered[c, f, k]) or act[c, f, s] > clustered[c, f, k]:
                        clustered[c, f, k] = act[c, f, s]
    a = aggregate(clustered, True, 0.0, defect)
    T = min(len(a), len(count))          # the two extents are equal: nothing is cropped
    mid = [0.5 * ((RF_START + t * RF_STEP) + (RF_START + t * RF_STEP + RF_DURATION)) for t in range(T)]
    raw = []
    for k in range(a.shape[1]):
        active, start, segs = False, None, []
        for t in range(T):
            best = 0
            for j in range(1, a.shape[1]):
                if a[t, j] > a[t, best] or (defect == "tie_high" and a[t, j] == a[t, best]):
                    best = j
            y = 1.0 if (min(int(count[t, 0]), 1) >= 1 and best == k) else 0.0
            if t == 0:
                start, active = mid[0], y > 0.5
            elif active and y < 0.5:
                segs.append([start, mid[t]])
                start, active = mid[t], False
            elif not active and y > 0.5:
                start, active = mid[t], True
        if active:
            segs.append([start, mid[T - 1]])
        if min_duration_off > 0.0:
            segs = join_close(segs, min_duration_off, lambda a, b: True)
        raw.extend((st, en, k) for st, en in segs)
    raw.sort(key=lambda x: x[0])
    names, segments = {}, []
    for st, en, k in raw:
        names.setdefault(k, len(names))
        segments.append({"start": round(st, 4), "end": round(en, 4), "speaker": names[k]})
    segments.sort(key=lambda s: s["start"])
    if centroids is not None and names:
        re = np.zeros((len(names), centroids.shape[1]), np.float32)
        for old, new in names.items():
            if old < centroids.shape[0]:
                re[new] = centroids[old]
        centroids = re
    return segments, centroids


def overlap_regions(binarized, chunk_starts, F, duration, min_duration=0.3):
    """_extract_overlap_regions (:512-552)."""
    fd = CHUNK_DURATION / F
    n_out = int(duration / fd) + 1
    over = np.zeros(n_out, np.float32)
    total = np.zeros(n_out, np.float32)
    for c, cs in enumerate(chunk_starts):
        t0 = cs / SAMPLE_RATE
        for f in range(F):
            o = int((t0 + f * fd) / fd)
            if 0 <= o < n_out:
                total[o] += 1
                if binarized[c, f].sum() >= 2:
                    over[o] += 1
    regions, inside, start = [], False, 0.0
    for f in range(n_out):
        on = total[f] > 0 and over[f] / total[f] > 0.5
        if on and not inside:
            start, inside = f * fd, True
        elif not on and inside:
            if f * fd - start >= min_duration:
                regions.append((start, min(f * fd, duration)))
            inside = False
    if inside and n_out * fd - start >= min_duration:
        regions.append((start, min(n_out * fd, duration)))
    return regions


def filter_mask(binarized, embeddings):
    b = np.asarray(binarized)
    C, F, S = b.shape
    out = np.zeros((C, S), bool)
    for c in range(C):
        single = b[c].sum(axis=1) == 1
        for s in range(S):
            out[c, s] = (b[c, single, s].sum() >= 0.2 * F) and not np.isnan(embeddings[c, s, 0])
    return out


def chunk_starts_1s(total):
    """_segment's starts (:714-726), the reference's float comparison kept."""
    starts, s = [], 0
    while True:
        starts.append(s)
        if (s + CHUNK_SAMPLES) / SAMPLE_RATE > total / SAMPLE_RATE:
            return starts
        s += STEP_SAMPLES


def diarize(binarized, embeddings, plda, threshold=0.6, Fa=0.07, Fb=0.8, min_duration_off=0.0):
    """Steps 4 to 8 of process (:591-671): (segments, centroids, hard)."""
    b = np.asarray(binarized, np.float32)
    count = speaker_count(b)
    hard, centroids = cluster(embeddings, filter_mask(b, embeddings), b, plda, threshold, Fa, Fb)
    hard = hard.copy()
    hard[b.sum(axis=1) == 0] = -2
    hard, remap = canonicalize(hard, b)
    if centroids is not None and remap:
        re = np.zeros_like(centroids)
        for old, new in remap.items():
            if old < len(centroids) and new < len(re):
                re[new] = centroids[old]
        centroids = re
    count = np.minimum(np.minimum(count, int(hard.max()) + 1).astype(np.int8), 1).astype(np.int8)
    segments, centroids = reconstruct(b, hard, count, min_duration_off, centroids)
    if min_duration_off > 0:
        spans = join_close([[g["start"], g["end"], g["speaker"]] for g in segments],
                           min_duration_off, lambda a, b: a[2] == b[2])
        segments = [{"start": a, "end": b, "speaker": k} for a, b, k in spans]
    return segments, centroids, hard
