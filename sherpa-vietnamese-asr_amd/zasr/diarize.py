"""Speaker diarization of the CAM++ window embeddings: who spoke when.

The reference's clustering and segment logic (core/speaker_diarization_senko_campp_optimized.py)
in numpy, around the device's spectral embedding (include/zasr.h zasr_diar_*): the N x N cosine
matrix, its prune and the eigenvectors of the Laplacian are the O(N^2) - O(N^3) part and run
on the GPU; what is O(N D) and branchy stays here -- the eigengap rule and k-means (:219-233),
Senko's minor-cluster filter, centre merge and relabel (:254-301), labels to segments
(:622-654), the overlap split (:769-774) and the post-processing 7a-7d (:778-819).

`embed` is the spectral embedding: embed(X, pval, min_pnum, k) -> (lambdas [k] ascending,
vecs [N][k]) of L = diag(sum |M|) - M.  The default runs on the device
(zasr.binding.Diarizer.spectral_embed); the CPU tests pass one built on numpy.linalg.eigh.

Deviations from the reference, both by design:
  - k-means is a deterministic Lloyd iteration from a farthest-point start, not sklearn's
    seeded k-means++; on well-separated spectral rows both find the same partition.
  - files of 20 minutes and more use the same spectral clustering; the reference switches to
    UMAP + HDBSCAN there (:747-756), which is unseeded and so not reproducible.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_EIGS = 16          # eigenpairs the device solver returns at most (max_num_spks 15 + 1)
WINDOW_SEC = 1.5       # :self.window
FRAME_SHIFT_MS = 10.0
WINDOW_FRAMES = 150

Embed = Callable[[np.ndarray, float, int, int], Tuple[np.ndarray, np.ndarray]]

_device = None


def device_embed(X: np.ndarray, pval: float, min_pnum: int, k: int):
    """The default `embed`: one zasr.binding.Diarizer on the current device, made on first use."""
    global _device
    if _device is None:
        from zasr.binding import Diarizer
        _device = Diarizer()
    return _device.spectral_embed(X, pval=pval, min_pnum=min_pnum, k=k)


def cosine_similarity(X: np.ndarray, Y: Optional[np.ndarray] = None) -> np.ndarray:
    """:183-189."""
    if Y is None:
        Y = X
    xn = X / (np.linalg.norm(X, axis=1, keepdims=True) + 1e-10)
    yn = Y / (np.linalg.norm(Y, axis=1, keepdims=True) + 1e-10)
    return xn @ yn.T


def kmeans(P: np.ndarray, n_clusters: int, max_iter: int = 100) -> np.ndarray:
    """Deterministic Lloyd iteration on the rows of P: farthest-point start from the row of
    largest norm, at most max_iter rounds, an empty cluster reseeded with the point farthest
    from its centre.  Ties go to the lowest index."""
    P = np.asarray(P, np.float64)
    n = P.shape[0]
    n_clusters = max(1, min(int(n_clusters), n))
    centres = np.empty((n_clusters, P.shape[1]))
    centres[0] = P[int(np.argmax((P * P).sum(1)))]
    d2 = ((P - centres[0]) ** 2).sum(1)
    for c in range(1, n_clusters):
        centres[c] = P[int(np.argmax(d2))]
        d2 = np.minimum(d2, ((P - centres[c]) ** 2).sum(1))
    labels = np.full(n, -1, np.int64)
    for _ in range(max_iter):
        dist = ((P[:, None, :] - centres[None, :, :]) ** 2).sum(2)
        new = np.argmin(dist, axis=1)
        own = dist[np.arange(n), new]
        for c in range(n_clusters):
            if not np.any(new == c):
                # among the points whose cluster keeps another member
                cand = np.where(np.bincount(new, minlength=n_clusters)[new] > 1)[0]
                far = int(cand[np.argmax(own[cand])])
                new[far] = c
                own[far] = 0.0
        if np.array_equal(new, labels):
            break
        labels = new
        for c in range(n_clusters):
            centres[c] = P[labels == c].mean(0)
    return labels.astype(np.int32)


def senko_spectral(X: np.ndarray, min_num_spks: int = 1, max_num_spks: int = 10,
                   pval: float = 0.02, min_pnum: int = 6, oracle_num: Optional[int] = None,
                   embed: Optional[Embed] = None) -> np.ndarray:
    """:192-233 with the similarity, prune, Laplacian and eigenvectors in `embed`."""
    X = np.asarray(X)
    N = X.shape[0]
    if N <= 1:
        return np.zeros(N, dtype=np.int32)
    need = int(oracle_num) if oracle_num is not None else int(max_num_spks) + 1
    if min(need, N) > MAX_EIGS:
        raise ValueError(f"at most {MAX_EIGS - 1} speakers: the solver returns {MAX_EIGS} eigenpairs")
    k = min(N, MAX_EIGS)
    lambdas, vecs = (embed or device_embed)(X, float(pval), int(min_pnum), k)
    if oracle_num is not None:
        num_of_spk = int(oracle_num)
    else:
        sub = lambdas[min_num_spks - 1:max_num_spks + 1]
        gaps = [float(sub[i + 1]) - float(sub[i]) for i in range(len(sub) - 1)]
        if not gaps:
            return np.zeros(N, dtype=np.int32)
        num_of_spk = int(np.argmax(gaps)) + min_num_spks
    num_of_spk = max(1, min(num_of_spk, N))
    return kmeans(np.asarray(vecs)[:, :num_of_spk], num_of_spk)


def senko_cluster(X: np.ndarray, cluster_type: str = "spectral", cluster_line: int = 10,
                  mer_cos: Optional[float] = 0.875, min_cluster_size: int = 4,
                  embed: Optional[Embed] = None, **kwargs) -> np.ndarray:
    """:254-301 (Senko CommonClustering)."""
    X = np.asarray(X)
    N = X.shape[0]
    if N < cluster_line:
        return np.ones(N, dtype=np.int32)
    if cluster_type == "umap_hdbscan":
        raise ValueError("cluster_type 'umap_hdbscan' is not built: the reference's UMAP + HDBSCAN "
                         "is unseeded (not reproducible); long files use the spectral clustering")
    if cluster_type != "spectral":
        raise ValueError(f"unknown cluster_type {cluster_type!r}")
    labels = senko_spectral(X, embed=embed, **kwargs).copy()

    # filter_minor_cluster
    cset = np.unique(labels)
    csize = np.array([(labels == i).sum() for i in cset])
    minor_idx = np.where(csize < min_cluster_size)[0]
    if len(minor_idx) > 0:
        minor_cset = cset[minor_idx]
        major_idx = np.where(csize >= min_cluster_size)[0]
        if len(major_idx) > 0:
            major_cset = cset[major_idx]
            major_center = np.stack([X[labels == i].mean(0) for i in major_cset])
            for i in range(len(labels)):
                if labels[i] in minor_cset:
                    cos_sim = cosine_similarity(X[i:i + 1], major_center)
                    labels[i] = major_cset[cos_sim.argmax()]
        else:
            labels = np.zeros(N, dtype=np.int32)

    # merge_by_cos
    if mer_cos is not None and mer_cos > 0:
        while True:
            cset = np.unique(labels)
            if len(cset) <= 1:
                break
            centers = np.stack([X[labels == i].mean(0) for i in cset])
            affinity = np.triu(cosine_similarity(centers, centers), 1)
            idx = np.unravel_index(np.argmax(affinity), affinity.shape)
            if affinity[idx] < mer_cos:
                break
            c1, c2 = cset[np.array(idx)]
            labels[labels == c2] = c1

    # relabel
    unique = np.unique(labels)
    remap = {old: new for new, old in enumerate(unique)}
    return np.array([remap[l] for l in labels], dtype=np.int32)


def segments_from_labels(window_times: Sequence[Tuple[float, float]], labels: Sequence[int],
                         min_duration_off: float = 0.0) -> List[Dict]:
    """:622-654: consecutive windows of one label closer than min_duration_off + 0.01 s merge."""
    if len(window_times) == 0:
        return []
    segments = []
    current_start, current_end = window_times[0]
    current_label = labels[0]
    for i in range(1, len(window_times)):
        w_start, w_end = window_times[i]
        label = labels[i]
        if label == current_label and (w_start - current_end) < min_duration_off + 0.01:
            current_end = w_end
        else:
            segments.append({"start": float(current_start), "end": float(current_end),
                             "speaker": int(current_label)})
            current_start, current_end, current_label = w_start, w_end, label
    segments.append({"start": float(current_start), "end": float(current_end),
                     "speaker": int(current_label)})
    return segments


def segments_from_windows(window_times: Sequence[Tuple[float, float]], labels: Sequence[int],
                          min_duration_off: float = 0.0) -> List[Dict]:
    """Labels to the reference's final segment list, in its order: segments_from_labels, the
    overlap split at the midpoint (:769-774), then 7a-7d (:778-819)."""
    segments = segments_from_labels(window_times, labels, min_duration_off)

    if len(segments) > 1:
        for i in range(len(segments) - 1):
            if segments[i]["end"] > segments[i + 1]["start"]:
                mid = (segments[i]["end"] + segments[i + 1]["start"]) / 2
                segments[i]["end"] = mid
                segments[i + 1]["start"] = mid

    # 7a: merge adjacent same-speaker segments with a gap <= 4 s
    if len(segments) > 1:
        merged = [segments[0]]
        for seg in segments[1:]:
            prev = merged[-1]
            if seg["speaker"] == prev["speaker"] and seg["start"] - prev["end"] <= 4.0:
                prev["end"] = seg["end"]
            else:
                merged.append(seg)
        segments = merged

    # 7b: drop segments <= 0.78 s (absorbed when the same speaker is on both sides)
    if len(segments) > 1:
        filtered: List[Dict] = []
        for i, seg in enumerate(segments):
            if seg["end"] - seg["start"] > 0.78:
                filtered.append(seg)
            else:
                prev_spk = filtered[-1]["speaker"] if filtered else None
                next_spk = segments[i + 1]["speaker"] if i + 1 < len(segments) else None
                if prev_spk is not None and prev_spk == next_spk:
                    filtered[-1]["end"] = seg["end"]
        if filtered:
            segments = filtered

    # 7c: final merge of adjacent same-speaker segments
    if len(segments) > 1:
        final = [segments[0]]
        for seg in segments[1:]:
            if seg["speaker"] == final[-1]["speaker"]:
                final[-1]["end"] = seg["end"]
            else:
                final.append(seg)
        segments = final

    # 7d: speakers re-ranked by total speaking time
    spk_dur: Dict[int, float] = {}
    for seg in segments:
        spk_dur[seg["speaker"]] = spk_dur.get(seg["speaker"], 0) + (seg["end"] - seg["start"])
    ranked = sorted(spk_dur.keys(), key=lambda s: spk_dur[s], reverse=True)
    rerank = {old: new for new, old in enumerate(ranked)}
    for seg in segments:
        seg["speaker"] = rerank[seg["speaker"]]
    return segments


def window_times(windows: np.ndarray, region_off: Sequence[int],
                 region_len: Sequence[int]) -> List[Tuple[float, float]]:
    """(start, end) seconds of the pipe's (region, first frame, frames) rows (:561-580): a
    window starts first * 10 ms into its region and lasts 1.5 s; a region shorter than one
    window is embedded whole and takes the region's own times."""
    out = []
    for r, first, frames in np.asarray(windows, np.int64).reshape(-1, 3):
        start = region_off[r] / 16000.0
        if frames < WINDOW_FRAMES:
            out.append((start, (region_off[r] + region_len[r]) / 16000.0))
        else:
            ws = start + int(first) * FRAME_SHIFT_MS / 1000.0
            out.append((ws, ws + WINDOW_SEC))
    return out


def cluster_windows(embeddings: np.ndarray, num_speakers: int = -1, min_speakers: int = 1,
                    mer_cos: float = 0.875, embed: Optional[Embed] = None) -> np.ndarray:
    """process()'s clustering step (:726-756) with the spectral parameters of :738-746 at any
    duration."""
    n_embs = embeddings.shape[0]
    min_spk = num_speakers if num_speakers > 0 else min_speakers
    if n_embs <= 2:
        return np.zeros(n_embs, dtype=np.int32)
    return senko_cluster(embeddings, cluster_type="spectral", cluster_line=10, mer_cos=mer_cos,
                         min_cluster_size=4, min_num_spks=min_spk, max_num_spks=15, pval=0.012,
                         embed=embed)


def diarize(embeddings: np.ndarray, windows: np.ndarray, region_off: Sequence[int],
            region_len: Sequence[int], duration: float, num_speakers: int = -1,
            min_speakers: int = 1, mer_cos: float = 0.875, embed: Optional[Embed] = None,
            return_labels: bool = False):
    """process() from the clustering on (:726-830) for the pipe's windows: the who-spoke-when
    list [{"start", "end", "speaker"}], speakers ranked by speaking time.  return_labels: also
    the per-window cluster labels (before the re-ranking 7d)."""
    embeddings = np.asarray(embeddings)
    if duration < 0.5 or embeddings.shape[0] == 0:
        return ([], np.zeros(0, np.int32)) if return_labels else []
    labels = cluster_windows(embeddings, num_speakers, min_speakers, mer_cos, embed)
    segments = segments_from_windows(window_times(windows, region_off, region_len), labels)
    return (segments, labels) if return_labels else segments
