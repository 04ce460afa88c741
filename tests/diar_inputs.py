"""Seeded inputs of the diarization tests: window embeddings and window plans regenerated from
a case's parameters, so the goldens carry only parameters and results
(tests/golden/make_golden_diar.py), and the LAPACK spectral embedding the host tests hand to
zasr.diarize in place of the device's."""
import numpy as np


def speaker_turns(rng, n: int, n_spk: int, lo: int = 5, hi: int = 40) -> np.ndarray:
    """Speaker id per window: turns of lo..hi windows, the speaker changing at every turn."""
    out = np.zeros(n, np.int64)
    i, cur = 0, int(rng.integers(n_spk))
    while i < n:
        t = int(rng.integers(lo, hi + 1))
        out[i:i + t] = cur
        i += t
        if n_spk > 1:
            cur = (cur + 1 + int(rng.integers(n_spk - 1))) % n_spk
    return out


def make_embeddings(seed: int, n: int, n_spk: int, spread: float = 0.35, dim: int = 192,
                    turns=None, centre_cos=None):
    """Unit float32 vectors [n][dim] around n_spk random unit centres (noise of norm about
    `spread` relative to the centre's), and the speaker of every window.  turns: explicit
    speaker ids (overrides the random turns of 5-40 windows).  centre_cos: the cosine between
    centres 0 and 1 (centre 1 is rebuilt at that angle from centre 0)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_spk, dim))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    if centre_cos is not None:
        o = centres[1] - (centres[1] @ centres[0]) * centres[0]
        o /= np.linalg.norm(o)
        centres[1] = centre_cos * centres[0] + np.sqrt(1.0 - centre_cos ** 2) * o
    spk = speaker_turns(rng, n, n_spk) if turns is None else np.asarray(turns, np.int64)
    assert spk.shape == (n,)
    x = centres[spk] + rng.standard_normal((n, dim)) * (spread / np.sqrt(dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), spk


def case_embeddings(case: dict):
    """The embeddings of one golden case (its "seed", "n", "spk", "spread" and the optional
    "turns" as [speaker, windows] runs and "centre_cos")."""
    turns = None
    if case.get("turns"):
        turns = np.concatenate([np.full(m, s, np.int64) for s, m in case["turns"]])
    return make_embeddings(case["seed"], case["n"], case["spk"], case["spread"], turns=turns,
                           centre_cos=case.get("centre_cos"))[0]


def window_plan(n: int, seed: int):
    """A pipe-shaped plan of exactly n windows: region offsets and lengths in samples and the
    (region, first frame, frames) rows of zasr.pipeline.FullPipe: regions of 2-40 s separated
    by 0.3-6 s, 150-frame windows every 60 frames while pos + 150 < frames plus the pulled-back
    tail, the third region shorter than one window (embedded whole)."""
    rng = np.random.default_rng(seed + 7919)
    off, length, rows = [], [], []
    t = 8000
    while len(rows) < n:
        r = len(off)
        sec = 1.2 if r == 2 else float(rng.uniform(2.0, 40.0))
        m = int(sec * 16000)
        frames = (m - 400) // 160 + 1
        off.append(t)
        length.append(m)
        if frames < 150:
            rows.append((r, 0, frames))
        else:
            pos = 0
            while pos + 150 < frames:
                rows.append((r, pos, 150))
                pos += 60
            rows.append((r, max(0, frames - 150), 150))
        t += m + int(rng.uniform(0.3, 6.0) * 16000)
    rows = rows[:n]
    return off, length, np.asarray(rows, np.int64).reshape(-1, 3), (t + 8000) / 16000.0


def pruned_similarity(X: np.ndarray, pval: float, min_pnum: int) -> np.ndarray:
    """The reference's float32 similarity after p_pruning, symmetrise and the zero diagonal
    (core/speaker_diarization_senko_campp_optimized.py:199-213), in numpy."""
    X = np.asarray(X, np.float32)
    N = X.shape[0]
    xn = X / (np.linalg.norm(X, axis=1, keepdims=True) + np.float32(1e-10))
    M = xn @ xn.T
    n_elems = max(min(int((1 - pval) * N), N - min_pnum), 0)
    for i in range(N):
        M[i, np.argsort(M[i])[:n_elems]] = 0
    M = np.float32(0.5) * (M + M.T)
    np.fill_diagonal(M, 0)
    return M


def lapack_embed(X, pval: float, min_pnum: int, k: int):
    """zasr.diarize's `embed` on LAPACK: numpy.linalg.eigh of the float64 Laplacian of
    pruned_similarity.  Not the code under test."""
    M = pruned_similarity(X, pval, min_pnum).astype(np.float64)
    L = np.diag(np.abs(M).sum(1)) - M
    w, v = np.linalg.eigh(L)
    return w[:k].copy(), v[:, :k].copy()


def canonical(labels) -> list:
    """Labels renumbered by first occurrence: equal lists = equal partitions."""
    seen = {}
    return [seen.setdefault(int(l), len(seen)) for l in labels]
