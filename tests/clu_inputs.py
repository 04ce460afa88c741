"""Seeded inputs of the centroid-AHC tests (test_vbx_reference.py on the CPU, test_gpu_clu.py on
the device): unnormalised float32 train rows [N][D] and the threshold of each case.

Exact partition equality is only meaningful away from ties; test_vbx_reference.py checks that
every non-degenerate case here keeps its partition under a +-2 ulp perturbation of the
normalised rows."""
import numpy as np

THRESHOLD = 0.6


def speakers(seed, N, n_spk, D, spread=(0.2, 0.3)):
    """Well-separated speakers: orthonormal centres, x = centre[label] + s g / sqrt(D) with
    s ~ U(spread) per row (rows of one speaker lie about s sqrt(2) apart after normalisation,
    different speakers about sqrt(2)), then every row rescaled by U(0.5, 2)."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((D, min(n_spk, D))))
    centres = q.T
    labels = rng.integers(0, centres.shape[0], N)
    s = rng.uniform(spread[0], spread[1], (N, 1))
    x = centres[labels] + s * rng.standard_normal((N, D)) / np.sqrt(D)
    x *= rng.uniform(0.5, 2.0, (N, 1))
    return np.ascontiguousarray(x, np.float32), labels


def close_speakers(seed, N=257, D=256):
    """Four tight speakers, two of them 0.5-0.7 apart after normalisation: the threshold
    decides between real candidates and the cluster count is not the speaker count."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((D, 5)))
    c = q.T[:4].copy()
    c[3] = c[2] + 0.62 * q.T[4]          # |c3/|c3| - c2| = 0.57
    c[3] /= np.linalg.norm(c[3])
    labels = rng.integers(0, 4, N)
    x = c[labels] + 0.08 * rng.standard_normal((N, D)) / np.sqrt(D)
    x *= rng.uniform(0.5, 2.0, (N, 1))
    return np.ascontiguousarray(x, np.float32), labels


def _tangent(points, D=3, scale=1.0):
    """Rows (u, v, 1, 0, ...) * scale: points of the plane z = 1, normalised by the AHC."""
    x = np.zeros((len(points), D), np.float32)
    for r, (u, v) in enumerate(points):
        x[r, 0], x[r, 1], x[r, 2] = u, v, 1.0
    return x * np.float32(scale)


def perturb_ulp(Xn, seed, ulps=2):
    """Every float32 entry moved by a seeded whole number of ulps in [-ulps, ulps]."""
    rng = np.random.default_rng(seed)
    steps = rng.integers(-ulps, ulps + 1, Xn.shape)
    out = np.array(Xn, np.float32)
    for s in range(1, ulps + 1):
        out = np.where(steps >= s, np.nextafter(out, np.float32(np.inf)), out)
        out = np.where(steps <= -s, np.nextafter(out, np.float32(-np.inf)), out)
    return out.astype(np.float32)


def threshold_case():
    """(X, the exact float64 distance of its two normalised rows as numpy computes it): a pair
    AT the threshold merges, as fcluster's `<=` has it.  CPU only: the comparison is exact."""
    X = _tangent([(-0.3, 0.0), (0.3, 0.0)])
    xn = X / (np.linalg.norm(X, axis=1, keepdims=True) + 1e-10)
    d = xn[0].astype(np.float64) - xn[1].astype(np.float64)
    return X, float(np.sqrt((d * d).sum()))


# name -> (X float32 [N][D], threshold, degenerate). A degenerate case has exact ties (its one
# partition does not depend on their order) and is left out of the perturbation check.
def cases():
    out = {}
    out["two_merged"] = (_tangent([(-0.2, 0.0), (0.2, 0.0)], scale=3.0), THRESHOLD, False)
    out["two_apart"] = (_tangent([(-0.5, 0.0), (0.5, 0.0)], scale=0.7), THRESHOLD, False)
    # rows 0 and 1 merge at about 0.52; row 2 is about 0.55 from either and 0.48 from their
    # centroid: the second merge is lower than the first (an inversion), one cluster
    out["inversion3"] = (_tangent([(-0.28, 0.0), (0.28, 0.0), (0.013, 0.52)], D=4), THRESHOLD, False)
    # rows 0 and 1 merge at 0.521; row 2 is 0.566 from their centroid but 0.623 away on average:
    # centroid linkage gives one cluster, average linkage two
    out["centroid_merges3"] = (_tangent([(-0.27, 0.0), (0.27, 0.0), (0.013, 0.66)], D=4),
                               THRESHOLD, False)
    # row 2 is 0.616 from the centroid: two clusters; the update without squares and roots
    # would give 0.54 and one cluster
    out["centroid_splits3"] = (_tangent([(-0.27, 0.0), (0.27, 0.0), (0.013, 0.74)], D=4),
                               THRESHOLD, False)
    # a zero row normalises to zero because of the + 1e-10 (without it: NaN); it stays alone
    z = _tangent([(-0.1, 0.0), (0.1, 0.0), (0.0, 0.1), (0.0, 0.0)], D=5)
    z[3] = 0.0
    out["zero_row4"] = (z, THRESHOLD, False)
    row = np.random.default_rng(8).standard_normal((1, 256)).astype(np.float32)
    out["identical8"] = (np.repeat(row, 8, axis=0), THRESHOLD, True)
    for N, k in ((65, 3), (257, 5), (1025, 8)):
        out[f"speakers_{N}"] = (speakers(100 + N, N, k, 256)[0], THRESHOLD, False)
    out["loader_d5"] = (speakers(205, 130, 3, 5)[0], THRESHOLD, False)
    out["loader_d511"] = (speakers(711, 130, 4, 511)[0], THRESHOLD, False)
    out["close_257"] = (close_speakers(31)[0], THRESHOLD, False)
    return out
