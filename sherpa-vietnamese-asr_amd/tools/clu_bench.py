#!/usr/bin/env python3
"""Community-1 back end timings: the device centroid AHC against scipy's
linkage + fcluster on the same host and the same rows, and the whole host back end (VBx,
assignment, reconstruction) at an hour's 3592 chunks.  Synthetic train rows: 6 speakers,
D = 256.  Medians of 3 after one warm-up.  Prints one JSON line per measurement.

    python tools/clu_bench.py [--sizes 2048 4096 8192] [--no-scipy] [--no-backend]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from zasr import vbx  # noqa: E402
from zasr.binding import CluSession  # noqa: E402


def train_rows(seed, N, n_spk=6, D=256):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((D, n_spk)))
    lab = rng.integers(0, n_spk, N)
    x = q.T[lab] + rng.uniform(0.2, 0.3, (N, 1)) * rng.standard_normal((N, D)) / np.sqrt(D)
    return np.ascontiguousarray(x * rng.uniform(0.5, 2.0, (N, 1)), np.float32), lab


def median3(fn):
    fn()
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return sorted(t)[1]


def synthetic_hour(seed=3, chunks=3592, frames=589, n_spk=6, D=256):
    """Binarized activities [chunks][frames][3] (turn-taking speakers, some overlap) and
    embeddings [chunks][3][D] that follow the speaker of each local slot."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((D, n_spk)))
    binar = np.zeros((chunks, frames, 3), np.float32)
    emb = np.zeros((chunks, 3, D), np.float32)
    for c in range(chunks):
        spk = rng.permutation(n_spk)[:3]
        cut = np.sort(rng.integers(0, frames, 2))
        binar[c, :cut[0], 0] = 1
        binar[c, max(cut[0] - 30, 0):cut[1], 1] = 1
        if rng.random() < 0.5:
            binar[c, cut[1]:, 2] = 1
        emb[c] = q.T[spk] + 0.25 * rng.standard_normal((3, D)) / np.sqrt(D)
    return binar, emb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[2048, 4096, 8192])
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--no-backend", action="store_true")
    a = ap.parse_args()
    clu = CluSession()
    for N in a.sizes:
        X, _ = train_rows(N, N)
        out = {"what": "ahc", "N": N, "D": X.shape[1]}
        for route in range(clu.n_routes()):
            clu.force_route(route)
            out[f"device_route{route}_s"] = round(median3(lambda: clu.ahc(X, 0.6)), 5)
        clu.force_route(0)
        lab = clu.ahc(X, 0.6)
        out["clusters"] = int(lab.max()) + 1
        out["merges"], out["rescans"] = clu.last_stats()
        clu.set_profile(True)
        clu.ahc(X, 0.6)
        out["stage_ms"] = {k: round(v, 3) for k, v in clu.stage_ms().items()}
        clu.set_profile(False)
        if not a.no_scipy:
            from scipy.cluster.hierarchy import fcluster, linkage
            xn = X / (np.linalg.norm(X, axis=1, keepdims=True) + 1e-10)
            sp = [None]

            def run():
                sp[0] = fcluster(linkage(xn, method="centroid", metric="euclidean"), 0.6,
                                 criterion="distance")
            out["scipy_s"] = round(median3(run), 5)
            _, first = np.unique(sp[0], return_index=True)
            order = {l: r for r, l in enumerate(sp[0][np.sort(first)])}
            out["same_partition"] = bool(np.array_equal([order[l] for l in sp[0]], lab))
        print(json.dumps(out), flush=True)
    if not a.no_backend:
        binar, emb = synthetic_hour()
        plda = vbx.synthetic_plda(seed=1, dim=emb.shape[2])
        chunks, frames = binar.shape[:2]
        res = {}

        def run():
            res["segments"], res["info"] = vbx.diarize_from_embeddings(binar, emb, clu, plda)
        t = median3(run)
        print(json.dumps({"what": "backend", "chunks": chunks, "total_s": round(t, 4),
                          "stages_s": {k: round(v, 4) for k, v in res["info"]["times"].items()},
                          "train_rows": res["info"]["train_rows"],
                          "segments": len(res["segments"])}), flush=True)
    clu.close()


if __name__ == "__main__":
    main()
