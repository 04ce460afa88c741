"""Times the diarization clustering (zasr.diarize over zasr_diar_*) against its
CPU restatement on the same inputs and the same machine.

    python sherpa-vietnamese-asr_amd/tools/diar_bench.py [--sizes 500,2000,6000] [--reps 5]
        [--warmup 2] [--no-cpu] [--out profiles/diarization/times.jsonl]

Inputs: N unit window embeddings (D = 192) around 6 speaker centres in turns of 5-40 windows
(seeded); N = 2000 is about 20 minutes of speech at the 0.6 s window step, 6000 an hour.  Per
size one JSON line:
  device_ms_*        zasr.diarize.senko_cluster with the device embedding (process()'s spectral
                     parameters): a host clock around the call, which ends synchronised
                     (median / min of `reps` after `warmup` untimed calls)
  stage_ms           similarity, prune (+ symmetrise + degrees) and eigs alone through the stage
                     entries (HIP events for the first two; eigs synchronises itself)
  passes, applications   the solver's outer passes and block Laplacian products
  eigs_GBps_per_application   N^2 * 4 bytes * applications / the eigs time: the matrix traffic
                     the algorithm needs over the whole solver time (Gram products, host
                     Rayleigh-Ritz and copies included, so a lower bound on the hot kernel's
                     rate; the kernel's own time comes from a rocprofv3 kernel trace)
  cpu_ms             the reference's spectral path restated in numpy on this machine (float32
                     similarity, argsort prune, numpy.linalg.eigh of the float32 Laplacian as
                     the reference calls it) plus the same host steps: one run
  speakers           found by both (they must agree)
ZASR_DIAR_LAP=fma in the environment times the plain-FMA product kernel instead of the
float64-MFMA one (profiles/diarization/README.md has both).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "sherpa-vietnamese-asr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

KW = dict(cluster_line=10, mer_cos=0.875, min_cluster_size=4, min_num_spks=1, max_num_spks=15,
          pval=0.012)


def embeddings(n: int, n_spk: int = 6, spread: float = 0.9, dim: int = 192, seed: int = 5):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_spk, dim))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    spk = np.zeros(n, np.int64)
    i, cur = 0, 0
    while i < n:
        t = int(rng.integers(5, 41))
        spk[i:i + t] = cur
        i += t
        cur = (cur + 1 + int(rng.integers(n_spk - 1))) % n_spk
    x = centres[spk] + rng.standard_normal((n, dim)) * (spread / np.sqrt(dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


def cpu_embed(X, pval, min_pnum, k):
    """core/speaker_diarization_senko_campp_optimized.py:199-218 in numpy, dtypes as there."""
    N = X.shape[0]
    xn = X / (np.linalg.norm(X, axis=1, keepdims=True) + 1e-10)
    M = xn @ xn.T
    n_elems = max(min(int((1 - pval) * N), N - min_pnum), 0)
    for i in range(N):
        M[i, np.argsort(M[i])[:n_elems]] = 0
    M = 0.5 * (M + M.T)
    np.fill_diagonal(M, 0)
    L = np.diag(np.abs(M).sum(axis=1)) - M
    w, v = np.linalg.eigh(L)
    return w[:k].astype(np.float64), v[:, :k].astype(np.float64)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500,2000,6000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    from zasr.binding import Diarizer
    from zasr.diarize import senko_cluster
    dz = Diarizer()
    lines = []
    for N in [int(s) for s in args.sizes.split(",")]:
        X = embeddings(N)

        def dev_embed(x, pval, min_pnum, k):
            return dz.spectral_embed(x, pval=pval, min_pnum=min_pnum, k=k)
        for _ in range(args.warmup):
            labels = senko_cluster(X, embed=dev_embed, **KW)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            labels = senko_cluster(X, embed=dev_embed, **KW)
            ts.append((time.perf_counter() - t0) * 1e3)
        passes, apps = dz.last_stats()
        # stages alone
        dX = torch.from_numpy(X).cuda()
        dM = torch.empty((N, N), dtype=torch.float32, device="cuda")
        ddeg = torch.empty(N, dtype=torch.float64, device="cuda")
        st = {"similarity": [], "prune": [], "eigs": []}
        for r in range(args.warmup + args.reps):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            dz.similarity(dX.data_ptr(), N, 192, dM.data_ptr())
            ev[1].record()
            dz.prune(dM.data_ptr(), N, KW["pval"], 6, ddeg.data_ptr())
            ev[2].record()
            ev[2].synchronize()
            t0 = time.perf_counter()
            dz.eigs(dM.data_ptr(), ddeg.data_ptr(), N, 16)
            te = (time.perf_counter() - t0) * 1e3
            if r >= args.warmup:
                st["similarity"].append(ev[0].elapsed_time(ev[1]))
                st["prune"].append(ev[1].elapsed_time(ev[2]))
                st["eigs"].append(te)
        stage = {k: float(np.median(v)) for k, v in st.items()}
        row = {"N": N, "D": 192, "reps": args.reps,
               "device_ms_median": float(np.median(ts)), "device_ms_min": float(np.min(ts)),
               "stage_ms": stage, "passes": passes, "applications": apps,
               "eigs_GBps_per_application": 4.0 * N * N * apps / (stage["eigs"] * 1e-3) / 1e9,
               "speakers": int(len(np.unique(labels)))}
        if not args.no_cpu:
            t0 = time.perf_counter()
            cl = senko_cluster(X, embed=cpu_embed, **KW)
            row["cpu_ms"] = (time.perf_counter() - t0) * 1e3
            row["cpu_speakers"] = int(len(np.unique(cl)))
            row["speedup"] = row["cpu_ms"] / row["device_ms_median"]
            assert row["cpu_speakers"] == row["speakers"], row
        lines.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
