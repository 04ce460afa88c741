"""Times WPE dereverberation on the device (zasr_wpe_*), split by stage, with the
float64 numpy restatement on the CPU and the drop-in run with preprocess_wpe beside it.

One measurement per process (one GPU program per call), each under its own time limit, stopping
at the first that fails; every call appends its JSON line to --out:

    T=sherpa-vietnamese-asr_amd/tools/wpe_bench.py; O=profiles/wpe/times.jsonl
    timeout -k 10 300 python $T --mode hour --out $O &&
    timeout -k 10 300 python $T --mode dropin --out $O &&
    timeout -k 10 600 python $T --mode cpu --out $O

    [--seconds 3600] [--reps 10] [--warmup 3] [--cpu-chunks 4]

Input: the synthetic speech of SURVEY 8d (zasr.synth_audio, one minute tiled to --seconds) cut
by the planner (zasr.plan.plan_chunks: ~30 s chunks with 3 s overlap).
  --mode hour    every chunk of the plan in one zasr.audio.apply_wpe_batch call on the signal in
                 HBM, output left on the device: wall time around the call (it ends synchronised),
                 median / min of `reps` after `warmup` untimed calls; stage_ms = the engine's
                 HIP-event split (STFT, iterations, inverse STFT; medians); with_limiter_ms = the
                 same with peak_limit=True (one peak read back per chunk).
  --mode dropin  the drop-in's two-worker loop over the plan with the rebound functions
                 (apply_wpe_dereverberation, adaptive_peak_limit, decode_chunk per chunk) on a
                 seeded Zipformer-M: chunk by chunk (ZASR_PLAN_AHEAD=0: one WPE call and one
                 batch-1 decode per chunk) against the WPE plan (one WPE batch, one batched
                 decode); wall times, and the WPE's share of each.
  --mode cpu     tests/wpe_reference.py (float64 numpy) on the first --cpu-chunks chunks of the
                 plan with this machine's threads, and the time that gives for the whole plan in
                 proportion to the samples (an extrapolation, marked as one).  No GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "sherpa-vietnamese-asr_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def _dropin(audio, plan, args) -> dict:
    from model_fixtures import m_model
    from zasr import asr_engine as ae
    from zasr import audio as za
    from zasr.dropin import install
    from zasr.plan import best_split, silent_regions
    eng, aud = types.ModuleType("ref_asr_engine"), types.ModuleType("ref_audio_preprocessing")
    eng.find_silent_regions = lambda a, *x, **k: silent_regions(a)
    eng.find_best_split_point = best_split
    install(eng, audio_module=aud, wpe=True)
    _, _, path = m_model()
    rec = ae.create_recognizer(path, 4, max_active_paths=8, hotwords=([], []))
    wpe_s = [0.0]
    lock = threading.Lock()

    def one(sig, i):
        s, e, _ = plan[i]
        t0 = time.perf_counter()
        c = aud.adaptive_peak_limit(aud.apply_wpe_dereverberation(sig[s:e]))
        with lock:
            wpe_s[0] += time.perf_counter() - t0
        return ae.decode_chunk(rec, c, s / 16000.0)

    def loop(sig):
        ts = [threading.Thread(target=lambda k=k: [one(sig, i) for i in range(k, len(plan), 2)])
              for k in (0, 1)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()

    class Pipe:
        config = {"preprocess_wpe": True}

        def plan(self, a):
            return eng.find_silent_regions(a)

    out = {}
    for name, env in (("chunk_by_chunk", "0"), ("wpe_plan", "1")):
        os.environ["ZASR_PLAN_AHEAD"] = env
        times = []
        for r in range(1 + max(1, args.reps // 3)):  # the first pass warms up
            wpe_s[0] = 0.0
            sig = audio.copy()  # a fresh signal: a fresh plan
            t0 = time.perf_counter()
            if env == "1":
                Pipe().plan(sig)
            loop(sig)
            times.append((time.perf_counter() - t0, wpe_s[0]))
        wall, w = min(times[1:])
        out[name] = {"wall_ms": wall * 1e3, "workers_in_wpe_calls_ms": w * 1e3}
    sig = audio.copy()
    t0 = time.perf_counter()
    za.apply_wpe_batch(sig, [(s, e) for s, e, _ in plan], peak_limit=True, device_out=True)
    out["wpe_batch_from_host_ms"] = (time.perf_counter() - t0) * 1e3
    out["wpe_share_of_plan_run"] = out["wpe_batch_from_host_ms"] / out["wpe_plan"]["wall_ms"]
    ae.clear_model_cache()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("hour", "dropin", "cpu"), default="hour")
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-chunks", type=int, default=4)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from zasr.plan import plan_chunks
    from zasr.synth_audio import synth_speech
    minute = synth_speech(60.0, 41)
    total = int(args.seconds * 16000)
    audio = np.ascontiguousarray(np.tile(minute, total // minute.shape[0] + 1)[:total])
    plan = plan_chunks(audio)
    spans = [(s, e) for s, e, _ in plan]
    samples = int(sum(e - s for s, e in spans))
    row = {"kind": args.mode, "seconds": args.seconds, "chunks": len(spans),
           "chunk_seconds": samples / 16000.0}
    if args.mode == "cpu":
        import wpe_reference as W
        n = min(args.cpu_chunks, len(spans))
        t0 = time.perf_counter()
        for s, e in spans[:n]:
            W.apply_wpe(audio[s:e])
        dt = time.perf_counter() - t0
        done = int(sum(e - s for s, e in spans[:n]))
        row.update(what="float64 numpy restatement (tests/wpe_reference.py)", threads=int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1)),
                   chunks_measured=n, ms_measured=dt * 1e3,
                   ms_whole_plan_extrapolated=dt * 1e3 * samples / done)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("no GPU: this mode measures on the device only")
        from zasr import audio as za
        if args.mode == "dropin":
            row.update(_dropin(audio, plan, args))
        else:
            d_audio = torch.from_numpy(audio).cuda()
            eng = za.wpe_engine()
            eng.set_profile(True)
            torch.cuda.synchronize()
            res = {}
            for name, lim in (("ms", False), ("with_limiter_ms", True)):
                ts, stages = [], []
                for r in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    za.apply_wpe_batch(d_audio, spans, peak_limit=lim, device_out=True)
                    torch.cuda.synchronize()
                    if r >= args.warmup:
                        ts.append((time.perf_counter() - t0) * 1e3)
                        stages.append(eng.stage_ms())
                res[name] = (ts, stages)
            ts, stages = res["ms"]
            med = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
            frames = int(sum(-(-(e - s + 256) // 128) + 1 for s, e in spans))
            row.update(groups=eng.last_groups, reps=args.reps, ms_median=float(np.median(ts)),
                       ms_min=float(np.min(ts)), stage_ms=med,
                       with_limiter_ms_median=float(np.median(res["with_limiter_ms"][0])),
                       frames=frames, problems=257 * len(spans),
                       realtime_factor=args.seconds * 1e3 / float(np.median(ts)))
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
