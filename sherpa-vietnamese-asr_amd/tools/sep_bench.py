"""Times the Conv-TasNet overlap separation stage (zasr_sep_*), split by stage,
with a CPU comparison.

One measurement per process (one GPU program per call), each under its own time limit, stopping
at the first that fails; every call appends its JSON line to --out:

    T=sherpa-vietnamese-asr_amd/tools/sep_bench.py; O=profiles/separation/times.jsonl
    timeout -k 10 300 python $T --mode hour --out $O &&
    timeout -k 10 300 python $T --mode region --out $O &&
    timeout -k 10 600 python $T --mode cpu --out $O

    [--regions 60] [--seed 3] [--reps 10] [--warmup 3] [--region-seconds 3]

Input: a two-voice mixture of synthetic speech (zasr.synth_audio, one minute tiled to an hour)
in HBM; seeded weights (zasr.convtasnet.synth_weights).
  --mode hour    one hour's overlap in one call: --regions regions of 1-10 s (seeded uniform
                 lengths, evenly spread starts; the share of the hour they cover is reported)
                 through zasr_sep_separate_device with the output left on the device.  HIP events
                 on the caller's stream around the call (it is ordered after that stream and
                 ends synchronised), median / min of `reps` after `warmup` untimed calls;
                 stage_ms = the engine's HIP-event split (encoder, 1x1 GEMMs, norms + depthwise,
                 mask + decoder; medians); GFLOP / GB per stage from zasr.convtasnet and the
                 TFLOP/s and TB/s they give.
  --mode region  one region of --region-seconds alone, the same way.
  --mode cpu     torch float32 evaluation of the SAME network (tests/convtasnet_reference.py
                 forward_modules: a port, not the reference's onnxruntime session) on one region
                 of --region-seconds with this machine's threads.  No GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "sherpa-vietnamese-asr_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("hour", "region", "cpu"), default="hour")
    ap.add_argument("--regions", type=int, default=60)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--region-seconds", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from zasr.convtasnet import (ConvTasNetConfig, region_bytes, region_flops, save_model_dir,
                                 synth_weights)
    from zasr.synth_audio import synth_speech
    cfg = ConvTasNetConfig()
    w = synth_weights(cfg)
    minute = (0.6 * synth_speech(60.0, 41) + 0.5 * synth_speech(60.0, 57)).astype(np.float32)
    total = 3600 * 16000
    if args.mode == "hour":
        rng = np.random.Generator(np.random.PCG64(args.seed))
        lengths = (rng.uniform(1.0, 10.0, args.regions) * 16000).astype(np.int64)
        starts = (np.arange(args.regions) * (total // args.regions)).astype(np.int64)
    else:
        lengths = np.array([int(args.region_seconds * 16000)], np.int64)
        starts = np.array([5 * 16000], np.int64)
    if args.mode == "cpu":
        from convtasnet_reference import forward_modules
        x = minute[int(starts[0]):int(starts[0] + lengths[0])]
        forward_modules(cfg, w, x[:16000], torch.float32)
        t0 = time.perf_counter()
        forward_modules(cfg, w, x, torch.float32)
        row = {"kind": "cpu", "what": "torch float32 port of the same network (not onnxruntime)",
               "threads": torch.get_num_threads(), "seconds": float(lengths[0]) / 16000.0,
               "ms": (time.perf_counter() - t0) * 1e3}
    else:
        if not torch.cuda.is_available():
            raise SystemExit("no GPU: this mode measures on the device only")
        from zasr.binding import SepSession
        with tempfile.TemporaryDirectory(prefix="zasr_sepbench_") as d:  # read at construction only
            save_model_dir(d, cfg, w)
            sess = SepSession(d)
        audio = np.tile(minute, total // minute.shape[0] + 1)[:total]
        d_audio = torch.from_numpy(audio).cuda()
        d_out = torch.empty(2 * int(lengths.sum()), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        flops, gbytes = {}, 0.0
        for T in lengths:
            for k, v in region_flops(cfg, int(T)).items():
                flops[k] = flops.get(k, 0.0) + v / 1e9
            gbytes += region_bytes(cfg, int(T)) / 1e9
        sess.set_profile(True)
        stream = torch.cuda.current_stream()
        ts, stages = [], []
        for r in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            sess.separate_device(d_audio.data_ptr(), total, starts, lengths, d_out=d_out.data_ptr(),
                                 stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            if r >= args.warmup:
                ts.append(e0.elapsed_time(e1))
                stages.append(sess.stage_ms())
        med = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
        secs = float(lengths.sum()) / 16000.0
        row = {"kind": args.mode, "regions": int(len(lengths)), "overlap_seconds": secs,
               "share_of_hour": secs / 3600.0, "frames": int(sum(cfg.num_frames(int(T)) for T in lengths)),
               "groups": sess.last_groups, "reps": args.reps, "ms_median": float(np.median(ts)),
               "ms_min": float(np.min(ts)), "stage_ms": med, "gflop": flops,
               "tflops": {k: flops[k] / med[k] if med[k] > 0 else 0.0 for k in flops},
               "activation_gb": gbytes, "tb_per_s": gbytes / float(np.median(ts)),
               "realtime_factor": secs * 1e3 / float(np.median(ts))}
        sess.close()
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
