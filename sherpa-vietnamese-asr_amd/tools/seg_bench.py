"""Times the PyanNet segmentation stage (zasr_seg_*) on one hour of audio as one
file, split by stage, with the recurrence's group-size A/B and a CPU comparison.

One measurement per process (one GPU program per call), each under its own time limit, stopping
at the first that fails; every call appends its JSON line to --out:

    T=sherpa-vietnamese-asr_amd/tools/seg_bench.py; O=profiles/segmentation/times.jsonl
    timeout -k 10 300 python $T --mode hour --out $O &&
    for B in 1 2 4 8 16; do timeout -k 10 300 python $T --mode group --group $B --out $O || break; done &&
    timeout -k 10 600 python $T --mode cpu --out $O

    [--hours 1] [--reps 10] [--warmup 3] [--cpu-chunks 16]

Input: synthetic speech (zasr.synth_audio, one minute tiled to the length asked for) in HBM;
seeded weights (zasr.pyannet.synth_weights).
  --mode hour    zasr_seg_classes_device on the whole file, the launcher's own recurrence group:
                 HIP events on the caller's stream around the call (it is ordered after that
                 stream and ends synchronised), median / min of `reps` after `warmup` untimed
                 calls; stage_ms = the engine's HIP-event split (front, convs, projections,
                 recurrence, head; medians); GFLOP per stage from zasr.pyannet.chunk_flops and
                 the TFLOP/s they give.
  --mode group   the same with the recurrence group forced to --group (packed-f32 FMA form, the
                 one form built): recurrence ms and total ms.
  --mode cpu     torch float32 evaluation of the SAME network (tests/pyannet_reference.py
                 forward_modules: a port, not the reference's onnxruntime session) on --cpu-chunks
                 chunks with this machine's threads, scaled to the file's chunk count.  No GPU.
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
    ap.add_argument("--mode", choices=("hour", "group", "cpu"), default="hour")
    ap.add_argument("--group", type=int, default=0)
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-chunks", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from zasr.pyannet import CHUNK, STEP, PyanNetConfig, chunk_flops, save_model_dir, synth_weights
    from zasr.segmentation import chunk_starts
    from zasr.synth_audio import synth_speech
    cfg = PyanNetConfig()
    w = synth_weights(cfg)
    minute = synth_speech(60.0, 41).astype(np.float32)
    total = int(args.hours * 3600 * 16000)
    audio = np.tile(minute, total // minute.shape[0] + 1)[:total]
    n_chunks = len(chunk_starts(total))
    if args.mode == "cpu":
        from pyannet_reference import forward_modules
        k = min(args.cpu_chunks, n_chunks)
        batch = np.stack([audio[i * STEP:i * STEP + CHUNK] for i in range(k)])
        forward_modules(w, batch[:1], torch.float32)
        t0 = time.perf_counter()
        forward_modules(w, batch, torch.float32)
        dt = (time.perf_counter() - t0) * 1e3
        row = {"kind": "cpu", "what": "torch float32 port of the same network (not onnxruntime)",
               "threads": torch.get_num_threads(), "chunks_timed": k, "ms": dt,
               "ms_scaled_to_file": dt * n_chunks / k}
    else:
        if not torch.cuda.is_available():
            raise SystemExit("no GPU: this mode measures on the device only")
        from zasr.binding import SegSession
        d = tempfile.mkdtemp(prefix="zasr_segbench_")
        save_model_dir(d, cfg, w)
        sess = SegSession(d)
        d_audio = torch.from_numpy(audio).cuda()
        torch.cuda.synchronize()
        flops = {k: v * n_chunks / 1e9 for k, v in chunk_flops(cfg).items()}
        sess.set_group(args.group if args.mode == "group" else 0)
        sess.set_profile(True)
        stream = torch.cuda.current_stream()
        ts, stages = [], []
        for r in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            sess.classes_device(d_audio.data_ptr(), total, stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            if r >= args.warmup:
                ts.append(e0.elapsed_time(e1))
                stages.append(sess.stage_ms())
        med = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
        if args.mode == "hour":
            row = {"kind": "hour", "seconds": total / 16000.0, "chunks": n_chunks,
                   "reps": args.reps, "ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)),
                   "stage_ms": med, "group": sess.last_group, "gflop": flops,
                   "tflops": {k: flops[k] / med[k] if med[k] > 0 else 0.0 for k in flops}}
        else:
            row = {"kind": "group", "form": "packed_f32_fma", "group": sess.last_group,
                   "chunks": n_chunks, "recurrence_ms": med["recurrence"],
                   "ms_median": float(np.median(ts)), "ms_min": float(np.min(ts))}
        sess.close()
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
