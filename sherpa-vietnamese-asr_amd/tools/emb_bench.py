"""Times the community-1 speaker-embedding stage (zasr_emb_*), split by stage.

One measurement per process (one GPU program per call), each under its own time limit, stopping
at the first that fails; every call appends its JSON line to --out:

    T=sherpa-vietnamese-asr_amd/tools/emb_bench.py; O=profiles/community1/times.jsonl
    timeout -k 10 300 python $T --mode hour --out $O &&
    timeout -k 10 120 python $T --mode chunks --chunks 64 --out $O

    [--seconds 3600] [--seed 3] [--reps 3] [--warmup 1] [--group 0]

Input: synthetic speech (zasr.synth_audio, one minute tiled) in HBM; seeded weights
(zasr.resnet34.synth_weights); masks from a seeded pattern (each speaker active in runs of 20-200
segmentation frames, about half the time).
  --mode hour    every chunk of --seconds of audio at the reference's 1 s step (an hour: 3592)
                 through zasr_emb_chunks_device.  HIP events on the caller's stream around the call
                 (it is ordered after that stream and ends synchronised), median / min of `reps`
                 after `warmup` untimed calls; stage_ms = the engine's HIP-event split (fbank +
                 windows, stem, layer1 .. layer4, pooling, projection; medians; `convs` is the
                 four layers' sum) with TFLOP/s and share of the peak per layer; the flop count is the
                 engine's own, from the model's config (zasr_emb_encoder_flops), and the TFLOP/s
                 and the share of the exact-f32 MFMA peak (157.3 TFLOP/s) it gives on the
                 convolution stage; the activation bytes of one launch group.
  --mode chunks  the first --chunks chunks only, the same way.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.join(REPO, "sherpa-vietnamese-asr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

F32_MFMA_PEAK_TFLOPS = 157.3
NSEG = 589


def chunk_starts(total: int, chunk: int = 160000, step: int = 16000):
    """core/speaker_diarization_pure_ort.py:714-726."""
    starts, s = [], 0
    while True:
        starts.append(s)
        if (s + chunk) > total:
            break
        s += step
    return np.asarray(starts, np.int64)


def seeded_masks(n: int, seed: int) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64(seed))
    m = np.zeros((n, 3, NSEG), np.uint8)
    for c in range(n):
        for s in range(3):
            t, on = 0, bool(rng.integers(2))
            while t < NSEG:
                run = int(rng.integers(20, 200))
                if on:
                    m[c, s, t:t + run] = 1
                t += run
                on = not on
    return m


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("hour", "chunks"), default="hour")
    ap.add_argument("--seconds", type=float, default=3600.0)
    ap.add_argument("--chunks", type=int, default=64)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--group", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from zasr.resnet34 import (CHUNK_FRAMES, ResNet34Config, chunk_flops, group_bytes, layer_flops,
                               save_model_dir, synth_weights)
    from zasr.synth_audio import synth_speech
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    from zasr.binding import EmbSession
    cfg = ResNet34Config()
    with tempfile.TemporaryDirectory(prefix="zasr_embbench_") as d:  # read at construction only
        save_model_dir(d, cfg, synth_weights(cfg))
        sess = EmbSession(d)
    total = int(args.seconds * 16000)
    minute = synth_speech(60.0, 41)
    audio = np.tile(minute, total // minute.shape[0] + 1)[:total]
    starts = chunk_starts(total)
    if args.mode == "chunks":
        starts = starts[:args.chunks]
    masks = seeded_masks(len(starts), args.seed)
    d_audio = torch.from_numpy(audio).cuda()
    torch.cuda.synchronize()
    sess.set_group(args.group)
    sess.set_profile(True)
    stream = torch.cuda.current_stream()
    ts, stages = [], []
    for r in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = sess.chunk_embeddings_device(d_audio.data_ptr(), total, starts, masks,
                                           stream=stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        if r >= args.warmup:
            ts.append(e0.elapsed_time(e1))
            stages.append(sess.stage_ms())
    assert out.shape == (len(starts), 3, 256) and not np.any(np.isnan(out))
    med = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
    enc = sess.encoder_flops(998)
    py = chunk_flops(cfg)
    assert abs(enc - py["encoder"]) < 1.0
    n = len(starts)
    lf = layer_flops(cfg, CHUNK_FRAMES)
    assert abs(sum(lf.values()) - enc) < 1.0
    layers = ("layer1", "layer2", "layer3", "layer4")
    med["convs"] = sum(med[k] for k in layers)
    conv_gflop = n * sum(lf[k] for k in layers) / 1e9
    conv_tflops = conv_gflop / med["convs"] if med["convs"] > 0 else 0.0
    layer_tflops = {k: n * lf[k] / 1e9 / med[k] if med[k] > 0 else 0.0 for k in layers}
    row = {"kind": args.mode, "audio_seconds": args.seconds, "chunks": n, "group": sess.last_group,
           "reps": args.reps, "ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)),
           "stage_ms": med, "gflop_per_chunk": {k: v / 1e9 for k, v in py.items()},
           "tflop_total": n * sum(py.values()) / 1e12, "conv_tflops": conv_tflops,
           "layer_gflop_per_chunk": {k: lf[k] / 1e9 for k in lf}, "layer_tflops": layer_tflops,
           "layer_share_of_peak": {k: v / F32_MFMA_PEAK_TFLOPS for k, v in layer_tflops.items()},
           "share_of_f32_mfma_peak": conv_tflops / F32_MFMA_PEAK_TFLOPS,
           "group_activation_gb": sess.last_group * group_bytes(cfg) / 1e9,
           "realtime_factor": args.seconds * 1e3 / float(np.median(ts)) if args.mode == "hour" else None}
    sess.close()
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
