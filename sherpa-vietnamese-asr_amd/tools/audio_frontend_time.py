"""Times the device audio front end on one hour of audio (zasr.audio, DESIGN.md "Audio front
end").

    python sherpa-vietnamese-asr_amd/tools/audio_frontend_time.py [--hours 1] [--reps 10]
        [--warmup 3] [--out profiles/audio_frontend/times.jsonl]

One process; per case `warmup` untimed calls, then `reps` calls each bracketed by HIP events
on the calling stream (host sources: a host clock around the call and a stream synchronise,
since the call itself stages the pieces).  Cases:
  48k_stereo_i16_device / _pinned   one hour of 48 kHz stereo int16 -> 16 kHz mono f32
  44k1_mono_f32_device              one hour of 44.1 kHz mono float32
  8k_mono_i16_device                one hour of 8 kHz mono int16
  preprocess_audio                  boost-free preprocess_audio (RMS normalisation on) over the
                                    16 kHz hour with the chunk planner's speech regions
  pinned_copy                       the plain pinned-host -> device copy of the 48 kHz source
Per case one JSON line: median and minimum milliseconds per hour, the bytes the algorithm
needs (source read + 4 N_out written; the conditioning passes: every pass's reads and
writes), bytes / time as a fraction of the 8 TB/s HBM peak, and for the host path the fraction
of the measured pinned-copy rate.
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

HBM_PEAK = 8.0e12  # bytes / s (MI355X)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    from zasr import audio as fe
    from zasr.binding import audio_out_len
    from zasr.plan import plan_chunks
    from zasr.synth_audio import synth_speech

    sec = int(3600 * args.hours)
    front = fe.front_end()
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def report(name, times_ms, nbytes, extra=None):
        t = np.array(times_ms)
        med, mn = float(np.median(t)), float(t.min())
        row = {"case": name, "audio_hours": args.hours, "reps": len(t),
               "ms_per_hour_median": med / args.hours, "ms_per_hour_min": mn / args.hours,
               "bytes": int(nbytes), "GBps_median": nbytes / med / 1e6,
               "fraction_of_hbm_peak": nbytes / (med * 1e-3) / HBM_PEAK}
        row.update(extra or {})
        lines.append(row)
        print(json.dumps(row), flush=True)

    def time_device(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return out

    def time_host(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    rng = np.random.default_rng(1)

    def resample_case(name, rate, ch, dtype, pinned=False):
        n = sec * rate
        es = np.dtype(dtype).itemsize
        if dtype == np.int16:
            host = rng.integers(-20000, 20000, (n, ch) if ch > 1 else n, dtype=np.int16)
        else:
            host = rng.uniform(-0.5, 0.5, (n, ch) if ch > 1 else n).astype(np.float32)
        n_out = audio_out_len(rate, n)
        out = torch.empty(n_out, dtype=torch.float32, device="cuda")
        nbytes = n * ch * es + 4 * n_out
        src = torch.from_numpy(host).cuda()
        fmt = "int16" if dtype == np.int16 else "float32"
        ts = time_device(lambda: front.to_16k(src.data_ptr(), rate, out.data_ptr(), n_out,
                                              channels=ch, n_frames=n, fmt=fmt, stream=stream))
        report(name + "_device", ts, nbytes)
        if pinned:
            hp = torch.from_numpy(host).pin_memory()
            tc = time_host(lambda: src.copy_(hp, non_blocking=True))
            copy_rate = n * ch * es / (float(np.median(tc)) * 1e-3)
            report("pinned_copy", tc, n * ch * es, {"note": "host -> device copy alone"})
            hv = hp.numpy()
            th = time_host(lambda: front.to_16k(hv, rate, out.data_ptr(), n_out, stream=stream))
            report(name + "_pinned", th, nbytes,
                   {"fraction_of_pinned_copy_rate":
                    (n * ch * es / (float(np.median(th)) * 1e-3)) / copy_rate})
        del src

    resample_case("48k_stereo_i16", 48000, 2, np.int16, pinned=True)
    resample_case("44k1_mono_f32", 44100, 1, np.float32)
    resample_case("8k_mono_i16", 8000, 1, np.int16)

    # preprocess_audio on the hour with the planner's speech regions
    block = synth_speech(min(300.0, float(sec)), 5)
    x = np.tile(block, -(-sec * 16000 // len(block)))[: sec * 16000].copy()
    x *= np.repeat(rng.uniform(0.3, 1.0, -(-len(x) // 160000)), 160000)[: len(x)].astype(np.float32)
    segs = [(s, e) for s, e, _ in plan_chunks(x, overlap_sec=0.0)]
    d0 = torch.from_numpy(x).cuda()
    d = torch.empty_like(d0)
    speech = sum(e - s for s, e in segs)

    def run():
        d.copy_(d0)
        fe.condition_device(d.data_ptr(), d.numel(), segs, 16000, boost=False,
                            enable_rms_normalize=True, stream=stream)
    tp = time_device(run)
    tc = time_device(lambda: d.copy_(d0))
    # sum of squares reads the speech; the gain pass reads and writes the signal
    nbytes = 4 * speech + 8 * len(x)
    net = [a - float(np.median(tc)) for a in tp]
    report("preprocess_audio", net, nbytes,
           {"segments": len(segs), "speech_fraction": speech / len(x),
            "note": "device copy of the signal (%.3f ms) subtracted" % float(np.median(tc))})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
