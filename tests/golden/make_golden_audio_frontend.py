"""Writes tests/golden/audio_frontend.npz: the reference's own preprocess_audio
(core/audio_preprocessing.py) run on the CPU over seeded signals, for the level-conditioning
tests of the device audio front end (tests/test_audio_frontend_host.py,
tests/test_gpu_audio_frontend.py).

    python tests/golden/make_golden_audio_frontend.py /path/to/reference

The reference is imported here only; the tests read the .npz.  Per case `k` the file holds
  k/audio      float32 [n]   the input (n = 9600: 0.6 s, so the whole file stays under 1 MB)
  k/segments   int64 [s, 2]  the VAD segments handed to preprocess_audio
  k/enable     bool          enable_rms_normalize
  k/expected   float32 [n]   preprocess_audio's output
  k/rms        float64 [r, 3]  (start, end, rms) of the segments the reference kept: the values
                             its own compute_segment_rms returned
  k/gain_map   float32 [n]   the reference's gain_map for those values (ones when it built none)
The gain map is read off the reference without touching its code: with compute_segment_rms
replaying the recorded values, per_segment_rms_normalize of an all-ones signal returns
1 * gain_map.  The generator asserts that audio * gain_map is bit-equal to the reference's
normalised signal, that every case is a factor 1.01 away from the branch thresholds (rms against
1e-8, peaks against 0.95), and that the limiter case's normalised peak is above 0.95.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N = 9600
MIN_SEG = 1600  # the reference's 100 ms


def noise(rng, n, amp):
    return (rng.uniform(-1.0, 1.0, n) * amp).astype(np.float32)


def make_cases():
    cases = {}
    # mixed: a segment at sample 0, an adjacent pair, a short one, a near-silent one, one
    # ending at len(audio); moderate gains
    rng = np.random.default_rng(101)
    a = noise(rng, N, 0.002)
    segs = [(0, 1700), (1700, 3400), (3600, 4000), (4200, 5900), (6000, 7700), (7900, N)]
    for (s, e), amp in zip(segs, (0.05, 0.12, 0.3, 1e-10, 0.08, 0.2)):
        a[s:e] = noise(rng, e - s, amp)
    cases["mixed"] = (a, segs, True)
    # clamp: a quiet segment far below the median (+20 dB clamp) and a loud one far above it
    # (-20 dB clamp)
    rng = np.random.default_rng(102)
    a = noise(rng, N, 0.001)
    segs = [(100, 1800), (2000, 3700), (3900, 5600), (5800, 7500), (7700, 9400)]
    for (s, e), amp in zip(segs, (0.0005, 0.03, 0.035, 0.04, 0.9)):
        a[s:e] = noise(rng, e - s, amp)
    cases["clamp"] = (a, segs, True)
    # limiter: a quiet segment with one spike is boosted past 0.95
    rng = np.random.default_rng(103)
    a = noise(rng, N, 0.001)
    segs = [(200, 2200), (2500, 4500), (5000, 7000)]
    for (s, e), amp in zip(segs, (0.3, 0.3, 0.04)):
        a[s:e] = noise(rng, e - s, amp)
    a[6000] = np.float32(0.45)
    cases["limiter"] = (a, segs, True)
    # long: a segment longer than one sum-of-squares chunk, starting off a 4-sample boundary
    rng = np.random.default_rng(104)
    a = noise(rng, N, 0.003)
    segs = [(3, 5301), (5500, 7333), (7400, 9597)]
    for (s, e), amp in zip(segs, (0.1, 0.25, 0.05)):
        a[s:e] = noise(rng, e - s, amp)
    cases["long"] = (a, segs, True)
    # RMS normalisation off: untouched below the limiter, scaled above it
    rng = np.random.default_rng(105)
    cases["rms_off"] = (noise(rng, N, 0.7), [(0, 4000), (5000, 9000)], False)
    b = noise(rng, N, 0.6)
    b[1234] = np.float32(-1.3)
    cases["rms_off_limited"] = (b, [(0, 4000)], False)
    # no segments
    cases["empty"] = (noise(rng, N, 0.4), [], True)
    return cases


def away(x, thr):
    return x > thr * 1.01 or x < thr / 1.01


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref_root = sys.argv[1]
    sys.path.insert(0, ref_root)
    import core.audio_preprocessing as ap
    real_rms = ap.compute_segment_rms
    out = {}
    for name, (audio, segs, enable) in make_cases().items():
        assert audio.dtype == np.float32 and audio.shape == (N,)
        expected = ap.preprocess_audio(audio, segs, enable_rms_normalize=enable)
        assert expected.dtype == np.float32 and expected is not audio
        # the rms values the reference computes, in its order
        seen = []

        def spy(x):
            r = real_rms(x)
            seen.append(r)
            return r
        ap.compute_segment_rms = spy
        try:
            normalised = ap.per_segment_rms_normalize(audio.copy(), segs) if enable else audio
        finally:
            ap.compute_segment_rms = real_rms
        long_enough = [(s, e) for s, e in segs if e - s >= MIN_SEG]
        assert len(seen) == (len(long_enough) if enable else 0), (name, len(seen))
        for r in seen:
            assert away(r, 1e-8), (name, r)
        kept = [(s, e, r) for (s, e), r in zip(long_enough, seen) if r > 1e-8] if enable else []
        # the gain map: replay those values over an all-ones signal
        replay = iter(seen)
        ap.compute_segment_rms = lambda x: next(replay)
        try:
            gain_map = (ap.per_segment_rms_normalize(np.ones(N, np.float32), segs)
                        if enable and segs else np.ones(N, np.float32))
        finally:
            ap.compute_segment_rms = real_rms
        gain_map = np.ascontiguousarray(gain_map, np.float32)
        assert np.array_equal(audio * gain_map, normalised), name
        peak = float(np.max(np.abs(normalised)))
        assert away(peak, 0.95), (name, peak)
        assert away(float(np.max(np.abs(audio))), 0.5), name
        if name in ("limiter", "rms_off_limited"):
            assert peak > 0.95, (name, peak)
        if name == "clamp":
            gains = sorted(set(np.round(gain_map[[900, 8500]].astype(np.float64), 4)))
            assert gains == [0.1, 10.0], gains
        if name in ("rms_off", "empty"):
            assert np.array_equal(expected, audio), name
        out[name + "/audio"] = audio
        out[name + "/segments"] = np.array(segs, np.int64).reshape(-1, 2)
        out[name + "/enable"] = np.array(enable)
        out[name + "/expected"] = expected
        out[name + "/rms"] = np.array(kept, np.float64).reshape(-1, 3)
        out[name + "/gain_map"] = gain_map
        print(f"{name}: {len(kept)} segments kept, gain {gain_map.min():.3f} .. "
              f"{gain_map.max():.3f}, normalised peak {peak:.4f}")
    path = os.path.join(HERE, "audio_frontend.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
