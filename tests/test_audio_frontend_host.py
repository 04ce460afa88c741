"""Host-side checks of the device audio front end (no GPU): the polyphase table against the
defining formula in float64, the output length, the sparse gain plan against the reference's
own gain_map (tests/golden/audio_frontend.npz, from make_golden_audio_frontend.py), and the
argument errors of the C ABI."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest

RATES = (8000, 11025, 22050, 32000, 44100, 48000, 96000, 44101)
# (P, taps) worked out from the definition, independently of the library
SIZES = {8000: (2, 13), 11025: (640, 13), 22050: (320, 17), 32000: (1, 25), 44100: (160, 34),
         48000: (1, 37), 96000: (1, 73), 44101: (16000, 34)}
FOUT = 16000
Z = 6


def formula_table(fin):
    """P, Q, lo[p], taps and the float64 weights h((lo[p] + t - p Q / P) / fin) / fin, straight
    from the definition: c = 0.99 * 0.5 * min(fin, fout), ww = Z / (2 c), h(t) = 0 for
    |t| >= ww, else 0.5 (1 + cos(2 pi c t / Z)) s(t), s(0) = 2 c, s(t) = sin(2 pi c t) / (pi t).
    The support's ends are decided in exact rational arithmetic."""
    g = math.gcd(fin, FOUT)
    P, Q = FOUT // g, fin // g
    c = 0.99 * 0.5 * min(fin, FOUT)
    ww = Z / (2.0 * c)
    W = Fraction(Z * fin, 1) / (2 * Fraction(99, 100) * Fraction(min(fin, FOUT), 2))  # ww * fin
    lo, hi = [], []
    for p in range(P):
        centre = Fraction(p * Q, P)
        lo.append(math.floor(centre - W) + 1)   # the smallest integer above centre - W
        hi.append(math.ceil(centre + W) - 1)    # the largest integer below centre + W
    taps = max(h - l + 1 for l, h in zip(lo, hi))
    lo = np.array(lo, np.int64)
    n = lo[:, None] + np.arange(taps)[None, :]
    t = (n - (np.arange(P, dtype=np.float64) * Q / P)[:, None]) / fin
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(t == 0.0, 2.0 * c, np.sin(2.0 * np.pi * c * t) / (np.pi * t))
    h = 0.5 * (1.0 + np.cos(2.0 * np.pi * c * t / Z)) * s
    h = np.where(np.abs(t) < ww, h, 0.0)
    return P, Q, lo, taps, h / fin


@pytest.mark.parametrize("rate", RATES)
def test_taps_match_the_formula(rate):
    from zasr.binding import audio_resample_taps
    P, Q, lo, taps, w64 = formula_table(rate)
    assert (P, taps) == SIZES[rate]
    t = audio_resample_taps(rate)
    assert (t["P"], t["Q"], t["taps"]) == (P, Q, taps)
    assert np.array_equal(t["lo"], lo)
    assert t["w"].dtype == np.float32 and t["w"].shape == (P, taps)
    err = np.abs(t["w"].astype(np.float64) - w64)
    assert np.all(err <= 2.0 ** -24 * np.abs(w64) + 1e-12), err.max()
    sums = t["w"].astype(np.float64).sum(axis=1)
    assert np.all(np.abs(sums - 1.0) <= 1e-3), (sums.min(), sums.max())
    # the tile the GPU tests step around: a whole number of waves of outputs, and the input
    # frames they span
    assert t["out_tile"] >= 64 and t["out_tile"] % 64 == 0
    assert t["in_tile"] == -(-t["out_tile"] * Q // P)


@pytest.mark.parametrize("rate", RATES)
def test_out_len_is_the_integer_ceil(rate):
    from zasr.binding import audio_out_len
    for n in (0, 1, 2, 3, 440, 441, 442, 2 ** 24 + 5000):
        assert audio_out_len(rate, n) == -(-n * FOUT // rate), (rate, n)


def expand(plan, n):
    """The sparse plan as the dense float32 map it stands for."""
    g = np.ones(n, np.float32)
    if plan is None:
        return g
    prev = 0
    for b, e, gain, off in zip(plan["begin"], plan["end"], plan["gain"], plan["ramp"]):
        assert prev <= b < e <= n  # ascending, disjoint, inside the signal
        prev = e
        g[b:e] = gain if off < 0 else plan["values"][off:off + e - b]
    return g


def fixture_cases():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                             "audio_frontend.npz"))
    names = sorted({k.split("/")[0] for k in z.files})
    return {n: {k.split("/")[1]: z[k] for k in z.files if k.startswith(n + "/")} for n in names}


def test_fixture_covers_the_cases():
    cases = fixture_cases()
    assert set(cases) == {"mixed", "clamp", "limiter", "long", "rms_off", "rms_off_limited", "empty"}
    m = cases["mixed"]
    segs = m["segments"].tolist()
    assert segs[0][0] == 0 and segs[-1][1] == len(m["audio"]) and segs[0][1] == segs[1][0]
    assert len(m["rms"]) == len(segs) - 2  # the short and the near-silent segment are skipped
    g = cases["clamp"]["gain_map"]
    assert g.max() == np.float32(10.0) and g.min() == np.float32(1.0 / 10.0)
    assert float(np.abs(cases["limiter"]["audio"] * cases["limiter"]["gain_map"]).max()) > 0.95
    assert sum(c["audio"].nbytes + c["expected"].nbytes for c in cases.values()) < 1 << 20


@pytest.mark.parametrize("name", ["mixed", "clamp", "limiter", "long", "rms_off",
                                  "rms_off_limited", "empty"])
def test_gain_plan_equals_the_reference_gain_map(name):
    """The builder, given the reference's own float32 rms values, reproduces its gain_map bit
    for bit -- the fades included, whose values depend on the order of the writes."""
    from zasr.audio import build_gain_plan
    c = fixture_cases()[name]
    n = len(c["audio"])
    seg_rms = [(int(s), int(e), float(r)) for s, e, r in c["rms"]]
    plan = build_gain_plan(n, seg_rms)
    assert (plan is None) == (len(seg_rms) == 0)
    got = expand(plan, n)
    assert np.array_equal(got.view(np.uint32), c["gain_map"].view(np.uint32))
    if plan is not None:  # sparse: constants and 5 ms ramps, never a full-length map
        assert len(plan["values"]) <= 2 * 80 * len(seg_rms)
        assert len(plan["begin"]) <= 3 * len(seg_rms)


def test_gain_plan_overlapping_writes_follow_assignment_order():
    """Later segments overwrite earlier ones as slice assignment does (the dense equivalent
    written out here)."""
    from zasr.audio import build_gain_plan
    n = 20000
    seg_rms = [(1000, 9000, 0.1), (5000, 12000, 0.02), (12000, 14000, 0.3), (2000, 4000, 0.05)]
    target = float(np.median(np.array([r for _, _, r in seg_rms])))
    g = np.ones(n, np.float32)
    for s, e, r in seg_rms:
        g[s:e] = max(min(target / r, 10.0), 0.1)
    for s, e, _ in seg_rms:
        k = min(80, (e - s) // 4)
        g[s:s + k] = np.linspace(g[s - 1], g[s], k, dtype=np.float32)
        g[e - k:e] = np.linspace(g[e - 1], g[e], k, dtype=np.float32)
    got = expand(build_gain_plan(n, seg_rms), n)
    assert np.array_equal(got.view(np.uint32), g.view(np.uint32))


def test_invalid_sources_are_refused():
    """Rates 0, 3999, 384001 and channel counts 0, 9 return ZASR_ERR_INVALID with a message,
    before anything touches a device."""
    from zasr.binding import ZasrError, audio_out_len, audio_resample_taps, load_library
    lib = load_library()
    n_out = C.c_int64()
    buf = (C.c_float * 16)()

    def call(fmt, ch, rate):
        return lib.zasr_audio_to_16k(None, C.cast(buf, C.c_void_p), fmt, ch, rate, 4, 0,
                                     C.cast(buf, C.c_void_p), 16, C.byref(n_out), None)
    for rate in (0, 3999, 384001):
        assert call(0, 1, rate) == 1
        assert b"sample rate" in lib.zasr_last_error()
        with pytest.raises(ZasrError):
            audio_resample_taps(rate)
        with pytest.raises(ZasrError):
            audio_out_len(rate, 10)
    for ch in (0, 9):
        assert call(1, ch, 48000) == 1
        assert b"channels" in lib.zasr_last_error()
    assert call(2, 1, 48000) == 1 and b"format" in lib.zasr_last_error()
    assert call(0, 2, 48000) == 1  # a valid source, no handle: still an argument error
