"""The device audio front end on an MI355X (zasr.audio / zasr.binding.AudioFrontEnd over the
zasr_audio_* C ABI): convert + downmix + resample against the defining sum evaluated here in
float64, the level conditioning against numpy and against the reference's preprocess_audio
(tests/golden/audio_frontend.npz), bit-reproducibility, and the opt-in hooks of the stream
surface, the full pipe and the drop-in."""
import glob
import math
import os
import types

import numpy as np
import pytest

from conftest import gpu_available
from test_audio_frontend_host import FOUT, RATES, Z, fixture_cases, formula_table

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def fe():
    if not gpu_available():
        pytest.skip("no GPU")
    from zasr import audio
    return audio


def h64(t, fin, fout=FOUT):
    """The defining filter at times t (float64)."""
    c = 0.99 * 0.5 * min(fin, fout)
    ww = Z / (2.0 * c)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(t == 0.0, 2.0 * c, np.sin(2.0 * np.pi * c * t) / (np.pi * t))
    return np.where(np.abs(t) < ww, 0.5 * (1.0 + np.cos(2.0 * np.pi * c * t / Z)) * s, 0.0)


def brute64(x, fin, ms=None, fout=FOUT):
    """y[m] = (1 / fin) sum_n x[n] h(n / fin - m / fout), x = 0 outside [0, N), in float64 for
    the outputs ms (default: all ceil(N fout / fin) of them).  n / fin - m / fout is formed
    from the exact integer n fout - m fin."""
    x = np.asarray(x, np.float64)
    N = len(x)
    if ms is None:
        ms = np.arange(-(-N * fout // fin), dtype=np.int64)
    ms = np.asarray(ms, np.int64)
    half = int(math.ceil(Z * fin / (0.99 * min(fin, fout)))) + 1  # support in input frames
    k = np.arange(-half, half + 1, dtype=np.int64)
    n = (ms * fin // fout)[:, None] + k[None, :]
    t = (n * fout - ms[:, None] * fin).astype(np.float64) / (float(fin) * float(fout))
    xv = np.where((n >= 0) & (n < N), x[np.clip(n, 0, max(N - 1, 0))] if N else 0.0, 0.0)
    return (xv * h64(t, fin, fout)).sum(axis=1) / fin


def bound(fin, xmax):
    """(taps + 2) 2^-24 max_phase(sum |w|) max |x|: the worst-case float32 rounding of the dot
    product plus the rounding of the taps, from this file's own float64 table."""
    _, _, _, taps, w64 = formula_table(fin)
    return (taps + 2) * EPS * np.abs(w64).sum(axis=1).max() * xmax


@pytest.mark.parametrize("rate", RATES)
def test_resampler_equals_the_float64_sum(fe, rate):
    from zasr.binding import audio_resample_taps
    t = audio_resample_taps(rate)
    taps, tile = t["taps"], t["in_tile"]
    rng = np.random.default_rng(rate)
    tol = bound(rate, 1.0)
    for n in (1, 2, taps - 1, taps, tile - 1, tile, tile + 1, 2 * tile + 3, 20017):
        x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        y = fe.to_16k(x, rate)
        again = fe.to_16k(x, rate)
        ref = brute64(x, rate)
        assert y.dtype == np.float32 and y.shape == ref.shape == (-(-n * FOUT // rate),)
        assert np.array_equal(y.view(np.uint32), again.view(np.uint32))
        err = np.abs(y - ref)
        assert err.max() <= tol, (rate, n, err.max(), tol)
        # the zero-extension edges, explicitly
        assert np.abs(y[:taps] - ref[:taps]).max() <= tol
        assert np.abs(y[-taps:] - ref[-taps:]).max() <= tol


def test_index_arithmetic_past_2_24_samples(fe):
    """44.1 kHz, N = 2^24 + 5000 input samples: a float time base loses sample positions
    here.  The last 2048 outputs and 2048 seeded random ones against the float64 sum."""
    rate, n = 44100, 2 ** 24 + 5000
    rng = np.random.default_rng(7)
    x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    y = fe.to_16k(x, rate)
    n_out = -(-n * FOUT // rate)
    assert y.shape == (n_out,)
    ms = np.concatenate([np.arange(n_out - 2048, n_out), rng.integers(0, n_out, 2048)])
    ref = brute64(x, rate, ms)
    err = np.abs(y[ms] - ref)
    tol = bound(rate, 1.0)
    assert err.max() <= tol, (err.max(), tol)


def test_formats_and_sources(fe):
    import torch
    rng = np.random.default_rng(11)
    n = 6001
    q = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    eq = lambda a, b: a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))  # noqa: E731
    # int16 = the float32 path fed x * 2^-15, bit for bit (mono and stereo, two rates)
    for rate in (48000, 16000, 11025):
        assert eq(fe.to_16k(q[:, 0].copy(), rate), fe.to_16k(q[:, 0].astype(np.float32) * 2.0 ** -15, rate))
        assert eq(fe.to_16k(q, rate), fe.to_16k(q.astype(np.float32) * 2.0 ** -15, rate))
    # downmix at 16 kHz = numpy's mean over channels, bit for bit below 8 channels
    for ch in (2, 3, 6):
        x = rng.uniform(-1.0, 1.0, (n, ch)).astype(np.float32)
        assert eq(fe.to_16k(x, 16000), x.mean(axis=1))
        xi = rng.integers(-32768, 32768, (n, ch)).astype(np.int16)
        assert eq(fe.to_16k(xi, 16000), (xi.astype(np.float32) * np.float32(2.0 ** -15)).mean(axis=1))
    # 8 channels (numpy's own sum is unrolled there): within 2 float32 ulps of the float64
    # mean, on signed noise whose channels cancel
    x8 = rng.uniform(-1.0, 1.0, (n, 8)).astype(np.float32)
    m64 = x8.astype(np.float64).mean(axis=1)
    y8 = fe.to_16k(x8, 16000).astype(np.float64)
    assert np.all(np.abs(y8 - m64) <= 2 * np.spacing(np.abs(m64).astype(np.float32)).astype(np.float64))
    # stereo 48 kHz int16 = the mono path fed the float32 downmix, within the rounding bound
    mono = (q.astype(np.float32) * np.float32(2.0 ** -15)).mean(axis=1)
    y_st, y_mono = fe.to_16k(q, 48000), fe.to_16k(mono, 48000)
    assert np.abs(y_st - y_mono).max() <= bound(48000, 1.0)
    assert np.abs(y_st - brute64(mono, 48000)).max() <= bound(48000, 1.0)
    # every channel count through the resampler (vector and scalar load forms)
    for ch in (1, 2, 3, 4, 5, 8):
        for dt in (np.float32, np.int16):
            x = (rng.uniform(-1.0, 1.0, (4099, ch)) * (1.0 if dt == np.float32 else 32767.0)).astype(dt)
            xf = x.astype(np.float32) * (np.float32(1.0) if dt == np.float32 else np.float32(2.0 ** -15))
            if ch == 8:  # summed in float64 and rounded once
                mix = xf.astype(np.float64).sum(axis=1).astype(np.float32) / np.float32(8)
            else:        # a float32 running sum in channel order, one float32 divide
                mix = xf[:, 0].copy()
                for c in range(1, ch):
                    mix += xf[:, c]
                mix = mix / np.float32(ch)
            y = fe.to_16k(x, 44100)
            assert np.abs(y - brute64(mix, 44100)).max() <= bound(44100, 1.0), (ch, dt)
    # a device-resident source = the host source, bit for bit (aligned and unaligned bases)
    for rate in (48000, 44100, 16000):
        host = fe.to_16k(q, rate)
        dev = fe.to_16k(torch.from_numpy(q).cuda(), rate)
        assert dev.is_cuda and eq(dev.cpu().numpy(), host)
        d1 = torch.from_numpy(np.concatenate([np.zeros(1, np.int16), q[:, 0]])).cuda()[1:]
        assert eq(fe.to_16k(d1, rate).cpu().numpy(), fe.to_16k(q[:, 0].copy(), rate))
    # a host source the caller has pinned (read in place) = the pageable one (staged)
    for rate in (48000, 16000):
        assert eq(fe.to_16k(torch.from_numpy(q).pin_memory().numpy(), rate), fe.to_16k(q, rate))
    # 16 kHz mono float32 comes back bit-identical
    x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    assert eq(fe.to_16k(x, 16000), x)
    assert eq(fe.to_16k(torch.from_numpy(x).cuda(), 16000).cpu().numpy(), x)
    assert fe.to_16k(np.zeros(0, np.float32), 48000).shape == (0,)


@pytest.mark.parametrize("rate", [48000, 44100, 8000])
def test_sine_comes_out_as_the_sine(fe, rate):
    """A 1 kHz sine of amplitude 0.5 comes out as the 1 kHz sine at 16 kHz: away from the
    ends the error is at most |H(1 kHz) - 1| * 0.5, the filter's own pass-band gain evaluated
    from the float64 tap table, plus the rounding bound."""
    f0, amp, n = 1000.0, 0.5, 12000
    x = (amp * np.sin(2.0 * np.pi * f0 * np.arange(n) / rate)).astype(np.float32)
    y = fe.to_16k(x, rate)
    P, Q, lo, taps, w64 = formula_table(rate)
    tau = (lo[:, None] + np.arange(taps)[None, :] - (np.arange(P) * Q / P)[:, None]) / rate
    H = (w64 * np.exp(2j * np.pi * f0 * tau)).sum(axis=1)
    tol = np.abs(H - 1.0).max() * amp + bound(rate, amp)
    m = np.arange(len(y))
    ref = amp * np.sin(2.0 * np.pi * f0 * m / FOUT)
    err = np.abs(y - ref)[taps:-taps]
    assert tol < 2e-3 and err.max() <= tol, (err.max(), tol)


@pytest.mark.parametrize("peak", [0.31, 0.62, 0.0, 0.5])
def test_boost_equals_numpy(fe, peak):
    rng = np.random.default_rng(5)
    a = (rng.uniform(-1.0, 1.0, 10007) * 0.9 * peak).astype(np.float32)
    a[4321] = np.float32(-peak)
    pk = np.max(np.abs(a))
    assert pk == np.float32(peak)
    want = a / pk * 0.95 if 0 < pk < 0.5 else a
    assert (peak == 0.31) == (want is not a)
    got, again = fe.boost_quiet(a), fe.boost_quiet(a)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


@pytest.mark.parametrize("name", ["mixed", "clamp", "limiter", "long", "rms_off",
                                  "rms_off_limited", "empty"])
def test_preprocess_audio_equals_the_reference(fe, name):
    c = fixture_cases()[name]
    audio, segs, enable = c["audio"], [tuple(s) for s in c["segments"].tolist()], bool(c["enable"])
    before = audio.copy()
    got = fe.preprocess_audio(audio, segs, enable_rms_normalize=enable)
    again = fe.preprocess_audio(audio, segs, enable_rms_normalize=enable)
    assert np.array_equal(audio, before) and got is not audio and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    ref = c["expected"]
    if not enable or not segs:
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        return
    longest = max(e - s for s, e in segs)
    tol = (math.log2(longest) + 4) * EPS * np.abs(ref.astype(np.float64))
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print(name, "max err / tol", float((err / np.maximum(tol, 1e-300)).max()))
    assert np.all(err <= tol), float((err / np.maximum(tol, 1e-300)).max())
    # the device sums of squares themselves: float64 sums of exact squares
    front = fe.front_end()
    import torch
    d = torch.from_numpy(audio).cuda()
    b, e = [s for s, _ in segs], [x for _, x in segs]
    ss = front.segment_sumsq(d.data_ptr(), len(audio), b, e)
    ss2 = front.segment_sumsq(d.data_ptr(), len(audio), b, e)
    assert np.array_equal(ss, ss2)
    want = np.array([np.sum(audio[s:x].astype(np.float64) ** 2) for s, x in segs])
    assert np.all(np.abs(ss - want) <= 1e-12 * want)


def test_peak_limit_and_segment_rms_names(fe):
    rng = np.random.default_rng(9)
    a = rng.uniform(-1.0, 1.0, 5003).astype(np.float32)
    a[77] = np.float32(1.7)
    want = a * (np.float32(0.95) / np.max(np.abs(a)))
    assert np.array_equal(fe.adaptive_peak_limit(a).view(np.uint32), want.view(np.uint32))
    quiet = a * np.float32(0.25)
    assert fe.adaptive_peak_limit(quiet) is quiet
    r = float(np.sqrt(np.mean(a ** 2)))
    assert abs(fe.compute_segment_rms(a) - r) <= 16 * EPS * r
    assert fe.compute_segment_rms(a[:0]) == 0.0
    assert fe.per_segment_rms_normalize(a, []) is a


@pytest.fixture(scope="module")
def onnx_dir(tmp_path_factory):
    if not gpu_available():
        pytest.skip("no GPU")
    from model_fixtures import tiny_model
    from write_onnx import write_model_dir
    from zasr.model import synth_tokens
    cfg, w, _ = tiny_model(3)
    d = str(tmp_path_factory.mktemp("audio_stream_model") / "model")
    write_model_dir(d, w, synth_tokens(cfg.vocab_size))
    return d


def test_stream_hook_resamples_each_call(fe, onnx_dir):
    from zasr.offline import OfflineRecognizer
    from zasr.synth_audio import synth_speech
    d = onnx_dir
    kw = {"tokens": os.path.join(d, "tokens.txt"),
          "encoder": glob.glob(os.path.join(d, "encoder*.onnx"))[0],
          "decoder": glob.glob(os.path.join(d, "decoder*.onnx"))[0],
          "joiner": glob.glob(os.path.join(d, "joiner*.onnx"))[0],
          "decoding_method": "greedy_search", "max_active_paths": 1, "precision": "fp32"}
    chunk = synth_speech(4.0, 4242)
    x8 = brute64(chunk, 16000, fout=8000).astype(np.float32)  # the chunk at 8 kHz
    rec = OfflineRecognizer.from_transducer(**kw, resample_input=True)
    s = rec.create_stream()
    s.accept_waveform(8000, x8)
    rec.decode_stream(s)
    t = rec.create_stream()
    t.accept_waveform(16000, fe.to_16k(x8, 8000))
    rec.decode_stream(t)
    assert len(s.result.token_ids) > 0
    assert s.result.token_ids == t.result.token_ids
    assert s.result.ys_log_probs == t.result.ys_log_probs


def test_pipe_hook_same_plan_and_signal(fe):
    from zasr.pipeline import FullPipe
    from zasr.synth_audio import synth_speech
    x = synth_speech(40.0, 31)
    q = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    x16 = q.astype(np.float32) * np.float32(2.0 ** -15)
    pipes = []
    for arg, kw in ((x16, {}), (np.stack([q, q], axis=1), {"sample_rate": 16000})):
        p = object.__new__(FullPipe)  # prepare() alone: no models needed
        p.shard, p.emb = False, types.SimpleNamespace(dim=8)
        p.prepare(arg, **kw)
        pipes.append(p)
    a, b = pipes
    assert (a.c_off, a.c_len, a.r_off, a.r_len, a.n) == (b.c_off, b.c_len, b.r_off, b.r_len, b.n)
    assert len(a.c_off) >= 2
    da, db = a.d_audio.cpu().numpy(), b.d_audio.cpu().numpy()
    assert np.array_equal(da.view(np.uint32), db.view(np.uint32))
    assert np.array_equal(da, x16)
    # conditioned: the boost, then preprocess_audio, on the device signal
    quiet = (x16 * np.float32(0.125)).astype(np.float32)
    c = object.__new__(FullPipe)
    c.shard, c.emb = False, types.SimpleNamespace(dim=8)
    segs = [(16000, 80000), (100000, 300000)]
    c.prepare(quiet, vad_segments=segs, rms_normalize=True, condition=True)
    want = fe.preprocess_audio(fe.boost_quiet(quiet), segs, enable_rms_normalize=True)
    assert np.array_equal(c.d_audio.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_dropin_hook_is_opt_in(fe):
    """install(engine) leaves an audio_preprocessing module alone; install(engine,
    audio_module=m) rebinds its four functions and nothing else (stand-in modules: the
    reference itself is not needed)."""
    from zasr import audio as ours
    from zasr.dropin import AUDIO_NAMES, install
    eng = types.ModuleType("core.asr_engine")
    mod = types.ModuleType("core.audio_preprocessing")
    orig = {}
    for n in AUDIO_NAMES + ("apply_wpe_dereverberation",):
        orig[n] = (lambda name: lambda *a, **k: name)(n)
        setattr(mod, n, orig[n])
    from zasr import asr_engine
    try:
        done = install(eng)
        assert all(getattr(mod, n) is f for n, f in orig.items())
        assert not [d for d in done if d.startswith("audio_preprocessing.")]
        done = install(eng, audio_module=mod)
    finally:
        asr_engine.set_host_module(None)
    assert sorted(d for d in done if d.startswith("audio_preprocessing.")) == \
        sorted("audio_preprocessing." + n for n in AUDIO_NAMES)
    for n in AUDIO_NAMES:
        assert getattr(mod, n) is getattr(ours, n)
    assert mod.apply_wpe_dereverberation is orig["apply_wpe_dereverberation"]
    with pytest.raises(ValueError):
        install(eng, audio_module=ours)
    # the rebound function is the device one
    c = fixture_cases()["rms_off_limited"]
    got = mod.preprocess_audio(c["audio"], [], enable_rms_normalize=False)
    assert np.array_equal(got.view(np.uint32), c["expected"].view(np.uint32))
