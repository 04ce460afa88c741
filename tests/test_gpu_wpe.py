"""WPE dereverberation on an MI355X (zasr.audio.apply_wpe_dereverberation / apply_wpe_batch over
zasr.binding.WpeEngine) against the float64 restatement of the contract in
tests/wpe_reference.py: every kernel alone, the whole chunk within four times the error of the
float32 precision model, the ragged batch bit for bit against each chunk alone, the peak limiter,
numpy against tensor input, and the drop-in's WPE plan against its chunk-by-chunk route."""
import types

import numpy as np
import pytest

import wpe_reference as W
from conftest import gpu_available

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
U64 = 2.0 ** -53
# worst-case rounding of the 512-point float32 transform relative to sum |input|: nine radix-2
# levels' worth of one complex twiddle product (about 2.5 u) and one addition (u) each, the
# window product, and the even / odd split (3 u)
FFT_U = (9 * 3.5 + 1 + 3) * U32


@pytest.fixture(scope="module")
def audio():
    if not gpu_available():
        pytest.skip("no GPU")
    from zasr import audio
    return audio


@pytest.fixture(scope="module")
def eng(audio):
    return audio.wpe_engine()


@pytest.fixture(scope="module")
def speech():
    """The parity inputs and their float64 / float32-model results, computed once."""
    out = {}
    for n, seed in ((48000, 0), (47999, 1)):
        x = W.reverberant_speech(n, seed)
        out[n] = (x, W.apply_wpe(x), W.apply_wpe(x, precision="f32"))
    return out


# ---- kernel by kernel --------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1024, 1151, 3000])
def test_stft_kernel(eng, n):
    x = W.reverberant_speech(n, 10 + n % 7)
    Y, mx = eng.selftest_stft(x)
    ref = W.stft(x).T  # [257][T]
    assert Y.shape == ref.shape == (257, W.num_frames(n))
    T = ref.shape[1]
    pad = np.zeros(W.HOP * (T - 1) + W.FFT)
    pad[W.FADE:W.FADE + n] = x
    l1 = np.array([np.sum(np.abs(pad[W.HOP * t:W.HOP * t + W.FFT] * W.window())) for t in range(T)])
    err = np.abs(Y.astype(np.complex128) - ref)
    print(f"stft n={n}: max err {err.max():.3g}, bound {FFT_U * l1.max():.3g}")
    assert np.isfinite(Y.view(np.float32)).all()
    assert (err <= FFT_U * l1[None, :] + 1e-30).all()
    assert Y[0].imag.max() == 0 and Y[256].imag.max() == 0
    got = np.max(Y.real.astype(np.float32) ** 2 + Y.imag.astype(np.float32) ** 2)
    assert mx == np.float32(got)


@pytest.mark.parametrize("n", [1024, 1025, 4700])  # T = 11, 12, 40
def test_istft_kernel(eng, n):
    T = W.num_frames(n)
    assert T == {1024: 11, 1025: 12, 4700: 40}[n]
    rng = np.random.default_rng(n)
    X = (rng.standard_normal((T, 257)) + 1j * rng.standard_normal((T, 257))).astype(np.complex64)
    out = eng.selftest_istft(X, n)
    ref = W.istft(X.astype(np.complex128), n)
    a = np.abs(X.astype(np.complex128))
    l1 = (a[:, 0] + a[:, 256] + 2 * a[:, 1:256].sum(axis=1)) / W.FFT  # bound on a frame's samples
    # four frames meet in a sample: each carries the transform's error and the synthesis
    # window's product, then three float32 additions
    bound = 4 * (FFT_U + 2 * U32) * l1.max() * np.abs(W.synthesis_window()).max() \
        + 3 * U32 * np.abs(ref).max()
    err = np.abs(out.astype(np.float64) - ref)
    print(f"istft n={n} T={T}: max err {err.max():.3g}, bound {bound:.3g}")
    assert np.isfinite(out).all()
    assert err.max() <= bound


def _iter_reference(Y, max_sq, taps, delay):
    y = Y.astype(np.complex64)
    yt = W.delayed(y, taps, delay)
    R, p = W.correlations(y, yt, y, max_sq, "f32")
    g = np.stack([W.solve_bin(R[f], p[f]) for f in range(257)])
    return g, W.cond_of(R), yt


@pytest.mark.parametrize("T,taps,delay", [(378, 10, 3), (40, 10, 3), (97, 16, 1), (300, 1, 16)])
def test_iter_kernel(eng, T, taps, delay):
    """One iteration with a given epsilon, compared on g: both sides take lambda in float32 from
    the same y and add R and p in float64, so they differ by the order of T float64 additions
    and by the solve: (T + 64 K) u64 cond(R) relative to |g|."""
    if T == 378:
        Y = np.ascontiguousarray(W.stft(W.reverberant_speech(48000, 0), "f32").T)
    else:
        rng = np.random.default_rng(T)
        Y = (rng.standard_normal((257, T)) + 1j * rng.standard_normal((257, T))).astype(np.complex64)
        Y[7] = 0  # an all-zero bin: x = y
    max_sq = np.float32(np.max(Y.real ** 2 + Y.imag ** 2))
    g, X, nm = eng.selftest_iter(Y, max_sq, taps, delay)
    ref, cond, yt = _iter_reference(Y, max_sq, taps, delay)
    assert np.isfinite(g.view(np.float64)).all()
    assert cond.max() <= 1e8
    err = np.linalg.norm(g - ref, axis=1)
    tol = (T + 64 * taps) * U64 * cond * np.linalg.norm(ref, axis=1)
    print(f"iter T={T} K={taps}: max cond {cond.max():.3g}, worst err/tol "
          f"{np.max(err / np.maximum(tol, 1e-300)):.3g}")
    assert (err <= tol + 1e-300).all()
    if T != 378:
        assert not g[7].any()
    # X = y - g^H ytilde in float32 from the device's own g
    g32 = g.astype(np.complex64).astype(np.complex128)
    y64, yt64 = Y.astype(np.complex128), yt.astype(np.complex128)
    x64 = y64 - np.einsum("fk,fkt->ft", np.conj(g32), yt64)
    mag = np.abs(y64) + np.einsum("fk,fkt->ft", np.abs(g32), np.abs(yt64))
    assert (np.abs(X.T.astype(np.complex128) - x64) <= (2 * taps + 2) * 2 * U32 * mag + 1e-30).all()
    assert nm == np.float32(np.max(X.real ** 2 + X.imag ** 2))
    # a zero g_prev is x = y: the same bits
    g0, X0, nm0 = eng.selftest_iter(Y, max_sq, taps, delay, g_prev=np.zeros((257, taps), np.complex128))
    assert g0.tobytes() == g.tobytes() and X0.tobytes() == X.tobytes() and nm0 == nm


def test_iter_kernel_short_series(eng):
    """T = 11 with delay 3: taps 8 and 9 reach before the first frame everywhere, their rows of
    R are zero and their coefficients 0; an all-zero chunk gives g = 0."""
    rng = np.random.default_rng(11)
    Y = (rng.standard_normal((257, 11)) + 1j * rng.standard_normal((257, 11))).astype(np.complex64)
    g, X, _ = eng.selftest_iter(Y, np.float32(np.max(np.abs(Y) ** 2)), 10, 3)
    assert np.isfinite(g.view(np.float64)).all() and np.isfinite(X.view(np.float32)).all()
    assert not g[:, 8:].any() and g[:, :8].any()
    g, X, nm = eng.selftest_iter(np.zeros((257, 11), np.complex64), 0.0, 10, 3)
    assert not g.any() and not X.any() and nm == 0


# ---- the whole chunk ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [48000, 47999])
def test_end_to_end_within_four_times_the_f32_model(audio, speech, n):
    x, ref, model = speech[n]
    out = audio.apply_wpe_dereverberation(x)
    assert out.dtype == np.float32 and out.shape == (n,)
    e32 = float(np.max(np.abs(model.astype(np.float64) - ref)))
    err = float(np.max(np.abs(out.astype(np.float64) - ref)))
    print(f"wpe n={n}: device max abs err {err:.3g}, float32 model e32 {e32:.3g}")
    assert np.isfinite(out).all()
    assert err <= 4 * e32


def test_non_default_setting(audio):
    x = W.reverberant_speech(48000, 0)
    kw = dict(taps=4, delay=2, iterations=1)
    ref = W.apply_wpe(x, **kw)
    e32 = float(np.max(np.abs(W.apply_wpe(x, precision="f32", **kw).astype(np.float64) - ref)))
    out = audio.apply_wpe_dereverberation(x, 16000, 512, 128, 4, 2, 1)
    err = float(np.max(np.abs(out.astype(np.float64) - ref)))
    print(f"wpe taps=4 delay=2 iterations=1: device {err:.3g}, e32 {e32:.3g}")
    assert err <= 4 * e32


def test_value_errors_and_guard(audio):
    x = W.reverberant_speech(3000, 2)
    for kw in (dict(fft_size=256), dict(hop_size=64), dict(taps=0), dict(taps=17), dict(delay=0),
               dict(delay=17), dict(iterations=0), dict(iterations=9)):
        with pytest.raises(ValueError):
            audio.apply_wpe_dereverberation(x, **kw)
    with pytest.raises(ValueError):
        audio.apply_wpe_dereverberation(np.zeros(60 * 16000 + 1, np.float32))
    short = x[:1023]
    assert audio.apply_wpe_dereverberation(short) is short
    z = audio.apply_wpe_dereverberation(np.zeros(2000, np.float32))
    assert z.shape == (2000,) and not z.any()
    edge = audio.apply_wpe_dereverberation(x[:1024])  # T = 11: taps with delay >= T
    assert edge.shape == (1024,) and np.isfinite(edge).all()


# ---- the ragged batch ----------------------------------------------------------------------------

SPANS = [(0, 1024), (500, 2000), (30000, 46000), (20000, 68000), (60000, 93000)]


@pytest.fixture(scope="module")
def ragged(audio):
    sig = W.reverberant_speech(93000, 3)
    sig[30000:46000] *= 0.01  # a quiet chunk: its epsilon must be its own
    alone = [audio.apply_wpe_dereverberation(sig[s:e].copy()) for s, e in SPANS]
    return sig, alone


def test_ragged_batch_equals_each_span_alone(audio, eng, ragged):
    sig, alone = ragged
    assert [e - s for s, e in SPANS] == [1024, 1500, 16000, 48000, 33000]
    got = audio.apply_wpe_batch(sig, SPANS)
    assert eng.last_groups == 1
    for a, b in zip(got, alone):
        assert a.dtype == np.float32 and a.tobytes() == b.tobytes()
    try:  # a budget of one 16000-sample chunk's spectra: the batch must split
        eng.set_budget(2 * 257 * W.num_frames(16000) * 8)
        split = audio.apply_wpe_batch(sig, SPANS)
        assert eng.last_groups >= 4
    finally:
        eng.set_budget(2 << 30)
    for a, b in zip(split, alone):
        assert a.tobytes() == b.tobytes()


def test_batch_with_a_short_span_and_device_out(audio, ragged):
    sig, alone = ragged
    spans = [(100, 900)] + SPANS[:2]
    packed, off = audio.apply_wpe_batch(sig, spans, device_out=True)
    assert off.tolist() == [0, 800, 1824, 3324] and packed.is_cuda
    host = packed.cpu().numpy()
    assert host[:800].tobytes() == sig[100:900].tobytes()  # under the guard: unchanged
    assert host[800:1824].tobytes() == alone[0].tobytes()
    assert host[1824:].tobytes() == alone[1].tobytes()


def test_peak_limit_equals_the_limiter_per_chunk(audio, ragged):
    sig, alone = ragged
    loud = sig * np.float32(1.6)  # peaks above 0.95 in some chunks, below in the quiet one
    plain = audio.apply_wpe_batch(loud, SPANS)
    limited = audio.apply_wpe_batch(loud, SPANS, peak_limit=True)
    changed = 0
    for p, l in zip(plain, limited):
        want = np.asarray(audio.adaptive_peak_limit(p))
        assert l.tobytes() == want.tobytes()
        changed += l.tobytes() != p.tobytes()
    assert 0 < changed < len(SPANS)


def test_numpy_input_equals_tensor_input(audio, ragged):
    import torch
    sig, alone = ragged
    t = torch.from_numpy(sig).cuda()
    got = audio.apply_wpe_batch(t, SPANS[2:4])
    assert all(g.is_cuda for g in got)
    for g, a in zip(got, alone[2:4]):
        assert g.cpu().numpy().tobytes() == a.tobytes()
    one = audio.apply_wpe_dereverberation(t[20000:68000])
    assert one.is_cuda and one.cpu().numpy().tobytes() == alone[3].tobytes()
    short = t[:1000]
    assert audio.apply_wpe_dereverberation(short) is short


# ---- the drop-in ---------------------------------------------------------------------------------

def _stand_ins():
    from zasr.plan import best_split, silent_regions
    eng = types.ModuleType("ref_asr_engine")
    eng.find_silent_regions = lambda audio, *a, **k: silent_regions(audio)
    eng.find_best_split_point = best_split
    aud = types.ModuleType("ref_audio_preprocessing")
    aud.apply_wpe_dereverberation = lambda audio, *a, **k: "reference"
    aud.adaptive_peak_limit = lambda audio, target_peak=0.95: "reference"
    return eng, aud


class _Pipe:
    """The planner's caller: a `self` whose config enables WPE (core/asr_engine.py:2248)."""

    def __init__(self, eng, wpe=True):
        self.eng, self.config = eng, {"preprocess_wpe": wpe}

    def plan(self, audio):
        return self.eng.find_silent_regions(audio)


@pytest.fixture(scope="module")
def dropin_rec(audio):
    from model_fixtures import m_model
    from zasr import asr_engine as ae
    cfg, w, path = m_model()
    rec = ae.create_recognizer(path, 4, max_active_paths=8, hotwords=([], []), precision="bf16x3")
    yield ae, rec
    ae.set_wpe_plan(False)
    ae.clear_model_cache()


def test_dropin_wpe_plan_equals_chunk_by_chunk(dropin_rec, monkeypatch):
    import threading

    from zasr.dropin import install
    from zasr.plan import plan_chunks
    from zasr.synth_audio import synth_speech
    ae, rec = dropin_rec
    eng, aud = _stand_ins()
    install(eng, audio_module=aud, wpe=True)
    concat = synth_speech(125.0, 41)
    plan = plan_chunks(concat)
    assert len(plan) >= 4

    def one(i):
        s, e, _ = plan[i]
        c = aud.adaptive_peak_limit(aud.apply_wpe_dereverberation(concat[s:e]))
        return ae.decode_chunk(rec, c, s / 16000.0)

    monkeypatch.setenv("ZASR_PLAN_AHEAD", "0")
    want = [one(i) for i in range(len(plan))]
    monkeypatch.setenv("ZASR_PLAN_AHEAD", "1")
    h = rec["handle"]
    n = {"decode": 0, "batches": 0}
    d0, b0 = h.decode, h.decode_device_batches

    def dec(chunks, beam=0):
        n["decode"] += 1
        return d0(chunks, beam=beam)

    def bat(*a, **k):
        n["batches"] += 1
        return b0(*a, **k)
    h.decode, h.decode_device_batches = dec, bat
    try:
        _Pipe(eng).plan(concat)  # the hook: regions on the GPU, the plan started in WPE mode
        out, errs = [None] * len(plan), []

        def worker(idx):
            try:
                for i in idx:
                    out[i] = one(i)
            except Exception as ex:  # pragma: no cover - surfaced below
                errs.append(ex)
        ts = [threading.Thread(target=worker, args=(list(range(k, len(plan), 2)),)) for k in (0, 1)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
        assert n == {"decode": 0, "batches": 1}, n  # ONE decode of the plan's packed chunks
    finally:
        del h.decode, h.decode_device_batches
    assert sum(len(w) for w in want) > 30
    assert out == want


def test_dropin_without_wpe_switch_behaves_as_before(dropin_rec):
    from zasr import audio as za
    from zasr.dropin import install
    from zasr.plan import plan_chunks
    from zasr.synth_audio import synth_speech
    ae, rec = dropin_rec
    eng, aud = _stand_ins()
    install(eng, audio_module=aud)
    assert aud.apply_wpe_dereverberation(None) == "reference"
    assert aud.adaptive_peak_limit is za.adaptive_peak_limit
    concat = synth_speech(70.0, 42)
    plan = plan_chunks(concat)
    _Pipe(eng).plan(concat)  # a WPE caller: the plan is registered, nothing decodes
    s, e, _ = plan[0]
    sig = ae._planned_span(concat[s:e])[0]
    assert sig.wpe is None and len(sig.jobs) == 0 and sig.d_audio is None
