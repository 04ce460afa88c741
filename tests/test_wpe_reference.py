"""CPU checks of the WPE contract's float64 restatement (tests/wpe_reference.py)
and of the drop-in's WPE host logic with stand-in modules (no GPU): the rebinding, the tag that
links a processed chunk to its plan span through adaptive_peak_limit and compute_fbank_ort, and
the per-chunk fall-back."""
import types

import numpy as np
import pytest

import wpe_reference as W
from test_dropin_plan import FakeHandle, _rec
from zasr import asr_engine as ae
from zasr.plan import best_split, plan_chunks, silent_regions
from zasr.synth_audio import synth_speech


# ---- the restatement's own checks ---------------------------------------------------------------

def test_stft_istft_reconstructs():
    rng = np.random.default_rng(0)
    for n in (1024, 5000, 16001):
        x = rng.standard_normal(n)
        assert np.max(np.abs(W.istft(W.stft(x), n) - x)) <= 1e-12


@pytest.mark.parametrize("n,T", [(1024, 11), (1151, 11 + 1), (1152, 12), (48000, 378), (480000, 3753)])
def test_frame_count(n, T):
    assert W.num_frames(n) == T == int(np.ceil((n + 768 - 512) / 128)) + 1
    if n <= 48000:
        assert W.stft(np.zeros(n)).shape == (T, 257)


def test_known_taps_are_recovered():
    """Each bin is driven by sparse impulses s through y_t = s_t + g^H ytilde_t with known taps:
    wherever s_t = 0 the prediction is exact, and once lambda follows |x|^2 those frames carry
    all the weight, so the iteration converges to g."""
    rng = np.random.default_rng(1)
    F, T, K, D = 257, 400, 10, 3
    g = (rng.standard_normal((F, K)) + 1j * rng.standard_normal((F, K))) * 0.08
    s = np.zeros((F, T), np.complex128)
    hits = rng.random((F, T)) < 0.06
    s[hits] = (rng.standard_normal(hits.sum()) + 1j * rng.standard_normal(hits.sum()))
    y = np.zeros((F, T), np.complex128)
    for t in range(T):
        acc = s[:, t].copy()
        for k in range(K):
            if t - D - k >= 0:
                acc += np.conj(g[:, k]) * y[:, t - D - k]
        y[:, t] = acc
    info = {}
    x = W.wpe(np.ascontiguousarray(y.T), K, D, 8, info=info)
    assert np.max(np.abs(info["g"][-1] - g)) <= 1e-6
    assert np.max(np.abs(x.T - s)) <= 1e-5


def test_degenerate_rules():
    x = W.reverberant_speech(3000, 2).astype(np.float64)
    short = x[:1023]
    assert W.apply_wpe(short) is short  # under 2 * fft_size: the input itself
    edge = W.apply_wpe(x[:1024])  # T = 11: taps 8 and 9 lie before the first frame everywhere
    assert edge.shape == (1024,) and np.isfinite(edge).all()
    info = {}
    W.apply_wpe(x[:1024], info=info)
    assert all(not g[:, 8:].any() for g in info["g"])
    zero = W.apply_wpe(np.zeros(2000))
    assert zero.shape == (2000,) and not zero.any()
    # an all-zero bin of a chunk that is not zero: g = 0, x = y
    Y = W.stft(x)
    Y[:, 9] = 0
    info = {}
    X = W.wpe(Y, info=info)
    assert not X[:, 9].any() and all(not g[9].any() for g in info["g"])
    assert np.isfinite(X.view(np.float64)).all()
    # a singular R (a constant series: every delayed copy is the same vector) keeps one tap
    R = np.ones((4, 4), np.complex128)
    g = W.solve_bin(R, np.ones(4, np.complex128))
    assert g[0] == 1 and not g[1:].any()


@pytest.mark.parametrize("n,seed,kw", [(48000, 0, {}), (47999, 1, {}),
                                       (48000, 0, dict(taps=4, delay=2, iterations=1))])
def test_parity_inputs_are_well_conditioned(n, seed, kw):
    """Parity with the float64 reference is claimed where its R is well conditioned: every input
    tests/test_gpu_wpe.py compares on stays under cond(R) = 1e8 over bins and iterations."""
    info = {}
    out = W.apply_wpe(W.reverberant_speech(n, seed), info=info, **kw)
    assert np.isfinite(out).all() and 0 < info["cond"] <= 1e8, info["cond"]


def test_f32_model_stays_close():
    x = W.reverberant_speech(16000, 4)
    a, b = W.apply_wpe(x), W.apply_wpe(x, precision="f32")
    assert b.dtype == np.float32 and np.max(np.abs(a - b)) <= 1e-5


# ---- the drop-in's host logic, with stand-ins ------------------------------------------------------

def _modules():
    eng = types.ModuleType("ref_asr_engine")
    eng.find_silent_regions = lambda audio, *a, **k: silent_regions(audio)
    eng.find_best_split_point = best_split
    aud = types.ModuleType("ref_audio_preprocessing")
    aud.apply_wpe_dereverberation = lambda audio, *a, **k: "reference"
    aud.adaptive_peak_limit = lambda audio, target_peak=0.95: "reference"
    return eng, aud


def _fake_batch(calls):
    def batch(src, plan, wpe, device_id):
        calls.append((len(plan), dict(wpe)))
        lens = [e - s for s, e in plan]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        host = np.concatenate([np.asarray(src[s:e]) * np.float32(0.5) for s, e in plan])
        return None, off, host
    return batch


def test_install_wpe_rebinds_and_needs_the_audio_module():
    from zasr import audio as za
    from zasr.dropin import install
    eng, aud = _modules()
    with pytest.raises(ValueError):
        install(eng, wpe=True)
    try:
        done = install(eng, audio_module=aud)
        assert aud.apply_wpe_dereverberation(None) == "reference"  # stays the reference's
        assert aud.adaptive_peak_limit is za.adaptive_peak_limit and not ae.wpe_plan_on()
        assert "audio_preprocessing.apply_wpe_dereverberation" not in done
        done = install(eng, audio_module=aud, wpe=True)
        assert aud.apply_wpe_dereverberation is ae.wpe_dereverberation_planned
        assert aud.adaptive_peak_limit is ae.peak_limit_planned and ae.wpe_plan_on()
        assert "audio_preprocessing.apply_wpe_dereverberation" in done
        assert done.count("audio_preprocessing.adaptive_peak_limit") == 1
        assert aud.preprocess_audio is za.preprocess_audio
    finally:
        ae.set_wpe_plan(False)


class _Pipe:
    """The caller the hook looks at: a `self` with a config (core/asr_engine.py:2248)."""

    def __init__(self, eng, wpe):
        self.eng, self.config = eng, {"preprocess_wpe": wpe}

    def plan(self, audio):
        return self.eng.find_silent_regions(audio)


def test_wpe_plan_serves_tagged_chunks_from_one_decode(monkeypatch):
    from zasr import audio as za
    from zasr.dropin import install
    eng, aud = _modules()
    monkeypatch.setenv("ZASR_GPU_PLANNER", "0")  # no GPU here: the reference's own detector
    calls = []
    monkeypatch.setattr(ae, "_wpe_batch", _fake_batch(calls))
    monkeypatch.setattr(za, "adaptive_peak_limit", lambda a, target_peak=0.95: a)
    h = FakeHandle()
    rec = _rec(h)
    monkeypatch.setattr(ae, "_recognizer_cache", {("m", 8): rec})
    monkeypatch.setattr(ae, "_last_handle", h)
    concat = synth_speech(150.0, 21)
    plan = plan_chunks(concat)
    assert len(plan) >= 4
    try:
        install(eng, audio_module=aud, wpe=True)
        _Pipe(eng, True).plan(concat)
        sig = ae._planned_span(concat[plan[0][0]:plan[0][1]], wpe=True)[0]
        assert sig.wpe == ae.WPE_DEFAULTS and ae._planned_span(concat[plan[0][0]:plan[0][1]]) is None
        sig.jobs[h][8].thread.join(timeout=30)
        assert h.calls == [len(plan)] and calls == [(len(plan), ae.WPE_DEFAULTS)]
        want = [ae.decode_chunk(_rec(FakeHandle()), concat[s:e] * np.float32(0.5), s / 16000.0)
                for s, e, _ in plan]
        got = []
        for i, (s, e, _) in enumerate(plan):
            chunk = aud.apply_wpe_dereverberation(concat[s:e])
            assert chunk.tobytes() == (concat[s:e] * np.float32(0.5)).tobytes()
            chunk = aud.adaptive_peak_limit(chunk)
            if i % 2:  # the ROVER path: features of the tagged chunk keep the link
                feats = ae.compute_fbank_ort(chunk)
                got.append(ae.decode_chunk(rec, chunk, s / 16000.0, precomputed_features=feats))
            else:
                got.append(ae.decode_chunk(rec, chunk, s / 16000.0))
        assert got == want
        assert h.calls == [len(plan)] and len(calls) == 1  # ONE batch, ONE decode
        # a raw view of a signal planned in WPE mode is not the plan's chunk
        s, e, _ = plan[1]
        ae.decode_chunk(rec, concat[s:e], 0.0)
        assert h.calls == [len(plan), 1]
    finally:
        ae.set_wpe_plan(False)


def test_limiter_passes_the_tag_to_a_new_array(monkeypatch):
    from zasr import audio as za
    monkeypatch.setattr(ae, "_wpe_batch", _fake_batch([]))
    monkeypatch.setattr(za, "adaptive_peak_limit", lambda a, target_peak=0.95: a * np.float32(0.9))
    concat = synth_speech(80.0, 22)
    plan = plan_chunks(concat)
    assert ae.register_plan_from_regions(concat, silent_regions(concat), best_split, start=False,
                                         wpe=dict(ae.WPE_DEFAULTS))
    s, e, _ = plan[1]
    chunk = ae.wpe_dereverberation_planned(concat[s:e])
    sig = ae._wpe_tag(chunk)[0]
    limited = ae.peak_limit_planned(chunk)
    assert limited is not chunk and ae._wpe_tag(limited) == (sig, (s, e))
    assert ae._wpe_tag(ae.peak_limit_planned(chunk, 0.5)) is None  # another target: no link
    h = FakeHandle()
    ae.decode_chunk(_rec(h), limited, 0.0)
    assert h.calls == [len(plan)]


def test_untagged_chunks_and_a_failed_batch_fall_back(monkeypatch, caplog):
    from zasr import audio as za
    seen = []
    monkeypatch.setattr(za, "apply_wpe_dereverberation",
                        lambda a, **kw: seen.append(kw) or np.asarray(a) * np.float32(0.25))
    concat = synth_speech(80.0, 23)
    plan = plan_chunks(concat)
    s, e, _ = plan[0]
    # no plan in WPE mode: processed on its own, untagged, decoded on its own
    out = ae.wpe_dereverberation_planned(concat[s:e].copy())
    assert seen == [ae.WPE_DEFAULTS] and ae._wpe_tag(out) is None
    h = FakeHandle()
    ae.decode_chunk(_rec(h), out, 0.0)
    assert h.calls == [1]

    def boom(*a):
        raise RuntimeError("hipErrorOutOfMemory (stand-in)")
    monkeypatch.setattr(ae, "_wpe_batch", boom)
    assert ae.register_plan_from_regions(concat, silent_regions(concat), best_split, start=False,
                                         wpe=dict(ae.WPE_DEFAULTS))
    with caplog.at_level("WARNING", logger="zasr.asr_engine"):
        outs = [ae.wpe_dereverberation_planned(concat[a:b]) for a, b, _ in plan]
    assert len(seen) == 1 + len(plan) and all(ae._wpe_tag(o) is None for o in outs)
    assert sum("WPE plan batch failed" in r.getMessage() for r in caplog.records) == 1
    # other arguments than the plan's: the per-chunk route too
    monkeypatch.setattr(ae, "_wpe_batch", _fake_batch([]))
    other = synth_speech(70.0, 24)
    assert ae.register_plan_from_regions(other, silent_regions(other), best_split, start=False,
                                         wpe=dict(ae.WPE_DEFAULTS))
    a, b, _ = plan_chunks(other)[0]
    assert ae._wpe_tag(ae.wpe_dereverberation_planned(other[a:b], taps=5)) is None
    assert ae._wpe_tag(ae.wpe_dereverberation_planned(other[a:b])) is not None
