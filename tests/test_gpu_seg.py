"""PyanNet segmentation on the MI355X (zasr_seg_*) against the float64
restatement of the network (tests/pyannet_reference.py), with the seeded weights of
zasr.pyannet.synth_weights and synthetic speech.

Tolerance.  On exactly the four logits cases below, torch's float32 evaluation of the same
network on the CPU (F.conv1d / F.instance_norm / nn.LSTM: the same precision class in another
summation order) deviates from the float64 restatement by at most 1.2623e-4 (largest absolute
log-probability difference; per case 2.14e-5, 1.26e-4, 8.22e-5, 1.02e-4 --
tests/test_pyannet_reference.py re-measures it).  The device is allowed 8x that:
BOUND = 1.0099e-3.  Class maps must equal the float64 argmax on every frame whose float64 top-2
margin exceeds 2 x BOUND; the frames excluded that way are 7 of 3545 (0.20 %, bound 1 %), and
the float32 evaluation itself has no flip outside them.
"""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

F32_DEV = 1.2623e-4          # measured: torch float32 vs float64 on LOGIT_CASES
BOUND = 8 * F32_DEV
CHUNK, STEP = 160000, 80000


@pytest.fixture(scope="module")
def sess(tmp_path_factory):
    if not gpu_available():
        pytest.skip("no GPU")
    import seg_inputs as S
    from zasr.binding import SegSession
    from zasr.pyannet import save_model_dir
    cfg, w = S.network()
    d = tmp_path_factory.mktemp("seg")
    save_model_dir(str(d), cfg, w)
    s = SegSession(str(d))
    yield s
    s.close()


@pytest.fixture(scope="module")
def file61():
    """A 61 s signal, its zero-padded chunk batch and the float64 logits of every chunk."""
    import seg_inputs as S
    from pyannet_reference import forward
    from zasr.segmentation import chunk_starts
    a = S.speech(61.0, 30)   # seed chosen for test_pyannote_vad_regions' precondition
    starts = chunk_starts(a.shape[0])
    batch = np.zeros((len(starts), CHUNK), np.float32)
    for i, cs in enumerate(starts):
        seg = a[cs:cs + CHUNK]
        batch[i, :seg.shape[0]] = seg
    return a, starts, batch, forward(S.network()[1], batch)


@pytest.mark.parametrize("n,T", [(1, 1261), (3, 1531), (1, CHUNK), (5, CHUNK)])
def test_logits_match_float64(sess, n, T):
    import seg_inputs as S
    ref = S.case_ref64(n, T)
    got = sess.logits(S.case_batch(n, T))
    assert got.shape == ref.shape and got.dtype == np.float32
    dev = float(np.abs(got - ref).max())
    print(f"seg logits ({n}, {T}): max |device - float64| = {dev:.3e} (bound {BOUND:.3e})")
    assert dev <= BOUND


def test_class_maps_match_float64_argmax(sess):
    import seg_inputs as S
    frames = excluded = 0
    for n, T in S.LOGIT_CASES:
        ref = S.case_ref64(n, T)
        got = sess.logits(S.case_batch(n, T)).argmax(-1)
        sure = S.top2_margin(ref) > 2 * BOUND
        assert np.array_equal(got[sure], ref.argmax(-1)[sure])
        frames += sure.size
        excluded += int((~sure).sum())
    print(f"seg class maps: {excluded} of {frames} frames excluded")
    assert excluded <= 0.01 * frames


@pytest.mark.parametrize("T,group", [(4000, 4), (4000, 2), (4000, 8), (4000, 16), (4000, 0), (CHUNK, 2)])
def test_chunk_is_bit_identical_in_any_batch(sess, T, group):
    """One chunk alone, first, last and in the middle of batches of 1, B - 1, B, B + 1 and
    2 B + 1 chunks, B = the recurrence group (forced, and the launcher's own choice with
    group = 0): full groups, group tails of 1 and of B - 1, every slot of a group, in both
    directions (each output row holds the forward and the backward half)."""
    import seg_inputs as S
    a = S.speech(35.0, 11)
    sess.set_group(0)
    probe = a[1000:1000 + T]
    alone = sess.logits(probe[None])
    B0 = sess.last_group
    try:
        sess.set_group(group)
        B = group if group else B0
        sizes = sorted({1, max(1, B - 1), B, B + 1, 2 * B + 1}) if T < CHUNK else [B + 1]
        for n in sizes:
            for pos in sorted({0, n // 2, n - 1}):
                batch = np.stack([a[7000 + 900 * i:7000 + 900 * i + T] for i in range(n)])
                batch[pos] = probe
                got = sess.logits(batch)
                assert sess.last_group == B
                assert np.array_equal(got[pos], alone[0]), (n, pos, B)
    finally:
        sess.set_group(0)


def test_whole_file_equals_host_batch(sess, file61):
    import torch
    a, starts, batch, _ = file61
    F = sess.num_frames(CHUNK)
    assert F == 589 and len(starts) == 12 == sess.num_chunks(a.shape[0])
    host = sess.logits(batch)
    sess.trim()     # the workspace is freed and allocated again: same bits
    assert np.array_equal(sess.logits(batch), host)
    d_audio = torch.from_numpy(a.copy()).cuda()
    d_logits = torch.empty((len(starts), F, 7), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    cls = sess.classes_device(d_audio.data_ptr(), a.shape[0], d_logits=d_logits.data_ptr())
    dev = d_logits.cpu().numpy()
    assert np.array_equal(dev, host)
    assert cls.shape == (12, F) and np.array_equal(cls, host.argmax(-1))
    d_logits.zero_()
    cls2 = sess.classes_device(d_audio.data_ptr(), a.shape[0], d_logits=d_logits.data_ptr())
    assert np.array_equal(cls2, cls) and np.array_equal(d_logits.cpu().numpy(), dev)
    # without a logits buffer
    assert np.array_equal(sess.classes_device(d_audio.data_ptr(), a.shape[0]), cls)
    # 3 s: one chunk, padded with zeros on the device
    short = torch.from_numpy(a[:48000].copy()).cuda()
    torch.cuda.synchronize()
    c1 = sess.classes_device(short.data_ptr(), 48000)
    pad = np.zeros((1, CHUNK), np.float32)
    pad[0, :48000] = a[:48000]
    assert c1.shape == (1, F) and np.array_equal(c1, sess.logits(pad).argmax(-1))


def test_bad_arguments(sess, tmp_path):
    from zasr.binding import SegSession, ZasrError
    with pytest.raises(ZasrError):
        sess.logits(np.zeros((1, 1260), np.float32))
    with pytest.raises(ZasrError):
        sess.logits(np.zeros((0, 2000), np.float32))
    with pytest.raises(ZasrError):
        sess.classes_device(0, 1000, chunk_samples=1000)
    fp = sess.lib.zasr_seg_logits.argtypes[1]
    assert sess.lib.zasr_seg_logits(sess.handle, fp(), 1, 2000, fp()) == 1      # null pointers
    x = np.zeros(1260, np.float32)
    assert sess.lib.zasr_seg_logits(sess.handle, x.ctypes.data_as(fp), 1, 1260,
                                    x.ctypes.data_as(fp)) == 1
    assert b"1261" in sess.lib.zasr_last_error()
    with pytest.raises(FileNotFoundError):
        SegSession(str(tmp_path / "nothing_here"))


def S_margin(logits):
    import seg_inputs as S
    return S.top2_margin(logits)


def test_pyannote_vad_regions(sess, file61):
    """Regions and overlap regions of the device path = the host logic on the float64 class
    maps.  Precondition (asserted): the frames the bound cannot decide (float64 top-2 margin
    <= 2 x BOUND) flip no > 0.5 decision -- with each of them voting for either of its two
    candidate classes, every output frame's speech and overlap ratios stay on the same side."""
    import torch
    from zasr.segmentation import OVERLAP_CLASSES_FROM, aggregate, output_frames, pyannote_vad
    a, starts, batch, ref = file61
    order = np.argsort(ref, -1)
    top, second = order[..., -1], order[..., -2]
    unsure = S_margin(ref) <= 2 * BOUND
    print(f"pyannote_vad: {int(unsure.sum())} of {unsure.size} frames within 2 x bound")
    assert unsure.mean() <= 0.01
    out_f, n_out = output_frames(starts, ref.shape[1], a.shape[0])
    keep = out_f < n_out
    total = np.bincount(out_f[keep], minlength=n_out).astype(np.float32)
    for first in (1, OVERLAP_CLASSES_FROM):
        lo = np.where(unsure, np.minimum(top >= first, second >= first), top >= first)
        hi = np.where(unsure, np.maximum(top >= first, second >= first), top >= first)
        with np.errstate(divide="ignore", invalid="ignore"):
            d_lo = np.bincount(out_f[keep & lo], minlength=n_out).astype(np.float32) / total > 0.5
            d_hi = np.bincount(out_f[keep & hi], minlength=n_out).astype(np.float32) / total > 0.5
        assert np.array_equal(d_lo, d_hi)
    want_speech, want_overlap = aggregate(ref.argmax(-1), starts, a.shape[0])
    assert len(want_speech) >= 2 and len(want_overlap) >= 1      # the decode is exercised
    d_audio = torch.from_numpy(a.copy()).cuda()
    torch.cuda.synchronize()
    got = pyannote_vad(d_audio, sess)
    assert list(got) == want_speech and got.overlap_regions == want_overlap

    # the session on a stub diarizer, through the host-batch surface the reference uses
    # (seg_sess.run on [n, 1, 160000] batches of at most 32)
    class Diarizer:
        pass
    dz = Diarizer()
    dz.seg_sess = sess
    got2 = pyannote_vad(a, dz.seg_sess)
    assert list(got2) == want_speech and got2.overlap_regions == want_overlap


def test_full_pipe_with_and_without_segmentation(sess, tmp_path_factory):
    from zasr.binding import CamppEmbedder, Recognizer, VibertSession
    from zasr.campp import CamppConfig, window_plan
    from zasr.campp import save_model_dir as campp_save
    from zasr.campp import synth_weights as campp_weights
    from zasr.model import save_model_dir, synth_tokens, synth_weights, zipformer_tiny
    from zasr.pipeline import FullPipe, l2_normalise
    from zasr.plan import plan_chunks
    from zasr.segmentation import pyannote_vad
    from zasr.synth_audio import synth_speech
    from zasr.vibert import save_model_dir as vib_save
    from zasr.vibert import synth_weights as vib_weights
    from zasr.vibert import vibert_tiny
    d = tmp_path_factory.mktemp("segpipe")
    cfg = zipformer_tiny(64)
    toks = synth_tokens(cfg.vocab_size)
    save_model_dir(str(d / "asr"), cfg, synth_weights(cfg, 5, blank_bias=-1.5), toks)
    rec = Recognizer(str(d / "asr"), "greedy_search", 1, precision="fp32")
    ccfg = CamppConfig()
    campp_save(str(d / "campp"), ccfg, campp_weights(ccfg, 3))
    emb = CamppEmbedder(str(d / "campp"))
    vcfg = vibert_tiny()
    vib_save(str(d / "vib"), vcfg, vib_weights(vcfg, 4))
    vib = VibertSession(str(d / "vib"))
    recd = {"id2token": dict(enumerate(toks)), "vocab_size": cfg.vocab_size}
    audio = synth_speech(75.0, 31)          # the existing pipe fixture's file
    try:
        plain = FullPipe(rec, recd, emb, vib, vcfg.vocab_size, beam=1, campp_batch=16, diarize=True)
        plain.prepare(audio)
        out0 = plain.run()
        regions = plan_chunks(audio.astype(np.float32), overlap_sec=0.0)
        assert plain.r_off_all == [s for s, _, _ in regions]
        assert plain.r_len_all == [e - s for s, e, _ in regions]
        assert set(out0) == {"words", "tokens", "text", "vibert_runs", "vibert_rows", "embeddings",
                             "windows", "token_ids", "speaker_segments", "speaker_labels"}
        # who-spoke-when of the default path: one label per window, and the same on a second run
        assert len(out0["speaker_segments"]) >= 1
        assert len(out0["speaker_labels"]) == len(out0["windows"])
        again = plain.run()
        assert again["speaker_segments"] == out0["speaker_segments"]
        assert np.array_equal(again["speaker_labels"], out0["speaker_labels"])
        assert np.array_equal(again["embeddings"], out0["embeddings"])

        p = FullPipe(rec, recd, emb, vib, vcfg.vocab_size, beam=1, campp_batch=16, diarize=True,
                     segmentation=sess)
        p.prepare(audio)
        out = p.run()
        speech = pyannote_vad(audio.astype(np.float32), sess)
        assert out["overlap_regions"] == speech.overlap_regions
        assert p.r_off_all == [int(s * 16000) for s, _ in speech]
        assert p.r_len_all == [min(int(e * 16000), audio.shape[0]) - int(s * 16000) for s, e in speech]
        assert set(out) == set(out0) | {"overlap_regions"}
        assert out["words"] == out0["words"] and out["text"] == out0["text"]
        # the CAM++ windows are cut from those regions: embed them directly
        a32 = audio.astype(np.float32)
        feats, meta = [], []
        for r, (o, n) in enumerate(zip(p.r_off, p.r_len)):
            fb = emb.fbank(a32[o:o + n])
            for s, k in window_plan(fb.shape[0]):
                x = np.zeros((150, 80), np.float32)
                x[:k] = fb[s:s + k]
                feats.append(x)
                meta.append((r, s, k))
        assert out["windows"].tolist() == [list(m) for m in meta]
        assert np.array_equal(out["embeddings"], l2_normalise(emb.embed(np.stack(feats))))
        assert len(out["speaker_labels"]) == len(meta)
    finally:
        rec.close()
        emb.close()
        vib.close()
