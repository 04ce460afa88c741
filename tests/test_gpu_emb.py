"""Community-1 speaker embeddings on the MI355X (zasr_emb_*) from a synthetic model
directory, against the float64 restatement of tests/resnet34_reference.py.

Tolerance.  On exactly the inputs below torch's float32 evaluation of the same network on the
CPU deviates from the float64 restatement, relative to the float64 peak, by 4.83e-7 (T = 40) and
3.40e-7 (T = 41) on the frame features, 5.79e-7 on the 12.3 s signal's embeddings and 7.80e-7 /
5.41e-7 on the segments of 9 / 250 frames (tests/test_resnet34_reference.py re-measures each).
The device is allowed 8 x its own case's figure.  The frame features also pass the reference's own acceptance rule for this stage
against the torch float32 run: max_abs <= 2e-3 or rel_l2 <= 2e-4 (core/calibration.py:84,
:1279-1286).

The end-to-end checks take the DEVICE's fbank rows as the restatement's input: the fbank kernel
is held to its own bound alone (tests/test_gpu_emb_kernels.py: 2e-3 absolute, three orders above
float32 rounding), and what is checked here is everything behind it -- the row windows, the zero
tail, the CMVN over all 998 rows, the encoder, the masks, the pooling and the projection -- at
float32's precision.  The chunk embeddings are then also held to the restatement driven by the
float64 fbank, at that bound plus what the fbank's 2e-3 tolerance propagates to (8.33e-5 of the
peak: the restatement's own deviation under a +-2e-3 perturbation of its fbank image).
"""
import numpy as np
import pytest

from conftest import gpu_available

import resnet34_reference as R

pytestmark = pytest.mark.gpu
f64 = np.float64


@pytest.fixture(scope="module")
def net():
    if not gpu_available():
        pytest.skip("no GPU")
    return R.network()


@pytest.fixture(scope="module")
def sess(net, tmp_path_factory):
    from zasr.binding import EmbSession
    from zasr.resnet34 import save_model_dir
    cfg, w, _ = net
    d = tmp_path_factory.mktemp("emb")
    save_model_dir(str(d), cfg, w)
    s = EmbSession(str(d))
    yield s
    s.close()


@pytest.mark.parametrize("T", R.MODEL_T)
def test_frame_features_match_float64(sess, net, T):
    cfg, _w, fold = net
    x = R.model_feats(T)
    ref = R.forward(cfg, fold, x)
    got = sess.encode(x)
    assert got.shape == ref.shape == (2, 2560, sess.num_feat_frames(T)) and got.dtype == np.float32
    dev = R.peak_dev(got, ref)
    print(f"T = {T}: max |device - float64| / peak = {dev:.3e} (bound {R.BOUND[T]:.3e})")
    assert dev <= R.BOUND[T]
    ma, rl = R.acceptance(got, R.torch_forward(cfg, fold, x, np.float32))
    print(f"T = {T}: against torch float32: max_abs {ma:.3e}, rel_l2 {rl:.3e}")
    assert ma <= 2e-3 or rl <= 2e-4
    # a sample alone, and behind another, gives the same bytes
    assert np.array_equal(sess.encode(x[1:]), got[1:])
    from zasr.resnet34 import encoder_flops
    assert abs(sess.encoder_flops(T) - encoder_flops(cfg, T)) < 1.0      # the engine's count, from its config


def test_ort_surface_returns_encodes_bytes(sess):
    x = R.model_feats(40)
    want = sess.encode(x)
    out = sess.run(None, {"fbank_features": x})
    assert len(out) == 1 and np.array_equal(out[0], want)
    name = sess.get_outputs()[0].name
    b = sess.io_binding()
    b.bind_cpu_input("fbank_features", x)
    b.bind_output(name)
    sess.run_with_iobinding(b)
    got = b.get_outputs()[0].numpy()
    assert got.dtype == np.float32 and np.array_equal(got, want)


@pytest.fixture(scope="module")
def e2e(sess, net):
    cfg, w, fold = net
    audio = R.speech(R.E2E_SEC, R.E2E_SEED)
    full, clean = R.e2e_masks()
    from zasr.community1 import extract_embeddings
    got = extract_embeddings(sess, audio, full, clean, R.NSEG, list(R.E2E_STARTS), R.MIN_SEG_FRAMES)
    rows = sess.fbank(audio, R.TAIL)
    ref = R.chunk_embeddings(cfg, w, fold, rows, R.E2E_STARTS, full, clean)
    return audio, full, clean, got, rows, ref


def test_chunk_embeddings_match_float64_end_to_end(sess, net, e2e):
    cfg, w, _fold = net
    audio, full, clean, got, rows, ref = e2e
    assert got.shape == (4, 3, 256) and got.dtype == np.float32 and not np.any(np.isnan(got))
    assert rows.shape[0] == 1 + (audio.shape[0] + 160000 - 400) // 160
    # the last chunk's window runs into the zero tail
    assert R.E2E_STARTS[-1] // 160 + R.CHUNK_FRAMES > R.fbank_rows(audio.shape[0])
    dev = R.peak_dev(got, ref)
    print(f"12.3 s, 4 chunks: max |device - float64| / peak = {dev:.3e} (bound {R.BOUND_EMB:.3e})")
    assert dev <= R.BOUND_EMB
    # the all-zero speaker's embedding is the bias, bit for bit; the switch speaker is not
    assert np.array_equal(got[1, 2], w["resnet.seg_1.bias"])
    assert not np.array_equal(got[0, 1], got[1, 1])
    # the device's own fbank rows against the float64 fbank of the same signal
    image = R.fbank(audio, R.TAIL)
    assert np.max(np.abs(rows.astype(f64) - image)) <= R.FBANK_ATOL
    # and the whole stage against the restatement driven by that float64 fbank: the fbank's error
    # is then an input perturbation, allowed what its 2e-3 tolerance propagates to (FBANK_PROP)
    full64 = R.chunk_embeddings(cfg, w, _fold, image, R.E2E_STARTS, full, clean)
    dev = R.peak_dev(got, full64)
    print(f"12.3 s, 4 chunks, float64 fbank: max |device - float64| / peak = {dev:.3e} "
          f"(bound {R.BOUND_EMB_FULL:.3e})")
    assert dev <= R.BOUND_EMB_FULL


def test_chunk_embeddings_from_hbm_equal_the_host_signal(sess, e2e):
    import torch
    from zasr.community1 import extract_embeddings
    audio, full, clean, got, _rows, _ref = e2e
    d = torch.from_numpy(audio.copy()).cuda()
    again = extract_embeddings(sess, d, full, clean, R.NSEG, list(R.E2E_STARTS), R.MIN_SEG_FRAMES)
    assert np.array_equal(again, got)


def test_chunk_is_bit_identical_alone_in_a_batch_and_through_any_group(sess):
    audio = R.speech(25.0, 77)
    starts = np.arange(0, 17) * 16000          # the 1 s step of a 25 s signal: 17 chunks
    rng = np.random.default_rng(5)
    masks = (rng.random((17, 3, R.NSEG)) < 0.5).astype(np.uint8)
    masks[8, 1] = 0
    sess.set_group(0)
    whole = sess.chunk_embeddings(audio, starts, masks)
    assert whole.shape == (17, 3, 256) and sess.last_group == 17
    alone = sess.chunk_embeddings(audio, starts[8:9], masks[8:9])
    assert sess.last_group == 1
    assert alone.tobytes() == whole[8:9].tobytes()
    for g in (1, 3):
        sess.set_group(g)
        again = sess.chunk_embeddings(audio, starts, masks)
        assert sess.last_group == g
        assert again.tobytes() == whole.tobytes(), g
    sess.set_group(0)
    sess.trim()


@pytest.mark.parametrize("frames", [9, 250])
def test_segment_embedding_matches_float64(sess, net, frames):
    cfg, w, fold = net
    audio = R.segment_audio(frames)
    got = sess.segment_embedding(audio)
    rows = sess.fbank(audio)
    assert rows.shape == (frames, 80) and got is not None and got.shape == (256,)
    ref = R.segment_embedding(cfg, w, fold, rows)
    dev = R.peak_dev(got, ref)
    print(f"segment of {frames} frames: max |device - float64| / peak = {dev:.3e} (bound {R.BOUND_SEG[frames]:.3e})")
    assert dev <= R.BOUND_SEG[frames]
    from zasr.community1 import compute_single_embedding
    assert np.array_equal(compute_single_embedding(sess, audio), got)


def test_segment_of_eight_frames_is_too_short(sess):
    audio = R.speech(3.0, 33)[:400 + 160 * 7 + 159]
    assert R.fbank_rows(audio.shape[0]) == 8
    assert sess.segment_embedding(audio) is None
    assert sess.segment_embedding(np.zeros(10, np.float32)) is None


def test_attach_serves_a_diarizer_shaped_object(sess, e2e):
    from zasr.community1 import attach

    class Diarizer:
        emb_sess = emb_W = emb_b = None

    audio, full, clean, got, _rows, _ref = e2e
    d = attach(Diarizer(), sess)
    assert d.emb_sess is sess and d.emb_W.shape == (256, 5120) and d.emb_b.shape == (256,)
    calls = []
    out = d._extract_embeddings(audio, full, clean, R.NSEG, list(R.E2E_STARTS), R.MIN_SEG_FRAMES,
                                lambda a, b: calls.append((a, b)))
    assert np.array_equal(out, got) and calls == [(85, 100)]
