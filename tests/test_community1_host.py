"""Host logic of the community-1 embedding drop-in (zasr/community1.py) and the onnxruntime
surface of binding.EmbSession, without a GPU: stub sessions stand in for the device."""
import numpy as np
import pytest

import resnet34_reference as R
from zasr import community1 as C1
from zasr.binding import EmbSession, ZasrError


class StubSession:
    """Records what the drop-in hands the device."""
    model_dir = None

    def __init__(self):
        self.calls = []

    def chunk_embeddings(self, audio, starts, masks):
        self.calls.append(("host", np.asarray(audio).copy(), np.asarray(starts).copy(), masks.copy()))
        return np.full((len(starts), 3, 256), 0.5, np.float32)

    def segment_embedding(self, audio):
        self.calls.append(("segment", np.asarray(audio).copy()))
        return None if len(audio) < 1680 else np.arange(256, dtype=np.float32)


class StubDiarizer:
    emb_sess = None
    emb_W = None
    emb_b = None


def test_feat_idx_is_the_reference_expression():
    for T, nseg in ((125, 589), (1, 589), (2, 589), (5, 589), (125, 293), (700, 589)):
        want = np.clip(np.floor(np.arange(T) * nseg / T).astype(int), 0, nseg - 1)
        assert np.array_equal(C1.feat_idx(T, nseg), want)
        assert np.array_equal(R.feat_idx(T, nseg), want)
        assert np.array_equal(want, np.minimum(np.arange(T) * nseg // T, nseg - 1))   # the kernel's integers
    assert C1.feat_idx(125, 589)[-1] == 584 and C1.feat_idx(2, 589).tolist() == [0, 294]


def test_min_seg_frames():
    assert C1.min_seg_frames_default() == 7 == R.MIN_SEG_FRAMES


def test_used_mask_rule_is_strictly_greater():
    full = np.zeros((3, 589, 3), np.float32)
    clean = np.zeros_like(full)
    full[:, :300, :] = 1.0
    clean[0, :7, 0] = 1.0        # exactly min_seg_frames: the full mask
    clean[0, :8, 1] = 1.0        # one more: the clean mask
    clean[1, :, 2] = 0.0         # nothing clean: the full mask
    m = C1.used_masks(full, clean, 7)
    assert m.shape == (3, 3, 589) and m.dtype == np.uint8
    assert m[0, 0].sum() == 300 and m[0, 1].sum() == 8 and m[1, 2].sum() == 300
    for c in range(3):
        for s in range(3):
            want = R.used_mask(full[c, :, s], clean[c, :, s], 7)
            assert np.array_equal(m[c, s], want.astype(np.uint8))
    with pytest.raises(ValueError):
        C1.used_masks(full, clean[:2], 7)


def test_extract_embeddings_hands_over_masks_and_starts():
    s = StubSession()
    full, clean = R.e2e_masks()
    audio = np.linspace(-1, 1, 1000).astype(np.float32)
    seen = []
    out = C1.extract_embeddings(s, audio, full, clean, 589, [0, 16000, 32000, 48000], 7,
                                lambda a, b: seen.append((a, b)))
    assert out.shape == (4, 3, 256) and out.dtype == np.float32 and seen == [(85, 100)]
    kind, a, starts, masks = s.calls[0]
    assert kind == "host" and np.array_equal(a, audio) and starts.tolist() == [0, 16000, 32000, 48000]
    assert np.array_equal(masks, C1.used_masks(full, clean, 7))
    with pytest.raises(ValueError):
        C1.extract_embeddings(s, audio, full, clean, 500, [0, 1, 2, 3], 7)
    with pytest.raises(ValueError):
        C1.extract_embeddings(s, audio, full, clean, 589, [0, 1, 2], 7)


def test_attach_rebinds_the_two_methods():
    d, s = StubDiarizer(), StubSession()
    W, b = np.ones((256, 5120), np.float32), np.zeros(256, np.float32)
    assert C1.attach(d, s, W, b) is d
    assert d.emb_sess is s and d.emb_W is W and d.emb_b is b
    full, clean = R.e2e_masks()
    out = d._extract_embeddings(np.zeros(100, np.float32), full, clean, 589, [0, 1, 2, 3], 7, None)
    assert out.shape == (4, 3, 256)
    assert d.compute_single_embedding(np.zeros(100, np.float32)) is None
    assert np.array_equal(d.compute_single_embedding(np.zeros(1680, np.float32)), np.arange(256, dtype=np.float32))
    d.emb_sess = None
    assert d.compute_single_embedding(np.zeros(1680, np.float32)) is None


def test_attach_reads_the_projection_from_the_model_dir(tmp_path):
    from zasr.resnet34 import ResNet34Config, save_model_dir, synth_weights
    cfg = ResNet34Config()
    w = synth_weights(cfg, 3)
    s = StubSession()
    s.model_dir = save_model_dir(str(tmp_path), cfg, w)
    d = C1.attach(StubDiarizer(), s)
    assert np.array_equal(d.emb_W, w["resnet.seg_1.weight"]) and np.array_equal(d.emb_b, w["resnet.seg_1.bias"])


class _NoDevice(EmbSession):
    """EmbSession's onnxruntime surface over a host encode."""

    def __init__(self):
        self.handle = None
        self.seen = []

    def encode(self, feats):
        x = np.asarray(feats, np.float32)
        self.seen.append(x.shape)
        return np.repeat(x.sum(axis=2)[:, None, :5], 2560, axis=1)


def test_io_binding_shim_follows_the_reference_call_sequence():
    s = _NoDevice()
    x = np.arange(2 * 40 * 80, dtype=np.float32).reshape(2, 40, 80)
    io = s.io_binding()                                   # :823
    name = s.get_outputs()[0].name                        # :824
    assert name == "/resnet/pool/Reshape_output_0"
    with pytest.raises(ZasrError):
        s.run_with_iobinding(io)                          # nothing bound yet
    io.bind_cpu_input("fbank_features", x)                # :842
    with pytest.raises(ZasrError):
        s.run_with_iobinding(io)                          # no output bound
    io.bind_output(name)                                  # :843
    s.run_with_iobinding(io)                              # :844
    out = io.get_outputs()[0].numpy()                     # :845
    assert out.shape == (2, 2560, 5) and np.array_equal(out, s.encode(x))
    assert np.array_equal(s.run(None, {"fbank_features": x})[0], out)
    io.bind_cpu_input("fbank_features", x[:1])            # the next batch rebinds the input
    io.bind_output(name)
    s.run_with_iobinding(io)
    assert io.get_outputs()[0].numpy().shape == (1, 2560, 5) and len(io.get_outputs()) == 1
