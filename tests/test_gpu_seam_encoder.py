"""The encoder's stack seams and layer starts through the tiny model (widths 64 / 96 / 128 / 96 /
64 / 64: a seam that zero-pads, ones that truncate, one that keeps the width; stack 2 has two
layers, so its second layer starts from the first one's output buffer), in every precision the
Recognizer accepts.

One ragged batch whose stack-0 lengths L = (T - 7) // 2 are {1, 2, 7, 8, 9, 17, 129}: shorter
than every downsampling factor, one below / at / one past the largest factor, an odd length
whose last output pair straddles the end, and one longer than a query tile.  Held: the batched
output equals each sequence encoded alone, bit for bit, and every output is within the mode's
tolerance of the oracle -- tests/test_gpu_attn_blockmap.py's 0.05 * max(1, |ref|) for the bf16
encoder and 2e-3 * max(1, |ref|) for the split modes, the latter also for fp32 (the bound
tests/test_gpu_e2e.py holds the fp32 encoder to).
"""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

LENS = [1, 2, 7, 8, 9, 17, 129]
TOL = {"bf16": 0.05, "bf16_enc": 0.05, "f16x3": 2e-3, "bf16x6": 2e-3, "bf16x3": 2e-3, "fp32": 2e-3}


@pytest.fixture(scope="module")
def batch():
    if not gpu_available():
        pytest.skip("no GPU")
    from model_fixtures import tiny_model
    from oracle.fbank import fbank
    from oracle.zipformer import ZipformerOracle
    from zasr.synth_audio import synth_speech
    cfg, w, path = tiny_model()
    assert tuple(cfg.encoder_dims) == (64, 96, 128, 96, 64, 64) and cfg.num_layers[2] == 2
    clip = fbank(synth_speech(4.0, 818))
    feats = []
    for i, L in enumerate(LENS):
        T = 2 * L + 7
        assert 13 * i + T <= clip.shape[0]
        feats.append(np.ascontiguousarray(clip[13 * i:13 * i + T]))
    orc = ZipformerOracle(cfg, w)
    refs = [orc.encoder(f) for f in feats]
    return path, feats, refs


def test_precisions_are_the_recognizers():
    from zasr.binding import PRECISIONS
    assert sorted(TOL) == sorted(PRECISIONS)


@pytest.mark.parametrize("precision", sorted(TOL))
def test_ragged_batch_through_the_seams(batch, precision):
    from zasr.binding import Recognizer
    path, feats, refs = batch
    rec = Recognizer(path, "greedy_search", 1, precision=precision)
    try:
        got = rec.encode_features(feats)
        alone = [rec.encode_features([f])[0] for f in feats]
    finally:
        rec.close()
    errs = []
    for L, g, a, ref in zip(LENS, got, alone, refs):
        assert g.shape == ref.shape == ((L + 1) // 2, ref.shape[1])
        np.testing.assert_array_equal(a, g)
        errs.append(float(np.max(np.abs(g - ref) / np.maximum(1.0, np.abs(ref)))))
    print(precision, "max scaled error per sequence:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= TOL[precision], errs
