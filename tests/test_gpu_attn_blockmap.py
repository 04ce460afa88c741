"""The flash attention kernels behind their block map (csrc/kernels.h build_attn_block_map):
one ragged batch with more sequences than XCD ranges, so the ranges' cuts fall inside a
sequence's heads, through the tiny model's encoder (heads 2,2,4,2,2,2) in bf16 (modes 1, 2, 3),
f16x3 (modes 1, 2, 3 on fp16 pieces) and bf16x6 (modes 0, 1, 2).

Stack 0 sees L = (T - 7) // 2 in {1, 31, 127, 128, 129, 255, 256, 257} (one key block mostly
masked, one query tile exactly, one frame into the second and the third tile), the deeper
stacks ceil(L / ds).  Held: the batched output equals each sequence encoded alone, bit for bit
(which block id serves a (sequence, head, tile) changes nothing it computes), and every output
is within the mode's tolerance of the oracle: 0.05 * max(1, |ref|) in bf16, 2e-3 * max(1, |ref|)
in f16x3 and bf16x6.
"""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

LENS = [1, 31, 127, 128, 129, 255, 256, 257] * 2 + [257, 1, 128]
TOL = {"bf16": 0.05, "f16x3": 2e-3, "bf16x6": 2e-3}
assert len(LENS) == 19


@pytest.fixture(scope="module")
def batch():
    """19 feature matrices (windows of one synthetic clip's fbank) and their oracle outputs."""
    if not gpu_available():
        pytest.skip("no GPU")
    from model_fixtures import tiny_model
    from oracle.fbank import fbank
    from oracle.zipformer import ZipformerOracle
    from zasr.synth_audio import synth_speech
    cfg, w, path = tiny_model()
    clip = fbank(synth_speech(8.0, 717))
    feats = []
    for i, L in enumerate(LENS):
        T = 2 * L + 7
        assert 11 * i + T <= clip.shape[0]
        feats.append(np.ascontiguousarray(clip[11 * i:11 * i + T]))
    orc = ZipformerOracle(cfg, w)
    refs = [orc.encoder(f) for f in feats]
    return path, feats, refs


def _scaled_err(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


@pytest.mark.parametrize("precision", sorted(TOL))
def test_ragged_batch_over_block_map(batch, precision):
    from zasr.binding import Recognizer
    path, feats, refs = batch
    rec = Recognizer(path, "greedy_search", 1, precision=precision)
    try:
        got = rec.encode_features(feats)
        alone = [rec.encode_features([f])[0] for f in feats]
    finally:
        rec.close()
    errs = []
    for g, a, ref in zip(got, alone, refs):
        assert g.shape == ref.shape
        np.testing.assert_array_equal(a, g)
        errs.append(_scaled_err(g, ref))
    print(precision, "max scaled error per sequence:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= TOL[precision], errs


@pytest.mark.parametrize("precision", sorted(TOL))
def test_single_sequence_grid_below_eight_ranges(batch, precision):
    """nseq = 1, L = 129: 2 query tiles x 2 heads, fewer blocks than ranges."""
    from zasr.binding import Recognizer
    path, feats, refs = batch
    k = LENS.index(129)
    rec = Recognizer(path, "greedy_search", 1, precision=precision)
    try:
        got = rec.encode_features([feats[k]])[0]
    finally:
        rec.close()
    assert got.shape == refs[k].shape
    err = _scaled_err(got, refs[k])
    print(precision, "scaled error:", f"{err:.2e}")
    assert err <= TOL[precision], err
