"""The float64 restatement of the PyanNet segmentation network (tests/pyannet_reference.py) is
the network zasr/pyannet.py describes -- it agrees with torch's own modules run in float64 --
and the seeded weights and inputs of the GPU tests (tests/seg_inputs.py) exercise the decode:
every class occurs, and the float32 deviation that sets the device tolerance is what
tests/test_gpu_seg.py records.  No GPU."""
import numpy as np
import torch

import seg_inputs as S
from pyannet_reference import forward, forward_modules
from zasr.pyannet import PyanNetConfig, num_params, param_shapes, synth_weights

F32_DEV = 1.2623e-4      # tests/test_gpu_seg.py
BOUND = 8 * F32_DEV


def test_restatement_is_the_module_network():
    cfg, w = S.network()
    for n, T in ((3, 1531), (2, 6000)):
        x = S.case_batch(n, T)
        a, b = forward(w, x), forward_modules(w, x, torch.float64)
        assert a.shape == b.shape == (n, cfg.num_frames(T), 7)
        assert np.abs(a - b).max() < 1e-10
        assert np.allclose(np.exp(a).sum(-1), 1.0, atol=1e-12)


def test_parameter_count():
    """1,493,265 parameters with the sinc bank stored as 80 x 251 weights; with pyannote's
    parametrised bank instead (40 low cut-offs + 40 bandwidths) 1,473,265, i.e. 5,893,060 B in
    float32 against the 5,916,375 B file the reference's manifest lists."""
    cfg = PyanNetConfig()
    assert num_params(cfg) == 1493265
    assert num_params(cfg) - cfg.sinc_filters * cfg.sinc_taps + 80 == 1473265
    w = synth_weights(cfg, 3)
    assert {k: v.shape for k, v in w.items()} == dict(param_shapes(cfg))
    assert all(v.dtype == np.float32 for v in w.values())


def test_every_class_occurs_on_the_gpu_test_inputs():
    counts = np.zeros(7)
    for n, T in S.LOGIT_CASES:
        counts += np.bincount(S.case_ref64(n, T).argmax(-1).ravel(), minlength=7)
    share = counts / counts.sum()
    print("class shares", np.round(share, 4))
    assert share.min() >= 0.01


def test_float32_deviation_sets_the_device_bound():
    """torch float32 on the CPU vs the float64 restatement on exactly the GPU logits cases: the
    recorded deviation holds (to the 10 % another BLAS build may move it), the frames the bound
    cannot decide are under 1 %, and float32 itself flips no class outside them."""
    worst, frames, excluded = 0.0, 0, 0
    for n, T in S.LOGIT_CASES:
        r64, r32 = S.case_ref64(n, T), S.case_f32(n, T)
        worst = max(worst, float(np.abs(r32 - r64).max()))
        sure = S.top2_margin(r64) > 2 * BOUND
        assert np.array_equal(r32.argmax(-1)[sure], r64.argmax(-1)[sure])
        frames += sure.size
        excluded += int((~sure).sum())
    print(f"float32 deviation {worst:.4e}; excluded {excluded} of {frames} frames")
    assert worst <= 1.1 * F32_DEV
    assert excluded <= 0.01 * frames
