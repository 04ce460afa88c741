"""The float64 restatement of the Conv-TasNet separation network (tests/convtasnet_reference.py)
is the network zasr/convtasnet.py describes -- it agrees with torch's own modules run in
float64 -- the seeded weights keep both relu masks alive on the GPU tests' mixtures
(tests/sep_inputs.py), and the float32 deviation that sets the device tolerance is what
tests/test_gpu_sep.py records.  No GPU."""
import numpy as np
import torch

import sep_inputs as S
from convtasnet_reference import forward, forward_modules
from zasr.convtasnet import (ConvTasNetConfig, num_params, param_shapes, region_bytes,
                             region_flops, synth_weights)

F32_DEV = 1.0756e-6      # tests/test_gpu_sep.py


def test_restatement_is_the_module_network():
    cfg, w = S.network()
    for T in (32, 47, 2080, 6400):
        a = S.ref64(T)
        b = forward_modules(cfg, w, S.mixture(T), torch.float64)
        assert a.shape == b.shape == (2, T) and a.dtype == np.float64
        assert np.abs(a - b).max() < 1e-12 * max(1.0, np.abs(a).max())
        n = cfg.decoded_samples(T)
        assert np.all(a[:, n:] == 0.0) and np.all(b[:, n:] == 0.0)


def test_shapes_and_parameter_count():
    cfg = ConvTasNetConfig()
    assert [cfg.num_frames(T) for T in (31, 32, 47, 48, 2064, 2080, 6400, 48000)] == \
        [0, 1, 1, 2, 128, 129, 399, 2999]
    assert cfg.decoded_samples(47) == 32 and cfg.decoded_samples(48000) == 48000
    w = synth_weights(cfg, 3)
    assert {k: v.shape for k, v in w.items()} == dict(param_shapes(cfg))
    assert all(v.dtype == np.float32 for v in w.values())
    # 24 blocks x (128 x 512 + 512 + 1 + 1024 + 512 x 3 + 512 + 1 + 1024 + 2 x (512 x 128 + 128))
    assert num_params(cfg) == 2 * 512 * 32 + 1024 + 512 * 128 + 128 + 24 * 201474 + 1 \
        + 1024 * 128 + 1024
    fl = region_flops(cfg, 16000)
    assert fl["gemms"] > 20 * fl["norms_depthwise"] > 0 and region_bytes(cfg, 16000) > 0
    assert ConvTasNetConfig.from_json(cfg.to_json()) == cfg


def test_both_masks_are_alive_on_the_gpu_test_inputs():
    """A dead relu mask would zero a stream and make every relative tolerance vacuous: on each
    mixture both masks are open on 30-70 % of their entries, change from frame to frame, and
    both streams carry signal that is not a copy of the other."""
    cfg, w = S.network()
    for T in (32, 2080, 16000):
        out, mask = forward(cfg, w, S.mixture(T), return_masks=True)
        for s in range(2):
            share = float((mask[s] > 0).mean())
            assert 0.3 < share < 0.7, (T, s, share)
            assert np.abs(out[s]).max() > 0.1 * np.abs(S.mixture(T)).max()
            if T > 32:
                flips = float(((mask[s][:, 1:] > 0) != (mask[s][:, :-1] > 0)).mean())
                assert flips > 0.01, (T, s, flips)
        if T > 32:
            assert abs(np.corrcoef(out[0], out[1])[0, 1]) < 0.9


def test_float32_deviation_sets_the_device_bound():
    """torch float32 on the CPU (F.conv1d / F.prelu / F.conv_transpose1d) vs the float64
    restatement on exactly the GPU cases (the six single regions and the ragged batch's
    lengths), per stream, relative to the stream's float64 peak: the recorded deviation holds
    (to the 10 % another BLAS build may move it)."""
    worst = 0.0
    for T in S.ALL_LENGTHS:
        d = S.peak_dev(S.ref_f32(T), S.ref64(T))
        print(f"T = {T}: float32 deviation {d:.4e}")
        worst = max(worst, d)
    print(f"float32 deviation {worst:.4e}")
    assert worst <= 1.1 * F32_DEV
