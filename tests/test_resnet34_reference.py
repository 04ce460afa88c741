"""The float64 restatements of tests/resnet34_reference.py, pinned on the CPU: to torch float64 on
the unfolded weights (the BatchNorm fold and the layout), to the reference's own
_masked_stats_pool (tests/golden/community1_pool_cases.json), the float32 deviations the GPU
tests take as bounds, and a single-defect sweep: every defect below, injected into the
restatement, moves its output past the bound the GPU tests allow, on the GPU tests' inputs."""
import hashlib
import json
import os

import numpy as np
import pytest

import resnet34_reference as R
from zasr import resnet34 as M

f64 = np.float64


@pytest.fixture(scope="module")
def net():
    return R.network()


@pytest.fixture(scope="module")
def model_runs(net):
    """{T: (float64 restatement, torch float32)} on the whole-model inputs."""
    cfg, _w, fold = net
    return {T: (R.forward(cfg, fold, R.model_feats(T)),
                R.torch_forward(cfg, fold, R.model_feats(T), np.float32)) for T in R.MODEL_T}


@pytest.fixture(scope="module")
def e2e(net):
    """The 12.3 s signal's fbank image, masks, and float64 / float32 embeddings."""
    cfg, w, fold = net
    image = R.fbank(R.speech(R.E2E_SEC, R.E2E_SEED), R.TAIL)
    full, clean = R.e2e_masks()
    r64 = R.chunk_embeddings(cfg, w, fold, image, R.E2E_STARTS, full, clean)
    r32 = R.chunk_embeddings(cfg, w, fold, image, R.E2E_STARTS, full, clean, dtype=np.float32)
    return image, full, clean, r64, r32


def test_config_shapes_and_flops():
    cfg = M.ResNet34Config()
    assert cfg.num_feat_frames(998) == 125 and cfg.out_bins == 10 and cfg.feat_width == 2560
    assert [M.ResNet34Config.down(998, k) for k in (1, 2, 3)] == [499, 250, 125]
    assert M.ResNet34Config.from_json(cfg.to_json()) == cfg
    shapes = M.param_shapes(cfg)
    assert shapes["resnet.seg_1.weight"] == (256, 5120)
    assert shapes["resnet.layer2.0.shortcut.0.weight"] == (64, 32, 1, 1)
    assert "resnet.layer1.0.shortcut.0.weight" not in shapes
    assert sum(1 for k in shapes if k.endswith("conv1.weight") and "layer" in k) == 16
    fl = M.encoder_flops(cfg, 998)
    print(f"encoder flops per 10 s chunk: {fl / 1e9:.2f} GFLOP; per hour (3591 chunks): {3591 * fl / 1e12:.1f} TFLOP")
    assert 20e9 < fl < 60e9


def test_restatement_equals_torch_float64_on_the_unfolded_weights(net):
    """The fold in float64 (no rounding) + the channels-last im2col restatement == F.conv2d +
    batch_norm(eval) on the raw weights, to 1e-12 of the peak; the float32 fold is that
    tensor rounded once."""
    cfg, w, fold = net
    fold64 = M.folded_weights(cfg, w, np.float64)
    for T in R.MODEL_T:
        x = R.model_feats(T)
        ref = R.torch_forward_unfolded(cfg, w, x)
        got = R.forward(cfg, fold64, x)
        assert got.shape == ref.shape == (2, 2560, cfg.num_feat_frames(T))
        assert R.peak_dev(got, ref) <= 1e-12
        assert R.peak_dev(R.torch_forward(cfg, fold64, x.astype(f64), f64), ref) <= 1e-12
    for k, (wf, bf) in fold.items():
        assert wf.dtype == np.float32 and np.array_equal(wf, fold64[k][0].astype(np.float32))
        assert np.array_equal(bf, fold64[k][1].astype(np.float32))


def test_frame_features_have_unit_scale(model_runs):
    for T, (r64, _r32) in model_runs.items():
        rms = float(np.sqrt(np.mean(r64 ** 2)))
        print(f"T = {T}: frame feature rms {rms:.3f}, peak {np.abs(r64).max():.2f}")
        assert 0.1 <= rms <= 10.0
        assert (r64 > 0).mean() > 0.2        # the ReLU stream is alive


def test_float32_deviation_is_the_named_constant(model_runs, e2e):
    devs = []
    for T, (r64, r32) in model_runs.items():
        devs.append(R.peak_dev(r32, r64))
        ma, rl = R.acceptance(r32, r64)
        print(f"T = {T}: torch float32 vs float64 / peak = {devs[-1]:.3e}; max_abs {ma:.3e}, rel_l2 {rl:.3e}")
        assert R.F32_DEV[T] * 0.5 <= devs[-1] <= R.F32_DEV[T] * 1.02
    _image, _f, _c, r64, r32 = e2e
    d = R.peak_dev(r32, r64)
    print(f"embeddings, 4 chunks: float32 vs float64 / peak = {d:.3e}")
    assert d <= R.F32_DEV_EMB * 1.02 and d >= R.F32_DEV_EMB * 0.5


def test_segment_float32_deviation_is_the_named_constant(net):
    cfg, w, fold = net
    assert set(R.F32_DEV_SEG) == {9, 250}
    for frames in sorted(R.F32_DEV_SEG):
        rows = R.fbank(R.segment_audio(frames)).astype(np.float32)
        assert rows.shape == (frames, 80)
        d = R.peak_dev(R.segment_embedding(cfg, w, fold, rows, np.float32),
                       R.segment_embedding(cfg, w, fold, rows))
        print(f"segment of {frames} frames: float32 vs float64 / peak = {d:.3e}")
        assert R.F32_DEV_SEG[frames] * 0.5 <= d <= R.F32_DEV_SEG[frames] * 1.02


def test_fbank_tolerance_propagated_to_the_embeddings(net, e2e):
    cfg, w, fold = net
    image, full, clean, r64, _r32 = e2e
    moved = R.chunk_embeddings(cfg, w, fold, R.perturbed_image(image), R.E2E_STARTS, full, clean)
    d = R.peak_dev(moved, r64)
    print(f"fbank image moved within +-{R.FBANK_ATOL}: embeddings move by {d:.3e} of the peak")
    assert R.FBANK_PROP * 0.5 <= d <= R.FBANK_PROP * 1.02


def test_pooling_equals_the_reference_method(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "community1_pool_cases.json")))
    block = R.pool_block(16)
    assert list(block.shape) == g["block_shape"]
    assert hashlib.sha256(block.tobytes()).hexdigest() == g["block_sha256"]
    assert g["min_seg_frames"] == R.MIN_SEG_FRAMES == 7
    idx = R.feat_idx(125, R.NSEG)
    assert set(g["cases"]) == set(R.POOL_MASKS)
    for name, (full, clean) in R.pool_masks().items():
        weights = R.used_mask(full, clean, R.MIN_SEG_FRAMES)[idx].astype(np.float32)
        assert np.flatnonzero(weights).tolist() == g["cases"][name]["weights_on"], name
        ref = np.array(g["cases"][name]["stats"], np.float32)
        got32 = R.masked_pool(block, weights, np.float32)
        assert got32.dtype == np.float32
        assert np.max(np.abs(got32.astype(f64) - ref)) <= 16 * R.U * max(1.0, np.abs(ref).max()), name
        r64, bound, dev = R.pool_bound(block, weights)
        assert np.max(np.abs(r64 - ref)) <= bound, (name, dev)
        assert not np.any(np.isnan(ref))
    z = g["cases"]["all_zero"]["stats"]
    assert z == [0.0] * 32
    # the named masks reach the weights: one and two active encoder frames, not none
    one, two = g["cases"]["one_frame"], g["cases"]["two_frames"]
    assert len(one["weights_on"]) == 1 and len(two["weights_on"]) == 2
    assert one["stats"][:16] == [float(v) for v in block[:, one["weights_on"][0]]]   # the mean is the frame
    assert one["stats"][16:] == [0.0] * 16 and any(v > 0 for v in two["stats"][16:])
    # the switch case used the FULL mask: its clean mask has exactly min_seg_frames frames
    assert g["cases"]["clean_switch"]["weights_on"] == g["cases"]["alternating"]["weights_on"]


def test_single_embedding_pooling_is_the_population_form():
    x = R.pool_block(16, 7)
    got = R.pop_pool(x)
    assert np.allclose(got[:16], x.astype(f64).mean(axis=1)) and np.allclose(got[16:], x.astype(f64).std(axis=1))


# ---- the single-defect sweep ------------------------------------------------------------------
CONV_DEFECTS = {
    "pad_missing_edge": "A", "stride_one_axis": "B", "neighbour_across_sample": "A",
    "rq_swapped": "A", "res_after_relu": "D", "bias_dropped_with_res": "D",
}


@pytest.mark.parametrize("defect,case", sorted(CONV_DEFECTS.items()))
def test_conv_defect_is_caught(defect, case):
    c = next(k for k in R.CONV_CASES if k.name == case)
    ref, bound = R.conv_case_ref(c)
    bad, _ = R.conv_case_ref(c, defect)
    ratio = float(np.max(np.abs(bad - ref) / bound))
    print(f"{defect} on case {case}: worst |defect - reference| / bound = {ratio:.3g}")
    assert ratio > 1.0
    assert ref.shape == ((c.n, (c.F - 1) // c.stride + 1, (c.T - 1) // c.stride + 1, c.co))


def test_every_conv_case_defect_pair_is_listed():
    assert {c.name for c in R.CONV_CASES} == set("ABCDEF")
    # strided cases catch the one-axis stride, 3x3 cases the swapped taps
    for c in R.CONV_CASES:
        ref, bound = R.conv_case_ref(c)
        if c.stride == 2:
            assert np.max(np.abs(R.conv_case_ref(c, "stride_one_axis")[0] - ref) / bound) > 1.0, c.name
        if c.ks == 3:
            assert np.max(np.abs(R.conv_case_ref(c, "rq_swapped")[0] - ref) / bound) > 1.0, c.name
            assert np.max(np.abs(R.conv_case_ref(c, "pad_missing_edge")[0] - ref) / bound) > 1.0, c.name


def test_channel_order_defect_is_caught(net, model_runs):
    cfg, _w, fold = net
    for T, (r64, _r32) in model_runs.items():
        bad = R.forward(cfg, fold, R.model_feats(T), "f_major_channels")
        assert bad.shape == r64.shape
        assert R.peak_dev(bad, r64) > R.BOUND[T]


@pytest.mark.parametrize("defect", ["feat_idx_round", "population_variance"])
def test_pool_defect_is_caught(defect):
    block = R.pool_block(2560)
    caught = []
    for name, (full, clean) in R.pool_masks().items():
        um = R.used_mask(full, clean, R.MIN_SEG_FRAMES)
        w = um[R.feat_idx(125, R.NSEG)].astype(np.float32)
        r64, bound, _ = R.pool_bound(block, w)
        if defect == "feat_idx_round":
            bad = R.masked_pool(block, um[R.feat_idx(125, R.NSEG, defect)].astype(np.float32))
        else:
            bad = R.masked_pool(block, w, f64, defect)
        if np.max(np.abs(bad - r64)) > bound:
            caught.append(name)
    print(defect, "caught by", caught)
    assert caught


def test_clean_rule_defect_is_caught():
    full, clean = R.pool_masks()["clean_switch"]
    assert clean.sum() == R.MIN_SEG_FRAMES
    block = R.pool_block(2560)
    idx = R.feat_idx(125, R.NSEG)
    w = R.used_mask(full, clean, R.MIN_SEG_FRAMES)[idx]
    wb = R.used_mask(full, clean, R.MIN_SEG_FRAMES, "clean_rule_ge")[idx]
    assert np.array_equal(w, full[idx]) and np.array_equal(wb, clean[idx])
    r64, bound, _ = R.pool_bound(block, w)
    assert np.max(np.abs(R.masked_pool(block, wb) - r64)) > bound


def test_fbank_option_set(e2e):
    image = e2e[0]
    n = int(R.E2E_SEC * 16000)
    assert image.shape == (1 + (n + 160000 - 400) // 160, 80)
    # rows wholly inside the zero tail are exactly log(FLT_EPSILON)
    first_zero = -(-n // 160)
    assert np.all(image[first_zero:] == np.log(R.FLT_EPSILON))
    for ns in (400, 401, 560, 16000):
        assert R.fbank(R.speech(1.0, 5)[:ns], R.TAIL).shape[0] == R.fbank_rows(ns, R.TAIL)
    assert R.fbank(np.zeros(399, np.float32)).shape == (0, 80)


@pytest.mark.parametrize("defect", ["povey_window", "zero_tail_omitted"])
def test_fbank_defect_is_caught(defect):
    a = R.speech(1.0, 5)[:16000]
    ref = R.fbank(a, R.TAIL)
    bad = R.fbank(a, R.TAIL, defect)
    if defect == "zero_tail_omitted":
        assert bad.shape[0] < ref.shape[0]      # the rows the last chunks need are missing
    else:
        assert np.max(np.abs(bad - ref)) > R.FBANK_ATOL


@pytest.mark.parametrize("defect", ["zero_tail_omitted", "cmvn_valid_rows_only", "feat_idx_round",
                                    "population_variance", "clean_rule_ge"])
def test_end_to_end_defect_is_caught(net, e2e, defect):
    cfg, w, fold = net
    image, full, clean, r64, _r32 = e2e
    img = R.fbank(R.speech(R.E2E_SEC, R.E2E_SEED), R.TAIL, defect) if defect == "zero_tail_omitted" else image
    bad = R.chunk_embeddings(cfg, w, fold, img, R.E2E_STARTS, full, clean, defect=defect,
                             signal_rows=R.fbank_rows(int(R.E2E_SEC * 16000)))
    d = R.peak_dev(bad, r64)
    print(f"{defect}: end-to-end deviation / peak = {d:.3e} (bound {R.BOUND_EMB:.3e})")
    assert d > R.BOUND_EMB
    assert not np.any(np.isnan(r64))
    assert np.array_equal(r64[1, 2], w["resnet.seg_1.bias"].astype(f64))     # the all-zero speaker
