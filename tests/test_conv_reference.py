"""The float64 references of tests/conv_reference.py against torch and the oracle, and the code
paths the GPU test's ragged fixtures meet (tests/test_gpu_conv_kernels.py), from the lengths
and the kernels' tile constants alone.  No GPU.

Each reference is compared sequence by sequence with torch.nn.functional.conv1d / conv2d
(groups = channels, float64, a batch of one: torch pads that sequence alone) and with
oracle.zipformer's swoosh_r / swoosh_l / bias_norm in float64, to 1e-12 of the sequence's
largest magnitude.
"""
import numpy as np
import pytest
import torch

import conv_reference as cr
from oracle.zipformer import bias_norm, swoosh_l, swoosh_r

F = torch.nn.functional
TOL = 1e-12


def close(got, want):
    want = want.detach().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64 and want.dtype == np.float64
    assert np.max(np.abs(got - want)) <= TOL * max(1.0, np.max(np.abs(want)))


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def sequences(L):
    off = cr.offsets(L)
    return [(int(off[s]), int(off[s + 1])) for s in range(len(L))]


# ---------------- the references ----------------
@pytest.mark.parametrize("K", cr.DW1_KERNEL_SIZES)
@pytest.mark.parametrize("L", cr.DW1_LENGTHS, ids=lambda L: f"nseq{len(L)}_rows{sum(L)}")
def test_conv_module_core_matches_torch(L, K):
    rng = np.random.default_rng(100 + K + sum(L))
    d = 36
    x2 = rng.standard_normal((sum(L), 2 * d)) * 2
    w = rng.standard_normal((d, K)) / np.sqrt(K)
    b = rng.standard_normal(d) * 0.5
    got = cr.conv_module_core(x2, L, w, b, True)
    got_post = cr.conv_module_core(cr.glu(x2), L, w, b, False)
    for lo, hi in sequences(L):
        a, s = t64(x2[lo:hi, :d]), t64(x2[lo:hi, d:])
        g = (a * torch.sigmoid(s)).t().unsqueeze(0)  # (1, d, T)
        y = F.conv1d(g, t64(w).unsqueeze(1), t64(b), padding=K // 2, groups=d)
        want = swoosh_r(y[0].t())
        close(got[lo:hi], want)
        close(got_post[lo:hi], want)


def test_conv0_matches_torch():
    T = cr.CONV1_FRAMES
    rng = np.random.default_rng(7)
    fb = rng.standard_normal((sum(T), 80)) * 3
    w = rng.standard_normal((8, 9)) / 3
    b = rng.standard_normal(8) * 0.5
    got = cr.swoosh_r(cr.conv0(fb, T, w, b))
    assert got.shape == (sum(t - 2 for t in T), 80, 8)
    lo2 = 0
    for (lo, hi), t in zip(sequences(T), T):
        y = F.conv2d(t64(fb[lo:hi]).unsqueeze(0).unsqueeze(0), t64(w).reshape(8, 1, 3, 3), t64(b),
                     padding=(0, 1))  # (1, 8, T - 2, 80)
        close(got[lo2:lo2 + t - 2], swoosh_r(y[0].permute(1, 2, 0)))
        lo2 += t - 2


@pytest.mark.parametrize("L", cr.CNX_LENGTHS, ids=lambda L: f"nseq{len(L)}_rows{sum(L)}")
def test_convnext_matches_torch(L):
    rng = np.random.default_rng(11 + sum(L))
    x = rng.standard_normal((sum(L), 19, 128))
    dw_w = rng.standard_normal((128, 7, 7)) / 7
    dw_b = rng.standard_normal(128) * 0.3
    w1 = rng.standard_normal((384, 128)) * 2 / np.sqrt(128)
    b1 = rng.standard_normal(384) * 0.5
    w2 = rng.standard_normal((128, 384)) / np.sqrt(384)
    b2 = rng.standard_normal(128) * 0.1
    y = cr.dwconv7x7(x, L, dw_w, dw_b)
    out = x + cr.convnext_mlp(y, w1, b1, w2, b2)
    for lo, hi in sequences(L):
        xt = t64(x[lo:hi]).permute(2, 0, 1).unsqueeze(0)  # (1, 128, T, 19)
        yt = F.conv2d(xt, t64(dw_w).unsqueeze(1), t64(dw_b), padding=(3, 3), groups=128)
        close(y[lo:hi], yt[0].permute(1, 2, 0))
        h = swoosh_l(F.conv2d(yt, t64(w1).reshape(384, 128, 1, 1), t64(b1)))
        ot = xt + F.conv2d(h, t64(w2).reshape(128, 384, 1, 1), t64(b2))
        close(out[lo:hi], ot[0].permute(1, 2, 0))


@pytest.mark.parametrize("d", cr.BN_WIDTHS)
def test_bias_norm_matches_oracle(d):
    rng = np.random.default_rng(300 + d)
    x = rng.standard_normal((9, d)) * 1.5
    bias = rng.standard_normal(d) * 0.3
    orig = rng.standard_normal((9, d))
    s = rng.uniform(0.3, 0.9, d)
    want = bias_norm(t64(x), t64(bias), torch.tensor(0.3, dtype=torch.float64))
    got, r = cr.bias_norm(x, bias, 0.3)
    close(got, want)
    close(r, want)
    got, r = cr.bias_norm(x, bias, 0.3, orig, s)
    close(r, want)
    close(got, t64(orig) + (want - t64(orig)) * t64(s))


def test_activations_match_oracle():
    v = np.linspace(-16.0, 16.0, 2401)  # (torch's softplus is the identity above 20)
    close(cr.swoosh_r(v), swoosh_r(t64(v)))
    close(cr.swoosh_l(v), swoosh_l(t64(v)))
    close(cr.sigmoid(v), torch.sigmoid(t64(v)))


# ---------------- what the GPU fixtures meet ----------------
def test_dwconv1d_fixture_meets_both_block_paths_of_every_instantiation():
    L = cr.DW1_LENGTHS[0]
    off = cr.offsets(L).tolist()
    assert off[-1] == 492 and off[1:-1] == [1, 8, 64, 67, 267, 331, 362]
    assert off[-1] % cr.DW1_TILE_ROWS == 44  # a row tail: 492 = 7 * 64 + 44
    # a one-frame sequence, a boundary on a tile edge, and one inside the next tile's first rows,
    # so within the halo of the tile before it at every compiled K
    assert 1 in L and any(b % cr.DW1_TILE_ROWS == 0 for b in off[1:-1])
    assert any(0 < b % cr.DW1_TILE_ROWS <= 3 for b in off[1:-1])
    for K in cr.DW1_COMPILED_K:
        m = cr.masked_tiles(L, cr.DW1_TILE_ROWS, K // 2)
        assert len(m) == 8 and m.any() and not m.all(), (K, m)
        assert any(l < K // 2 for l in L)  # a sequence shorter than the half-window
    # K = 31: rows 128-191 and 384-447 lie inside the sequences of 200 and 130 frames (the
    # unmasked fast path); every other tile is masked
    assert cr.masked_tiles(L, cr.DW1_TILE_ROWS, 15).tolist() == \
        [True, True, False, True, True, True, False, True]
    for L1 in cr.DW1_LENGTHS[1:]:  # a batch that is one short sequence: one masked tile
        assert all(cr.masked_tiles(L1, cr.DW1_TILE_ROWS, K // 2).tolist() == [True]
                   for K in cr.DW1_COMPILED_K)


def test_dwconv1d_fixture_meets_every_instantiation_exact_and_padded():
    by_k = {}
    for kr in cr.DW1_KERNEL_SIZES:
        by_k.setdefault(cr.compiled_k(kr), []).append(kr)
    assert by_k == {7: [5, 7], 15: [9, 15], 31: [17, 31]}
    # channel blocks: one partial block, one exact block, a full block and a 32-channel tail
    blocks = {d: [min(cr.DW1_TILE_CH, d - c) for c in range(0, d, cr.DW1_TILE_CH)]
              for d in cr.DW1_WIDTHS}
    assert blocks == {36: [36], 64: [64], 96: [64, 32]}
    assert all(d % 4 == 0 for d in cr.DW1_WIDTHS)


def test_conv1_fixture_shifts_every_sequence_and_leaves_a_block_tail():
    T = cr.CONV1_FRAMES
    rows = sum(t - 2 for t in T)
    assert rows == 51 and min(T) == 3  # a sequence with one output frame
    # the two levels' offsets differ by 2 per sequence: every sequence but the first maps rows
    assert (cr.offsets(T) - cr.offsets([t - 2 for t in T])).tolist() == [0, 2, 4, 6, 8, 10]
    assert rows * 80 > cr.CONV1_BLOCK and (rows * 80) % cr.CONV1_BLOCK != 0


def test_convnext_fixture_meets_both_block_paths_and_the_mlp_tail():
    L = cr.CNX_LENGTHS[0]
    rows = sum(L)
    assert rows == 102 and rows % cr.CNX_TILE_ROWS == 6
    m = cr.masked_tiles(L, cr.CNX_TILE_ROWS, cr.CNX_HALF)
    # tiles 32-47 and 80-95 lie inside the sequences of 40 and 33 frames: the unmasked path
    assert m.tolist() == [True, True, False, True, True, False, True]
    npos = rows * 19
    assert npos == 1938 == 15 * cr.MLP_TILE_POS + 18
    assert cr.CNX_LENGTHS[1] == [1] and 19 < cr.MLP_TILE_POS  # one partial MLP block
    assert cr.masked_tiles([1], cr.CNX_TILE_ROWS, cr.CNX_HALF).tolist() == [True]


def test_bias_norm_fixture_crosses_every_instantiation():
    by_nq = {}
    for d in cr.BN_WIDTHS:
        assert d % 4 == 0
        by_nq.setdefault(cr.bias_norm_nq(d), []).append(d)
    assert by_nq == {1: [4, 64, 192, 256], 2: [260, 384, 512], 4: [516, 1024]}
    for nq, ds in by_nq.items():
        lanes = [d // 4 for d in ds]
        assert max(lanes) == 64 * nq          # every lane's every load is live
        assert min(lanes) % 64 != 0 or min(lanes) < 64 * nq  # rows with idle lanes
        assert any(l % 64 != 0 for l in lanes)
    # one wave per row, four per block: a partial block, a full one, and a second block
    per = cr.BIAS_NORM_ROWS
    assert {r % per == 0 for r in cr.BN_ROWS} == {True, False}
    assert min(cr.BN_ROWS) < per < max(cr.BN_ROWS) and max(cr.BN_ROWS) > 2 * per
