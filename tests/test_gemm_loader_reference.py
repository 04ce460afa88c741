"""tests/gemm_loader_reference.py held to torch, its emulations to its bound, and the GPU test's
fixture shown to see each single defect of a loader.  No GPU.

The references: conv.4 / conv.7 against torch.nn.functional.conv2d and the im2col1d reference
against conv1d, float64, sequence by sequence (window by window) on the ragged fixtures, to 1e-12
of the largest magnitude.  torch's weight is [N][C][kt][kf]; the kernels' k order is tap-major,
channel-minor, W[n][(kt * 3 + kf) * C + c] = Wt[n][c][kt][kf], i.e. Wt.permute(0, 2, 3, 1)
flattened -- stated here once (torch_weight below), the reference module only reshapes.

The emulation (the loaders' index arithmetic transcribed from the kernels, f32 products, each
mode's operand rounding) stays within the bound on every case of tests/test_gpu_gemm_loaders.py.
With one defect switched on it must leave the bound, lose an output row, or touch bytes it should
not, on at least one case of that fixture.
"""
import numpy as np
import pytest
import torch

import gemm_loader_reference as gr

F = torch.nn.functional
TOL = 1e-12


def close(got, want):
    want = want.detach().numpy()
    assert got.shape == want.shape and got.dtype == np.float64 and want.dtype == np.float64
    assert np.max(np.abs(got - want)) <= TOL * max(1.0, np.max(np.abs(want)))


def torch_weight(W, C):
    """The kernels' [N][(kt * 3 + kf) * C + c] -> torch's [N][C][kt][kf]."""
    return torch.from_numpy(np.asarray(W, np.float64).reshape(W.shape[0], 3, 3, C)).permute(0, 3, 1, 2)


# ---------------- the references against torch ----------------
@pytest.mark.parametrize("which", [4, 7])
@pytest.mark.parametrize("T", [gr.EDGE_T] + list(gr.SINGLE_T), ids=lambda T: "T" + "-".join(map(str, T)))
def test_conv_reference_matches_torch(which, T):
    g = gr.CONV_GEOM[which]
    o = gr.conv_operands(which, T)
    v, S = gr._conv_pre(which, T, False)
    Wt, b = torch_weight(o["W"], g["cin"]), torch.from_numpy(o["bias"].astype(np.float64))
    rin, rout = gr.conv_lengths(which, T)
    io, oo = np.concatenate([[0], np.cumsum(rin)]), np.concatenate([[0], np.cumsum(rout)])
    for q in range(len(T)):
        x = torch.from_numpy(o["A"][io[q]:io[q + 1]].astype(np.float64)).permute(2, 0, 1).unsqueeze(0)
        y = F.conv2d(x, Wt, b, stride=(g["st"], 2))[0].permute(1, 2, 0)  # [t][f][N]
        assert y.shape[0] == rout[q] and y.shape[1] == g["fout"]
        close(v[oo[q]:oo[q + 1]], y)
        ys = F.conv2d(x.abs(), Wt.abs(), b.abs(), stride=(g["st"], 2))[0].permute(1, 2, 0)
        close(S[oo[q]:oo[q + 1]], ys)
    # the activation: icefall's SwooshR
    z = torch.from_numpy(v.copy())
    close(gr.swoosh_r(v), torch.logaddexp(torch.zeros_like(z), z - 1.0) - 0.08 * z - 0.313261687)


@pytest.mark.parametrize("c", gr.ALOAD_GROUPS["tdnn"] + gr.ALOAD_GROUPS["local"], ids=lambda c: c.name)
def test_im2col1d_reference_matches_torch(c):
    o = gr.aload_operands(c)
    Tin, Tout, C, stride, dil, pad = c.i2c
    taps = c.K // C
    ref, _ = gr.aload_reference(c._replace(epi="NONE"), o)
    Wt = torch.from_numpy(o["W"].astype(np.float64).reshape(c.N, taps, C)).permute(0, 2, 1)  # [N][C][taps]
    b = torch.from_numpy(o["bias"].astype(np.float64))
    for n in range(c.M // Tout):
        x = torch.from_numpy(o["A"][n * Tin:(n + 1) * Tin, :C].astype(np.float64)).t().unsqueeze(0)
        y = F.conv1d(x, Wt, b, stride=stride, padding=pad, dilation=dil)[0].t()
        assert y.shape[0] == Tout
        close(ref[n * Tout:(n + 1) * Tout], y)


def test_bnrelu_reference_is_the_plain_formula():
    c = next(c for c in gr.ALOAD_GROUPS["bnrelu"] if c.K == 36 and c.M == 65 and c.epi == "NONE")
    o = gr.aload_operands(c)
    ref, _ = gr.aload_reference(c, o)
    a = torch.from_numpy(o["A"][:, :c.K].astype(np.float64))
    ap = torch.relu(a * torch.from_numpy(o["scale"].astype(np.float64)) + torch.from_numpy(o["shift"].astype(np.float64)))
    close(ref, F.linear(ap, torch.from_numpy(o["W"].astype(np.float64)), torch.from_numpy(o["bias"].astype(np.float64))))
    cut = float((ap == 0).double().mean())
    assert 0.35 < cut < 0.65, cut  # the loader's ReLU is live: a s + b is symmetric, about half is cut


# ---------------- the fixture's facts ----------------
def test_fixture_shapes_and_tiles():
    assert gr.conv_rows(7, gr.EDGE_T) == [19, 19, 133, 266, 38, 133]
    assert gr.conv_rows(4, gr.EDGE_T) == [117, 117, 351, 624, 156, 351]
    # the edge batch and both single sequences take the 64-row tile: tiles are per slice, so a
    # sequence alone computes its rows exactly as inside the batch
    for w in (4, 7):
        for T in (gr.EDGE_T,) + gr.SINGLE_T:
            assert gr.conv_tile(w, T) == (32 if w == 4 else 128, False)
        # the dispatch batch is the shortest of 8 equal sequences on the 128-row tile
        T = gr.dispatch_T(w)
        assert gr.conv_tile(w, T)[1] and not gr.conv_tile(w, (T[0] - 1,) * 8)[1]
        assert -(-gr.conv_rows(w, T)[0] // 128) == 64
    assert gr.dispatch_T(7) == (857,) * 8 and gr.dispatch_T(4) == (417,) * 8
    assert len(gr.EDGE_CASES) == 13 * 3 and len(gr.DISPATCH_CASES) == 12
    # local convolution: rows of two windows share a 64-row tile; dilation 2 at T2 <= 2 pads
    # every neighbour tap
    assert any(c.M > c.i2c[1] and c.i2c[1] % 64 for c in gr.ALOAD_GROUPS["local"])


# ---------------- the emulation within the bound ----------------
@pytest.mark.parametrize("c", gr.EDGE_CASES + gr.DISPATCH_CASES, ids=gr.conv_case_id)
def test_conv_emulation_within_bound(c):
    got, guards = gr.emulate_conv(c)
    ratio, kept = gr.conv_verdict(c, got)
    print(f"{gr.conv_case_id(c)}: emulation worst ratio {ratio:.3f}")
    assert ratio <= 1.0 and kept == 0 and guards


@pytest.mark.parametrize("group", list(gr.ALOAD_GROUPS))
def test_aload_emulation_within_bound(group):
    for c in gr.ALOAD_GROUPS[group]:
        o = gr.aload_operands(c)
        img, guards = gr.emulate_aload(c, o)
        ratio, outside = gr.aload_verdict(c, o, img)
        assert ratio <= 1.0 and outside and guards, (c.name, ratio, outside, guards)


# ---------------- every single defect is visible on the GPU test's fixture ----------------
def _conv_caught(c, defect):
    got, guards = gr.emulate_conv(c, defect)
    ratio, kept = gr.conv_verdict(c, got)
    return (not ratio <= 1.0) or kept > 0 or not guards


@pytest.mark.parametrize("defect", gr.CONV_DEFECTS)
def test_conv_defect_is_caught(defect):
    # the f32 loader, the bf16-A loader and the f16x3 LDS-DMA kernel each carry their own copy
    # of the index arithmetic: a defect must show in whichever copies have it
    layers = {"c4_tstride1": (4,), "c4_fstride1": (4,), "c7_fstride1": (7,)}.get(defect, (4, 7))
    for mode, a16, c16 in (("fp32", 0, 0), ("bf16", 1, 1), ("f16x3", 0, 0)):
        for w in layers:
            cases = [c for c in gr.EDGE_CASES if (c.mode, c.a16, c.c16, c.which) == (mode, a16, c16, w)]
            assert cases
            hit = [gr.conv_case_id(c) for c in cases if _conv_caught(c, defect)]
            assert hit, (defect, mode, w)
            if defect not in ("prev_sequence",):  # (a sequence alone has no previous one)
                assert len(hit) == len(cases), (defect, hit)


@pytest.mark.parametrize("defect", gr.ALOAD_DEFECTS)
def test_aload_defect_is_caught(defect):
    hit = []
    for cases in gr.ALOAD_GROUPS.values():
        for c in cases:
            o = gr.aload_operands(c)
            img, guards = gr.emulate_aload(c, o, defect)
            ratio, outside = gr.aload_verdict(c, o, img)
            if (not ratio <= 1.0) or not outside or not guards:
                hit.append(c.name)
    assert hit, defect
    print(f"{defect}: seen by {len(hit)} cases, e.g. {hit[:3]}")
