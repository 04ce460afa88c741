"""tests/attention_reference.py without a GPU: its float64 formulas equal the oracle's attention,
a numpy emulation of every mode stays inside the bound, and single-defect emulations leave it.

(a) one sequence of the reference = oracle/zipformer.py `_attn_weights` (with its as_strided
    relative-to-absolute indexing), `_self_attn` and `_nonlin_attn` in float64, the projections set
    to the identity so the oracle sees the same q, k, p, pe, v and h3;
(b) the emulation (f32 arithmetic, the modes' bf16 / fp16 pieces, key blocks of 32, the online
    rescale) is at ratio <= 1 on every GPU case: the bound is not wrong;
(c) each defect below pushes an element over ratio 1 (or into the zero padding) in every mode it
    applies to: the bound is not slack.
"""
import numpy as np
import pytest

import attention_reference as ar


def worst(got, pair):
    """The worst ratio of an output; a NaN is outside every bound."""
    r = ar.ratio(got, *pair)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


# ---- (a) the formulas ----
class _Cfg:
    query_head_dim, pos_head_dim = 32, 4


@pytest.mark.parametrize("mode", ["fp32", "bf16", "f16x3"])
def test_reference_equals_the_oracle_formulas(mode):
    import torch

    from oracle.zipformer import ZipformerOracle
    L, H, hid = 37, 2, 16
    c = ar.Case("nonlin", mode, H, (L,), L, hid)  # pmax = L: the oracle's table has 2 L - 1 rows
    o = ar.operands(c)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    eye = lambda n: torch.eye(n, dtype=torch.float64)
    orc = ZipformerOracle.__new__(ZipformerOracle)
    orc.cfg = _Cfg()
    orc.w = {"a.self_attn_weights.in_proj.weight": eye(68 * H),
             "a.self_attn_weights.in_proj.bias": torch.zeros(68 * H, dtype=torch.float64),
             "a.self_attn_weights.linear_pos.weight": eye(4 * H)}
    for name, n in (("sa", 12 * H), ("na", hid)):
        orc.w[name + ".in_proj.weight"] = eye(n * (3 if name == "na" else 1))
        orc.w[name + ".in_proj.bias"] = torch.zeros(n * (3 if name == "na" else 1), dtype=torch.float64)
        orc.w[name + ".out_proj.weight"] = eye(n)
        orc.w[name + ".out_proj.bias"] = torch.zeros(n, dtype=torch.float64)
    # the split modes' natural softmax of s is the oracle's; the bf16 mode's stored q and p carry
    # log2(e), so its base-2 softmax is the oracle's softmax of ln 2 times the stored scores
    qkp = o["qkp"].astype(np.float64).copy()
    if mode == "bf16":
        qkp[:, :32 * H] *= np.log(2.0)
        qkp[:, 64 * H:] *= np.log(2.0)
    A = orc._attn_weights("a.", t64(qkp)[:, None, :], t64(o["pos"]), H)  # (H, 1, L, L)
    for h in range(H):
        hr = ar.head_reference(c, o, 0, h)
        np.testing.assert_allclose(hr["P"], A[h, 0].numpy(), rtol=1e-12, atol=1e-300)
        lse = torch.logsumexp(_scores(qkp, o, H, h), dim=1).numpy()
        scale = np.log(2.0) if mode != "fp32" else 1.0
        np.testing.assert_allclose(hr["c"] * scale, lse, rtol=1e-12)
    sa = ar.reference_sa(c._replace(route="sa"), o)
    y = orc._self_attn("sa", t64(o["v1"])[:, None, :], A)[:, 0].numpy()
    np.testing.assert_allclose(sa["out1"][0], y, rtol=1e-11, atol=1e-13)
    z = orc._nonlin_attn("na", t64(o["h3"])[:, None, :], A[0:1])[:, 0].numpy()
    if mode != "fp32":
        np.testing.assert_allclose(ar.reference_nonlin(c, o)["z"][0], z, rtol=1e-11, atol=1e-13)


def _scores(qkp, o, H, h):
    """The natural-domain scores of head h, written out once more (j - i + L - 1 indexing)."""
    import torch
    L = qkp.shape[0]
    q, k = qkp[:, 32 * h:32 * h + 32], qkp[:, 32 * H + 32 * h:32 * H + 32 * h + 32]
    p = qkp[:, 64 * H + 4 * h:64 * H + 4 * h + 4]
    R = o["pos"][:, 4 * h:4 * h + 4].astype(np.float64)
    s = q @ k.T
    for i in range(L):
        for j in range(L):
            s[i, j] += p[i] @ R[j - i + L - 1]
    return torch.from_numpy(s)


# ---- (b) the emulation stays inside the bound ----
def emulated_ratios(c, o, emu_case=None, mut=None):
    """Worst ratio per output of a case's emulation (emu_case: the case the emulation runs as)."""
    e = emu_case or c
    if c.route == "weights":
        return {"A0": worst(ar.emulate_weights(e, o, mut), ar.reference_weights(c, o))}
    if c.route == "sa":
        out1, stats, out2 = ar.emulate_sa(e, o, mut)
        ref = ar.reference_sa(c, o)
        return {"out1": worst(out1, ref["out1"]), "stats": worst(stats, ref["stats"]),
                "out2": worst(out2, ref["out2"])}
    img, z = ar.emulate_nonlin(e, o, mut)
    ref = ar.reference_nonlin(c, o)
    res = {"t1t": worst(img, ref["t1t"])}
    if "z" in ref and z is not None:
        res["z"] = worst(z, ref["z"])
    return res


GROUPS = [(r, m) for r in ("weights", "sa", "nonlin") for m in ar.ROUTE_MODES[r]]


@pytest.mark.parametrize("route,mode", GROUPS, ids=["{}_{}".format(*g) for g in GROUPS])
def test_emulation_is_inside_the_bound(route, mode):
    bad = []
    for c in ar.route_cases(route, mode):
        if c.H == 8 and c.L == ar.RAGGED and route != "sa":
            continue  # head 0 alone: the H = 2 case already holds it
        r = emulated_ratios(c, ar.operands(c))
        print(ar.case_id(c), {k: round(v, 3) for k, v in r.items()})
        bad += [(ar.case_id(c), k, v) for k, v in r.items() if not v <= 1.0]
    assert not bad, bad


# ---- (c) single defects leave the bound ----
ONLINE_SA = ar.MODES                      # flash mode 1 and attn_sa online
MUTANTS = [
    ("mask_extra", "weights", ar.ROUTE_MODES["weights"]), ("mask_extra", "sa", ar.MODES),
    ("mask_extra", "nonlin", ["bf16", "f16x3"]),
    ("mask_short", "weights", ar.ROUTE_MODES["weights"]), ("mask_short", "sa", ar.MODES),
    ("mask_short", "nonlin", ["bf16", "f16x3"]),
    ("pos_shift", "weights", ar.ROUTE_MODES["weights"]), ("pos_shift", "sa", ar.MODES),
    ("pos_shift", "nonlin", ["bf16", "f16x3"]),
    ("skip_rescale", "sa", ONLINE_SA), ("skip_rescale", "nonlin", ["bf16", "f16x3"]),
    ("v_dim11", "sa", ar.MODES),
    ("z_chunk_shift", "nonlin", ["bf16", "f16x3"]),
    ("pad_nonzero", "weights", ar.ROUTE_MODES["weights"]), ("pad_nonzero", "nonlin", ar.ROUTE_MODES["nonlin"]),
    ("half_stat", "sa", ar.MODES),
]
MUTANT_CASES = [(m, r, mode) for m, r, modes in MUTANTS for mode in modes]


def mutant_case(mut, route, mode):
    """The committed ragged case the defect applies to (z_chunk_shift: a hid with two z-chunks)."""
    hid = 288 if mut == "z_chunk_shift" else 144 if route == "nonlin" else 0
    return ar.Case(route, mode, 2, ar.RAGGED, ar.pmax_default(ar.RAGGED), hid)


@pytest.mark.parametrize("mut,route,mode", MUTANT_CASES, ids=["{}_{}_{}".format(*m) for m in MUTANT_CASES])
def test_single_defect_leaves_the_bound(mut, route, mode):
    c = mutant_case(mut, route, mode)
    assert c in ar.route_cases(route, mode)
    o = ar.operands(c)
    r = emulated_ratios(c, o, mut=mut)
    print(ar.case_id(c), mut, {k: round(v, 3) for k, v in r.items()})
    assert max(r.values()) > 1.0, r
    if mut == "pad_nonzero":  # and the padding check proper sees it
        if route == "weights":
            assert np.any(ar.emulate_weights(c, o, mut)[ar.padding_mask_weights(c)] != 0)
            assert np.all(ar.emulate_weights(c, o)[ar.padding_mask_weights(c)] == 0)
        else:
            assert np.any(ar.emulate_nonlin(c, o, mut)[0][ar.padding_mask_t1t(c)] != 0)


LOWER = [(r, m) for r in ("weights", "sa", "nonlin") for m in ("bf16x3", "bf16x6", "f16x3")
         if m in ar.ROUTE_MODES[r]]


@pytest.mark.parametrize("route,mode", LOWER, ids=["{}_{}".format(*g) for g in LOWER])
def test_one_precision_step_lower_leaves_the_bound(route, mode):
    """bf16x3's emulation fails the bf16x6 and f16x3 bounds; one bf16 piece fails bf16x3's."""
    c = mutant_case(None, route, mode)
    o = ar.operands(c)
    r = emulated_ratios(c, o, emu_case=c._replace(mode=ar.lower_mode(mode)))
    print(ar.case_id(c), "as", ar.lower_mode(mode), {k: round(v, 3) for k, v in r.items()})
    assert max(r.values()) > 1.0, r


def test_ramp_rows_move_the_maximum_and_the_others_do_not():
    """The inputs make the edges bite: on the ramp rows of the 289-frame sequence the running
    maximum rises at several key-block boundaries; on most other rows it never moves after the
    second block."""
    c = ar.Case("sa", "bf16x6", 2, ar.RAGGED, ar.pmax_default(ar.RAGGED), 0)
    o = ar.operands(c)
    b = ar.RAGGED.index(289)
    t = ar.emu_scores(c, o, b, 0)
    bm = np.maximum.accumulate(t.reshape(289, -1, 32).max(axis=2), axis=1)
    rises = (bm[:, 1:] > bm[:, :-1]).sum(axis=1)
    ramp = ar.is_ramp(np.arange(289))
    assert np.median(rises[ramp]) >= 4, np.median(rises[ramp])
    assert np.mean(rises[~ramp][:, None] <= 1) > 0.5, np.mean(rises[~ramp] <= 1)


def test_padding_masks_and_layout():
    c = ar.Case("weights", "bf16x3", 2, ar.RAGGED, ar.pmax_default(ar.RAGGED), 0)
    ref, bound = ar.reference_weights(c, ar.operands(c))
    pad = ar.padding_mask_weights(c)
    assert ref.shape == pad.shape == (sum(L * ar.stride("bf16x3", L) for L in c.L),)
    assert np.all(ref[pad] == 0) and np.all(bound[pad] == 0) and np.all(bound[~pad] > 0)
    f = c._replace(mode="fp32")
    assert ar.padding_mask_weights(f).size == sum(L * ((L + 3) // 4 * 4) for L in c.L)
    n = c._replace(route="nonlin", hid=144)
    assert ar.padding_mask_t1t(n).shape == (144, 32 + 32 + 64 + 0 + 160 + 64 + 320)
    assert ar.pmax_min("fp32", ar.RAGGED) == 320 and ar.pmax_min("bf16", ar.RAGGED) == 289
