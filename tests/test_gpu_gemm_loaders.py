"""The general GEMMs behind their implicit-im2col / BN-ReLU loaders and over ragged z-slices,
alone, against float64 (tests/gemm_loader_reference.py: cases, operands, references, bound).

conv.4 / conv.7 run through zasr_selftest_conv_gemm, which builds the slices and picks the GEMM
with the functions the decode calls (engine.h frontend_conv_slices / launch_frontend_conv_gemm):
one launch, no route override.  The CAM++ projections run through zasr_selftest_gemm_aload.

Edge batch T = [9, 10, 21, 35, 12, 22]: conv.7 slices of 19, 19, 133, 266, 38 and 133 rows (below
a tile, either side of 128, two tiles and a tail), conv.4 slices of 117 .. 624 rows; every slice
shorter than the longest leaves whole blocks at the early exit.  T = [9] and T = [35] alone must
return byte for byte the rows those sequences have inside the batch: tiles are laid per slice
from the slice's own row 0, every one of these launches stays under pick_tile's 512 blocks and
so takes the 64-row tile (conv.4: 64 x 32, conv.7: 64 x 128; checked on the host by
test_gemm_loader_reference.py::test_fixture_shapes_and_tiles), and f16x3 conv.7 is
gemm_glds_h3_kernel's 128 x 128 tile in all three.  No pair's picks differ, so byte equality is
asserted for every combination.

Kernel reached, edge batch and single sequences (z-sliced: never the DEEP variants):

    fp32            gemm_f32_kernel<64, 32 | 128, ALOAD_CONV2 | CONV3, SWOOSHR>
    bf16  (any)     gemm_bf16_kernel<64, 32 | 128, BK 32, ...>; bf16 A: load_a8's own branches;
                    bf16 C at conv.7: the paired-fragment store
    bf16x3 / x6     gemm_x3_kernel<64, 32 | 128, NP 2 | 3>
    f16x3           conv.4: gemm_x3_kernel<64, 32, FMT 1>; conv.7: gemm_glds_h3_kernel<ALOAD_CONV3>

Dispatch cases: 8 equal sequences, the shortest that reach 512 blocks of 128 rows (pick_tile
counts the slices): conv.7 T = 857 (L = 425, 8075 rows, 64 row tiles each), conv.4 T = 417
(l2 = 207, 8073 rows, 64 row tiles each: N = 32 is one column tile, as conv.7's N = 128 is).

    fp32            gemm_f32_kernel<128, 32 (4 x 1 waves) | 128, 128>
    bf16  (any)     gemm_bf16_kernel<128, 32 | 128, 128, BK 32>
    bf16x3 / x6     gemm_x3_kernel<128, 32 | 128, 128>
    f16x3 conv.4    gemm_x3_kernel<128, 32, FMT 1>     (conv.7: the edge batch is its case)

CAM++ shapes (gemm_f32_kernel<64, BN>, DEEP where K % 32 == 0): the TDNN (5 taps, stride 2,
pad 2, RELU, C = 160 and 8, 3 windows of T in {1, 2, 97, 150}), the local convolution (C = 128, 3
taps, dilation 1 and 2, N = 32 written at column 128 of ldc = 224, MULAUX with ldaux = 32 -- and
48 -- 3 windows of T2 in {1 .. 115}: rows of two windows share a 64-row tile, and at T2 <= 2 with
dilation 2 every neighbour tap is padding), and BN-ReLU over (K, lda) x N x M x epilogue x ldc.

Every test prints its worst |got - ref| / bound.  Measured on the MI355X (profiles/gemm_loaders/).
"""
import numpy as np
import pytest

import gemm_loader_reference as gr
from conftest import gpu_available
from test_gpu_gemm import EPI

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")


def run_conv(c):
    from zasr.binding import selftest_conv_gemm
    o = gr.conv_operands(c.which, c.T)
    return selftest_conv_gemm(c.mode, c.which, c.T, o["A"], o["W"], o["bias"], bool(c.a16), bool(c.c16),
                              fill=gr.FILL)


def check_conv(c):
    """Guards intact (the entry raises otherwise), every element within the bound, no output
    row left at its initial contents."""
    got = run_conv(c)
    ratio, kept = gr.conv_verdict(c, got)
    print(f"{gr.conv_case_id(c)}: worst |got - ref| / bound = {ratio:.3f}")
    assert ratio <= 1.0, (gr.conv_case_id(c), ratio)
    assert kept == 0, (gr.conv_case_id(c), kept)
    return got


COMBOS = [(m, a, c, w) for m, a, c, ws in gr.CONV_COMBOS for w in ws]


@pytest.mark.parametrize("combo", COMBOS, ids=["{}_a{}c{}_conv{}".format(*x) for x in COMBOS])
def test_conv_gemm_edge_batch_matches_f64(need_gpu, combo):
    batch = check_conv(gr.ConvCase(*combo, gr.EDGE_T))
    _, rout = gr.conv_lengths(combo[3], gr.EDGE_T)
    off = np.concatenate([[0], np.cumsum(rout)])
    for T in gr.SINGLE_T:
        alone = check_conv(gr.ConvCase(*combo, T))
        q = gr.EDGE_T.index(T[0])
        # same tile in both launches (module docstring): the same bytes
        assert np.array_equal(alone.view(np.uint32), batch[off[q]:off[q + 1]].view(np.uint32)), (combo, T)


@pytest.mark.parametrize("case", gr.DISPATCH_CASES, ids=gr.conv_case_id)
def test_conv_gemm_dispatch_128_row_tile_matches_f64(need_gpu, case):
    check_conv(case)


def run_aload(c, o):
    from zasr.binding import selftest_gemm_aload
    bn = c.kind == "bn"
    return selftest_gemm_aload(gr.ALOAD_BNRELU if bn else gr.ALOAD_IM2COL1D, o["A"], o["W"], o["bias"],
                               o["C0"], c.M, c.lda, EPI[c.epi], c.c_col, o["scale"], o["shift"],
                               (0, 0, 0, 1, 1, 0) if bn else c.i2c, o["aux"])


def check_aload(c):
    o = gr.aload_operands(c)
    img = run_aload(c, o)
    ratio, outside = gr.aload_verdict(c, o, img)
    print(f"{c.name}: worst |got - ref| / bound = {ratio:.3f}")
    return ratio, outside


@pytest.mark.parametrize("group", list(gr.ALOAD_GROUPS))
def test_gemm_aload_campp_shapes_match_f64(need_gpu, group):
    res = [(c.name, *check_aload(c)) for c in gr.ALOAD_GROUPS[group]]
    bad = [r for r in res if not r[1] <= 1.0 or not r[2]]
    assert not bad, bad


VALID_CONV = gr.ConvCase("fp32", 0, 0, 7, (9,))
VALID_ALOAD = gr.ALOAD_GROUPS["local"][2]
REFUSED_CONV = [
    gr.ConvCase("fp32", 1, 1, 4, (9, 12)),    # bf16 A / C outside the bf16 mode
    gr.ConvCase("f16x3", 0, 1, 7, (9, 12)),   # bf16 C outside the bf16 mode
    gr.ConvCase("bf16", 1, 0, 7, (9, 12)),    # bf16 A with f32 C: no such kernel
    gr.ConvCase("bf16", 0, 1, 4, (9, 12)),    # f32 A with bf16 C is conv.7's only
    gr.ConvCase("fp32", 0, 0, 5, (9, 12)),    # which = 5
    gr.ConvCase("fp32", 0, 0, 7, (9, 8)),     # T below 9
]


@pytest.mark.parametrize("case", REFUSED_CONV, ids=lambda c: f"{c.mode}_a{c.a16}c{c.c16}_conv{c.which}_T{min(c.T)}")
def test_conv_gemm_refused_combinations_report_an_error(need_gpu, case):
    from zasr.binding import ZasrError, selftest_conv_gemm
    ok = case.which in (4, 7) and min(case.T) >= 9
    o = gr.conv_operands(case.which if ok else 7, case.T if ok else (9, 12))
    with pytest.raises(ZasrError):
        selftest_conv_gemm(case.mode, case.which, case.T, o["A"], o["W"], o["bias"], bool(case.a16),
                           bool(case.c16))
    check_conv(VALID_CONV)  # the refusal is not sticky


REFUSED_ALOAD = [
    VALID_ALOAD._replace(name="i2c_swooshl", epi="SWOOSHL"),             # an epilogue the loader lacks
    VALID_ALOAD._replace(name="i2c_resadd", epi="RESADD"),
    gr.ALOAD_GROUPS["bnrelu"][0]._replace(name="bn_mulaux", epi="MULAUX", ldaux=128),  # MULAUX: im2col only
    VALID_ALOAD._replace(name="i2c_K_not_C", K=380),                     # K % C != 0
    VALID_ALOAD._replace(name="i2c_M_not_Tout", M=8),                    # M % Tout != 0 (Tout = 3)
    VALID_ALOAD._replace(name="i2c_C_not_4", K=12, i2c=(3, 3, 6, 1, 1, 1)),  # C % 4 != 0
]


@pytest.mark.parametrize("case", REFUSED_ALOAD, ids=lambda c: c.name)
def test_gemm_aload_refused_combinations_report_an_error(need_gpu, case):
    from zasr.binding import ZasrError
    with pytest.raises(ZasrError):
        run_aload(case, gr.aload_operands(case))
    ratio, outside = check_aload(VALID_ALOAD)  # the refusal is not sticky
    assert ratio <= 1.0 and outside
