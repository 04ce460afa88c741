"""The diarization clustering on an MI355X (zasr.binding.Diarizer over the zasr_diar_* C ABI,
zasr.diarize, FullPipe(diarize=True)): each stage against numpy on the same inputs, the
eigen-solver against numpy.linalg.eigh on the device's own matrix, and the whole path against
the reference's answers (tests/golden/diar_cases.*).  Reads no reference path."""
import json
import os

import numpy as np
import pytest

from conftest import gpu_available
from diar_inputs import canonical, case_embeddings, lapack_embed, make_embeddings, window_plan

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [2, 7, 10, 24, 33, 130, 257, 1000, 2048]
PVAL, MIN_PNUM = 0.012, 6
STAGE = {}


@pytest.fixture(scope="module")
def dz():
    if not gpu_available():
        pytest.skip("no GPU")
    from zasr.binding import Diarizer
    d = Diarizer()
    yield d
    d.close()


@pytest.fixture(scope="module")
def gold():
    return (json.load(open(os.path.join(GOLD, "diar_cases.json"))),
            np.load(os.path.join(GOLD, "diar_cases.npz")))


def n_elems(N, pval=PVAL, min_pnum=MIN_PNUM):
    return max(min(int((1 - pval) * N), N - min_pnum), 0)


def inputs(N):
    return make_embeddings(1000 + N, N, max(1, min(6, N // 12)), 0.6)[0]


def device_stage(dz, N):
    """similarity -> prune -> eigs of inputs(N) through the stage entries, each result copied
    back; computed once per N and shared by the stage tests."""
    import torch
    if N in STAGE:
        return STAGE[N]
    X = inputs(N)
    dX = torch.from_numpy(X).cuda()
    dM = torch.empty((N, N), dtype=torch.float32, device="cuda")
    ddeg = torch.empty(N, dtype=torch.float64, device="cuda")
    dz.similarity(dX.data_ptr(), N, X.shape[1], dM.data_ptr())
    torch.cuda.synchronize()
    sim = dM.cpu().numpy()
    dz.prune(dM.data_ptr(), N, PVAL, MIN_PNUM, ddeg.data_ptr())
    torch.cuda.synchronize()
    Mp, deg = dM.cpu().numpy(), ddeg.cpu().numpy()
    k = min(16, N)
    lam, vec, passes = dz.eigs(dM.data_ptr(), ddeg.data_ptr(), N, k)
    STAGE[N] = dict(X=X, sim=sim, M=Mp, deg=deg, lam=lam, vec=vec, passes=passes,
                    apps=dz.last_stats()[1])
    return STAGE[N]


@pytest.mark.parametrize("N", SHAPES)
def test_similarity(dz, N):
    """Against numpy float64; bound: 3x numpy float32's own worst distance from float64 on the
    same input (the exact-f32 MFMA sum differs from sgemm only in order)."""
    s = device_stage(dz, N)
    X = s["X"]
    x64 = X.astype(np.float64)
    x64 = x64 / (np.linalg.norm(x64, axis=1, keepdims=True) + 1e-10)
    ref = x64 @ x64.T
    x32 = X / (np.linalg.norm(X, axis=1, keepdims=True) + np.float32(1e-10))
    own = np.abs((x32 @ x32.T).astype(np.float64) - ref).max()
    err = np.abs(s["sim"].astype(np.float64) - ref).max()
    print(f"N={N} device err {err:.3e} numpy f32 err {own:.3e}")
    assert err <= 3 * own


def test_similarity_plain_kernel(dz):
    """A D the MFMA GEMM does not take (D % 4 != 0) and D = 1, same bound."""
    import torch
    for N, D in ((37, 7), (65, 1), (130, 510)):
        X = np.random.default_rng(N).standard_normal((N, D)).astype(np.float32)
        dX = torch.from_numpy(X).cuda()
        dM = torch.empty((N, N), dtype=torch.float32, device="cuda")
        dz.similarity(dX.data_ptr(), N, D, dM.data_ptr())
        torch.cuda.synchronize()
        x64 = X.astype(np.float64)
        x64 = x64 / (np.linalg.norm(x64, axis=1, keepdims=True) + 1e-10)
        ref = x64 @ x64.T
        x32 = X / (np.linalg.norm(X, axis=1, keepdims=True) + np.float32(1e-10))
        own = np.abs((x32 @ x32.T).astype(np.float64) - ref).max()
        err = np.abs(dM.cpu().numpy().astype(np.float64) - ref).max()
        print(f"N={N} D={D} device err {err:.3e} numpy f32 err {own:.3e}")
        assert err <= 3 * max(own, 2.0 ** -24)


def host_prune(M, ne):
    """numpy's p_pruning on a float32 matrix: (kept mask, pruned matrix)."""
    N = M.shape[0]
    P = M.copy()
    for i in range(N):
        P[i, np.argsort(M[i], kind="stable")[:ne]] = 0
    keep = np.ones((N, N), bool)
    for i in range(N):
        keep[i, np.argsort(M[i], kind="stable")[:ne]] = False
    return keep, P


@pytest.mark.parametrize("N", SHAPES)
def test_prune_symmetrise_degree(dz, N):
    """A host-made float32 M through zasr_diar_prune: the kept set of every row is numpy's,
    the symmetrised matrix is bit-equal to 0.5 (P + P^T) in float32 with a zero diagonal, deg
    is within 1e-12 relative of the float64 row sums."""
    import torch
    X = inputs(N)
    x32 = X / (np.linalg.norm(X, axis=1, keepdims=True) + np.float32(1e-10))
    M = (x32 @ x32.T).astype(np.float32)
    ne = n_elems(N)
    srt = np.sort(M, axis=1)
    if 0 < ne < N:
        assert (srt[:, ne] > srt[:, ne - 1]).all(), "input has a tie at the threshold"
    _, P = host_prune(M, ne)
    want = np.float32(0.5) * (P + P.T)
    np.fill_diagonal(want, 0)
    dM = torch.from_numpy(M).cuda()
    ddeg = torch.empty(N, dtype=torch.float64, device="cuda")
    dz.prune(dM.data_ptr(), N, PVAL, MIN_PNUM, ddeg.data_ptr())
    torch.cuda.synchronize()
    got = dM.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    deg64 = np.abs(want.astype(np.float64)).sum(1)
    np.testing.assert_allclose(ddeg.cpu().numpy(), deg64, rtol=1e-12, atol=0)
    if N <= 6:
        assert ne == 0  # keep all


def test_prune_ties_keep_lowest_columns(dz):
    """Rows with equal values at the threshold keep the lowest column indices among them
    (pval = 0, min_pnum = 6: exactly six entries survive per row): rows of nothing but ties,
    a row without ties, ten tied leaders, one leader above ties, negative ties.  The expected
    matrix is the symmetrised form of the expected kept entries, compared bit for bit."""
    import torch
    N, keep = 40, 6
    M = np.full((N, N), 0.25, np.float32)          # every entry ties
    M[3, :] = np.linspace(0.9, 0.1, N, dtype=np.float32)   # a row without ties: columns 0..5
    M[5, 10:20] = 0.75                              # ten tied leaders: columns 10..15 survive
    M[7, 30] = 0.5                                  # one leader, then ties: 30 and 0..4
    M[9, :] = -0.25                                 # negative ties
    M[9, 38] = 0.0
    dM = torch.from_numpy(M).cuda()
    ddeg = torch.empty(N, dtype=torch.float64, device="cuda")
    dz.prune(dM.data_ptr(), N, 0.0, keep, ddeg.data_ptr())
    torch.cuda.synchronize()
    got = dM.cpu().numpy()
    # undo the symmetrise: P = kept entries; got = 0.5 (P + P^T) off the diagonal
    P = np.zeros((N, N), np.float32)
    for i in range(N):
        P[i, :keep] = M[i, :keep]
    P[3] = 0
    P[3, :keep] = M[3, :keep]
    P[5] = 0
    P[5, 10:16] = 0.75
    P[7] = 0
    P[7, 30] = 0.5
    P[7, :5] = 0.25
    P[9] = 0
    P[9, 38] = 0.0
    P[9, :5] = -0.25
    want = np.float32(0.5) * (P + P.T)
    np.fill_diagonal(want, 0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("N", SHAPES)
def test_eigs_on_device_matrix(dz, N):
    """The solver on the device's own pruned matrix (copied back) against numpy.linalg.eigh in
    float64: eigenvalues within 1e-6 ub (10x the stopping residual; a residual r bounds the
    eigenvalue error by r), residuals |L v - lambda v| <= 1e-7 ub, |V^T V - I|_max <= 1e-10."""
    s = device_stage(dz, N)
    M = s["M"].astype(np.float64)
    assert np.array_equal(s["M"], s["M"].T) and not np.diag(s["M"]).any()
    L = np.diag(s["deg"]) - M
    ub = 1.01 * 2 * s["deg"].max()
    k = min(16, N)
    ref = np.linalg.eigvalsh(L)[:k]
    lam, V = s["lam"], s["vec"]
    res = np.linalg.norm(L @ V - V * lam, axis=0)
    orth = np.abs(V.T @ V - np.eye(k)).max()
    print(f"N={N} passes {s['passes']} applications {s['apps']} eig err "
          f"{np.abs(lam - ref).max():.3e} residual {res.max():.3e} orth {orth:.3e} ub {ub:.3f}")
    assert s["passes"] >= 1
    assert np.abs(lam - ref).max() <= 1e-6 * ub
    assert res.max() <= 1e-7 * ub
    assert orth <= 1e-10


def test_eigs_disconnected_components(dz):
    """S exactly-disconnected components: a zero eigenvalue of multiplicity S (the degenerate
    start), the next eigenvalue apart; the null vectors are constant on every component."""
    import torch
    S, m = 5, 23
    N = S * m
    rng = np.random.default_rng(9)
    M = np.zeros((N, N), np.float32)
    for c in range(S):
        a = rng.uniform(0.2, 1.0, (m, m)).astype(np.float32)
        M[c * m:(c + 1) * m, c * m:(c + 1) * m] = np.float32(0.5) * (a + a.T)
    np.fill_diagonal(M, 0)
    deg = np.abs(M.astype(np.float64)).sum(1)
    dM, ddeg = torch.from_numpy(M).cuda(), torch.from_numpy(deg).cuda()
    lam, V, passes = dz.eigs(dM.data_ptr(), ddeg.data_ptr(), N, 16)
    ub = 1.01 * 2 * deg.max()
    ref = np.linalg.eigvalsh(np.diag(deg) - M.astype(np.float64))[:16]
    print(f"passes {passes} lam {lam[:7]}")
    assert np.abs(lam - ref).max() <= 1e-6 * ub
    assert np.abs(lam[:S]).max() <= 1e-6 * ub and lam[S] > 0.1
    for c in range(S):
        blk = V[c * m:(c + 1) * m, :S]
        assert np.abs(blk - blk[0]).max() <= 1e-6
    assert np.abs(V.T @ V - np.eye(16)).max() <= 1e-10


CLUSTER = ["c10", "c24", "c33", "c130", "c257", "c1000", "c2048", "minor", "merge", "forced"]
PROCESS = ["s_general", "s_forced", "s_two", "s_seven"]


@pytest.mark.parametrize("name", CLUSTER)
def test_end_to_end_cluster(dz, gold, name):
    """spectral_embed -> senko_cluster on the golden cases: the speaker count and the
    partition are the reference's; two runs give the same bits; the share of rows whose kept
    set differs from numpy's is at most the case's ambiguous share (rows whose threshold is
    within 1e-5 of the next entry)."""
    import torch
    from zasr.diarize import senko_cluster
    doc, arr = gold
    case = doc[name]
    X = case_embeddings(case)
    kw = dict(case["kw"])
    kw.pop("cluster_type")
    runs = []

    def embed(x, pval, min_pnum, k):
        runs.append(dz.spectral_embed(x, pval=pval, min_pnum=min_pnum, k=k))
        return runs[-1]
    labels = senko_cluster(X, embed=embed, **kw)
    again = senko_cluster(X, embed=embed, **kw)
    assert len(np.unique(labels)) == case["speakers"]
    assert canonical(labels) == canonical(arr[f"{name}/labels"])
    assert np.array_equal(labels, again)
    assert runs[0][0].tobytes() == runs[1][0].tobytes()
    assert runs[0][1].tobytes() == runs[1][1].tobytes()
    # kept sets of the device's own similarity against numpy's
    N = X.shape[0]
    dX = torch.from_numpy(X).cuda()
    dM = torch.empty((N, N), dtype=torch.float32, device="cuda")
    dz.similarity(dX.data_ptr(), N, X.shape[1], dM.data_ptr())
    torch.cuda.synchronize()
    ne = n_elems(N, kw["pval"], kw.get("min_pnum", 6))
    kd, _ = host_prune(dM.cpu().numpy(), ne)
    x32 = X / (np.linalg.norm(X, axis=1, keepdims=True) + np.float32(1e-10))
    kn, _ = host_prune(x32 @ x32.T, ne)
    differ = float((kd != kn).any(axis=1).mean())
    print(f"{name}: rows with another kept set {differ:.4f}, ambiguous {float(arr[f'{name}/ambiguous']):.4f}, "
          f"passes {dz.last_stats()}")
    assert differ <= float(arr[f"{name}/ambiguous"])


@pytest.mark.parametrize("name", PROCESS)
def test_end_to_end_segments(dz, gold, name):
    """diarize() with the device embedding = the reference's process() segment list."""
    from zasr.diarize import diarize
    doc, arr = gold
    case = doc[name]
    off, length, rows, duration = window_plan(case["n"], case["seed"])

    def embed(x, pval, min_pnum, k):
        return dz.spectral_embed(x, pval=pval, min_pnum=min_pnum, k=k)
    segs, labels = diarize(case_embeddings(case), rows, off, length, duration,
                           num_speakers=case["num_speakers"], embed=embed, return_labels=True)
    assert segs == case["segments"]
    assert canonical(labels) == canonical(arr[f"{name}/labels"])


def test_errors(dz):
    """N = 1, N = 8193 and D = 0 are ZASR_ERR_INVALID with a message (no device call)."""
    from zasr.binding import ZasrError
    lam = np.zeros(16)
    import ctypes as C
    dp = C.POINTER(C.c_double)
    for N, D in ((1, 192), (8193, 192), (16, 0), (16, 513)):
        x = np.zeros((max(N, 1), max(D, 1)), np.float32)
        vec = np.zeros((max(N, 1), 16))
        rc = dz.lib.zasr_diar_spectral_embed(dz.handle, C.c_void_p(x.ctypes.data), 0, N, D, 0.02, 6,
                                             1, lam.ctypes.data_as(dp), vec.ctypes.data_as(dp), None)
        assert rc == 1, (N, D, rc)  # ZASR_ERR_INVALID
        assert dz.lib.zasr_last_error().decode()
    with pytest.raises(ZasrError, match="k must be"):
        dz.spectral_embed(np.ones((5, 8), np.float32), k=6)
    with pytest.raises(ZasrError, match="pval"):
        dz.spectral_embed(np.ones((5, 8), np.float32), pval=1.5, k=2)


@pytest.fixture(scope="module")
def diar_pipe(tmp_path_factory):
    """tests/test_gpu_pipe.py's fixture recipe with diarize=True."""
    if not gpu_available():
        pytest.skip("no GPU")
    from zasr.binding import CamppEmbedder, Recognizer, VibertSession
    from zasr.campp import CamppConfig
    from zasr.campp import save_model_dir as campp_save
    from zasr.campp import synth_weights as campp_weights
    from zasr.model import save_model_dir, synth_tokens, synth_weights, zipformer_tiny
    from zasr.pipeline import FullPipe
    from zasr.synth_audio import synth_speech
    from zasr.vibert import save_model_dir as vib_save
    from zasr.vibert import synth_weights as vib_weights
    from zasr.vibert import vibert_tiny
    d = tmp_path_factory.mktemp("diarpipe")
    cfg = zipformer_tiny(64)
    toks = synth_tokens(cfg.vocab_size)
    save_model_dir(str(d / "asr"), cfg, synth_weights(cfg, 5, blank_bias=-1.5), toks)
    rec = Recognizer(str(d / "asr"), "greedy_search", 1, precision="fp32")
    ccfg = CamppConfig()
    campp_save(str(d / "campp"), ccfg, campp_weights(ccfg, 3))
    emb = CamppEmbedder(str(d / "campp"))
    vcfg = vibert_tiny()
    vib_save(str(d / "vib"), vcfg, vib_weights(vcfg, 4))
    vib = VibertSession(str(d / "vib"))
    recd = {"id2token": dict(enumerate(toks)), "vocab_size": cfg.vocab_size}
    p = FullPipe(rec, recd, emb, vib, vcfg.vocab_size, beam=1, campp_batch=16, diarize=True)
    audio = synth_speech(75.0, 31)
    p.prepare(audio)
    out = p.run()
    yield p, audio, out
    rec.close()
    emb.close()
    vib.close()


def test_pipe_speaker_segments(diar_pipe):
    """FullPipe(diarize=True) on the 75 s file: segments cover only window times, are ordered
    and do not overlap, and equal zasr.diarize.diarize on the returned embeddings with the
    LAPACK embed (the device clusters the un-normalised device embeddings, the host copy is
    L2-normalised: the same cosines up to float32 rounding)."""
    from zasr.diarize import diarize, window_times
    p, audio, out = diar_pipe
    segs, labels = out["speaker_segments"], out["speaker_labels"]
    win = out["windows"]
    assert len(labels) == len(win) == out["embeddings"].shape[0] > 10
    times = window_times(win, p.r_off_all, p.r_len_all)
    lo, hi = min(t[0] for t in times), max(t[1] for t in times)
    assert segs and all(lo <= s["start"] < s["end"] <= hi for s in segs)
    assert all(a["end"] <= b["start"] for a, b in zip(segs, segs[1:]))
    assert sorted({s["speaker"] for s in segs}) == list(range(len({s["speaker"] for s in segs})))
    want, wl = diarize(out["embeddings"], win, p.r_off_all, p.r_len_all, len(audio) / 16000.0,
                       embed=lapack_embed, return_labels=True)
    print("pipe speakers", len(np.unique(labels)), "segments", segs)
    assert canonical(labels) == canonical(wl)
    assert segs == want


def test_pipe_default_has_no_speaker_keys():
    """diarize defaults to off: FullPipe's signature keeps it False (the default dict is what
    tests/test_gpu_pipe.py pins)."""
    import inspect
    from zasr.pipeline import FullPipe
    assert inspect.signature(FullPipe.__init__).parameters["diarize"].default is False
