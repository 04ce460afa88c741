"""The community-1 diarizer end to end on an MI355X (zasr.community1.process over SegSession,
EmbSession, CluSession and zasr/vbx.py; FullPipe(diarize="community1")), against the restatement
(vbx_reference) driven by the same device class maps and embeddings.  The models are the
synthetic directories of test_gpu_seg.py and test_gpu_emb.py and the PLDA is synthetic, so the
speakers mean nothing: what is held is that the device path computes what the restatement
computes.  Reads no reference path."""
import json
import os

import numpy as np
import pytest

import community1_cases as CC
import resnet34_reference as RN
import seg_inputs as S
import vbx_reference as R
from conftest import gpu_available

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def sessions(tmp_path_factory):
    if not gpu_available():
        pytest.skip("no GPU")
    from zasr import vbx
    from zasr.binding import CluSession, EmbSession, SegSession
    from zasr.pyannet import save_model_dir as seg_save
    from zasr.resnet34 import save_model_dir as emb_save
    d = tmp_path_factory.mktemp("c1")
    cfg, w = S.network()
    seg_save(str(d / "seg"), cfg, w)
    ecfg, ew, _ = RN.network()
    emb_save(str(d / "emb"), ecfg, ew)
    seg, emb, clu = SegSession(str(d / "seg")), EmbSession(str(d / "emb")), CluSession()
    yield seg, emb, clu, vbx.synthetic_plda(seed=2, dim=emb.embedding_dim)
    for s in (seg, emb, clu):
        s.close()


# 12.3 s: 4 chunks by either rule.  11.0 s: total - 160000 is a multiple of 16000, so the
# reference makes a third chunk that classes_device's rule does not.
@pytest.mark.parametrize("seconds,chunks", [(12.3, 4), (11.0, 3)])
def test_process_equals_restatement(sessions, seconds, chunks):
    import torch
    from zasr import community1, vbx
    seg, emb, clu, plda = sessions
    a = S.speech(seconds, 17)
    d_a = torch.from_numpy(np.array(a)).cuda()
    out = community1.process(d_a, seg, emb, clu, plda)
    classes, starts = community1.segment_classes(d_a, seg)
    assert starts == R.chunk_starts_1s(a.shape[0]) and classes.shape == (chunks, 589)
    # the chunk beyond the device rule, and every other, equal the session's own run()
    classes_h, starts_h = community1.segment_classes(np.array(a), seg)
    assert starts_h == starts and np.array_equal(classes_h, classes)
    b = vbx.POWERSET_MAP[classes]
    clean = b * (b.sum(axis=2, keepdims=True) < 2).astype(np.float32)
    e = community1.extract_embeddings(emb, d_a, b, clean, 589, starts,
                                      community1.min_seg_frames_default(589))
    segs, cent, _ = R.diarize(b, e, plda)
    assert list(out) == segs
    assert out.overlap_regions == R.overlap_regions(b, starts, 589, a.shape[0] / 16000.0)
    if cent is None:
        assert out.speaker_centroids is None
    else:
        np.testing.assert_allclose(out.speaker_centroids, cent, rtol=1e-9)
    again = community1.process(np.array(a), seg, emb, clu, plda)      # the host signal
    assert list(again) == list(out) and again.overlap_regions == out.overlap_regions


def test_back_end_on_a_file_with_speakers(sessions):
    """The back end with the device AHC on the 26 s synthetic file of the CPU goldens (three
    speakers found, eleven segments): the reference's own answer."""
    from zasr import vbx
    _, _, clu, _ = sessions
    xv, pl = CC.synthetic_plda_files()
    plda = {"mean1": xv["mean1"], "mean2": xv["mean2"], "lda": xv["lda"], "plda_mu": pl["mu"]}
    gold = np.load(os.path.join(GOLD, "community1_cluster_cases.npz"))
    plda["plda_tr"], plda["plda_psi"] = gold["plda_plda_tr"], gold["plda_plda_psi"]
    want = json.load(open(os.path.join(GOLD, "community1_cluster_cases.json")))["cases"]["f26_mdo0.0"]
    seed, samples, n_spk = CC.FILES["f26"]
    sc = CC.scenario(seed, samples, n_spk)
    b = vbx.POWERSET_MAP[sc["classes"]]
    segs, info = vbx.diarize_from_embeddings(b, sc["embeddings"], clu, plda)
    assert segs == want["segments"] and len({s["speaker"] for s in segs}) == 3
    np.testing.assert_allclose(info["speaker_centroids"], gold[want["centroids"]], rtol=1e-6)
    assert segs == R.diarize(b, sc["embeddings"], plda)[0]


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def test_full_pipe_community1_mode(sessions, tmp_path_factory):
    import torch
    from zasr import community1
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
    seg, e_sess, clu, plda = sessions
    d = tmp_path_factory.mktemp("c1pipe")
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
    audio = synth_speech(24.0, 31)
    args = (rec, recd, emb, vib, vcfg.vocab_size)
    kw = dict(beam=1, campp_batch=16)
    try:
        plain = FullPipe(*args, diarize=True, **kw)
        plain.prepare(audio)
        before = plain.run()
        off = FullPipe(*args, **kw)
        off.prepare(audio)
        out_off = off.run()

        for bad in (dict(segmentation=seg, embedding=e_sess), dict(segmentation=seg, plda=plda),
                    dict(embedding=e_sess, plda=plda),
                    dict(segmentation=seg, embedding=e_sess, plda=plda, shard=True)):
            with pytest.raises(ValueError):
                FullPipe(*args, diarize="community1", **kw, **bad)
        with pytest.raises(ValueError):
            FullPipe(*args, diarize="community2", segmentation=seg, embedding=e_sess, plda=plda, **kw)

        p = FullPipe(*args, diarize="community1", segmentation=seg, embedding=e_sess, plda=plda, **kw)
        p.prepare(audio)
        out = p.run()
        assert set(out) == set(out_off) | {"speaker_segments", "overlap_regions"}
        for k in out_off:
            assert same(out[k], out_off[k]), k
        want = community1.process(torch.from_numpy(audio.astype(np.float32)).cuda(), seg, e_sess,
                                  clu, plda)
        assert out["speaker_segments"] == list(want)
        assert out["overlap_regions"] == list(want.overlap_regions)
        # the stage depends on the signal alone: computed once per prepare(), copied per pass
        first = p.community1_speakers()
        two = p.run_many(2)
        assert p.community1_speakers() is first
        assert all(o["speaker_segments"] == out["speaker_segments"] for o in two)
        assert two[0]["speaker_segments"] is not two[1]["speaker_segments"]
        p.prepare(audio)
        assert p.community1_speakers() is not first and list(p.community1_speakers()) == list(first)

        # diarize=True and diarize=False after the new paths were constructed and run: fresh
        # pipes give the dicts they gave before
        plain2 = FullPipe(*args, diarize=True, **kw)
        plain2.prepare(audio)
        after = plain2.run()
        assert set(after) == set(before)
        for k in before:
            assert same(after[k], before[k]), k
        off2 = FullPipe(*args, diarize=False, **kw)
        off2.prepare(audio)
        assert same(off2.run(), out_off)
    finally:
        rec.close()
        emb.close()
        vib.close()
