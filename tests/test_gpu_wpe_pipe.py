"""FullPipe.prepare(..., wpe=True) on the MI355X: the pipe's decode reads the plan's chunks after
WPE dereverberation and the peak limiter, one device batch (zasr.audio.apply_wpe_batch), and its
words equal the host route's: each chunk processed alone, then a batch decode of the host chunks.
Off by default: without the switch the decode reads the signal itself."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    if not gpu_available():
        pytest.skip("no GPU")
    from zasr.binding import CamppEmbedder, Recognizer, VibertSession
    from zasr.campp import CamppConfig
    from zasr.campp import save_model_dir as campp_save
    from zasr.campp import synth_weights as campp_weights
    from zasr.model import save_model_dir, synth_tokens, synth_weights, zipformer_tiny
    from zasr.pipeline import FullPipe
    from zasr.vibert import save_model_dir as vib_save
    from zasr.vibert import synth_weights as vib_weights
    from zasr.vibert import vibert_tiny
    d = tmp_path_factory.mktemp("wpe_pipe")
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
    yield FullPipe(rec, recd, emb, vib, vcfg.vocab_size, beam=1, campp_batch=16)
    rec.close()
    emb.close()
    vib.close()


def test_pipe_with_wpe_equals_the_host_route(pipe):
    import torch

    from zasr import audio as za
    from zasr.asr_engine import result_words
    from zasr.merge import merge_chunks_with_overlap
    from zasr.synth_audio import synth_speech
    audio = (synth_speech(75.0, 33) * np.float32(1.5)).astype(np.float32)  # the limiter has work
    pipe.prepare(audio, wpe=True)
    assert len(pipe.c_off) >= 3 and pipe.d_decode is not pipe.d_audio
    words, tokens = pipe.decode_words(torch.cuda.current_stream().cuda_stream)
    chunks = []
    for a, n in zip(pipe.c_off, pipe.c_len):
        c = za.apply_wpe_dereverberation(audio[a:a + n].copy())
        chunks.append(np.asarray(za.adaptive_peak_limit(c)))
    packed = pipe.d_decode.cpu().numpy()
    assert packed.tobytes() == np.concatenate(chunks).tobytes()
    assert any(c.tobytes() != audio[a:a + n].tobytes() for c, a, n in zip(chunks, pipe.c_off, pipe.c_len))
    res = pipe.rec.decode(chunks, beam=1)
    per = [{"words": result_words(pipe.recd, r, n, a / 16000.0), "audio_start_abs": a / 16000.0,
            "audio_end_abs": (a + n) / 16000.0} for r, a, n in zip(res, pipe.c_off, pipe.c_len)]
    want, _ = merge_chunks_with_overlap(per)
    assert tokens == sum(int(r.token_ids.size) for r in res) > 0
    assert [(w["text"], w["start"]) for w in words] == [(w["text"], w["start"]) for w in want]


def test_pipe_without_the_switch_reads_the_signal(pipe):
    from zasr.synth_audio import synth_speech
    pipe.prepare(synth_speech(40.0, 34))
    assert pipe.d_decode is pipe.d_audio and pipe.c_decode_off == pipe.c_off
