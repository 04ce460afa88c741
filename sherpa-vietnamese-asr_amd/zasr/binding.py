"""ctypes binding of libzasr.so (include/zasr.h).

This is the thin host layer the drop-in `core/asr_engine.py` sits on.  There is no CPU
fallback: if the shared library is missing or fails to load, construction raises.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
from typing import List, Optional, Sequence

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(_PKG, "lib", "libzasr.so")

# every symbol declared in include/zasr.h (the CPU test checks the .so exports them all)
EXPORTS = (
    "zasr_create", "zasr_destroy", "zasr_convert_model", "zasr_convert_stage_model", "zasr_fbank", "zasr_decode_batch", "zasr_decode_features",
    "zasr_decode_device", "zasr_decode_device_batches", "zasr_encode_features", "zasr_search_encoder_out",
    "zasr_result_count", "zasr_result_num_tokens", "zasr_result_num_frames",
    "zasr_result_tokens", "zasr_result_frames", "zasr_result_log_probs",
    "zasr_result_token_stats", "zasr_result_free", "zasr_vocab_size", "zasr_joiner_dim",
    "zasr_profile_enable", "zasr_profile_reset", "zasr_profile_report", "zasr_last_error",
    "zasr_version", "zasr_campp_create", "zasr_campp_destroy", "zasr_campp_embedding_dim",
    "zasr_campp_fbank", "zasr_campp_embed", "zasr_campp_embed_device", "zasr_campp_windows_device",
    "zasr_vibert_create", "zasr_vibert_destroy", "zasr_vibert_num_labels",
    "zasr_vibert_num_detect", "zasr_vibert_run",
    "zasr_vad_create", "zasr_vad_destroy", "zasr_vad_probs", "zasr_vad_probs_device",
    "zasr_vad_window", "zasr_vad_last_passes", "zasr_silence_flags",
    "zasr_seg_create", "zasr_seg_destroy", "zasr_seg_num_frames", "zasr_seg_logits",
    "zasr_seg_classes_device", "zasr_seg_num_chunks", "zasr_seg_last_group", "zasr_seg_set_group",
    "zasr_seg_set_profile", "zasr_seg_stage_ms", "zasr_seg_trim",
    "zasr_sep_create", "zasr_sep_destroy", "zasr_sep_min_samples", "zasr_sep_separate",
    "zasr_sep_separate_device", "zasr_sep_set_budget", "zasr_sep_last_groups", "zasr_sep_trim",
    "zasr_sep_set_profile", "zasr_sep_stage_ms",
    "zasr_emb_create", "zasr_emb_destroy", "zasr_emb_embedding_dim", "zasr_emb_num_feat_frames",
    "zasr_emb_encoder_flops", "zasr_emb_fbank", "zasr_emb_encode", "zasr_emb_chunks_device",
    "zasr_emb_segment", "zasr_emb_set_group", "zasr_emb_last_group", "zasr_emb_trim",
    "zasr_emb_set_profile", "zasr_emb_stage_ms",
    "zasr_selftest_emb_conv2d", "zasr_selftest_emb_pool",
    "zasr_create_stream", "zasr_destroy_stream", "zasr_stream_accept_waveform",
    "zasr_decode_stream", "zasr_decode_streams", "zasr_stream_is_decoded",
    "zasr_stream_num_tokens", "zasr_stream_num_frames", "zasr_stream_tokens",
    "zasr_stream_frames", "zasr_stream_log_probs", "zasr_stream_token_stats",
    "zasr_stream_result_json", "zasr_set_tokens", "zasr_model_routes",
    "zasr_fbank_set_mel_banks", "zasr_selftest_launch", "zasr_decode_host_batches",
    "zasr_selftest_gemm_h3r", "zasr_selftest_ffn_h3", "zasr_selftest_ffn_bf16",
    "zasr_selftest_attn_block_map", "zasr_selftest_seam", "zasr_selftest_ffn_bf16_oop",
    "zasr_selftest_ffn_h3_oop", "zasr_selftest_gemm", "zasr_selftest_joiner",
    "zasr_selftest_conv_gemm", "zasr_selftest_gemm_aload",
    "zasr_selftest_dwconv1d", "zasr_selftest_conv1", "zasr_selftest_convnext",
    "zasr_selftest_bias_norm", "zasr_selftest_attn_weights", "zasr_selftest_attn_sa",
    "zasr_selftest_nonlin", "zasr_selftest_search_step", "zasr_selftest_greedy_spec",
    "zasr_selftest_search_final", "zasr_selftest_hotword_dfa",
    "zasr_selftest_campp_conv2d", "zasr_selftest_campp_cam_mask", "zasr_selftest_campp_stats",
    "zasr_selftest_campp_cmvn", "zasr_selftest_campp_gather", "zasr_selftest_vad_frames",
    "zasr_selftest_vad_im2col", "zasr_selftest_vad_lstm", "zasr_selftest_vibert_ln",
    "zasr_selftest_vibert_attn", "zasr_selftest_vibert_gather",
    "zasr_selftest_seg_chunk_stats", "zasr_selftest_seg_front", "zasr_selftest_seg_pool3",
    "zasr_selftest_seg_frame_stats", "zasr_selftest_seg_norm_act", "zasr_selftest_seg_lstm",
    "zasr_selftest_seg_head", "zasr_selftest_sep_frames", "zasr_selftest_sep_tile_sums",
    "zasr_selftest_sep_region_stats", "zasr_selftest_sep_gln_apply", "zasr_selftest_sep_mid",
    "zasr_selftest_sep_prelu", "zasr_selftest_sep_overlap_add",
    "zasr_audio_create", "zasr_audio_destroy", "zasr_audio_out_len", "zasr_audio_resample_taps",
    "zasr_audio_to_16k", "zasr_audio_peak", "zasr_audio_scale", "zasr_audio_segment_sumsq",
    "zasr_audio_apply_gain",
    "zasr_wpe_create", "zasr_wpe_destroy", "zasr_wpe_frames", "zasr_wpe_run_device", "zasr_wpe_run",
    "zasr_wpe_set_budget", "zasr_wpe_last_groups", "zasr_wpe_trim", "zasr_wpe_set_profile",
    "zasr_wpe_stage_ms", "zasr_selftest_wpe_stft", "zasr_selftest_wpe_iter",
    "zasr_selftest_wpe_istft",
    "zasr_diar_create", "zasr_diar_destroy", "zasr_diar_similarity", "zasr_diar_prune",
    "zasr_diar_eigs", "zasr_diar_spectral_embed", "zasr_diar_last_stats",
    "zasr_clu_create", "zasr_clu_destroy", "zasr_clu_ahc", "zasr_clu_last_stats",
    "zasr_clu_set_profile", "zasr_clu_stage_ms", "zasr_selftest_clu_route",
)


# include/zasr.h ZASR_PRECISION_*: "bf16_enc" = the bf16 encoder with the f32 joiner + search;
# "bf16x3" / "bf16x6" = f32 storage, split-bf16 products (2 / 3 pieces per operand) on the
# bf16 MFMA
PRECISIONS = {"fp32": 0, "bf16": 1, "bf16_enc": 2, "bf16x3": 3, "bf16x6": 4, "f16x3": 5}


C_FP = C.POINTER(C.c_float)


class ZasrError(RuntimeError):
    pass


class _Config(C.Structure):
    _fields_ = [
        ("model_dir", C.c_char_p),
        ("decoding_method", C.c_char_p),
        ("max_active_paths", C.c_int32),
        ("blank_penalty", C.c_float),
        ("hotword_tokens", C.POINTER(C.c_int32)),
        ("hotword_lens", C.POINTER(C.c_int32)),
        ("hotword_scores", C.POINTER(C.c_float)),
        ("num_hotwords", C.c_int32),
        ("device_id", C.c_int32),
        ("precision", C.c_int32),
    ]


class _StState(C.Structure):  # include/zasr.h zasr_st_state
    _fields_ = [("S", C.c_int32), ("Hmax", C.c_int32), ("node_cap", C.c_int32)] + [
        (n, C.c_void_p) for n in ("lp", "lpf", "hash", "len", "y1", "y2", "hw", "node", "nh",
                                  "node_tok", "node_frame", "node_parent", "node_lp",
                                  "node_stats", "node_count")]


class _StHotwords(C.Structure):
    _fields_ = [("tokens", C.c_void_p), ("lens", C.c_void_p), ("scores", C.c_void_p),
                ("n", C.c_int32)]


class _StTable(C.Structure):
    _fields_ = [("D", C.c_int32), ("jfmt", C.c_int32), ("enc_rows", C.c_int32),
                ("a", C.c_void_p), ("b", C.c_void_p), ("enc", C.c_void_p),
                ("enc_off", C.c_void_p), ("J", C.c_void_p), ("j_bytes", C.c_int64)]


class _SepCall(C.Structure):  # include/zasr.h zasr_sep_call
    _fields_ = [("n_regions", C.c_int32), ("sig_off", C.POINTER(C.c_int64)),
                ("T", C.POINTER(C.c_int32)), ("r0", C.c_int32), ("ng", C.c_int32),
                ("win", C.c_int32), ("hop", C.c_int32)]


_lib = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load libzasr.so (raises if absent: the product has no fallback path)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("ZASR_LIB", DEFAULT_LIB)
    if not os.path.exists(p):
        raise ZasrError(f"libzasr.so not found at {p}; build it with "
                        f"`make -C sherpa-vietnamese-asr_amd/csrc` (or __graft_entry__.build())")
    lib = C.CDLL(p)
    P, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    fp = C.POINTER(C.c_float)
    lib.zasr_create.argtypes = [C.POINTER(_Config), C.POINTER(P)]
    lib.zasr_create.restype = C.c_int
    lib.zasr_destroy.argtypes = [P]
    lib.zasr_destroy.restype = None
    lib.zasr_convert_model.argtypes = [C.c_char_p, C.c_char_p]
    lib.zasr_convert_model.restype = C.c_int
    lib.zasr_convert_stage_model.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
    lib.zasr_convert_stage_model.restype = C.c_int
    lib.zasr_fbank.argtypes = [P, fp, I64, I32, fp, I64, C.POINTER(I64)]
    lib.zasr_fbank.restype = C.c_int
    lib.zasr_decode_batch.argtypes = [P, C.POINTER(fp), C.POINTER(I64), I32, I32, C.POINTER(P)]
    lib.zasr_decode_batch.restype = C.c_int
    lib.zasr_decode_features.argtypes = [P, C.POINTER(fp), C.POINTER(I64), I32, I32, C.POINTER(P)]
    lib.zasr_decode_features.restype = C.c_int
    lib.zasr_decode_device.argtypes = [P, P, C.POINTER(I64), C.POINTER(I64), I32, I32, P,
                                       C.POINTER(P)]
    lib.zasr_decode_device.restype = C.c_int
    lib.zasr_decode_device_batches.argtypes = [P, P, C.POINTER(I64), C.POINTER(I64), I32,
                                               C.POINTER(I32), I32, I32, P, C.POINTER(P)]
    lib.zasr_decode_device_batches.restype = C.c_int
    lib.zasr_decode_host_batches.argtypes = [P, P, C.POINTER(I64), C.POINTER(I64), I32,
                                             C.POINTER(I32), I32, I32, P, C.POINTER(P)]
    lib.zasr_decode_host_batches.restype = C.c_int
    lib.zasr_encode_features.argtypes = [P, C.POINTER(fp), C.POINTER(I64), I32, fp, I64,
                                         C.POINTER(I64)]
    lib.zasr_encode_features.restype = C.c_int
    lib.zasr_search_encoder_out.argtypes = [P, C.POINTER(fp), C.POINTER(I64), I32, I32,
                                            C.POINTER(P)]
    lib.zasr_search_encoder_out.restype = C.c_int
    for n in ("zasr_result_count",):
        getattr(lib, n).argtypes = [P]
        getattr(lib, n).restype = I32
    for n in ("zasr_result_num_tokens", "zasr_result_num_frames"):
        getattr(lib, n).argtypes = [P, I32]
        getattr(lib, n).restype = I32
    lib.zasr_result_tokens.argtypes = [P, I32]
    lib.zasr_result_tokens.restype = C.POINTER(I32)
    lib.zasr_result_frames.argtypes = [P, I32]
    lib.zasr_result_frames.restype = C.POINTER(I32)
    lib.zasr_result_log_probs.argtypes = [P, I32]
    lib.zasr_result_log_probs.restype = C.POINTER(C.c_double)
    lib.zasr_result_token_stats.argtypes = [P, I32]
    lib.zasr_result_token_stats.restype = fp
    lib.zasr_result_free.argtypes = [P]
    lib.zasr_result_free.restype = None
    lib.zasr_vocab_size.argtypes = [P]
    lib.zasr_vocab_size.restype = I32
    lib.zasr_joiner_dim.argtypes = [P]
    lib.zasr_joiner_dim.restype = I32
    lib.zasr_profile_enable.argtypes = [P, I32]
    lib.zasr_profile_enable.restype = C.c_int
    lib.zasr_profile_reset.argtypes = [P]
    lib.zasr_profile_reset.restype = C.c_int
    lib.zasr_profile_report.argtypes = [P, C.c_char_p, I64]
    lib.zasr_profile_report.restype = C.c_int
    lib.zasr_last_error.argtypes = []
    lib.zasr_last_error.restype = C.c_char_p
    lib.zasr_version.argtypes = []
    lib.zasr_version.restype = C.c_char_p
    lib.zasr_campp_create.argtypes = [C.c_char_p, I32, C.POINTER(P)]
    lib.zasr_campp_create.restype = C.c_int
    lib.zasr_campp_destroy.argtypes = [P]
    lib.zasr_campp_destroy.restype = None
    lib.zasr_campp_embedding_dim.argtypes = [P]
    lib.zasr_campp_embedding_dim.restype = I32
    lib.zasr_campp_fbank.argtypes = [P, fp, I64, fp, I64, C.POINTER(I64)]
    lib.zasr_campp_fbank.restype = C.c_int
    lib.zasr_campp_embed.argtypes = [P, fp, I32, I32, fp]
    lib.zasr_campp_embed.restype = C.c_int
    lib.zasr_campp_embed_device.argtypes = [P, P, I32, I32, P, P]
    lib.zasr_campp_embed_device.restype = C.c_int
    i32p = C.POINTER(I32)
    lib.zasr_campp_windows_device.argtypes = [P, P, C.POINTER(I64), C.POINTER(I64), I32, I32, I32,
                                              P, I64, i32p, i32p, i32p, C.POINTER(I64), P]
    lib.zasr_campp_windows_device.restype = C.c_int
    lib.zasr_vibert_create.argtypes = [C.c_char_p, I32, C.POINTER(P)]
    lib.zasr_vibert_create.restype = C.c_int
    lib.zasr_vibert_destroy.argtypes = [P]
    lib.zasr_vibert_destroy.restype = None
    for n in ("zasr_vibert_num_labels", "zasr_vibert_num_detect"):
        getattr(lib, n).argtypes = [P]
        getattr(lib, n).restype = I32
    i64p = C.POINTER(I64)
    lib.zasr_vibert_run.argtypes = [P, i64p, i64p, i64p, i64p, I32, I32, I32, fp, fp]
    lib.zasr_vibert_run.restype = C.c_int
    lib.zasr_vad_create.argtypes = [C.c_char_p, I32, C.POINTER(P)]
    lib.zasr_vad_create.restype = C.c_int
    lib.zasr_vad_destroy.argtypes = [P]
    lib.zasr_vad_destroy.restype = None
    lib.zasr_vad_probs.argtypes = [P, fp, i64p, i64p, I32, I32, fp]
    lib.zasr_vad_probs.restype = C.c_int
    lib.zasr_vad_probs_device.argtypes = [P, P, i64p, i64p, I32, I32, P, P]
    lib.zasr_vad_probs_device.restype = C.c_int
    lib.zasr_vad_window.argtypes = [P, fp, fp, I32, fp, fp]
    lib.zasr_vad_window.restype = C.c_int
    lib.zasr_vad_last_passes.argtypes = [P]
    lib.zasr_vad_last_passes.restype = I32
    lib.zasr_seg_create.argtypes = [C.c_char_p, I32, C.POINTER(P)]
    lib.zasr_seg_create.restype = C.c_int
    lib.zasr_seg_destroy.argtypes = [P]
    lib.zasr_seg_destroy.restype = None
    lib.zasr_seg_num_frames.argtypes = [P, I64]
    lib.zasr_seg_num_frames.restype = I32
    lib.zasr_seg_logits.argtypes = [P, fp, I32, I32, fp]
    lib.zasr_seg_logits.restype = C.c_int
    lib.zasr_seg_classes_device.argtypes = [P, P, I64, I32, I32, C.POINTER(C.c_uint8), P, P]
    lib.zasr_seg_classes_device.restype = C.c_int
    lib.zasr_seg_num_chunks.argtypes = [I64, I32, I32]
    lib.zasr_seg_num_chunks.restype = I64
    lib.zasr_seg_last_group.argtypes = [P]
    lib.zasr_seg_last_group.restype = I32
    lib.zasr_seg_set_group.argtypes = [P, I32]
    lib.zasr_seg_set_group.restype = C.c_int
    lib.zasr_seg_trim.argtypes = [P]
    lib.zasr_seg_trim.restype = C.c_int
    lib.zasr_seg_set_profile.argtypes = [P, I32]
    lib.zasr_seg_set_profile.restype = C.c_int
    lib.zasr_seg_stage_ms.argtypes = [P, fp]
    lib.zasr_seg_stage_ms.restype = C.c_int
    lib.zasr_sep_create.argtypes = [C.c_char_p, I32, C.POINTER(P)]
    lib.zasr_sep_create.restype = C.c_int
    lib.zasr_sep_destroy.argtypes = [P]
    lib.zasr_sep_destroy.restype = None
    lib.zasr_sep_min_samples.argtypes = [P]
    lib.zasr_sep_min_samples.restype = I32
    lib.zasr_sep_separate.argtypes = [P, fp, I64, C.POINTER(I64), C.POINTER(I64), I32, fp]
    lib.zasr_sep_separate.restype = C.c_int
    lib.zasr_sep_separate_device.argtypes = [P, P, I64, C.POINTER(I64), C.POINTER(I64), I32, P, I32, P]
    lib.zasr_sep_separate_device.restype = C.c_int
    lib.zasr_sep_set_budget.argtypes = [P, I64]
    lib.zasr_sep_set_budget.restype = C.c_int
    lib.zasr_sep_last_groups.argtypes = [P]
    lib.zasr_sep_last_groups.restype = I32
    lib.zasr_sep_trim.argtypes = [P]
    lib.zasr_sep_trim.restype = C.c_int
    lib.zasr_sep_set_profile.argtypes = [P, I32]
    lib.zasr_sep_set_profile.restype = C.c_int
    lib.zasr_sep_stage_ms.argtypes = [P, fp]
    lib.zasr_sep_stage_ms.restype = C.c_int
    lib.zasr_emb_create.argtypes = [C.c_char_p, I32, C.POINTER(P)]
    lib.zasr_emb_create.restype = C.c_int
    lib.zasr_emb_destroy.argtypes = [P]
    lib.zasr_emb_destroy.restype = None
    lib.zasr_emb_embedding_dim.argtypes = [P]
    lib.zasr_emb_embedding_dim.restype = I32
    lib.zasr_emb_num_feat_frames.argtypes = [P, I32]
    lib.zasr_emb_num_feat_frames.restype = I32
    lib.zasr_emb_encoder_flops.argtypes = [P, I32]
    lib.zasr_emb_encoder_flops.restype = C.c_double
    lib.zasr_emb_fbank.argtypes = [P, fp, I64, I64, fp, I64, C.POINTER(I64)]
    lib.zasr_emb_fbank.restype = C.c_int
    lib.zasr_emb_encode.argtypes = [P, fp, I32, I32, fp]
    lib.zasr_emb_encode.restype = C.c_int
    lib.zasr_emb_chunks_device.argtypes = [P, P, I64, C.POINTER(I64), I32, C.POINTER(C.c_uint8), I32, fp, P]
    lib.zasr_emb_chunks_device.restype = C.c_int
    lib.zasr_emb_segment.argtypes = [P, fp, I64, fp, C.POINTER(I32)]
    lib.zasr_emb_segment.restype = C.c_int
    lib.zasr_emb_set_group.argtypes = [P, I32]
    lib.zasr_emb_set_group.restype = C.c_int
    lib.zasr_emb_last_group.argtypes = [P]
    lib.zasr_emb_last_group.restype = I32
    lib.zasr_emb_trim.argtypes = [P]
    lib.zasr_emb_trim.restype = C.c_int
    lib.zasr_emb_set_profile.argtypes = [P, I32]
    lib.zasr_emb_set_profile.restype = C.c_int
    lib.zasr_emb_stage_ms.argtypes = [P, fp]
    lib.zasr_emb_stage_ms.restype = C.c_int
    lib.zasr_selftest_emb_conv2d.argtypes = [I32] * 9 + [fp, fp, fp, fp, fp, C.POINTER(I32)]
    lib.zasr_selftest_emb_conv2d.restype = C.c_int
    lib.zasr_selftest_emb_pool.argtypes = [I32] * 7 + [fp, C.POINTER(C.c_uint8), fp]
    lib.zasr_selftest_emb_pool.restype = C.c_int
    lib.zasr_silence_flags.argtypes = [P, I64, I32, C.c_float, P, P]
    lib.zasr_silence_flags.restype = C.c_int
    # offline streams (the sherpa-onnx OfflineStream surface, zasr/offline.py)
    lib.zasr_create_stream.argtypes = [P, C.POINTER(P)]
    lib.zasr_create_stream.restype = C.c_int
    lib.zasr_destroy_stream.argtypes = [P]
    lib.zasr_destroy_stream.restype = None
    lib.zasr_stream_accept_waveform.argtypes = [P, I32, fp, I64]
    lib.zasr_stream_accept_waveform.restype = C.c_int
    lib.zasr_decode_stream.argtypes = [P, P]
    lib.zasr_decode_stream.restype = C.c_int
    lib.zasr_decode_streams.argtypes = [P, C.POINTER(P), I32]
    lib.zasr_decode_streams.restype = C.c_int
    for n in ("zasr_stream_is_decoded", "zasr_stream_num_tokens", "zasr_stream_num_frames"):
        getattr(lib, n).argtypes = [P]
        getattr(lib, n).restype = I32
    lib.zasr_stream_tokens.argtypes = [P]
    lib.zasr_stream_tokens.restype = C.POINTER(I32)
    lib.zasr_stream_frames.argtypes = [P]
    lib.zasr_stream_frames.restype = C.POINTER(I32)
    lib.zasr_stream_log_probs.argtypes = [P]
    lib.zasr_stream_log_probs.restype = C.POINTER(C.c_double)
    lib.zasr_stream_token_stats.argtypes = [P]
    lib.zasr_stream_token_stats.restype = fp
    lib.zasr_stream_result_json.argtypes = [P, C.c_char_p, I64, C.POINTER(I64)]
    lib.zasr_stream_result_json.restype = C.c_int
    lib.zasr_set_tokens.argtypes = [P, C.c_char_p]
    lib.zasr_set_tokens.restype = C.c_int
    lib.zasr_model_routes.argtypes = [P, C.c_char_p, I64]
    lib.zasr_model_routes.restype = C.c_int
    lib.zasr_fbank_set_mel_banks.argtypes = [P, fp, I32]
    lib.zasr_fbank_set_mel_banks.restype = C.c_int
    lib.zasr_selftest_launch.argtypes = [I32]
    lib.zasr_selftest_launch.restype = C.c_int
    lib.zasr_selftest_gemm_h3r.argtypes = [I32, I32, I32, I32, fp, fp, fp, fp]
    lib.zasr_selftest_gemm_h3r.restype = C.c_int
    lib.zasr_selftest_gemm.argtypes = [I32] * 7 + [fp] * 7
    lib.zasr_selftest_gemm.restype = C.c_int
    lib.zasr_selftest_conv_gemm.argtypes = [I32] * 5 + [C.POINTER(I32)] + [fp] * 4
    lib.zasr_selftest_conv_gemm.restype = C.c_int
    lib.zasr_selftest_gemm_aload.argtypes = [I32] * 8 + [fp] * 5 + [I32] * 6 + [fp, I32, fp]
    lib.zasr_selftest_gemm_aload.restype = C.c_int
    lib.zasr_selftest_joiner.argtypes = [I32] * 5 + [fp] * 3 + [C.POINTER(I32)] * 2 + [I32, fp]
    lib.zasr_selftest_joiner.restype = C.c_int
    lib.zasr_selftest_ffn_h3.argtypes = [I32, I32, I32, fp, fp, fp, fp, fp, fp, fp, fp]
    lib.zasr_selftest_ffn_h3.restype = C.c_int
    lib.zasr_selftest_ffn_bf16.argtypes = [I32, I32, I32, fp, fp, fp, fp, fp, fp, fp, I32]
    lib.zasr_selftest_ffn_bf16.restype = C.c_int
    lib.zasr_selftest_attn_block_map.argtypes = [C.POINTER(I32), I32, I32, I32,
                                                 C.POINTER(C.c_uint32), I64, C.POINTER(I32)]
    lib.zasr_selftest_attn_block_map.restype = C.c_int
    lib.zasr_selftest_seam.argtypes = [I32, C.POINTER(I32)] + [I32] * 6 + [fp] * 11
    lib.zasr_selftest_seam.restype = C.c_int
    lib.zasr_selftest_ffn_bf16_oop.argtypes = [I32, I32, I32] + [fp] * 8 + [I32]
    lib.zasr_selftest_ffn_bf16_oop.restype = C.c_int
    lib.zasr_selftest_ffn_h3_oop.argtypes = [I32, I32, I32] + [fp] * 8
    lib.zasr_selftest_ffn_h3_oop.restype = C.c_int
    lib.zasr_selftest_dwconv1d.argtypes = [I32, C.POINTER(I32)] + [I32] * 4 + [fp] * 4
    lib.zasr_selftest_dwconv1d.restype = C.c_int
    lib.zasr_selftest_conv1.argtypes = [I32, C.POINTER(I32), I32] + [fp] * 4
    lib.zasr_selftest_conv1.restype = C.c_int
    lib.zasr_selftest_convnext.argtypes = [I32, C.POINTER(I32), I32] + [fp] * 9
    lib.zasr_selftest_convnext.restype = C.c_int
    lib.zasr_selftest_bias_norm.argtypes = [I32, I32, fp, C.c_float, fp, fp, I32, fp, fp]
    lib.zasr_selftest_bias_norm.restype = C.c_int
    lib.zasr_selftest_attn_weights.argtypes = [I32] * 3 + [C.POINTER(I32), I32] + [fp] * 3
    lib.zasr_selftest_attn_weights.restype = C.c_int
    lib.zasr_selftest_attn_sa.argtypes = [I32] * 3 + [C.POINTER(I32), I32] + [fp] * 7
    lib.zasr_selftest_attn_sa.restype = C.c_int
    lib.zasr_selftest_nonlin.argtypes = [I32] * 3 + [C.POINTER(I32), I32, I32] + [fp] * 3 + [
        C.POINTER(C.c_uint16), fp]
    lib.zasr_selftest_nonlin.restype = C.c_int
    sp, hp, tp = C.POINTER(_StState), C.POINTER(_StHotwords), C.POINTER(_StTable)
    ip32 = C.POINTER(I32)
    lib.zasr_selftest_search_step.argtypes = [I32, I32, I32, ip32, sp, fp, hp, tp]
    lib.zasr_selftest_search_step.restype = C.c_int
    lib.zasr_selftest_greedy_spec.argtypes = [I32] * 4 + [ip32] * 3 + [sp, fp, hp, tp]
    lib.zasr_selftest_greedy_spec.restype = C.c_int
    lib.zasr_selftest_search_final.argtypes = [I32, sp, hp, I32, ip32, ip32,
                                               C.POINTER(C.c_double), fp, ip32]
    lib.zasr_selftest_search_final.restype = C.c_int
    lib.zasr_selftest_hotword_dfa.argtypes = [I32, hp, I32, ip32, ip32, ip32, ip32,
                                              C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.zasr_selftest_hotword_dfa.restype = C.c_int
    ip64 = C.POINTER(I64)
    lib.zasr_selftest_campp_conv2d.argtypes = [I32] * 11 + [fp] * 6 + [ip32, ip32]
    lib.zasr_selftest_campp_cam_mask.argtypes = [I32] * 3 + [fp] * 6
    lib.zasr_selftest_campp_stats.argtypes = [I32] * 3 + [fp] * 4
    lib.zasr_selftest_campp_cmvn.argtypes = [I32, I32, ip32, fp]
    lib.zasr_selftest_campp_gather.argtypes = [I32, I32, I32, fp, ip32, ip32, fp]
    lib.zasr_selftest_vad_frames.argtypes = [I32, I64, I64, fp, ip64, ip64, ip64, fp,
                                             C.POINTER(C.c_uint32), fp]
    lib.zasr_selftest_vad_im2col.argtypes = [I32, I64] + [I32] * 5 + [fp, fp]
    lib.zasr_selftest_vad_lstm.argtypes = [I64, I32, fp, fp, fp, fp, C.c_float, ip64, ip32, ip32,
                                           fp, fp, fp, fp]
    lib.zasr_selftest_vibert_ln.argtypes = [I64, I32, I32, ip64, ip64, I32, I32, I32] + [fp] * 5 + [
        C.c_float, fp]
    lib.zasr_selftest_vibert_attn.argtypes = [I32] * 4 + [fp, ip64, fp]
    lib.zasr_selftest_vibert_gather.argtypes = [I32] * 4 + [fp, ip64, fp]
    for _n in ("campp_conv2d", "campp_cam_mask", "campp_stats", "campp_cmvn", "campp_gather",
               "vad_frames", "vad_im2col", "vad_lstm", "vibert_ln", "vibert_attn", "vibert_gather"):
        getattr(lib, "zasr_selftest_" + _n).restype = C.c_int
    dp, u8p, cp, fl = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(_SepCall), C.c_float
    for _n, _a in (("seg_chunk_stats", [I64, I32, I32, fp, ip64, fp]),
                   ("seg_front", [I64, I32, I32, fp, ip64, fp, fl, fl, fp, fp]),
                   ("seg_pool3", [I32] * 5 + [fp, fp]),
                   ("seg_frame_stats", [I32] * 3 + [fp, fp]),
                   ("seg_norm_act", [I32] * 4 + [fp] * 4),
                   ("seg_lstm", [I32] * 3 + [fp] * 3),
                   ("seg_head", [I64, fp, fp, fp, fp, u8p]),
                   ("sep_frames", [cp, I64, fp, fp]),
                   ("sep_tile_sums", [cp, I32, fp, dp]),
                   ("sep_region_stats", [cp, I32, dp, fp]),
                   ("sep_gln_apply", [cp, I32, I32] + [fp] * 5),
                   ("sep_mid", [cp, I32, I32, fl] + [fp] * 7 + [dp]),
                   ("sep_prelu", [I64, I32, I32, I32, fl, I32, fp]),
                   ("sep_overlap_add", [cp, ip64, I64, fp, fp, fp])):
        getattr(lib, "zasr_selftest_" + _n).argtypes = _a
        getattr(lib, "zasr_selftest_" + _n).restype = C.c_int
    # device audio front end (zasr/audio.py)
    lib.zasr_audio_create.argtypes = [I32, C.POINTER(P)]
    lib.zasr_audio_create.restype = C.c_int
    lib.zasr_audio_destroy.argtypes = [P]
    lib.zasr_audio_destroy.restype = None
    lib.zasr_audio_out_len.argtypes = [I32, I64]
    lib.zasr_audio_out_len.restype = I64
    lib.zasr_audio_resample_taps.argtypes = [I32, i32p, i32p, i32p, i32p, i32p, i32p, fp, I64]
    lib.zasr_audio_resample_taps.restype = C.c_int
    lib.zasr_audio_to_16k.argtypes = [P, P, I32, I32, I32, I64, I32, P, I64, i64p, P]
    lib.zasr_audio_to_16k.restype = C.c_int
    lib.zasr_audio_peak.argtypes = [P, P, I64, fp, P]
    lib.zasr_audio_peak.restype = C.c_int
    lib.zasr_audio_scale.argtypes = [P, P, I64, C.c_float, C.c_float, P]
    lib.zasr_audio_scale.restype = C.c_int
    lib.zasr_audio_segment_sumsq.argtypes = [P, P, I64, i64p, i64p, I32, C.POINTER(C.c_double), P]
    lib.zasr_audio_segment_sumsq.restype = C.c_int
    lib.zasr_audio_apply_gain.argtypes = [P, P, I64, i64p, i64p, fp, i64p, I32, fp, I64, fp, P]
    lib.zasr_audio_apply_gain.restype = C.c_int
    # WPE dereverberation (zasr/audio.py)
    dp, DBL = C.POINTER(C.c_double), C.c_double
    lib.zasr_wpe_create.argtypes = [I32, C.POINTER(P)]
    lib.zasr_wpe_destroy.argtypes = [P]
    lib.zasr_wpe_destroy.restype = None
    lib.zasr_wpe_frames.argtypes = [I64]
    lib.zasr_wpe_frames.restype = I64
    lib.zasr_wpe_run_device.argtypes = [P, P, I64, i64p, i64p, I32, I32, I32, I32, P, i64p, P]
    lib.zasr_wpe_run.argtypes = [P, fp, I64, i64p, i64p, I32, I32, I32, I32, fp, i64p]
    lib.zasr_wpe_set_budget.argtypes = [P, I64]
    lib.zasr_wpe_last_groups.argtypes = [P]
    lib.zasr_wpe_last_groups.restype = I32
    lib.zasr_wpe_trim.argtypes = [P]
    lib.zasr_wpe_set_profile.argtypes = [P, I32]
    lib.zasr_wpe_stage_ms.argtypes = [P, fp]
    lib.zasr_selftest_wpe_stft.argtypes = [P, fp, I64, fp, fp]
    lib.zasr_selftest_wpe_iter.argtypes = [P, fp, I32, I32, I32, C.c_float, dp, dp, fp, fp]
    lib.zasr_selftest_wpe_istft.argtypes = [P, fp, I32, I64, fp]
    for _n in ("wpe_create", "wpe_run_device", "wpe_run", "wpe_set_budget", "wpe_trim",
               "wpe_set_profile", "wpe_stage_ms", "selftest_wpe_stft", "selftest_wpe_iter",
               "selftest_wpe_istft"):
        getattr(lib, "zasr_" + _n).restype = C.c_int
    lib.zasr_diar_create.argtypes = [I32, C.POINTER(P)]
    lib.zasr_diar_create.restype = C.c_int
    lib.zasr_diar_destroy.argtypes = [P]
    lib.zasr_diar_destroy.restype = None
    lib.zasr_diar_similarity.argtypes = [P, P, I32, I32, P, P]
    lib.zasr_diar_similarity.restype = C.c_int
    lib.zasr_diar_prune.argtypes = [P, P, I32, DBL, I32, P, P]
    lib.zasr_diar_prune.restype = C.c_int
    lib.zasr_diar_eigs.argtypes = [P, P, P, I32, I32, dp, dp, i32p, P]
    lib.zasr_diar_eigs.restype = C.c_int
    lib.zasr_diar_spectral_embed.argtypes = [P, P, I32, I32, I32, DBL, I32, I32, dp, dp, P]
    lib.zasr_diar_spectral_embed.restype = C.c_int
    lib.zasr_diar_last_stats.argtypes = [P, i32p, i64p]
    lib.zasr_diar_last_stats.restype = C.c_int
    lib.zasr_clu_create.argtypes = [I32, C.POINTER(P)]
    lib.zasr_clu_create.restype = C.c_int
    lib.zasr_clu_destroy.argtypes = [P]
    lib.zasr_clu_destroy.restype = None
    lib.zasr_clu_ahc.argtypes = [P, P, I32, I32, I32, DBL, P, P]
    lib.zasr_clu_ahc.restype = C.c_int
    lib.zasr_clu_last_stats.argtypes = [P, i64p, i64p]
    lib.zasr_clu_last_stats.restype = C.c_int
    lib.zasr_clu_set_profile.argtypes = [P, I32]
    lib.zasr_clu_set_profile.restype = C.c_int
    lib.zasr_clu_stage_ms.argtypes = [P, fp]
    lib.zasr_clu_stage_ms.restype = C.c_int
    lib.zasr_selftest_clu_route.argtypes = [P, I32, i32p]
    lib.zasr_selftest_clu_route.restype = C.c_int
    if path is None:
        _lib = lib
    return lib


def convert_model(model_dir: str, out_dir: str, lib_path: Optional[str] = None) -> None:
    """Host-only load of a model directory (config.json + model.safetensors, or the
    reference's encoder-/decoder-/joiner-*.onnx) through libzasr's loader, written as
    out_dir/config.json + out_dir/model.safetensors (include/zasr.h zasr_convert_model)."""
    lib = load_library(lib_path)
    os.makedirs(out_dir, exist_ok=True)
    rc = lib.zasr_convert_model(model_dir.encode(), out_dir.encode())
    if rc != 0:
        msg = lib.zasr_last_error().decode()
        if rc == 2:
            raise FileNotFoundError(msg)
        raise ZasrError(msg)


def convert_stage_model(kind: str, model_dir: str, out_dir: str,
                        lib_path: Optional[str] = None) -> None:
    """Host-only load of a Silero VAD / CAM++ / ViBERT model directory (the reference's .onnx
    or the engine's own files) through libzasr's reader, written as out_dir/<kind>_config.json
    + the engine's safetensors file (include/zasr.h zasr_convert_stage_model)."""
    lib = load_library(lib_path)
    os.makedirs(out_dir, exist_ok=True)
    rc = lib.zasr_convert_stage_model(kind.encode(), model_dir.encode(), out_dir.encode())
    if rc != 0:
        msg = lib.zasr_last_error().decode()
        if rc == 2:
            raise FileNotFoundError(msg)
        raise ZasrError(msg)


def selftest_launch(block_threads: int, lib_path: Optional[str] = None) -> None:
    """A no-op kernel of block_threads threads through the library's checked launch path
    (include/zasr.h zasr_selftest_launch): an invalid configuration raises ZasrError."""
    lib = load_library(lib_path)
    rc = lib.zasr_selftest_launch(int(block_threads))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())


def selftest_gemm_h3r(A, W, bias, C, epi: int = 0, lib_path: Optional[str] = None) -> np.ndarray:
    """gemm_h3r_kernel alone on host operands (zasr_selftest_gemm_h3r): returns C after
    C = epi(A W^T + bias) (epi 3: C += ..., 8: GLU over interleaved rows)."""
    lib = load_library(lib_path)
    A, W, C = _f32(A), _f32(W), _f32(C).copy()
    b = None if bias is None else _f32(bias)
    p = lambda x: None if x is None else x.ctypes.data_as(C_FP)
    rc = lib.zasr_selftest_gemm_h3r(A.shape[0], A.shape[1], W.shape[0], int(epi), p(A), p(W),
                                    p(b), p(C))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return C


def selftest_gemm(mode: str, A, W, bias, C, epi: int = 0, a_bf16: bool = False,
                  c_bf16: bool = False, aux=None, byp_orig=None, byp_scale=None,
                  lib_path: Optional[str] = None) -> np.ndarray:
    """gemm_f32 / gemm_bf16 / gemm_x3 alone on one dense host problem (zasr_selftest_gemm;
    mode: a PRECISIONS name): returns C after C = epi(A W^T + bias) as float32."""
    lib = load_library(lib_path)
    A, W, C = _f32(A), _f32(W), _f32(C).copy()
    opt = [None if x is None else _f32(x) for x in (bias, aux, byp_orig, byp_scale)]
    p = lambda x: None if x is None else x.ctypes.data_as(C_FP)
    rc = lib.zasr_selftest_gemm(PRECISIONS[mode], A.shape[0], A.shape[1], W.shape[0], int(epi),
                                int(a_bf16), int(c_bf16), p(A), p(W), *(p(x) for x in opt), p(C))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return C


def conv_gemm_shapes(which: int, T):
    """(A shape, W shape, C shape) of zasr_selftest_conv_gemm for conv.4 / conv.7 on fbank
    lengths T."""
    T = _lens(T)
    t1, l2, L = int((T - 2).sum()), int(((T - 3) // 2).sum()), int(((T - 7) // 2).sum())
    if which == 4:
        return (t1, 80, 8), (32, 72), (l2, 39, 32)
    return (l2, 39, 32), (128, 288), (L, 19, 128)


def selftest_conv_gemm(mode: str, which: int, T, A, W, bias, a_bf16: bool = False,
                       c_bf16: bool = False, fill: float = -777.25,
                       lib_path: Optional[str] = None) -> np.ndarray:
    """conv.4 / conv.7 + SwooshR for a ragged batch as a decode launches them
    (zasr_selftest_conv_gemm; mode: a PRECISIONS name; T: fbank frames per sequence): A, W
    (k = (kt * 3 + kf) * channels + c), bias as conv_gemm_shapes gives them; returns C, which
    started as `fill`, as float32."""
    lib = load_library(lib_path)
    T, A, W, bias = _lens(T), _f32(A), _f32(W), _f32(bias)
    out = None
    if which in (4, 7) and len(T) and int(T.min()) >= 9:
        sa, sw, sc = conv_gemm_shapes(which, T)
        assert A.shape == sa and W.shape == sw and bias.shape == (sw[0],)
        out = np.full(sc, fill, dtype=np.float32)
    else:  # a refusal under test: the library answers before it reads an operand
        out = np.full((1,), fill, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C_FP)
    rc = lib.zasr_selftest_conv_gemm(PRECISIONS[mode], int(which), int(a_bf16), int(c_bf16), len(T),
                                     T.ctypes.data_as(C.POINTER(C.c_int32)), p(A), p(W), p(bias),
                                     p(out))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return out


def selftest_gemm_aload(aload: int, A, W, bias, C, M: int, lda: int, epi: int = 0, c_col: int = 0,
                        a_scale=None, a_shift=None, i2c=(0, 0, 0, 1, 1, 0), aux=None,
                        lib_path: Optional[str] = None) -> np.ndarray:
    """One gemm_f32 problem behind ALOAD_BNRELU (aload 4) or ALOAD_IM2COL1D (5)
    (zasr_selftest_gemm_aload): A [rows][lda], W [N][K], C [M][ldc] whole, the GEMM writing its
    columns [c_col, c_col + N); i2c = (Tin, Tout, C, stride, dil, pad); aux [M][ldaux] for the
    multiply epilogue.  Returns C's image afterwards."""
    lib = load_library(lib_path)
    A, W, C_ = _f32(A), _f32(W), _f32(C).copy()
    opt = [None if x is None else _f32(x) for x in (bias, a_scale, a_shift, aux)]
    assert A.ndim == 2 and A.shape[1] == lda and C_.shape[0] == M
    p = lambda x: None if x is None else x.ctypes.data_as(C_FP)
    ldaux = 0 if opt[3] is None else opt[3].shape[1]
    rc = lib.zasr_selftest_gemm_aload(int(aload), int(M), W.shape[1], W.shape[0], int(lda),
                                      C_.shape[1], int(c_col), int(epi), p(A), p(W), p(opt[0]),
                                      p(opt[1]), p(opt[2]), *(int(v) for v in i2c), p(opt[3]),
                                      ldaux, p(C_))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return C_


def selftest_joiner(mode: str, J, W, bias, out, layout: int = 0, live_t=None, live_len=None,
                    live_f: int = 0, lib_path: Optional[str] = None) -> np.ndarray:
    """The joiner kernels alone on one host problem (zasr_selftest_joiner; mode: a PRECISIONS
    name; layout 0: row-major J, 1: fragment-packed J and W): returns out [M][V] after
    out = J W^T + bias; rows of tiles the finished-stream filter skips keep out's values."""
    lib = load_library(lib_path)
    J, W, bias, out = _f32(J), _f32(W), _f32(bias), _f32(out).copy()
    live = [None if x is None else np.ascontiguousarray(x, np.int32) for x in (live_t, live_len)]
    p = lambda x: x.ctypes.data_as(C_FP)
    ip = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_int32))
    rc = lib.zasr_selftest_joiner(PRECISIONS[mode], int(layout), J.shape[0], W.shape[0], J.shape[1],
                                  p(J), p(W), p(bias), ip(live[0]), ip(live[1]), int(live_f), p(out))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return out



# ---- the transducer search kernels alone (include/zasr.h zasr_selftest_search_*) ----
SEARCH_STATE_FIELDS = (("lp", np.float64), ("lpf", np.int32), ("hash", np.uint64),
                       ("len", np.int32), ("y1", np.int32), ("y2", np.int32), ("hw", np.int32),
                       ("node", np.int32))
SEARCH_NODE_FIELDS = (("node_tok", np.int32), ("node_frame", np.int32),
                      ("node_parent", np.int32), ("node_lp", np.float64))


def search_state_alloc(S: int, Hmax: int, node_cap: int, fill: int = 0x6b) -> dict:
    """A search state of S streams x Hmax slots as a dict of numpy arrays, every byte `fill`
    (what a call does not write stays recognisable): the SEARCH_STATE_FIELDS [S][Hmax], nh [S],
    the SEARCH_NODE_FIELDS [S][node_cap], node_stats [S][node_cap][4] and node_count [S]."""
    def arr(shape, dt):
        a = np.empty(shape, dtype=dt)
        a.view(np.uint8)[...] = fill
        return a
    st = {k: arr((S, Hmax), dt) for k, dt in SEARCH_STATE_FIELDS}
    st["nh"] = arr((S,), np.int32)
    st.update({k: arr((S, node_cap), dt) for k, dt in SEARCH_NODE_FIELDS})
    st["node_stats"] = arr((S, node_cap, 4), np.float32)
    st["node_count"] = arr((S,), np.int32)
    return st


def _st_struct(st: dict):
    S, Hmax = st["lp"].shape
    c = _StState(S, Hmax, st["node_tok"].shape[1])
    for k, dt in SEARCH_STATE_FIELDS + SEARCH_NODE_FIELDS + (
            ("nh", np.int32), ("node_stats", np.float32), ("node_count", np.int32)):
        a = st[k]
        if a.dtype != dt or not a.flags.c_contiguous or not a.flags.writeable:
            raise ValueError(f"search state field {k}: a writable C-contiguous {dt.__name__} array")
        setattr(c, k, a.ctypes.data)
    return c


def _hw_struct(phrases, scores):
    phrases = [list(p) for p in (phrases or [])]
    toks = np.ascontiguousarray([t for p in phrases for t in p], dtype=np.int32)
    lens = np.ascontiguousarray([len(p) for p in phrases], dtype=np.int32)
    sc = np.ascontiguousarray(list(scores or []), dtype=np.float32)
    if len(sc) != len(phrases):
        raise ValueError("one score per hotword phrase")
    return _StHotwords(toks.ctypes.data, lens.ctypes.data, sc.ctypes.data, len(phrases)), (toks, lens, sc)


def _tab_struct(tab: dict):
    """tab: D, jfmt, a, b [V][D] f32, enc [rows][D] f32, enc_off [S] i32, J (uint8 image, in / out)"""
    a, b, enc = (_f32(tab[k]) for k in ("a", "b", "enc"))
    off = np.ascontiguousarray(tab["enc_off"], dtype=np.int32)
    J = tab["J"]
    if J.dtype != np.uint8 or not J.flags.c_contiguous or not J.flags.writeable:
        raise ValueError("J: a writable C-contiguous uint8 image")
    c = _StTable(int(tab["D"]), int(tab["jfmt"]), enc.shape[0], a.ctypes.data, b.ctypes.data,
                 enc.ctypes.data, off.ctypes.data, J.ctypes.data, J.size)
    return c, (a, b, enc, off)


def _ip(x):
    return x.ctypes.data_as(C.POINTER(C.c_int32))


def selftest_search_step(V: int, beam: int, t: int, enc_len, st: dict, logits=None, phrases=None,
                         scores=None, tab: Optional[dict] = None,
                         lib_path: Optional[str] = None) -> None:
    """One frame of launch_search_step on the state `st` (search_state_alloc's dict, updated in
    place, as is tab["J"]); t < 0: launch_search_init (+ launch_table_init) instead."""
    lib = load_library(lib_path)
    el = np.ascontiguousarray(enc_len, dtype=np.int32)
    lg = None if logits is None else _f32(logits)
    hw, keep = _hw_struct(phrases, scores)
    tb, keep2 = _tab_struct(tab) if tab is not None else (None, None)
    rc = lib.zasr_selftest_search_step(int(V), int(beam), int(t), _ip(el), C.byref(_st_struct(st)),
                                       None if lg is None else lg.ctypes.data_as(C_FP),
                                       C.byref(hw), None if tb is None else C.byref(tb))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())


def selftest_greedy_spec(V: int, F: int, init: int, parity: int, enc_len, t_cur, active, st: dict,
                         logits, tab: dict, phrases=None, scores=None,
                         lib_path: Optional[str] = None) -> None:
    """One super-step of launch_greedy_spec (init 1: after the two init launches; 2: those
    alone); st, t_cur [S] i32, active [2] i32 and tab["J"] are updated in place."""
    lib = load_library(lib_path)
    el = np.ascontiguousarray(enc_len, dtype=np.int32)
    for x in (t_cur, active):
        if x.dtype != np.int32 or not x.flags.c_contiguous:
            raise ValueError("t_cur / active: C-contiguous int32 arrays")
    lg = None if logits is None else _f32(logits)
    hw, keep = _hw_struct(phrases, scores)
    tb, keep2 = _tab_struct(tab)
    rc = lib.zasr_selftest_greedy_spec(int(V), int(F), int(init), int(parity), _ip(el), _ip(t_cur),
                                       _ip(active), C.byref(_st_struct(st)),
                                       None if lg is None else lg.ctypes.data_as(C_FP),
                                       C.byref(hw), C.byref(tb))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())


def selftest_search_final(V: int, st: dict, out_cap: int, phrases=None, scores=None,
                          fill: int = 0x6b, lib_path: Optional[str] = None) -> dict:
    """launch_search_final on the state: returns tok, frame [S][out_cap] i32, lp f64, stats
    [S][out_cap][4] f32 and count [S] i32, every byte `fill` where the kernel wrote nothing."""
    lib = load_library(lib_path)
    S = st["lp"].shape[0]
    out = {"tok": np.empty((S, out_cap), np.int32), "frame": np.empty((S, out_cap), np.int32),
           "lp": np.empty((S, out_cap), np.float64), "stats": np.empty((S, out_cap, 4), np.float32),
           "count": np.empty((S,), np.int32)}
    for a in out.values():
        a.view(np.uint8)[...] = fill
    hw, keep = _hw_struct(phrases, scores)
    rc = lib.zasr_selftest_search_final(int(V), C.byref(_st_struct(st)), C.byref(hw), int(out_cap),
                                        _ip(out["tok"]), _ip(out["frame"]),
                                        out["lp"].ctypes.data_as(C.POINTER(C.c_double)),
                                        out["stats"].ctypes.data_as(C_FP), _ip(out["count"]))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return out


def selftest_hotword_dfa(V: int, phrases, scores, lib_path: Optional[str] = None) -> dict:
    """build_hotword_dfa's tables (host only): tok2cls [V], next / delta [states][cls],
    node_score [states]."""
    lib = load_library(lib_path)
    hw, keep = _hw_struct(phrases, scores)
    n = sum(len(p) for p in phrases) + 1
    cap = max(n * n, 1)
    ns, nc = C.c_int32(0), C.c_int32(0)
    t2c = np.empty(V, np.int32)
    nxt = np.empty(cap, np.int32)
    dl, sc = np.empty(cap, np.float64), np.empty(cap, np.float64)
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.zasr_selftest_hotword_dfa(int(V), C.byref(hw), cap, C.byref(ns), C.byref(nc), _ip(t2c),
                                       _ip(nxt), dp(dl), dp(sc))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    k = ns.value * nc.value
    return {"tok2cls": t2c, "next": nxt[:k].reshape(ns.value, nc.value).copy(),
            "delta": dl[:k].reshape(ns.value, nc.value).copy(), "node_score": sc[:ns.value].copy()}


def selftest_ffn_h3(Y, W1, b1, W2, b2, X, byp_orig=None, byp_scale=None,
                    lib_path: Optional[str] = None) -> np.ndarray:
    """ffn_wide_h3_kernel alone on host operands (zasr_selftest_ffn_h3): returns
    X + W2 SwooshL(W1 Y + b1) + b2 (then the bypass_mid blend when byp_orig is given)."""
    lib = load_library(lib_path)
    Y, W1, b1, W2, b2, X = (_f32(v) for v in (Y, W1, b1, W2, b2, X))
    X = X.copy()
    bo = None if byp_orig is None else _f32(byp_orig)
    bs = None if byp_scale is None else _f32(byp_scale)
    p = lambda x: None if x is None else x.ctypes.data_as(C_FP)
    rc = lib.zasr_selftest_ffn_h3(Y.shape[0], Y.shape[1], W1.shape[0], p(Y), p(W1), p(b1), p(W2),
                                  p(b2), p(bo), p(bs), p(X))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return X


def selftest_ffn_bf16(W1, b1, W2, b2, X, byp_orig=None, byp_scale=None, form: int = 0,
                      lib_path: Optional[str] = None) -> np.ndarray:
    """The bf16 fused FFN alone on host operands (zasr_selftest_ffn_bf16): returns
    X + W2 SwooshL(W1 bf16(X) + b1) + b2 (bf16 weights and hidden activation; then the
    bypass_mid blend when byp_orig is given).  form 1: the opt-in rows form at D = 384."""
    lib = load_library(lib_path)
    W1, b1, W2, b2, X = (_f32(v) for v in (W1, b1, W2, b2, X))
    X = X.copy()
    bo = None if byp_orig is None else _f32(byp_orig)
    bs = None if byp_scale is None else _f32(byp_scale)
    p = lambda x: None if x is None else x.ctypes.data_as(C_FP)
    rc = lib.zasr_selftest_ffn_bf16(X.shape[0], X.shape[1], W1.shape[0], p(W1), p(b1), p(W2),
                                    p(b2), p(bo), p(bs), p(X), int(form))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return X


def selftest_attn_block_map(lens, units_per_seq: int, order: int = 0,
                            lib_path: Optional[str] = None) -> np.ndarray:
    """The attention kernels' block map alone, host only (zasr_selftest_attn_block_map):
    returns the uint32 entry of every block id (sequence << 12 | unit << 8 | tile, 0xffffffff
    past a range's end); its length is the launch's grid."""
    lib = load_library(lib_path)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    # every (unit, tile) at most once per range, and a range may hold them all
    cap = 8 * int(units_per_seq) * int(((lens.astype(np.int64) + 127) // 128).sum())
    out = np.empty(max(cap, 1), dtype=np.uint32)
    grid = C.c_int32(-1)
    rc = lib.zasr_selftest_attn_block_map(lens.ctypes.data_as(C.POINTER(C.c_int32)), len(lens),
                                          int(units_per_seq), int(order),
                                          out.ctypes.data_as(C.POINTER(C.c_uint32)), cap,
                                          C.byref(grid))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return out[:grid.value].copy()


def selftest_ffn_oop(kind: str, W1, b1, W2, b2, X, byp_orig=None, byp_scale=None, form: int = 0,
                     fill: float = -777.25, lib_path: Optional[str] = None):
    """A fused FFN out of place on host operands (zasr_selftest_ffn_bf16_oop, kind "bf16", or
    zasr_selftest_ffn_h3_oop, kind "h3"): returns (the output buffer, which started as `fill`,
    the input buffer after the call)."""
    lib = load_library(lib_path)
    W1, b1, W2, b2, X = (_f32(v) for v in (W1, b1, W2, b2, X))
    X = X.copy()
    out = np.full(X.shape, fill, dtype=np.float32)
    bo = None if byp_orig is None else _f32(byp_orig)
    bs = None if byp_scale is None else _f32(byp_scale)
    p = lambda x: None if x is None else x.ctypes.data_as(C_FP)
    args = (X.shape[0], X.shape[1], W1.shape[0], p(W1), p(b1), p(W2), p(b2), p(bo), p(bs), p(X),
            p(out))
    if kind == "bf16":
        rc = lib.zasr_selftest_ffn_bf16_oop(*args, int(form))
    elif kind == "h3":
        rc = lib.zasr_selftest_ffn_h3_oop(*args)
    else:
        raise ValueError(kind)
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return out, X


def selftest_seam(L, d: int, ds: int, dn: int, ds_next: int, c0: int, ldo: int, xd, orig, s,
                  wn8, wo2, fill: float = -777.25, lib_path: Optional[str] = None) -> dict:
    """The fused stack seam and the glue -> downsample -> downsample composition it replaces on
    the same host operands (zasr_selftest_seam).  Every destination starts as `fill`; returns
    {"next", "xnext", "out"} (fused) and {"next_ref", "xnext_ref", "out_ref"} (composition):
    next [sum L][dn], xnext [sum ceil(L / ds_next)][dn], out [sum ceil(L / 2)][ldo]."""
    lib = load_library(lib_path)
    L = np.ascontiguousarray(L, dtype=np.int32)
    orig, wn8, wo2 = _f32(orig), _f32(wn8), _f32(wo2)
    xd = None if xd is None else _f32(xd)
    s = None if s is None else _f32(s)
    rows = int(L.sum())
    rn = int(((L + ds_next - 1) // ds_next).sum())
    ro = int(((L + 1) // 2).sum())
    assert orig.shape == (rows, d) and wn8.shape == (8,) and wo2.shape == (2,)
    assert ds == 1 or (xd.shape == (int(((L + ds - 1) // ds).sum()), d) and s.shape == (d,))
    res = {}
    for name, shape in (("next", (rows, dn)), ("xnext", (rn, dn)), ("out", (ro, ldo))):
        for k in (name, name + "_ref"):
            res[k] = np.full(shape, fill, dtype=np.float32)
    p = lambda x: None if x is None else x.ctypes.data_as(C_FP)
    rc = lib.zasr_selftest_seam(len(L), L.ctypes.data_as(C.POINTER(C.c_int32)), int(d), int(ds),
                                int(dn), int(ds_next), int(c0), int(ldo), p(xd), p(orig), p(s),
                                p(wn8), p(wo2), p(res["next"]), p(res["xnext"]), p(res["out"]),
                                p(res["next_ref"]), p(res["xnext_ref"]), p(res["out_ref"]))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return res


def _lens(L) -> np.ndarray:
    return np.ascontiguousarray(L, dtype=np.int32)


def selftest_dwconv1d(L, x, w, b, glu: bool, bf16: bool = False, fill: float = -777.25,
                      lib_path: Optional[str] = None) -> np.ndarray:
    """The ConvolutionModule's depthwise kernel alone on a ragged batch of len(L) sequences
    (zasr_selftest_dwconv1d): x [sum L][2 d] (glu) or [sum L][d], w [d][K], b [d]; returns
    out [sum L][d], which started as `fill`.  bf16: x rounded to bf16, out widened."""
    lib = load_library(lib_path)
    L, x, w, b = _lens(L), _f32(x), _f32(w), _f32(b)
    rows, (d, K) = int(L.sum()), w.shape
    assert x.shape == (rows, 2 * d if glu else d) and b.shape == (d,)
    out = np.full((rows, d), fill, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C_FP)
    rc = lib.zasr_selftest_dwconv1d(len(L), L.ctypes.data_as(C.POINTER(C.c_int32)), d, K,
                                    int(glu), int(bf16), p(x), p(w), p(b), p(out))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return out


def _attn_operands(L, H, pmax, qkp, pos_tab):
    L, qkp, pos_tab = _lens(L), _f32(qkp), _f32(pos_tab)
    rows = int(L.sum()) if L.size and L.min() >= 0 else -1
    if rows >= 0:  # (a negative length goes to the entry, which refuses it)
        assert qkp.shape == (rows, 68 * H) and pos_tab.shape == (2 * pmax - 1, 4 * H)
    return L, qkp, pos_tab, rows


def attn_head0_strides(L, mode: str) -> np.ndarray:
    """Row stride of each sequence's head-0 weight block: L rounded up to 32 (4 in fp32)."""
    L = np.asarray(L, dtype=np.int64)
    return (L + 3) // 4 * 4 if mode == "fp32" else (L + 31) // 32 * 32


def selftest_attn_weights(mode: str, H: int, L, pmax: int, qkp, pos_tab, fill: float = -777.25,
                          lib_path: Optional[str] = None) -> np.ndarray:
    """Head 0's normalised attention weights as a decode materialises them
    (zasr_selftest_attn_weights): the flat buffer of the per-sequence [L][stride] blocks
    (attn_head0_strides), which started as `fill`."""
    lib = load_library(lib_path)
    L, qkp, pos_tab, _ = _attn_operands(L, H, pmax, qkp, pos_tab)
    n = int((np.maximum(L, 0).astype(np.int64) * attn_head0_strides(np.maximum(L, 0), mode)).sum())
    A0 = np.full(max(n, 1), fill, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C_FP)
    rc = lib.zasr_selftest_attn_weights(PRECISIONS[mode], int(H), len(L),
                                        L.ctypes.data_as(C.POINTER(C.c_int32)), int(pmax), p(qkp),
                                        p(pos_tab), p(A0))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return A0[:n]


def selftest_attn_sa(mode: str, H: int, L, pmax: int, qkp, pos_tab, v1, v2, fill: float = -777.25,
                     lib_path: Optional[str] = None):
    """A layer's two self-attentions alone (zasr_selftest_attn_sa): returns (out1 [R][12 H] from
    running statistics on v1, stats [R][H] (fp32: [R][H][2]), out2 from those statistics on
    v2); every output started as `fill`."""
    lib = load_library(lib_path)
    L, qkp, pos_tab, rows = _attn_operands(L, H, pmax, qkp, pos_tab)
    v1, v2 = _f32(v1), _f32(v2)
    rows = max(rows, 0)
    out1 = np.full((rows, 12 * H), fill, dtype=np.float32)
    out2 = out1.copy()
    stats = np.full((rows, H, 2) if mode == "fp32" else (rows, H), fill, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C_FP)
    rc = lib.zasr_selftest_attn_sa(PRECISIONS[mode], int(H), len(L),
                                   L.ctypes.data_as(C.POINTER(C.c_int32)), int(pmax), p(qkp),
                                   p(pos_tab), p(v1), p(v2), p(out1), p(stats), p(out2))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return out1, stats, out2


def selftest_nonlin(mode: str, H: int, L, pmax: int, hid: int, qkp, pos_tab, h3,
                    fill: float = -777.25, lib_path: Optional[str] = None):
    """NonlinAttention's kernels alone (zasr_selftest_nonlin): returns (t1t
    [pieces][hid][sum L32] uint16 as stored, which started as 0x7e7e; z [R][hid], which started
    as `fill`, or None in bf16x3 / bf16x6 where the route stops at the image)."""
    lib = load_library(lib_path)
    L, qkp, pos_tab, rows = _attn_operands(L, H, pmax, qkp, pos_tab)
    h3 = _f32(h3)
    rows = max(rows, 0)
    planes = {"bf16": 1, "bf16x3": 2, "bf16x6": 3, "f16x3": 2}.get(mode, 1)
    r32 = int(((np.maximum(L, 0) + 31) // 32 * 32).sum())
    t1t = np.full((planes, max(hid, 0), r32), 0x7e7e, dtype=np.uint16)
    z = np.full((rows, max(hid, 0)), fill, dtype=np.float32) if mode in ("bf16", "f16x3") else None
    p = lambda a: None if a is None else a.ctypes.data_as(C_FP)
    rc = lib.zasr_selftest_nonlin(PRECISIONS[mode], int(H), len(L),
                                  L.ctypes.data_as(C.POINTER(C.c_int32)), int(pmax), int(hid),
                                  p(qkp), p(pos_tab), p(h3),
                                  t1t.ctypes.data_as(C.POINTER(C.c_uint16)), p(z))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return t1t, z


def selftest_conv1(T, fb, w, b, form: int, fill: float = -777.25,
                   lib_path: Optional[str] = None) -> np.ndarray:
    """conv.0 + SwooshR alone (zasr_selftest_conv1): fb [sum T][80], w [8][9], b [8]; returns
    out [sum (T - 2)][80][8], which started as `fill`.  form 0: libm SwooshR, 1: the native
    form, 2: the native form with bf16 out."""
    lib = load_library(lib_path)
    T, fb, w, b = _lens(T), _f32(fb), _f32(w), _f32(b)
    assert fb.shape == (int(T.sum()), 80) and w.shape == (8, 9) and b.shape == (8,)
    out = np.full((int((T - 2).sum()), 80, 8), fill, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C_FP)
    rc = lib.zasr_selftest_conv1(len(T), T.ctypes.data_as(C.POINTER(C.c_int32)), int(form), p(fb),
                                 p(w), p(b), p(out))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return out


def selftest_convnext(L, x, dw_w, dw_b, w1=None, b1=None, w2=None, b2=None, form: int = 0,
                      fill: float = -777.25, lib_path: Optional[str] = None):
    """The ConvNeXt block's kernels alone (zasr_selftest_convnext): x [sum L][19][128], dw_w
    [128][7][7], dw_b [128], w1 [384][128], b1 [384], w2 [128][384], b2 [128].  Returns
    (y, out): the depthwise output and the block output (form 0: out is None), both started as
    `fill` (form 2 runs the MLP in place over x's buffer, as a decode does).  form 0: the f32
    depthwise kernel, 1: the bf16 pair, 2: the f32 depthwise kernel + the f16x3 MLP."""
    lib = load_library(lib_path)
    L, x, dw_w, dw_b = _lens(L), _f32(x), _f32(dw_w), _f32(dw_b)
    rows = int(L.sum())
    assert x.shape == (rows, 19, 128) and dw_w.shape == (128, 7, 7) and dw_b.shape == (128,)
    mlp = [None if v is None else _f32(v) for v in (w1, b1, w2, b2)]
    if form != 0:
        assert [v.shape for v in mlp] == [(384, 128), (384,), (128, 384), (128,)]
    y = np.full(x.shape, fill, dtype=np.float32)
    out = None if form == 0 else np.full(x.shape, fill, dtype=np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C_FP)
    rc = lib.zasr_selftest_convnext(len(L), L.ctypes.data_as(C.POINTER(C.c_int32)), int(form),
                                    p(x), p(dw_w), p(dw_b), *(p(v) for v in mlp), p(y), p(out))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return y, out


def selftest_bias_norm(x, bias, log_scale: float, orig=None, bscale=None, copy_mode: int = 0,
                       fill: float = -777.25, lib_path: Optional[str] = None) -> dict:
    """bias_norm_kernel alone (zasr_selftest_bias_norm): x [rows][d], bias [d], optionally the
    bypass blend with orig [rows][d] and bscale [d].  copy_mode 1: the result also to a second
    buffer (which started as `fill`), 2: also over orig's own device buffer.  Returns {"x",
    "orig" (what its buffer holds afterwards, or None), "copy" (copy_mode 1, else None)}."""
    lib = load_library(lib_path)
    x, bias = _f32(x).copy(), _f32(bias)
    rows, d = x.shape
    o = None if orig is None else _f32(orig).copy()
    s = None if bscale is None else _f32(bscale)
    cp = np.full(x.shape, fill, dtype=np.float32) if copy_mode == 1 else None
    p = lambda a: None if a is None else a.ctypes.data_as(C_FP)
    rc = lib.zasr_selftest_bias_norm(rows, d, p(bias), float(log_scale), p(o), p(s),
                                     int(copy_mode), p(x), p(cp))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return {"x": x, "orig": o, "copy": cp}


# ---- the CAM++, Silero VAD and ViBERT kernels alone (include/zasr.h zasr_selftest_campp_* /
# _vad_* / _vibert_*).  Every returned array started as `fill` (or as the given image).
def _aux_ptr(a, t=None):
    return None if a is None else a.ctypes.data_as(C_FP if t is None else C.POINTER(t))


def _aux_check(lib, rc):
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())


def _i64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int64)


def selftest_campp_conv2d(x, w, scale, shift, res=None, *, ks: int, ci: int, fi: int, sf: int, T: int,
                          n: int, relu: bool, tdnn_out: bool, in_tf: bool, use_mfma: bool,
                          rb: int = 0, fill: float = -777.25, lib_path: Optional[str] = None):
    """launch_campp_conv2d alone: returns (y [n][32][fo][T] or, tdnn_out, [n][T][32 fo]; route
    (1: the MFMA kernel ran, 0: the direct one); the MFMA kernel's rows per block, or 0)."""
    lib = load_library(lib_path)
    x, w, scale, shift = _f32(x), _f32(w), _f32(scale), _f32(shift)
    res = None if res is None else _f32(res)
    fo = (fi - 1) // sf + 1 if fi >= 1 and sf >= 1 else 1
    assert x.size == n * ci * fi * T and w.size == 32 * ci * ks * ks and scale.size == shift.size == 32
    assert res is None or res.size == n * 32 * fo * T
    y = np.full((n, T, 32 * fo) if tdnn_out else (n, 32, fo, T), fill, dtype=np.float32)
    route, used = C.c_int32(-1), C.c_int32(-1)
    p = _aux_ptr
    _aux_check(lib, lib.zasr_selftest_campp_conv2d(
        ks, ci, fi, sf, T, n, int(relu), int(tdnn_out), int(in_tf), int(use_mfma), int(rb), p(x),
        p(w), p(scale), p(shift), p(res), p(y), C.byref(route), C.byref(used)))
    return y, route.value, used.value


def selftest_campp_cam_mask(h, w1, b1, w2, b2, seg_len: int, fill: float = -777.25,
                            lib_path: Optional[str] = None) -> np.ndarray:
    """launch_campp_cam_mask alone: h [n][T][128] -> mexp [n][T][32]."""
    lib = load_library(lib_path)
    h, w1, b1, w2, b2 = (_f32(a) for a in (h, w1, b1, w2, b2))
    n, T, _ = h.shape
    assert h.shape[2] == 128 and w1.shape == (64, 128) and b1.shape == (64,) and w2.shape == (32, 64) and b2.shape == (32,)
    m = np.full((n, T, 32), fill, dtype=np.float32)
    p = _aux_ptr
    _aux_check(lib, lib.zasr_selftest_campp_cam_mask(n, T, int(seg_len), p(h), p(w1), p(b1), p(w2),
                                                     p(b2), p(m)))
    return m


def selftest_campp_stats(x, s, b, fill: float = -777.25, lib_path: Optional[str] = None) -> np.ndarray:
    """launch_campp_stats alone: x [N][T][C] -> out [N][2 C]."""
    lib = load_library(lib_path)
    x, s, b = _f32(x), _f32(s), _f32(b)
    N, T, Cc = x.shape
    assert s.shape == (Cc,) and b.shape == (Cc,)
    out = np.full((N, 2 * Cc), fill, dtype=np.float32)
    p = _aux_ptr
    _aux_check(lib, lib.zasr_selftest_campp_stats(N, T, Cc, p(x), p(s), p(b), p(out)))
    return out


def selftest_campp_cmvn(x, fr_off, lib_path: Optional[str] = None) -> np.ndarray:
    """launch_campp_cmvn alone: returns x [rows][80] after the in-place mean removal."""
    lib = load_library(lib_path)
    x, fr_off = _f32(x).copy(), _lens(fr_off)
    assert x.ndim == 2 and x.shape[1] == 80 and fr_off.size >= 2
    _aux_check(lib, lib.zasr_selftest_campp_cmvn(fr_off.size - 1, x.shape[0],
                                                 _aux_ptr(fr_off, C.c_int32), _aux_ptr(x)))
    return x


def selftest_campp_gather(rows, win_row, win_n, wf: int, fill: float = -777.25,
                          lib_path: Optional[str] = None) -> np.ndarray:
    """launch_campp_gather alone: rows [nrows][80] -> out [nwin][wf][80]."""
    lib = load_library(lib_path)
    rows, win_row, win_n = _f32(rows), _lens(win_row), _lens(win_n)
    assert rows.ndim == 2 and rows.shape[1] == 80 and win_row.shape == win_n.shape
    out = np.full((win_row.size, wf, 80), fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_campp_gather(win_row.size, int(wf), rows.shape[0], _aux_ptr(rows),
                                                   _aux_ptr(win_row, C.c_int32),
                                                   _aux_ptr(win_n, C.c_int32), _aux_ptr(out)))
    return out


def selftest_emb_conv2d(x, w, bias, ks: int, stride: int, res=None, relu: bool = True, route: int = 0,
                        fill: float = -777.25, lib_path: Optional[str] = None):
    """launch_emb_conv2d (or, for Ci = 1, launch_emb_stem) alone: x [n][Fi][Ti][Ci] (the stem:
    [n][Ti][Fi]), w [Co][ks][ks][Ci] (tap-major, ci contiguous), bias [Co], res like the output;
    returns (y [n][Fo][To][Co], routes the layer takes)."""
    lib = load_library(lib_path)
    x, w, bias = _f32(x), _f32(w), _f32(bias)
    co = w.shape[0]
    if x.ndim == 3:
        n, ti, fi = x.shape
        ci = 1
    else:
        n, fi, ti, ci = x.shape
    assert w.size == co * ks * ks * ci and bias.shape == (co,)
    fo, to = (fi - 1) // stride + 1, (ti - 1) // stride + 1
    y = np.full((n, fo, to, co), fill, dtype=np.float32)
    res = None if res is None else _f32(res)
    assert res is None or res.shape == y.shape
    routes = C.c_int32(0)
    _aux_check(lib, lib.zasr_selftest_emb_conv2d(int(ks), int(stride), ci, co, n, fi, ti, int(bool(relu)),
                                                 int(route), _aux_ptr(x), _aux_ptr(w), _aux_ptr(bias),
                                                 _aux_ptr(res), _aux_ptr(y), C.byref(routes)))
    return y, int(routes.value)


def selftest_emb_pool(x, mask=None, fill: float = -777.25, lib_path: Optional[str] = None) -> np.ndarray:
    """launch_emb_pool alone: x [n][F][T][C], mask uint8 [n][S][nseg] (None: the unmasked
    population form, S = 1) -> stats [n][S][2 C F]."""
    lib = load_library(lib_path)
    x = _f32(x)
    n, F, T, Cc = x.shape
    if mask is None:
        S, nseg, m = 1, 0, None
    else:
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        assert m.ndim == 3 and m.shape[0] == n
        S, nseg = m.shape[1], m.shape[2]
    out = np.full((n, S, 2 * Cc * F), fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_emb_pool(n, F, T, Cc, S, nseg, int(m is None), _aux_ptr(x),
                                               _aux_ptr(m, C.c_uint8), _aux_ptr(out)))
    return out


def selftest_vad_frames(n_windows: int, audio=None, off=None, win_start=None, lens=None, rows576=None,
                        fill: float = -777.25, lib_path: Optional[str] = None):
    """launch_vad_frames alone: returns (frames [n_windows * 4][256], maxabs [files] uint32 or
    None).  rows576 [n_windows][576]: row mode; else file mode, with `lens` after
    launch_vad_maxabs on a zeroed table."""
    lib = load_library(lib_path)
    frames = np.full((n_windows * 4, 256), fill, dtype=np.float32)
    i64 = lambda a: _aux_ptr(a, C.c_int64)
    if rows576 is not None:
        rows576 = _f32(rows576)
        assert rows576.shape == (n_windows, 576)
        _aux_check(lib, lib.zasr_selftest_vad_frames(0, n_windows, 0, None, None, None, None,
                                                     _aux_ptr(rows576), None, _aux_ptr(frames)))
        return frames, None
    audio, off, win_start = _f32(audio), _i64(off), _i64(win_start)
    lens = None if lens is None else _i64(lens)
    mx = None if lens is None else np.full(off.size, 0x7e7e7e7e, dtype=np.uint32)
    assert off.shape == win_start.shape and (lens is None or lens.shape == off.shape)
    _aux_check(lib, lib.zasr_selftest_vad_frames(off.size, n_windows, audio.size, _aux_ptr(audio),
                                                 i64(off), i64(win_start), i64(lens), None,
                                                 _aux_ptr(mx, C.c_uint32), _aux_ptr(frames)))
    return frames, mx


def selftest_vad_mag_im2col(S, bins: int, Kp: int, fill: float = -777.25,
                            lib_path: Optional[str] = None) -> np.ndarray:
    """launch_vad_mag_im2col alone: S [windows * 4][ldS] -> A [windows * 4][Kp]."""
    lib = load_library(lib_path)
    S = _f32(S)
    assert S.ndim == 2 and S.shape[0] % 4 == 0
    A = np.full((S.shape[0], Kp), fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_vad_im2col(0, S.shape[0] // 4, 0, int(bins), 0, S.shape[1],
                                                 int(Kp), _aux_ptr(S), _aux_ptr(A)))
    return A


def selftest_vad_im2col(Y, N: int, T: int, stride: int, fill: float = -777.25,
                        lib_path: Optional[str] = None) -> np.ndarray:
    """launch_vad_im2col alone: Y [N * T][C] -> A [N * Tout][3 C]."""
    lib = load_library(lib_path)
    Y = _f32(Y)
    assert Y.ndim == 2 and Y.shape[0] == N * T
    Cc = Y.shape[1]
    A = np.full((N * ((T - 1) // stride + 1), 3 * Cc), fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_vad_im2col(1, N, T, Cc, int(stride), 0, 0, _aux_ptr(Y),
                                                 _aux_ptr(A)))
    return A


def selftest_vad_lstm(gx, whh, bhh, wd, bd: float, seg_start, seg_count, seg_warm=None, init=None,
                      want_s: bool = True, want_e: bool = True, fill: float = -777.25,
                      lib_path: Optional[str] = None):
    """launch_vad_lstm alone: returns (probs [windows], s_out, e_out [segments][2][128] or None)."""
    lib = load_library(lib_path)
    gx, whh, bhh, wd = _f32(gx), _f32(whh), _f32(bhh), _f32(wd)
    seg_start, seg_count = _i64(seg_start), _lens(seg_count)
    seg_warm = None if seg_warm is None else _lens(seg_warm)
    init = None if init is None else _f32(init)
    nseg = seg_start.size
    assert gx.ndim == 2 and gx.shape[1] == 512 and whh.shape == (512, 128) and bhh.shape == (512,) and wd.shape == (128,)
    assert seg_count.size == nseg and (seg_warm is None or seg_warm.size == nseg)
    assert init is None or init.shape == (nseg, 2, 128)
    probs = np.full(gx.shape[0], fill, dtype=np.float32)
    s_out = np.full((nseg, 2, 128), fill, dtype=np.float32) if want_s else None
    e_out = np.full((nseg, 2, 128), fill, dtype=np.float32) if want_e else None
    p = _aux_ptr
    _aux_check(lib, lib.zasr_selftest_vad_lstm(gx.shape[0], nseg, p(gx), p(whh), p(bhh), p(wd), float(bd),
                                               p(seg_start, C.c_int64), p(seg_count, C.c_int32),
                                               p(seg_warm, C.c_int32), p(init), p(probs), p(s_out),
                                               p(e_out)))
    return probs, s_out, e_out


def selftest_vibert_ln(g, b, eps: float, x=None, ids=None, tt=None, L: int = 0, word=None, pos=None,
                       type_=None, H: Optional[int] = None, fill: float = -777.25,
                       lib_path: Optional[str] = None) -> np.ndarray:
    """launch_vibert_layernorm on x [rows][H] (in place; returned), or, with ids,
    launch_vibert_embed: ids / tt [rows], L, word [V][H], pos [P][H], type_ [TT][H]."""
    lib = load_library(lib_path)
    g, b = _f32(g), _f32(b)
    H = g.size if H is None else H
    p = _aux_ptr
    if ids is None:
        x = _f32(x).copy()
        assert x.ndim == 2 and x.shape[1] == H
        _aux_check(lib, lib.zasr_selftest_vibert_ln(x.shape[0], H, 0, None, None, 0, 0, 0, None, None,
                                                    None, p(g), p(b), float(eps), p(x)))
        return x
    ids, tt, word, pos, type_ = _i64(ids), _i64(tt), _f32(word), _f32(pos), _f32(type_)
    assert ids.shape == tt.shape and word.shape[1] == pos.shape[1] == type_.shape[1] == H
    x = np.full((ids.size, H), fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_vibert_ln(ids.size, H, int(L), p(ids, C.c_int64), p(tt, C.c_int64),
                                                word.shape[0], pos.shape[0], type_.shape[0], p(word),
                                                p(pos), p(type_), p(g), p(b), float(eps), p(x)))
    return x


def selftest_vibert_attn(qkv, mask, B: int, L: int, heads: int, H: int, fill: float = -777.25,
                         lib_path: Optional[str] = None) -> np.ndarray:
    """launch_vibert_attention alone: qkv [B L][3 H], mask [B L] -> ctx [B L][H]."""
    lib = load_library(lib_path)
    qkv, mask = _f32(qkv), _i64(mask)
    assert qkv.shape == (B * L, 3 * H) and mask.shape == (B * L,)
    ctx = np.full((B * L, H), fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_vibert_attn(B, L, heads, H, _aux_ptr(qkv),
                                                  _aux_ptr(mask, C.c_int64), _aux_ptr(ctx)))
    return ctx


def selftest_vibert_gather(x, offsets, L: int, fill: float = -777.25,
                           lib_path: Optional[str] = None) -> np.ndarray:
    """launch_vibert_gather alone: x [B L][H], offsets [B][W] -> g [B W][H]."""
    lib = load_library(lib_path)
    x, offsets = _f32(x), _i64(offsets)
    B, W = offsets.shape
    assert x.ndim == 2 and x.shape[0] == B * L
    g = np.full((B * W, x.shape[1]), fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_vibert_gather(B, int(L), W, x.shape[1], _aux_ptr(x),
                                                    _aux_ptr(offsets, C.c_int64), _aux_ptr(g)))
    return g


# ---- the PyanNet and Conv-TasNet kernels alone (include/zasr.h zasr_selftest_seg_* / _sep_*).
# Every returned array started as `fill` (or as the given image).
def selftest_seg_chunk_stats(audio, starts, T: int, fill: float = -777.25,
                             lib_path: Optional[str] = None) -> np.ndarray:
    """launch_seg_chunk_stats alone: stats [n][2] = (mean, rstd) of the T samples at starts[k]."""
    lib = load_library(lib_path)
    audio, starts = _f32(audio), _i64(starts)
    stats = np.full((starts.size, 2), fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_seg_chunk_stats(audio.size, starts.size, int(T), _aux_ptr(audio),
                                                      _aux_ptr(starts, C.c_int64), _aux_ptr(stats)))
    return stats


def selftest_seg_front(audio, starts, T: int, stats, in_w: float, in_b: float, w0t,
                       fill: float = -777.25, lib_path: Optional[str] = None) -> np.ndarray:
    """launch_seg_front alone on the caller's stats [n][2]: out [n][F1][80]."""
    lib = load_library(lib_path)
    audio, starts, stats, w0t = _f32(audio), _i64(starts), _f32(stats), _f32(w0t)
    n = starts.size
    assert stats.shape == (n, 2) and w0t.shape == (251, 80)
    F1 = max(((int(T) - 251) // 10 + 1) // 3, 0)
    out = np.full((n, F1, 80), fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_seg_front(audio.size, n, int(T), _aux_ptr(audio),
                                                _aux_ptr(starts, C.c_int64), _aux_ptr(stats), float(in_w),
                                                float(in_b), _aux_ptr(w0t), _aux_ptr(out)))
    return out


def selftest_seg_pool3(x, Fp: int, max_blocks: int = 0, fill: float = -777.25,
                       lib_path: Optional[str] = None) -> np.ndarray:
    """launch_seg_pool3 alone: x [n][L][C] -> out [n][Fp][C]."""
    lib = load_library(lib_path)
    x = _f32(x)
    n, L, Cc = x.shape
    out = np.full((n, int(Fp), Cc), fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_seg_pool3(n, L, Cc, int(Fp), int(max_blocks), _aux_ptr(x), _aux_ptr(out)))
    return out


def selftest_seg_frame_stats(x, fill: float = -777.25, lib_path: Optional[str] = None) -> np.ndarray:
    """launch_seg_frame_stats alone: x [n][F][C] -> stats [n][C][2]."""
    lib = load_library(lib_path)
    x = _f32(x)
    n, F, Cc = x.shape
    stats = np.full((n, Cc, 2), fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_seg_frame_stats(n, F, Cc, _aux_ptr(x), _aux_ptr(stats)))
    return stats


def selftest_seg_norm_act(x, stats, w, b, max_blocks: int = 0, lib_path: Optional[str] = None) -> np.ndarray:
    """launch_seg_norm_act alone: returns x [n][F][C] after the in-place normalise + leaky_relu."""
    lib = load_library(lib_path)
    x, stats, w, b = _f32(x).copy(), _f32(stats), _f32(w), _f32(b)
    n, F, Cc = x.shape
    assert stats.shape == (n, Cc, 2) and w.shape == (Cc,) and b.shape == (Cc,)
    _aux_check(lib, lib.zasr_selftest_seg_norm_act(n, F, Cc, int(max_blocks), _aux_ptr(stats), _aux_ptr(w),
                                                   _aux_ptr(b), _aux_ptr(x)))
    return x


def selftest_seg_lstm(gx, whh, group: int, fill: float = -777.25, lib_path: Optional[str] = None) -> np.ndarray:
    """launch_seg_lstm alone: gx [n][F][1024], whh [2][512][128] -> out [n][F][256]."""
    lib = load_library(lib_path)
    gx, whh = _f32(gx), _f32(whh)
    n, F, _ = gx.shape
    assert gx.shape[2] == 1024 and whh.shape == (2, 512, 128)
    out = np.full((n, F, 256), fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_seg_lstm(n, F, int(group), _aux_ptr(gx), _aux_ptr(whh), _aux_ptr(out)))
    return out


def selftest_seg_head(x, w, b, fill: float = -777.25, lib_path: Optional[str] = None):
    """launch_seg_head alone: x [rows][128] -> (logits [rows][7], classes uint8 [rows], which
    start as 255)."""
    lib = load_library(lib_path)
    x, w, b = _f32(x), _f32(w), _f32(b)
    assert x.ndim == 2 and x.shape[1] == 128 and w.shape == (7, 128) and b.shape == (7,)
    logits = np.full((x.shape[0], 7), fill, dtype=np.float32)
    classes = np.full(x.shape[0], 255, dtype=np.uint8)
    _aux_check(lib, lib.zasr_selftest_seg_head(x.shape[0], _aux_ptr(x), _aux_ptr(w), _aux_ptr(b),
                                               _aux_ptr(logits), _aux_ptr(classes, C.c_uint8)))
    return logits, classes


class SepCall:
    """One separation call's regions (sig_off, T each) and the launch group [r0, r0 + ng) of it
    that an entry runs: F frames per region, M rows and nt tiles of the group."""

    def __init__(self, sig_off, T, r0: int, ng: int, win: int = 32, hop: int = 16):
        self.sig_off, self.T = _i64(sig_off), _lens(T)
        assert self.sig_off.shape == self.T.shape
        self.r0, self.ng, self.win, self.hop = int(r0), int(ng), int(win), int(hop)
        self.F = (self.T.astype(np.int64) - self.win) // self.hop + 1
        Fg = self.F[self.r0:self.r0 + self.ng]
        self.M, self.nt = int(Fg.sum()), int(((Fg + 31) // 32).sum())
        self.c = _SepCall(self.T.size, _aux_ptr(self.sig_off, C.c_int64), _aux_ptr(self.T, C.c_int32),
                          self.r0, self.ng, self.win, self.hop)

    def ref(self):
        return C.byref(self.c)


def selftest_sep_frames(call: SepCall, signal, fill: float = -777.25, lib_path: Optional[str] = None) -> np.ndarray:
    """launch_sep_frames alone: frames [M][win]."""
    lib = load_library(lib_path)
    signal = _f32(signal)
    frames = np.full((call.M, call.win), fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_sep_frames(call.ref(), signal.size, _aux_ptr(signal), _aux_ptr(frames)))
    return frames


def selftest_sep_tile_sums(call: SepCall, x, fill: float = -777.25, lib_path: Optional[str] = None) -> np.ndarray:
    """launch_sep_tile_sums alone: x [M][C] -> partial float64 [nt][2]."""
    lib = load_library(lib_path)
    x = _f32(x)
    assert x.ndim == 2 and x.shape[0] == call.M
    partial = np.full((call.nt, 2), fill, dtype=np.float64)
    _aux_check(lib, lib.zasr_selftest_sep_tile_sums(call.ref(), x.shape[1], _aux_ptr(x),
                                                    _aux_ptr(partial, C.c_double)))
    return partial


def selftest_sep_region_stats(call: SepCall, partial, Cc: int, fill: float = -777.25,
                              lib_path: Optional[str] = None) -> np.ndarray:
    """launch_sep_region_stats alone: partial [nt][2] -> stats [n_regions][2] (the group's rows
    written)."""
    lib = load_library(lib_path)
    partial = np.ascontiguousarray(partial, dtype=np.float64)
    assert partial.shape == (call.nt, 2)
    stats = np.full((call.T.size, 2), fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_sep_region_stats(call.ref(), int(Cc), _aux_ptr(partial, C.c_double),
                                                       _aux_ptr(stats)))
    return stats


def selftest_sep_gln_apply(call: SepCall, x, stats, gamma, beta, in_place: bool, fill: float = -777.25,
                           lib_path: Optional[str] = None) -> np.ndarray:
    """launch_sep_gln_apply alone on x [M][C], out of place or in place: returns the result."""
    lib = load_library(lib_path)
    x, stats, gamma, beta = _f32(x), _f32(stats), _f32(gamma), _f32(beta)
    Cc = x.shape[1]
    assert x.shape[0] == call.M and stats.shape == (call.T.size, 2) and gamma.shape == beta.shape == (Cc,)
    dst = x.copy() if in_place else np.full(x.shape, fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_sep_gln_apply(call.ref(), Cc, int(bool(in_place)), _aux_ptr(stats),
                                                    _aux_ptr(gamma), _aux_ptr(beta),
                                                    None if in_place else _aux_ptr(x), _aux_ptr(dst)))
    return dst


def selftest_sep_mid(call: SepCall, h, stats, gamma, beta, w, bias, slope: float, dil: int,
                     fill: float = -777.25, lib_path: Optional[str] = None):
    """launch_sep_mid alone: h [M][C], w [3][C] -> (y [M][C], partial float64 [nt][2])."""
    lib = load_library(lib_path)
    h, stats, gamma, beta, w, bias = (_f32(a) for a in (h, stats, gamma, beta, w, bias))
    Cc = h.shape[1]
    assert h.shape[0] == call.M and stats.shape == (call.T.size, 2) and w.shape == (3, Cc)
    assert gamma.shape == beta.shape == bias.shape == (Cc,)
    y = np.full(h.shape, fill, dtype=np.float32)
    partial = np.full((call.nt, 2), fill, dtype=np.float64)
    p = _aux_ptr
    _aux_check(lib, lib.zasr_selftest_sep_mid(call.ref(), Cc, int(dil), float(slope), p(stats), p(gamma), p(beta),
                                              p(w), p(bias), p(h), p(y), p(partial, C.c_double)))
    return y, partial


def selftest_sep_prelu(x, Cc: int, col0: int, slope: float, max_blocks: int = 0,
                       lib_path: Optional[str] = None) -> np.ndarray:
    """launch_sep_prelu alone, in place on columns [col0, col0 + C) of x [rows][ld]."""
    lib = load_library(lib_path)
    x = _f32(x).copy()
    rows, ld = x.shape
    _aux_check(lib, lib.zasr_selftest_sep_prelu(rows, int(Cc), ld, int(col0), float(slope), int(max_blocks),
                                                _aux_ptr(x)))
    return x


def selftest_sep_overlap_add(call: SepCall, dec0, dec1, out_off, n_out: int, fill: float = -777.25,
                             lib_path: Optional[str] = None) -> np.ndarray:
    """launch_sep_overlap_add alone: dec0 / dec1 [M][win] -> out [n_out]."""
    lib = load_library(lib_path)
    dec0, dec1, out_off = _f32(dec0), _f32(dec1), _i64(out_off)
    assert dec0.shape == dec1.shape == (call.M, call.win) and out_off.shape == call.T.shape
    out = np.full(int(n_out), fill, dtype=np.float32)
    _aux_check(lib, lib.zasr_selftest_sep_overlap_add(call.ref(), _aux_ptr(out_off, C.c_int64), int(n_out),
                                                      _aux_ptr(dec0), _aux_ptr(dec1), _aux_ptr(out)))
    return out


def silence_flags(d_wav_ptr: int, n: int, frame_len: int, threshold: float, d_flags_ptr: int,
                  stream: int = 0, lib_path: Optional[str] = None) -> None:
    """Per-frame silence flags of an HBM-resident signal (include/zasr.h zasr_silence_flags):
    d_flags[f] = sqrt(mean(frame_f ** 2)) < threshold in numpy float32 arithmetic."""
    lib = load_library(lib_path)
    rc = lib.zasr_silence_flags(C.c_void_p(d_wav_ptr), int(n), int(frame_len),
                                float(threshold), C.c_void_p(d_flags_ptr), C.c_void_p(stream))
    if rc != 0:
        raise ZasrError(lib.zasr_last_error().decode())


@dataclasses.dataclass
class SearchResult:
    """One chunk's search output: the tuple of core/asr_engine.py:1153 with per-token
    entropy statistics (entropy, sum p^(1/3), top1, top2) in place of raw logits rows."""
    token_ids: np.ndarray
    frames: np.ndarray
    log_probs: np.ndarray
    stats: np.ndarray
    T: int


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _ptr_array(arrs: Sequence[np.ndarray]):
    fp = C.POINTER(C.c_float)
    return (fp * len(arrs))(*[a.ctypes.data_as(fp) for a in arrs])


class Recognizer:
    def __init__(self, model_dir: str, decoding_method: str = "modified_beam_search",
                 max_active_paths: int = 8, hotwords: Optional[Sequence[Sequence[int]]] = None,
                 hotword_scores: Optional[Sequence[float]] = None, device_id: int = 0,
                 precision: str = "fp32", lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        hotwords = [list(map(int, h)) for h in (hotwords or [])]
        scores = list(hotword_scores or [1.5] * len(hotwords))
        flat = np.array([t for h in hotwords for t in h] or [0], dtype=np.int32)
        lens = np.array([len(h) for h in hotwords] or [0], dtype=np.int32)
        sc = np.array(scores or [0.0], dtype=np.float32)
        self._keep = (flat, lens, sc)
        cfg = _Config(model_dir.encode(), decoding_method.encode(), max_active_paths, 0.0,
                      flat.ctypes.data_as(C.POINTER(C.c_int32)),
                      lens.ctypes.data_as(C.POINTER(C.c_int32)),
                      sc.ctypes.data_as(C.POINTER(C.c_float)), len(hotwords), device_id,
                      PRECISIONS[precision])
        h = C.c_void_p()
        rc = self.lib.zasr_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            msg = self.lib.zasr_last_error().decode()
            if rc == 2:
                raise FileNotFoundError(msg)
            raise ZasrError(msg)
        self.handle = h
        self.device_id = int(device_id)
        self.precision = precision
        self.vocab_size = self.lib.zasr_vocab_size(h)
        self.joiner_dim = self.lib.zasr_joiner_dim(h)
        self._args = (model_dir, decoding_method, max_active_paths, hotwords, scores, device_id,
                      lib_path)
        self._fallback = None

    def close(self):
        if getattr(self, "handle", None):
            self.lib.zasr_destroy(self.handle)
            self.handle = None
        fb = getattr(self, "_fallback", None)
        if fb is not None:
            fb.close()
            self._fallback = None

    # f16x3 stores the split operands as fp16 pieces (|x| < 65504); an activation beyond that
    # range makes the encoder output non-finite, which the engine detects per batch (after
    # draining every stream) and reports.  The decode is then redone by a bf16x6 engine of the
    # same model: the other exact-f32-quality mode, whose bf16 pieces have f32's range
    # (DESIGN.md §6), so the caller still gets the token-exact transcript.
    FALLBACK_PRECISION = "bf16x6"

    def _retry(self, e: "ZasrError", name: str, *args, **kw):
        if self.precision != "f16x3" or "non-finite encoder output" not in str(e):
            raise e
        if self._fallback is None:
            import logging
            logging.getLogger("zasr").warning(
                "[zasr] f16x3 operand range exceeded; re-decoding with %s", self.FALLBACK_PRECISION)
            md, method, beam, hw, sc, dev, lp = self._args
            self._fallback = Recognizer(md, method, beam, hotwords=hw, hotword_scores=sc,
                                        device_id=dev, precision=self.FALLBACK_PRECISION,
                                        lib_path=lp)
        return getattr(self._fallback, name)(*args, **kw)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ZasrError(self.lib.zasr_last_error().decode())

    def _collect(self, res) -> List[SearchResult]:
        out = []
        try:
            n = self.lib.zasr_result_count(res)
            for i in range(n):
                k = self.lib.zasr_result_num_tokens(res, i)
                T = self.lib.zasr_result_num_frames(res, i)
                if k > 0:
                    tok = np.ctypeslib.as_array(self.lib.zasr_result_tokens(res, i), (k,)).copy()
                    fr = np.ctypeslib.as_array(self.lib.zasr_result_frames(res, i), (k,)).copy()
                    lp = np.ctypeslib.as_array(self.lib.zasr_result_log_probs(res, i), (k,)).copy()
                    st = np.ctypeslib.as_array(self.lib.zasr_result_token_stats(res, i),
                                               (k * 4,)).copy().reshape(k, 4)
                else:
                    tok = np.zeros(0, np.int32)
                    fr = np.zeros(0, np.int32)
                    lp = np.zeros(0, np.float64)
                    st = np.zeros((0, 4), np.float32)
                out.append(SearchResult(tok, fr, lp, st, T))
        finally:
            self.lib.zasr_result_free(res)
        return out

    def routes(self) -> dict:
        """Which kernel each part of the loaded model was routed to (zasr_model_routes)."""
        import json
        buf = C.create_string_buffer(1024)
        self._check(self.lib.zasr_model_routes(self.handle, buf, len(buf)))
        return json.loads(buf.value.decode())

    def set_mel_banks(self, banks) -> None:
        """Replace the fbank's 80 triangular filters ([80][256] or [80][257] weights;
        zasr_fbank_set_mel_banks)."""
        b = _f32(banks)
        if b.ndim != 2 or b.shape[0] != 80 or b.shape[1] not in (256, 257):
            raise ValueError("mel banks must be [80][256] or [80][257]")
        self._check(self.lib.zasr_fbank_set_mel_banks(
            self.handle, b.ctypes.data_as(C.POINTER(C.c_float)), b.shape[1]))

    def fbank(self, audio) -> np.ndarray:
        a = _f32(audio)
        n = a.shape[0]
        frames = (n + 80) // 160 if n > 0 else 0
        out = np.empty((max(frames, 1), 80), dtype=np.float32)
        nf = C.c_int64()
        fp = C.POINTER(C.c_float)
        self._check(self.lib.zasr_fbank(self.handle, a.ctypes.data_as(fp), n, 16000,
                                        out.ctypes.data_as(fp), out.size, C.byref(nf)))
        return out[: nf.value]

    def decode(self, chunks: Sequence, beam: int = 0) -> List[SearchResult]:
        arrs = [_f32(c) for c in chunks]
        ns = (C.c_int64 * len(arrs))(*[a.shape[0] for a in arrs])
        res = C.c_void_p()
        try:
            self._check(self.lib.zasr_decode_batch(self.handle, _ptr_array(arrs), ns, len(arrs),
                                                   beam, C.byref(res)))
        except ZasrError as e:
            return self._retry(e, "decode", arrs, beam=beam)
        return self._collect(res)

    def decode_features(self, feats: Sequence, beam: int = 0) -> List[SearchResult]:
        arrs = [_f32(f) for f in feats]
        ns = (C.c_int64 * len(arrs))(*[a.shape[0] for a in arrs])
        res = C.c_void_p()
        try:
            self._check(self.lib.zasr_decode_features(self.handle, _ptr_array(arrs), ns,
                                                      len(arrs), beam, C.byref(res)))
        except ZasrError as e:
            return self._retry(e, "decode_features", arrs, beam=beam)
        return self._collect(res)

    def decode_device(self, d_wav_ptr: int, offsets: Sequence[int], lengths: Sequence[int],
                      beam: int = 0, stream: int = 0) -> List[SearchResult]:
        n = len(lengths)
        off = (C.c_int64 * n)(*offsets)
        ln = (C.c_int64 * n)(*lengths)
        res = C.c_void_p()
        try:
            self._check(self.lib.zasr_decode_device(self.handle, C.c_void_p(d_wav_ptr), off, ln,
                                                    n, beam, C.c_void_p(stream), C.byref(res)))
        except ZasrError as e:
            return self._retry(e, "decode_device", d_wav_ptr, offsets, lengths, beam=beam,
                               stream=stream)
        return self._collect(res)

    def decode_device_batches(self, d_wav_ptr: int, offsets: Sequence[int],
                              lengths: Sequence[int], batch_sizes: Sequence[int],
                              beam: int = 0, stream: int = 0) -> List[SearchResult]:
        """Consecutive batches (batch_sizes[i] chunks each) decoded with batch k+1's encoder
        overlapping batch k's search; results for every chunk, in chunk order."""
        n = len(lengths)
        off = (C.c_int64 * n)(*offsets)
        ln = (C.c_int64 * n)(*lengths)
        bs = (C.c_int32 * len(batch_sizes))(*batch_sizes)
        res = C.c_void_p()
        try:
            self._check(self.lib.zasr_decode_device_batches(
                self.handle, C.c_void_p(d_wav_ptr), off, ln, n, bs, len(batch_sizes), beam,
                C.c_void_p(stream), C.byref(res)))
        except ZasrError as e:
            return self._retry(e, "decode_device_batches", d_wav_ptr, offsets, lengths,
                               batch_sizes, beam=beam, stream=stream)
        return self._collect(res)

    def decode_host_batches(self, h_wav_ptr: int, offsets: Sequence[int],
                            lengths: Sequence[int], batch_sizes: Sequence[int],
                            beam: int = 0, stream: int = 0) -> List[SearchResult]:
        """decode_device_batches from HOST waveforms at h_wav_ptr (pinned for an asynchronous
        upload): each batch's samples are copied on the engine's copy stream under the
        previous batch's work (zasr_decode_host_batches)."""
        n = len(lengths)
        off = (C.c_int64 * n)(*offsets)
        ln = (C.c_int64 * n)(*lengths)
        bs = (C.c_int32 * len(batch_sizes))(*batch_sizes)
        res = C.c_void_p()
        try:
            self._check(self.lib.zasr_decode_host_batches(
                self.handle, C.c_void_p(h_wav_ptr), off, ln, n, bs, len(batch_sizes), beam,
                C.c_void_p(stream), C.byref(res)))
        except ZasrError as e:
            return self._retry(e, "decode_host_batches", h_wav_ptr, offsets, lengths,
                               batch_sizes, beam=beam, stream=stream)
        return self._collect(res)

    def encode_features(self, feats: Sequence) -> List[np.ndarray]:
        arrs = [_f32(f) for f in feats]
        ns = (C.c_int64 * len(arrs))(*[a.shape[0] for a in arrs])
        tot = sum(((a.shape[0] - 7) // 2 + 1) // 2 for a in arrs)
        out = np.empty((max(tot, 1), self.joiner_dim), dtype=np.float32)
        tout = (C.c_int64 * len(arrs))()
        fp = C.POINTER(C.c_float)
        self._check(self.lib.zasr_encode_features(self.handle, _ptr_array(arrs), ns, len(arrs),
                                                  out.ctypes.data_as(fp), out.size, tout))
        res, pos = [], 0
        for i in range(len(arrs)):
            res.append(out[pos: pos + tout[i]].copy())
            pos += tout[i]
        return res

    def search(self, enc_outs: Sequence, beam: int = 0) -> List[SearchResult]:
        arrs = [_f32(e).reshape(-1, self.joiner_dim) for e in enc_outs]
        ns = (C.c_int64 * len(arrs))(*[a.shape[0] for a in arrs])
        res = C.c_void_p()
        self._check(self.lib.zasr_search_encoder_out(self.handle, _ptr_array(arrs), ns,
                                                     len(arrs), beam, C.byref(res)))
        return self._collect(res)

    # profiling (HIP events on the library's stream)
    def profile(self, on=True):
        """on: False/0 off, True/1 kernel classes, 2 = GEMMs split by shape."""
        self._check(self.lib.zasr_profile_enable(self.handle, int(on)))

    def profile_reset(self):
        self._check(self.lib.zasr_profile_reset(self.handle))

    def profile_report(self) -> dict:
        buf = C.create_string_buffer(1 << 16)
        self._check(self.lib.zasr_profile_report(self.handle, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, cnt, ms = line.split()
            out[name] = (int(cnt), float(ms))
        return out


class CamppEmbedder:
    """CAM++ speaker embeddings on the GPU (include/zasr.h zasr_campp_*): the reference's
    numpy fbank (core/speaker_diarization_senko_campp_optimized.py:86-159) and its batched
    ONNX CAM++ session (:589-605)."""

    def __init__(self, model_dir: str, device_id: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        rc = self.lib.zasr_campp_create(model_dir.encode(), device_id, C.byref(h))
        if rc != 0:
            msg = self.lib.zasr_last_error().decode()
            if rc == 2:
                raise FileNotFoundError(msg)
            raise ZasrError(msg)
        self.handle = h
        self.dim = self.lib.zasr_campp_embedding_dim(h)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.zasr_campp_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ZasrError(self.lib.zasr_last_error().decode())

    def routes(self) -> dict:
        """Which kernel each part of the loaded model was routed to (zasr_model_routes)."""
        import json
        buf = C.create_string_buffer(1024)
        self._check(self.lib.zasr_model_routes(self.handle, buf, len(buf)))
        return json.loads(buf.value.decode())

    def set_mel_banks(self, banks) -> None:
        """Replace the fbank's 80 triangular filters ([80][256] or [80][257] weights;
        zasr_fbank_set_mel_banks)."""
        b = _f32(banks)
        if b.ndim != 2 or b.shape[0] != 80 or b.shape[1] not in (256, 257):
            raise ValueError("mel banks must be [80][256] or [80][257]")
        self._check(self.lib.zasr_fbank_set_mel_banks(
            self.handle, b.ctypes.data_as(C.POINTER(C.c_float)), b.shape[1]))

    def fbank(self, audio) -> np.ndarray:
        a = _f32(audio)
        n = a.shape[0]
        frames = 1 + (n - 400) // 160 if n >= 400 else 0
        out = np.empty((max(frames, 1), 80), dtype=np.float32)
        nf = C.c_int64()
        fp = C.POINTER(C.c_float)
        self._check(self.lib.zasr_campp_fbank(self.handle, a.ctypes.data_as(fp), n,
                                              out.ctypes.data_as(fp), out.size, C.byref(nf)))
        return out[: nf.value]

    def embed(self, feats) -> np.ndarray:
        x = _f32(feats)
        if x.ndim != 3 or x.shape[2] != 80:
            raise ValueError("feats must be [N, T, 80]")
        out = np.empty((x.shape[0], self.dim), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.zasr_campp_embed(self.handle, x.ctypes.data_as(fp), x.shape[0],
                                              x.shape[1], out.ctypes.data_as(fp)))
        return out

    def embed_device(self, d_feats: int, count: int, n_frames: int, d_out: int, stream: int = 0):
        self._check(self.lib.zasr_campp_embed_device(self.handle, C.c_void_p(d_feats), count,
                                                     n_frames, C.c_void_p(d_out),
                                                     C.c_void_p(stream)))


    def windows_device(self, d_wav: int, region_off: Sequence[int], region_len: Sequence[int],
                       d_feats: int, max_windows: int, window_frames: int = 150,
                       step_frames: int = 60, stream: int = 0):
        """fbank + CMVN of every speech region of a waveform in HBM and its 1.5 s windows
        gathered into d_feats [n][window_frames][80] (zasr_campp_windows_device; the reference's
        _sliding_window_embeddings front end, core/speaker_diarization_senko_campp_optimized.py:
        540-600).  Returns (region, first frame, frame count) int32 arrays of the n windows."""
        off = np.ascontiguousarray(region_off, dtype=np.int64)
        ln = np.ascontiguousarray(region_len, dtype=np.int64)
        if off.shape != ln.shape:
            raise ValueError("region_off and region_len differ in length")
        cap = max(0, int(max_windows))
        reg = np.empty(max(cap, 1), np.int32)
        first = np.empty(max(cap, 1), np.int32)
        nfr = np.empty(max(cap, 1), np.int32)
        n = C.c_int64()
        i64p = C.POINTER(C.c_int64)
        i32p = C.POINTER(C.c_int32)
        self._check(self.lib.zasr_campp_windows_device(
            self.handle, C.c_void_p(d_wav), off.ctypes.data_as(i64p), ln.ctypes.data_as(i64p),
            off.size, window_frames, step_frames, C.c_void_p(d_feats), cap,
            reg.ctypes.data_as(i32p), first.ctypes.data_as(i32p), nfr.ctypes.data_as(i32p),
            C.byref(n), C.c_void_p(stream)))
        k = n.value
        return reg[:k], first[:k], nfr[:k]


class VibertSession:
    """ViBERT-capu on the GPU with the onnxruntime InferenceSession surface the reference's
    GecBERTModel uses (core/gec_model.py:366-412): run(None, feeds) -> [logits,
    detect_logits] for feeds {input_ids, attention_mask, token_type_ids, input_offsets}."""

    def __init__(self, model_dir: str, device_id: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        rc = self.lib.zasr_vibert_create(model_dir.encode(), device_id, C.byref(h))
        if rc != 0:
            msg = self.lib.zasr_last_error().decode()
            if rc == 2:
                raise FileNotFoundError(msg)
            raise ZasrError(msg)
        self.handle = h
        self.num_labels = self.lib.zasr_vibert_num_labels(h)
        self.num_detect = self.lib.zasr_vibert_num_detect(h)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.zasr_vibert_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, output_names, feeds):
        i64 = lambda k: np.ascontiguousarray(np.asarray(feeds[k]), dtype=np.int64)  # noqa: E731
        ids, am, tt, off = (i64(k) for k in ("input_ids", "attention_mask", "token_type_ids",
                                              "input_offsets"))
        B, L = ids.shape
        W = off.shape[1]
        lg = np.empty((B, W, self.num_labels), np.float32)
        dl = np.empty((B, W, self.num_detect), np.float32)
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
        fp = C.POINTER(C.c_float)
        rc = self.lib.zasr_vibert_run(self.handle, p(ids), p(am), p(tt), p(off), B, L, W,
                                      lg.ctypes.data_as(fp), dl.ctypes.data_as(fp))
        if rc != 0:
            raise ZasrError(self.lib.zasr_last_error().decode())
        outs = {"logits": lg, "detect_logits": dl}
        return [lg, dl] if output_names is None else [outs[n] for n in output_names]


class VadSession:
    """Silero VAD on the GPU.  probs() runs whole files (the reference's
    per-window loop at core/vad_utils.py:80-111, batched); run(None, feeds) is the
    onnxruntime session surface ({input [n, 576], state [2, n, 128], sr} -> [prob [n, 1],
    state]) for the reference's per-window callers."""

    def __init__(self, model_dir: str, device_id: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        rc = self.lib.zasr_vad_create(model_dir.encode(), device_id, C.byref(h))
        if rc != 0:
            msg = self.lib.zasr_last_error().decode()
            if rc == 2:
                raise FileNotFoundError(msg)
            raise ZasrError(msg)
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.lib.zasr_vad_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ZasrError(self.lib.zasr_last_error().decode())

    def probs(self, audios: Sequence[np.ndarray], auto_boost: bool = False) -> List[np.ndarray]:
        audios = [np.ascontiguousarray(a, np.float32) for a in audios]
        lens = np.array([a.shape[0] for a in audios], np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        flat = np.concatenate(audios) if audios else np.zeros(0, np.float32)
        nw = lens // 512
        out = np.empty(int(nw.sum()), np.float32)
        fp = C.POINTER(C.c_float)
        i64 = C.POINTER(C.c_int64)
        if out.size:
            self._check(self.lib.zasr_vad_probs(self.handle, flat.ctypes.data_as(fp),
                                                offs.ctypes.data_as(i64), lens.ctypes.data_as(i64),
                                                len(audios), int(auto_boost),
                                                out.ctypes.data_as(fp)))
        bounds = np.concatenate([[0], np.cumsum(nw)])
        return [out[bounds[i]:bounds[i + 1]] for i in range(len(audios))]

    @property
    def last_passes(self) -> int:
        return int(self.lib.zasr_vad_last_passes(self.handle))

    def probs_device(self, d_audio: int, offsets: Sequence[int], lengths: Sequence[int],
                     d_probs: int, auto_boost: bool = False, stream: int = 0) -> None:
        offs = np.ascontiguousarray(offsets, np.int64)
        lens = np.ascontiguousarray(lengths, np.int64)
        i64 = C.POINTER(C.c_int64)
        self._check(self.lib.zasr_vad_probs_device(
            self.handle, C.c_void_p(d_audio), offs.ctypes.data_as(i64), lens.ctypes.data_as(i64),
            len(offs), int(auto_boost), C.c_void_p(d_probs), C.c_void_p(stream)))

    def run(self, output_names, feeds):
        x = np.ascontiguousarray(feeds["input"], np.float32)
        st = np.ascontiguousarray(feeds["state"], np.float32)
        sr = int(np.asarray(feeds.get("sr", 16000)))
        if sr != 16000 or x.ndim != 2 or x.shape[1] != 576 or st.shape != (2, x.shape[0], 128):
            raise ZasrError("Silero VAD session: input [n, 576] at 16 kHz, state [2, n, 128]")
        n = x.shape[0]
        p = np.empty(n, np.float32)
        so = np.empty_like(st)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.zasr_vad_window(self.handle, x.ctypes.data_as(fp),
                                             st.ctypes.data_as(fp), n, p.ctypes.data_as(fp),
                                             so.ctypes.data_as(fp)))
        return [p[:, None], so]


class SegSession:
    """PyanNet segmentation on the GPU.  run(None, {"input_values": batch
    [n, 1, T]}) -> [log-probabilities [n, F, 7]] is the onnxruntime session surface, so
    `diarizer.seg_sess = SegSession(model_dir)` serves the reference's own _pyannote_vad
    (core/speaker_diarization_senko_campp_optimized.py:435); classes_device() runs every chunk
    of a file from the 16 kHz signal already in HBM."""

    CHUNK = 160000   # :413
    STEP = 80000     # :415
    MIN_SAMPLES = 1261

    def __init__(self, model_dir: str, device_id: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        rc = self.lib.zasr_seg_create(model_dir.encode(), device_id, C.byref(h))
        if rc != 0:
            msg = self.lib.zasr_last_error().decode()
            if rc == 2:
                raise FileNotFoundError(msg)
            raise ZasrError(msg)
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.lib.zasr_seg_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ZasrError(self.lib.zasr_last_error().decode())

    def num_frames(self, chunk_samples: int) -> int:
        return int(self.lib.zasr_seg_num_frames(self.handle, int(chunk_samples)))

    def num_chunks(self, total: int, chunk_samples: int = CHUNK, step_samples: int = STEP) -> int:
        return int(self.lib.zasr_seg_num_chunks(int(total), int(chunk_samples), int(step_samples)))

    @property
    def last_group(self) -> int:
        """Sequences per recurrence workgroup of the last call (diagnostic)."""
        return int(self.lib.zasr_seg_last_group(self.handle))

    def set_group(self, group: int) -> None:
        """Force the recurrence group (1, 2, 4, 8, 16; 0 = automatic).  Results do not change."""
        self._check(self.lib.zasr_seg_set_group(self.handle, int(group)))

    def trim(self) -> None:
        """Free the activation workspace the handle keeps between calls (8.6 MB per 10 s chunk
        of the longest file seen, at most 8 GiB)."""
        self._check(self.lib.zasr_seg_trim(self.handle))

    STAGES = ("front", "convs", "projections", "recurrence", "head")

    def set_profile(self, on: bool) -> None:
        self._check(self.lib.zasr_seg_set_profile(self.handle, int(bool(on))))

    def stage_ms(self) -> dict:
        """Milliseconds of the last call's stages (after set_profile(True))."""
        ms = (C.c_float * 5)()
        self._check(self.lib.zasr_seg_stage_ms(self.handle, ms))
        return dict(zip(self.STAGES, (float(v) for v in ms)))

    def logits(self, batch: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(batch, np.float32)
        if x.ndim == 3 and x.shape[1] == 1:
            x = x[:, 0, :]
        if x.ndim != 2:
            raise ZasrError("segmentation session: input_values [n, 1, T] or [n, T]")
        n, T = x.shape
        if n <= 0 or T < self.MIN_SAMPLES:
            raise ZasrError(f"segmentation session: n >= 1 and T >= {self.MIN_SAMPLES} "
                            f"(got n = {n}, T = {T})")
        x = np.ascontiguousarray(x)
        out = np.empty((n, self.num_frames(T), 7), np.float32)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.zasr_seg_logits(self.handle, x.ctypes.data_as(fp), n, T,
                                             out.ctypes.data_as(fp)))
        return out

    def run(self, output_names, feeds):
        return [self.logits(feeds["input_values"])]

    def classes_device(self, d_audio: int, total: int, chunk_samples: int = CHUNK,
                       step_samples: int = STEP, d_logits: int = 0, stream: int = 0) -> np.ndarray:
        """Class map [n_chunks, F] (uint8) of the signal d_audio[0, total) (a device pointer);
        d_logits (device, [n_chunks, F, 7] float32) is filled when given."""
        if chunk_samples < self.MIN_SAMPLES:
            raise ZasrError(f"segmentation session: chunks need >= {self.MIN_SAMPLES} samples")
        n = self.num_chunks(total, chunk_samples, step_samples)
        out = np.empty((n, self.num_frames(chunk_samples)), np.uint8)
        if n:
            self._check(self.lib.zasr_seg_classes_device(
                self.handle, C.c_void_p(d_audio), int(total), int(chunk_samples), int(step_samples),
                out.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_void_p(d_logits), C.c_void_p(stream)))
        return out


class SepSession:
    """Conv-TasNet overlap separation on the GPU.  run(None, {"mixture": x[1, T]})
    -> [sources [1, 2, T]] is the onnxruntime session surface the reference calls once per
    region (core/overlap_separator.py:291); separate() takes every region of a file in one
    call and separate_device() cuts them from the 16 kHz signal already in HBM.  A region's
    result does not depend on the other regions of the call."""

    STAGES = ("encoder", "gemms", "norms_depthwise", "mask_decoder")

    def __init__(self, model_dir: str, device_id: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        rc = self.lib.zasr_sep_create(model_dir.encode(), device_id, C.byref(h))
        if rc != 0:
            msg = self.lib.zasr_last_error().decode()
            if rc == 2:
                raise FileNotFoundError(msg)
            raise ZasrError(msg)
        self.handle = h
        self.min_samples = int(self.lib.zasr_sep_min_samples(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.zasr_sep_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ZasrError(self.lib.zasr_last_error().decode())

    def trim(self) -> None:
        """Free the activation workspace the handle keeps between calls."""
        self._check(self.lib.zasr_sep_trim(self.handle))

    def set_budget(self, nbytes: int) -> None:
        """Activation bytes one launch group may take (default 4 GiB).  Results do not change."""
        self._check(self.lib.zasr_sep_set_budget(self.handle, int(nbytes)))

    @property
    def last_groups(self) -> int:
        """Launch groups of the last call (diagnostic)."""
        return int(self.lib.zasr_sep_last_groups(self.handle))

    def set_profile(self, on: bool) -> None:
        self._check(self.lib.zasr_sep_set_profile(self.handle, int(bool(on))))

    def stage_ms(self) -> dict:
        """Milliseconds of the last call's stages (after set_profile(True))."""
        ms = (C.c_float * 4)()
        self._check(self.lib.zasr_sep_stage_ms(self.handle, ms))
        return dict(zip(self.STAGES, (float(v) for v in ms)))

    @staticmethod
    def _split(flat: np.ndarray, lengths) -> List[np.ndarray]:
        out, o = [], 0
        for T in lengths:
            out.append(flat[o:o + 2 * T].reshape(2, T))
            o += 2 * T
        return out

    def separate(self, mixtures: Sequence[np.ndarray]) -> List[np.ndarray]:
        """Raw network output [2, T_r] (float32) of every mixture [T_r], one device call."""
        xs = [np.ascontiguousarray(m, np.float32).reshape(-1) for m in mixtures]
        if not xs:
            return []
        lengths = np.array([x.shape[0] for x in xs], np.int64)
        offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
        return self.separate_concat(np.concatenate(xs), offsets, lengths)

    def separate_concat(self, samples: np.ndarray, offsets, lengths) -> List[np.ndarray]:
        """The C entry's own form: region r = samples[offsets[r] : offsets[r] + lengths[r]]."""
        samples = np.ascontiguousarray(samples, np.float32).reshape(-1)
        offsets = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        lengths = np.ascontiguousarray(lengths, np.int64).reshape(-1)
        if offsets.shape != lengths.shape:
            raise ValueError("offsets and lengths differ in length")
        out = np.empty(max(1, 2 * int(np.clip(lengths, 0, None).sum())), np.float32)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int64)
        self._check(self.lib.zasr_sep_separate(
            self.handle, samples.ctypes.data_as(fp), samples.shape[0], offsets.ctypes.data_as(ip),
            lengths.ctypes.data_as(ip), lengths.shape[0], out.ctypes.data_as(fp)))
        return self._split(out, [int(t) for t in lengths])

    def separate_device(self, d_audio: int, total: int, starts, lengths, d_out: int = 0,
                        stream: int = 0) -> Optional[List[np.ndarray]]:
        """Regions [starts[r], starts[r] + lengths[r]) of the signal d_audio[0, total) (a device
        pointer).  With d_out (a device pointer to 2 * sum(lengths) float32) the result stays on
        the device and None is returned; else the host arrays [2, T_r]."""
        starts = np.ascontiguousarray(starts, np.int64).reshape(-1)
        lengths = np.ascontiguousarray(lengths, np.int64).reshape(-1)
        if starts.shape != lengths.shape:
            raise ValueError("starts and lengths differ in length")
        ip = C.POINTER(C.c_int64)
        host = None if d_out else np.empty(max(1, 2 * int(np.clip(lengths, 0, None).sum())), np.float32)
        dst = C.c_void_p(d_out) if d_out else C.c_void_p(host.ctypes.data)
        self._check(self.lib.zasr_sep_separate_device(
            self.handle, C.c_void_p(d_audio), int(total), starts.ctypes.data_as(ip),
            lengths.ctypes.data_as(ip), lengths.shape[0], dst, int(bool(d_out)), C.c_void_p(stream)))
        return None if d_out else self._split(host, [int(t) for t in lengths])

    def run(self, output_names, feeds):
        x = np.ascontiguousarray(feeds["mixture"], np.float32)
        if x.ndim != 2 or x.shape[0] != 1:
            raise ZasrError("separation session: mixture [1, T]")
        return [self.separate([x[0]])[0][None]]


class _EmbValue:
    """OrtValue-shaped holder: .numpy()."""

    def __init__(self, a: np.ndarray):
        self._a = a

    def numpy(self) -> np.ndarray:
        return self._a


class _EmbOutput:
    def __init__(self, name: str):
        self.name = name


class _EmbIoBinding:
    """The io-binding surface core/speaker_diarization_pure_ort.py:823-845 drives."""

    def __init__(self):
        self.inputs = {}
        self.output_names = []
        self.outputs = []

    def bind_cpu_input(self, name: str, array) -> None:
        self.inputs[name] = array

    def bind_output(self, name: str, *args, **kwargs) -> None:
        if name not in self.output_names:
            self.output_names.append(name)

    def get_outputs(self):
        return self.outputs

    def clear_binding_inputs(self) -> None:
        self.inputs = {}

    def clear_binding_outputs(self) -> None:
        self.output_names, self.outputs = [], []


class EmbSession:
    """Community-1 speaker embeddings on the GPU: the encoder session of
    core/speaker_diarization_pure_ort.py.  run(None, {"fbank_features": x [n, T, 80]}) ->
    [frame features [n, 2560, T']], get_outputs(), io_binding() and run_with_iobinding() are
    the onnxruntime surface the reference drives (:823-845, :699); chunk_embeddings() runs the
    whole of _extract_embeddings from the 16 kHz signal (host, or already in HBM) and
    segment_embedding() compute_single_embedding.  A chunk's embedding does not depend on the
    other chunks of the call."""

    INPUT_NAME = "fbank_features"
    OUTPUT_NAME = "/resnet/pool/Reshape_output_0"   # convert_onnx/split_pyannote_embedding.py:6
    STAGES = ("front", "stem", "layer1", "layer2", "layer3", "layer4", "pooling", "projection")
    CHUNK_FRAMES = 998
    TAIL = 160000
    SPEAKERS = 3

    def __init__(self, model_dir: str, device_id: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        rc = self.lib.zasr_emb_create(model_dir.encode(), device_id, C.byref(h))
        if rc != 0:
            msg = self.lib.zasr_last_error().decode()
            if rc == 2:
                raise FileNotFoundError(msg)
            raise ZasrError(msg)
        self.handle = h
        self.model_dir = model_dir
        self.embedding_dim = int(self.lib.zasr_emb_embedding_dim(self.handle))
        self.feat_width = 2560   # 256 channels x 10 bins: the engine takes feat_dim 80, m_channels 32

    def close(self):
        if getattr(self, "handle", None):
            self.lib.zasr_emb_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ZasrError(self.lib.zasr_last_error().decode())

    def num_feat_frames(self, T: int) -> int:
        return int(self.lib.zasr_emb_num_feat_frames(self.handle, int(T)))

    def encoder_flops(self, T: int) -> float:
        """Multiply-adds x 2 of the encoder on one input of T frames (from the model's config)."""
        return float(self.lib.zasr_emb_encoder_flops(self.handle, int(T)))

    def set_group(self, group: int) -> None:
        """Inputs per launch group (1 .. 128; 0 = from the free memory).  Results do not change."""
        self._check(self.lib.zasr_emb_set_group(self.handle, int(group)))

    @property
    def last_group(self) -> int:
        return int(self.lib.zasr_emb_last_group(self.handle))

    def trim(self) -> None:
        """Free the activation workspace the handle keeps between calls."""
        self._check(self.lib.zasr_emb_trim(self.handle))

    def set_profile(self, on: bool) -> None:
        self._check(self.lib.zasr_emb_set_profile(self.handle, int(bool(on))))

    def stage_ms(self) -> dict:
        """Milliseconds of the last call's stages (after set_profile(True))."""
        ms = (C.c_float * 8)()
        self._check(self.lib.zasr_emb_stage_ms(self.handle, ms))
        return dict(zip(self.STAGES, (float(v) for v in ms)))

    def fbank(self, audio: np.ndarray, tail: int = 0) -> np.ndarray:
        """compute_emb_fbank's rows before its CMVN (:271-301) of the samples followed by `tail`
        zeros: [rows, 80]."""
        x = np.ascontiguousarray(audio, np.float32).reshape(-1)
        n = x.shape[0]
        rows = 1 + (n + tail - 400) // 160 if n + tail >= 400 else 0
        out = np.empty((rows, 80), np.float32)
        got = C.c_int64(0)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.zasr_emb_fbank(self.handle, x.ctypes.data_as(fp), n, int(tail),
                                            out.ctypes.data_as(fp), out.size, C.byref(got)))
        assert got.value == rows
        return out

    def encode(self, feats: np.ndarray) -> np.ndarray:
        """feats [n, T, 80] -> frame features [n, 2560, T'] (channel c * 10 + f)."""
        x = np.ascontiguousarray(feats, np.float32)
        if x.ndim != 3 or x.shape[2] != 80 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ZasrError("embedding session: fbank_features [n, T, 80]")
        n, T, _ = x.shape
        out = np.empty((n, self.feat_width, self.num_feat_frames(T)), np.float32)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.zasr_emb_encode(self.handle, x.ctypes.data_as(fp), n, T,
                                             out.ctypes.data_as(fp)))
        return out

    def chunk_embeddings_device(self, d_audio: int, total: int, chunk_starts, masks_u8,
                                stream: int = 0) -> np.ndarray:
        """Embeddings [n_chunks, 3, 256] of the chunks at chunk_starts of the signal
        d_audio[0, total) (a device pointer) under masks_u8 [n_chunks, 3, n_seg_frames]."""
        starts = np.ascontiguousarray(chunk_starts, np.int64).reshape(-1)
        m = np.ascontiguousarray(masks_u8, np.uint8)
        if m.ndim != 3 or m.shape[0] != starts.shape[0] or m.shape[1] != self.SPEAKERS:
            raise ZasrError("embedding session: masks [n_chunks, 3, n_seg_frames]")
        out = np.empty((starts.shape[0], self.SPEAKERS, self.embedding_dim), np.float32)
        if starts.shape[0] == 0:
            return out
        self._check(self.lib.zasr_emb_chunks_device(
            self.handle, C.c_void_p(d_audio), int(total), starts.ctypes.data_as(C.POINTER(C.c_int64)),
            starts.shape[0], m.ctypes.data_as(C.POINTER(C.c_uint8)), m.shape[2],
            out.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(stream)))
        return out

    def chunk_embeddings(self, audio: np.ndarray, chunk_starts, masks_u8) -> np.ndarray:
        """The same from a host signal (uploaded through torch for the call)."""
        import torch
        x = torch.from_numpy(np.ascontiguousarray(audio, np.float32).reshape(-1)).cuda()
        torch.cuda.synchronize()
        return self.chunk_embeddings_device(x.data_ptr(), x.shape[0], chunk_starts, masks_u8)

    def segment_embedding(self, audio: np.ndarray) -> Optional[np.ndarray]:
        """compute_single_embedding (:681-707): [256], or None under 9 fbank frames.  Any length
        up to 2^20 fbank frames (2.9 h)."""
        x = np.ascontiguousarray(audio, np.float32).reshape(-1)
        out = np.empty(self.embedding_dim, np.float32)
        ok = C.c_int32(0)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.zasr_emb_segment(self.handle, x.ctypes.data_as(fp), x.shape[0],
                                              out.ctypes.data_as(fp), C.byref(ok)))
        return out if ok.value else None

    # ---- the onnxruntime surface ----
    def run(self, output_names, feeds):
        return [self.encode(feeds[self.INPUT_NAME])]

    def get_outputs(self):
        return [_EmbOutput(self.OUTPUT_NAME)]

    def io_binding(self) -> _EmbIoBinding:
        return _EmbIoBinding()

    def run_with_iobinding(self, binding: _EmbIoBinding) -> None:
        if self.INPUT_NAME not in binding.inputs:
            raise ZasrError("embedding session: bind_cpu_input('fbank_features', ...) first")
        if not binding.output_names:
            raise ZasrError("embedding session: bind_output(...) first")
        binding.outputs = [_EmbValue(self.encode(binding.inputs[self.INPUT_NAME]))]


AUDIO_FORMATS = {"float32": 0, "int16": 1}  # include/zasr.h ZASR_AUDIO_F32 / ZASR_AUDIO_I16


def audio_out_len(sample_rate: int, n_frames: int, lib_path: Optional[str] = None) -> int:
    """Samples the front end makes of n_frames frames at sample_rate (zasr_audio_out_len,
    host only): ceil(n_frames * 16000 / sample_rate)."""
    lib = load_library(lib_path)
    n = int(lib.zasr_audio_out_len(int(sample_rate), int(n_frames)))
    if n < 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return n


def audio_resample_taps(sample_rate: int, lib_path: Optional[str] = None) -> dict:
    """The front end's polyphase table of one input rate (zasr_audio_resample_taps, host only):
    {"P", "Q", "taps", "out_tile", "in_tile", "lo" int32 [P], "w" float32 [P, taps]}."""
    lib = load_library(lib_path)
    v = [C.c_int32() for _ in range(5)]
    refs = [C.byref(x) for x in v]
    if lib.zasr_audio_resample_taps(int(sample_rate), *refs, None, None, 0) != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    Pn, Q, taps, out_tile, in_tile = (x.value for x in v)
    lo = np.empty(Pn, np.int32)
    w = np.empty((Pn, taps), np.float32)
    if lib.zasr_audio_resample_taps(int(sample_rate), *refs,
                                    lo.ctypes.data_as(C.POINTER(C.c_int32)),
                                    w.ctypes.data_as(C_FP), w.size) != 0:
        raise ZasrError(lib.zasr_last_error().decode())
    return {"P": Pn, "Q": Q, "taps": taps, "out_tile": out_tile, "in_tile": in_tile,
            "lo": lo, "w": w}


class AudioFrontEnd:
    """The device audio front end (include/zasr.h zasr_audio_*): raw PCM to the 16 kHz mono
    float32 signal in HBM, and the level passes of the reference's load_audio boost and
    preprocess_audio on that signal.  Signals and outputs are device pointers (ints); a PCM
    source is a numpy array (host) or a device pointer.  zasr/audio.py is the numpy / torch
    surface over this class."""

    def __init__(self, device_id: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        if self.lib.zasr_audio_create(int(device_id), C.byref(h)) != 0:
            raise ZasrError(self.lib.zasr_last_error().decode())
        self.handle = h
        self.device_id = int(device_id)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.zasr_audio_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ZasrError(self.lib.zasr_last_error().decode())

    def to_16k(self, src, sample_rate: int, d_out: int, cap: int, channels: int = 1,
               n_frames: Optional[int] = None, fmt: Optional[str] = None,
               stream: int = 0) -> int:
        """src: a C-contiguous numpy array [n] or [n, C] of float32 / int16 (host source), or
        a device pointer with n_frames, channels and fmt ("float32" | "int16").  Writes the
        16 kHz signal at device pointer d_out (cap samples); returns its length."""
        if isinstance(src, np.ndarray):
            if src.dtype.name not in AUDIO_FORMATS or src.ndim not in (1, 2):
                raise ValueError("samples must be float32 or int16, shaped [n] or [n, channels]")
            keep = np.ascontiguousarray(src)
            n_frames, channels = keep.shape[0], (keep.shape[1] if keep.ndim == 2 else 1)
            fmt, ptr, on_device = keep.dtype.name, keep.ctypes.data, 0
        else:
            if n_frames is None or fmt not in AUDIO_FORMATS:
                raise ValueError("a device source needs n_frames and fmt")
            keep, ptr, on_device = None, int(src), 1
        n_out = C.c_int64()
        self._check(self.lib.zasr_audio_to_16k(
            self.handle, C.c_void_p(ptr), AUDIO_FORMATS[fmt], int(channels), int(sample_rate),
            int(n_frames), on_device, C.c_void_p(d_out), int(cap), C.byref(n_out),
            C.c_void_p(stream)))
        del keep
        return int(n_out.value)

    def peak(self, d_wav: int, n: int, stream: int = 0) -> np.float32:
        v = C.c_float()
        self._check(self.lib.zasr_audio_peak(self.handle, C.c_void_p(d_wav), int(n), C.byref(v),
                                             C.c_void_p(stream)))
        return np.float32(v.value)

    def scale(self, d_wav: int, n: int, divisor, multiplier, stream: int = 0) -> None:
        """d_wav = (d_wav / divisor) * multiplier in float32."""
        self._check(self.lib.zasr_audio_scale(self.handle, C.c_void_p(d_wav), int(n),
                                              float(np.float32(divisor)),
                                              float(np.float32(multiplier)), C.c_void_p(stream)))

    def segment_sumsq(self, d_wav: int, n: int, seg_begin, seg_end, stream: int = 0) -> np.ndarray:
        b = np.ascontiguousarray(seg_begin, np.int64)
        e = np.ascontiguousarray(seg_end, np.int64)
        if b.shape != e.shape or b.ndim != 1:
            raise ValueError("seg_begin and seg_end differ in length")
        out = np.zeros(b.size, np.float64)
        i64 = C.POINTER(C.c_int64)
        self._check(self.lib.zasr_audio_segment_sumsq(
            self.handle, C.c_void_p(d_wav), int(n), b.ctypes.data_as(i64), e.ctypes.data_as(i64),
            b.size, out.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(stream)))
        return out

    def apply_gain(self, d_wav: int, n: int, piece_begin, piece_end, piece_gain, piece_ramp,
                   ramp_values, stream: int = 0) -> np.float32:
        """d_wav *= the sparse gain plan (zasr_audio_apply_gain); returns max |result|."""
        pb = np.ascontiguousarray(piece_begin, np.int64)
        pe = np.ascontiguousarray(piece_end, np.int64)
        pg = np.ascontiguousarray(piece_gain, np.float32)
        po = np.ascontiguousarray(piece_ramp, np.int64)
        rv = np.ascontiguousarray(ramp_values, np.float32)
        if not (pb.shape == pe.shape == pg.shape == po.shape) or pb.ndim != 1:
            raise ValueError("plan arrays differ in length")
        i64 = C.POINTER(C.c_int64)
        v = C.c_float()
        self._check(self.lib.zasr_audio_apply_gain(
            self.handle, C.c_void_p(d_wav), int(n), pb.ctypes.data_as(i64),
            pe.ctypes.data_as(i64), pg.ctypes.data_as(C_FP), po.ctypes.data_as(i64), pb.size,
            rv.ctypes.data_as(C_FP), rv.size, C.byref(v), C.c_void_p(stream)))
        return np.float32(v.value)


class WpeEngine:
    """WPE dereverberation on the GPU (include/zasr.h zasr_wpe_*): every chunk of a
    file in one call, each frequency bin on its own.  zasr/audio.py is the numpy / torch surface
    over this class; the selftest_* methods run one kernel on one chunk's host operands."""

    STAGES = ("stft", "iterations", "istft")
    BINS = 257

    def __init__(self, device_id: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        if self.lib.zasr_wpe_create(int(device_id), C.byref(h)) != 0:
            raise ZasrError(self.lib.zasr_last_error().decode())
        self.handle = h
        self.device_id = int(device_id)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.zasr_wpe_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ZasrError(self.lib.zasr_last_error().decode())

    def trim(self) -> None:
        self._check(self.lib.zasr_wpe_trim(self.handle))

    def set_budget(self, nbytes: int) -> None:
        """Spectrum bytes one launch group may take (default 2 GiB).  Results do not change."""
        self._check(self.lib.zasr_wpe_set_budget(self.handle, int(nbytes)))

    @property
    def last_groups(self) -> int:
        return int(self.lib.zasr_wpe_last_groups(self.handle))

    def set_profile(self, on: bool) -> None:
        self._check(self.lib.zasr_wpe_set_profile(self.handle, int(bool(on))))

    def stage_ms(self) -> dict:
        ms = (C.c_float * 3)()
        self._check(self.lib.zasr_wpe_stage_ms(self.handle, ms))
        return dict(zip(self.STAGES, (float(v) for v in ms)))

    @staticmethod
    def _spans(offsets, lens, out_offsets):
        o = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        n = np.ascontiguousarray(lens, np.int64).reshape(-1)
        if out_offsets is None:
            out_offsets = np.concatenate([[0], np.cumsum(np.clip(n, 0, None))[:-1]]) if n.size else n
        q = np.ascontiguousarray(out_offsets, np.int64).reshape(-1)
        if not (o.shape == n.shape == q.shape):
            raise ValueError("offsets, lens and out_offsets differ in length")
        return o, n, q

    def run_device(self, d_audio: int, total: int, offsets, lens, d_out: int, out_offsets=None,
                   taps: int = 10, delay: int = 3, iterations: int = 3, stream: int = 0) -> np.ndarray:
        """Chunks [offsets[c], offsets[c] + lens[c]) of the device signal d_audio[0, total) ->
        device pointer d_out at out_offsets (default: packed in order).  Returns out_offsets."""
        o, n, q = self._spans(offsets, lens, out_offsets)
        ip = C.POINTER(C.c_int64)
        self._check(self.lib.zasr_wpe_run_device(
            self.handle, C.c_void_p(d_audio), int(total), o.ctypes.data_as(ip), n.ctypes.data_as(ip),
            o.size, int(taps), int(delay), int(iterations), C.c_void_p(d_out), q.ctypes.data_as(ip),
            C.c_void_p(stream)))
        return q

    def run(self, audio: np.ndarray, offsets, lens, taps: int = 10, delay: int = 3,
            iterations: int = 3) -> List[np.ndarray]:
        """The same on a host signal: the chunks' float32 outputs."""
        a = np.ascontiguousarray(audio, np.float32).reshape(-1)
        o, n, q = self._spans(offsets, lens, None)
        out = np.zeros(max(1, int(np.clip(n, 0, None).sum())), np.float32)
        ip = C.POINTER(C.c_int64)
        self._check(self.lib.zasr_wpe_run(
            self.handle, a.ctypes.data_as(C_FP), a.size, o.ctypes.data_as(ip), n.ctypes.data_as(ip),
            o.size, int(taps), int(delay), int(iterations), out.ctypes.data_as(C_FP),
            q.ctypes.data_as(ip)))
        return [out[int(b):int(b) + int(m)] for b, m in zip(q, n)]

    def selftest_stft(self, signal):
        """wpe_stft alone: (Y [257][T] complex64, max |Y|^2)."""
        x = np.ascontiguousarray(signal, np.float32).reshape(-1)
        T = wpe_frames(x.size)
        Y = np.empty((self.BINS, T), np.complex64)
        mx = C.c_float()
        self._check(self.lib.zasr_selftest_wpe_stft(
            self.handle, x.ctypes.data_as(C_FP), x.size, Y.ctypes.data_as(C_FP), C.byref(mx)))
        return Y, np.float32(mx.value)

    def selftest_iter(self, Y, max_sq, taps: int = 10, delay: int = 3, g_prev=None, want_x: bool = True):
        """wpe_iter alone on Y [257][T]: (g [257][taps] complex128, X [T][257] complex64 or None,
        max |X|^2)."""
        Y = np.ascontiguousarray(Y, np.complex64)
        if Y.ndim != 2 or Y.shape[0] != self.BINS:
            raise ValueError("Y must be [257][T]")
        T = Y.shape[1]
        gp = None if g_prev is None else np.ascontiguousarray(g_prev, np.complex128)
        if gp is not None and gp.shape != (self.BINS, taps):
            raise ValueError("g_prev must be [257][taps]")
        g = np.empty((self.BINS, taps), np.complex128)
        X = np.empty((T, self.BINS), np.complex64) if want_x else None
        nm = C.c_float()
        dp = C.POINTER(C.c_double)
        self._check(self.lib.zasr_selftest_wpe_iter(
            self.handle, Y.ctypes.data_as(C_FP), T, int(taps), int(delay), float(np.float32(max_sq)),
            None if gp is None else gp.ctypes.data_as(dp), g.ctypes.data_as(dp),
            None if X is None else X.ctypes.data_as(C_FP), C.byref(nm)))
        return g, X, np.float32(nm.value)

    def selftest_istft(self, X, n: int) -> np.ndarray:
        """wpe_istft alone on X [T][257], T = wpe_frames(n): the n output samples."""
        X = np.ascontiguousarray(X, np.complex64)
        if X.ndim != 2 or X.shape[1] != self.BINS:
            raise ValueError("X must be [T][257]")
        out = np.empty(int(n), np.float32)
        self._check(self.lib.zasr_selftest_wpe_istft(
            self.handle, X.ctypes.data_as(C_FP), X.shape[0], int(n), out.ctypes.data_as(C_FP)))
        return out


def wpe_frames(n: int, lib_path: Optional[str] = None) -> int:
    """STFT frames of a chunk of n samples (zasr_wpe_frames, host only)."""
    lib = load_library(lib_path)
    T = int(lib.zasr_wpe_frames(int(n)))
    if T < 0:
        raise ValueError(lib.zasr_last_error().decode())
    return T


class Diarizer:
    """The device side of the diarization clustering (include/zasr.h zasr_diar_*): cosine
    similarity, prune + symmetrise + degrees, and the smallest eigenpairs of the Laplacian.
    Stage entries take device pointers (ints); spectral_embed takes a numpy array [N][D]
    (host) or a device pointer with N and D.  zasr/diarize.py is the host logic over it."""

    def __init__(self, device_id: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        if self.lib.zasr_diar_create(int(device_id), C.byref(h)) != 0:
            raise ZasrError(self.lib.zasr_last_error().decode())
        self.handle = h
        self.device_id = int(device_id)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.zasr_diar_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ZasrError(self.lib.zasr_last_error().decode())

    def similarity(self, d_X: int, N: int, D: int, d_M: int, stream: int = 0) -> None:
        self._check(self.lib.zasr_diar_similarity(self.handle, C.c_void_p(d_X), int(N), int(D),
                                                  C.c_void_p(d_M), C.c_void_p(stream)))

    def prune(self, d_M: int, N: int, pval: float, min_pnum: int, d_deg: int,
              stream: int = 0) -> None:
        self._check(self.lib.zasr_diar_prune(self.handle, C.c_void_p(d_M), int(N), float(pval),
                                             int(min_pnum), C.c_void_p(d_deg), C.c_void_p(stream)))

    def eigs(self, d_M: int, d_deg: int, N: int, k: int, stream: int = 0):
        """(lambdas [k], vecs [N][k], outer passes)."""
        dp = C.POINTER(C.c_double)
        lam = np.zeros(max(int(k), 0), np.float64)
        vec = np.zeros((max(int(N), 0), max(int(k), 0)), np.float64)
        passes = C.c_int32()
        self._check(self.lib.zasr_diar_eigs(self.handle, C.c_void_p(d_M), C.c_void_p(d_deg), int(N),
                                            int(k), lam.ctypes.data_as(dp), vec.ctypes.data_as(dp),
                                            C.byref(passes), C.c_void_p(stream)))
        return lam, vec, int(passes.value)

    def spectral_embed(self, X, pval: float = 0.02, min_pnum: int = 6, k: int = 16,
                       N: Optional[int] = None, D: Optional[int] = None, stream: int = 0):
        """(lambdas [k], vecs [N][k]) of the pruned cosine Laplacian of the rows of X."""
        if isinstance(X, np.ndarray):
            if X.ndim != 2:
                raise ValueError("X must be [N][D]")
            keep = np.ascontiguousarray(X, np.float32)
            N, D = keep.shape
            ptr, on_device = keep.ctypes.data, 0
        else:
            if N is None or D is None:
                raise ValueError("a device X needs N and D")
            keep, ptr, on_device = None, int(X), 1
        dp = C.POINTER(C.c_double)
        lam = np.zeros(max(int(k), 0), np.float64)
        vec = np.zeros((max(int(N), 0), max(int(k), 0)), np.float64)
        self._check(self.lib.zasr_diar_spectral_embed(
            self.handle, C.c_void_p(ptr), on_device, int(N), int(D), float(pval), int(min_pnum),
            int(k), lam.ctypes.data_as(dp), vec.ctypes.data_as(dp), C.c_void_p(stream)))
        del keep
        return lam, vec

    def last_stats(self):
        """(outer passes, block Laplacian products) of the last eigs / spectral_embed."""
        p, a = C.c_int32(), C.c_int64()
        self._check(self.lib.zasr_diar_last_stats(self.handle, C.byref(p), C.byref(a)))
        return int(p.value), int(a.value)


class CluSession:
    """Centroid-linkage AHC of the community-1 diarizer on the device (include/zasr.h
    zasr_clu_*): fcluster(linkage(l2norm(X), "centroid"), threshold, "distance") as labels
    numbered by each cluster's lowest member row.  zasr/vbx.py is the host back end over it."""

    STAGES = ("normalise", "pairwise", "nearest", "merge")

    def __init__(self, device_id: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        if self.lib.zasr_clu_create(int(device_id), C.byref(h)) != 0:
            raise ZasrError(self.lib.zasr_last_error().decode())
        self.handle = h
        self.device_id = int(device_id)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.zasr_clu_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ZasrError(self.lib.zasr_last_error().decode())

    def ahc_into(self, ptr: int, on_device: bool, N: int, D: int, threshold: float,
                 labels_ptr: int, stream: int = 0) -> int:
        """The raw call (the tests hand it a guarded output buffer); returns the status."""
        return self.lib.zasr_clu_ahc(self.handle, C.c_void_p(ptr), int(bool(on_device)), int(N),
                                     int(D), float(threshold), C.c_void_p(labels_ptr),
                                     C.c_void_p(stream))

    def ahc(self, X, threshold: float, N: Optional[int] = None, D: Optional[int] = None,
            stream: int = 0) -> np.ndarray:
        """int32 labels [N] of the rows of X: a numpy array [N][D] (host) or a device pointer
        with N and D."""
        if isinstance(X, np.ndarray):
            if X.ndim != 2:
                raise ValueError("X must be [N][D]")
            keep = np.ascontiguousarray(X, np.float32)
            N, D = keep.shape
            ptr, on_device = keep.ctypes.data, False
        else:
            if N is None or D is None:
                raise ValueError("a device X needs N and D")
            keep, ptr, on_device = None, int(X), True
        labels = np.full(max(int(N), 0), -1, np.int32)
        self._check(self.ahc_into(ptr, on_device, N, D, threshold, labels.ctypes.data, stream))
        del keep
        return labels

    def last_stats(self):
        """(merges, rows rescanned) of the last ahc."""
        m, r = C.c_int64(), C.c_int64()
        self._check(self.lib.zasr_clu_last_stats(self.handle, C.byref(m), C.byref(r)))
        return int(m.value), int(r.value)

    def set_profile(self, on: bool) -> None:
        self._check(self.lib.zasr_clu_set_profile(self.handle, int(bool(on))))

    def stage_ms(self) -> dict:
        ms = (C.c_float * 4)()
        self._check(self.lib.zasr_clu_stage_ms(self.handle, ms))
        return dict(zip(self.STAGES, (float(v) for v in ms)))

    def n_routes(self) -> int:
        n = C.c_int32()
        self.lib.zasr_selftest_clu_route(None, 0, C.byref(n))
        return int(n.value)

    def force_route(self, route: int) -> None:
        self._check(self.lib.zasr_selftest_clu_route(self.handle, int(route), None))
