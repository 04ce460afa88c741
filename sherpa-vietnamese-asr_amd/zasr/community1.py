"""Drop-in for the embedding stage of the reference's production diarizer:
PureOrtDiarizer._extract_embeddings (core/speaker_diarization_pure_ort.py:769-879) and
.compute_single_embedding (:681-707) on a binding.EmbSession.

The host keeps what the reference decides per (chunk, speaker) in numpy -- which mask is used
(:859-861) -- and hands the device uint8 masks; fbank, windows, CMVN, the ResNet34 encoder, the
masked pooling and the projection run on the GPU in one call.  AHC + PLDA + VBx and the
reconstruction (:904-1052) stay the reference's.
"""
from __future__ import annotations

import math
import os
import types
from typing import Optional

import numpy as np

SAMPLE_RATE = 16000
CHUNK_SAMPLES = 160000
MAX_SPEAKERS_PER_CHUNK = 3
EMBED_DIM = 256


def min_seg_frames_default(num_seg_frames: int = 589, min_samples: int = 1680,
                           chunk_samples: int = CHUNK_SAMPLES) -> int:
    """ceil(num_seg_frames * min_num_samples / chunk_samples), the reference's min_seg_frames."""
    return int(math.ceil(num_seg_frames * min_samples / chunk_samples))


def feat_idx(n_feat_frames: int, num_seg_frames: int) -> np.ndarray:
    """Segmentation frame under every encoder frame (:850-853)."""
    idx = np.floor(np.arange(n_feat_frames) * num_seg_frames / n_feat_frames).astype(int)
    return np.clip(idx, 0, num_seg_frames - 1)


def used_masks(binarized: np.ndarray, clean_binarized: np.ndarray, min_seg_frames) -> np.ndarray:
    """uint8 [chunks][speakers][frames]: the clean mask where it has MORE than min_seg_frames
    active frames, else the full one (:859-861)."""
    b = np.asarray(binarized)
    cb = np.asarray(clean_binarized)
    if b.shape != cb.shape or b.ndim != 3:
        raise ValueError("binarized and clean_binarized: [chunks, frames, speakers], same shape")
    out = np.empty((b.shape[0], b.shape[2], b.shape[1]), np.uint8)
    for c in range(b.shape[0]):
        for s in range(b.shape[2]):
            cm = cb[c, :, s]
            um = cm if cm.sum() > min_seg_frames else b[c, :, s]
            out[c, s] = (um.astype(np.float32) > 0.5)
    return out


def _device_signal(x):
    """(device pointer, samples) of a CUDA float32 tensor, or None for host audio."""
    if hasattr(x, "data_ptr") and getattr(x, "is_cuda", False):
        import torch
        if x.dtype != torch.float32 or x.dim() != 1 or not x.is_contiguous():
            raise ValueError("device signal: a contiguous 1-D float32 CUDA tensor")
        torch.cuda.current_stream(x.device).synchronize()
        return x.data_ptr(), int(x.shape[0])
    return None


def extract_embeddings(session, audio_or_device_signal, binarized, clean_binarized, num_seg_frames,
                       chunk_starts, min_seg_frames, progress_callback=None) -> np.ndarray:
    """float32 [chunks][3][256], the contract of _extract_embeddings on its encoder-only path.
    The masks here are 0 / 1 (the reference's binarized arrays are)."""
    masks = used_masks(binarized, clean_binarized, min_seg_frames)
    if masks.shape[2] != num_seg_frames or masks.shape[1] != MAX_SPEAKERS_PER_CHUNK:
        raise ValueError("binarized: [chunks, num_seg_frames, 3]")
    starts = np.asarray(chunk_starts, np.int64).reshape(-1)
    if starts.shape[0] != masks.shape[0]:
        raise ValueError("chunk_starts and binarized differ in length")
    dev = _device_signal(audio_or_device_signal)
    if dev is not None:
        out = session.chunk_embeddings_device(dev[0], dev[1], starts, masks)
    else:
        out = session.chunk_embeddings(np.asarray(audio_or_device_signal, np.float32), starts, masks)
    if progress_callback:
        progress_callback(85, 100)   # the reference's 25 + 60 after the last batch (:875)
    return out


def compute_single_embedding(session, audio) -> Optional[np.ndarray]:
    """[256], or None when the segment has fewer than 9 fbank frames (:690)."""
    return session.segment_embedding(np.asarray(audio, np.float32))


def load_projection(model_dir: str):
    """(emb_W [256, 5120], emb_b [256]) of a model directory: resnet.seg_1."""
    from safetensors.numpy import load_file
    w = load_file(os.path.join(model_dir, "model.safetensors"))
    return (np.ascontiguousarray(w["resnet.seg_1.weight"], np.float32),
            np.ascontiguousarray(w["resnet.seg_1.bias"], np.float32))


def attach(diarizer, session, emb_W=None, emb_b=None):
    """Serve a PureOrtDiarizer-shaped object from `session`: sets emb_sess, emb_W, emb_b (the
    session's model directory's seg_1 unless given) and rebinds _extract_embeddings and
    compute_single_embedding.  Duck-typed: nothing of the reference is imported."""
    if emb_W is None or emb_b is None:
        emb_W, emb_b = load_projection(session.model_dir)
    diarizer.emb_sess = session
    diarizer.emb_W = emb_W
    diarizer.emb_b = emb_b

    def _extract_embeddings(self, audio, binarized, clean_binarized, num_seg_frames, chunk_starts,
                            min_seg_frames, progress_callback=None):
        return extract_embeddings(self.emb_sess, audio, binarized, clean_binarized, num_seg_frames,
                                  chunk_starts, min_seg_frames, progress_callback)

    def _compute_single_embedding(self, audio_segment):
        if self.emb_sess is None:
            return None
        return compute_single_embedding(self.emb_sess, audio_segment)

    diarizer._extract_embeddings = types.MethodType(_extract_embeddings, diarizer)
    diarizer.compute_single_embedding = types.MethodType(_compute_single_embedding, diarizer)
    return diarizer
