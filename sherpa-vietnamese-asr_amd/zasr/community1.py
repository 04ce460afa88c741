"""Drop-in for the embedding stage of the reference's production diarizer:
PureOrtDiarizer._extract_embeddings (core/speaker_diarization_pure_ort.py:769-879) and
.compute_single_embedding (:681-707) on a binding.EmbSession.

The host keeps what the reference decides per (chunk, speaker) in numpy -- which mask is used
(:859-861) -- and hands the device uint8 masks; fbank, windows, CMVN, the ResNet34 encoder, the
masked pooling and the projection run on the GPU in one call.

process() is the whole diarizer on this project's sessions: PyanNet segmentation
(binding.SegSession), the embeddings (binding.EmbSession), the centroid AHC
(binding.CluSession) and the host back end zasr/vbx.py.  attach(..., clu_session=...) instead
serves the reference's own object, _cluster included.
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


class Segments(list):
    """process()'s result: the list of {"start", "end", "speaker"} segments, with the
    reference's two side results as attributes."""

    def __init__(self, segments=()):
        super().__init__(segments)
        self.overlap_regions = []
        self.speaker_centroids = None
        self.info = {}


def segment_classes(signal, seg_session, batch: int = 32):
    """(classes uint8 [chunks][frames], chunk starts) of _segment (:709-740) and the argmax of
    :583.  A device signal runs through classes_device(); the one chunk the reference makes
    beyond that rule (vbx.chunk_starts_1s) and every chunk of a host signal go through the
    session's run(), which is bit-identical."""
    from . import vbx
    dev = _device_signal(signal)
    total = dev[1] if dev is not None else int(np.asarray(signal).shape[0])
    starts = vbx.chunk_starts_1s(total)
    done = None
    if dev is not None:
        done = seg_session.classes_device(dev[0], total, CHUNK_SAMPLES, vbx.STEP_SAMPLES)
        if done.shape[0] > len(starts):
            raise ValueError("segmentation session made more chunks than the reference's rule")
    first = 0 if done is None else done.shape[0]
    rest = []
    for b in range(first, len(starts), batch):
        idx = starts[b:b + batch]
        x = np.zeros((len(idx), 1, CHUNK_SAMPLES), np.float32)
        for i, s0 in enumerate(idx):
            e = min(s0 + CHUNK_SAMPLES, total)
            piece = signal[s0:e]
            x[i, 0, :e - s0] = piece.cpu().numpy() if dev is not None else np.asarray(piece, np.float32)
        rest.append(np.argmax(seg_session.run(None, {"input_values": x})[0], axis=-1).astype(np.uint8))
    parts = ([done] if done is not None and done.shape[0] else []) + rest
    return np.concatenate(parts, axis=0), starts


def process(signal, seg_session, emb_session, clu_session, plda, num_speakers: int = 0,
            max_speakers: Optional[int] = None, threshold: float = 0.6, Fa: float = 0.07,
            Fb: float = 0.8, min_duration_off: float = 0.0) -> Segments:
    """PureOrtDiarizer.process (:554-679) on a 16 kHz mono signal: a host float32 array or a
    1-D float32 CUDA tensor.  plda is vbx.load_plda's dict or a model directory.  Returns the
    segments; .overlap_regions (:512-552) and .speaker_centroids (reindexed as at :641-646 and
    :1041-1050) ride on the result."""
    from . import vbx
    if isinstance(plda, (str, os.PathLike)):
        plda = vbx.load_plda(os.fspath(plda))
    dev = _device_signal(signal)
    if dev is None:
        signal = np.ascontiguousarray(signal, np.float32)
    total = dev[1] if dev is not None else int(signal.shape[0])
    duration = total / SAMPLE_RATE
    classes, starts = segment_classes(signal, seg_session)
    num_seg_frames = classes.shape[1]
    binarized = vbx.POWERSET_MAP[classes]                                    # :583
    out = Segments()
    out.overlap_regions = vbx.overlap_regions(binarized, starts, num_seg_frames, duration)
    clean = binarized * (binarized.sum(axis=2, keepdims=True) < 2).astype(np.float32)   # :600-601
    embeddings = extract_embeddings(emb_session, signal, binarized, clean, num_seg_frames, starts,
                                    min_seg_frames_default(num_seg_frames))
    segments, info = vbx.diarize_from_embeddings(
        binarized, embeddings, clu_session, plda, num_speakers, max_speakers, threshold, Fa, Fb,
        min_duration_off)
    out.extend(segments)
    out.speaker_centroids = info["speaker_centroids"]
    out.info = info
    return out


def attach(diarizer, session, emb_W=None, emb_b=None, clu_session=None):
    """Serve a PureOrtDiarizer-shaped object from `session`: sets emb_sess, emb_W, emb_b (the
    session's model directory's seg_1 unless given) and rebinds _extract_embeddings and
    compute_single_embedding.  With a binding.CluSession, _cluster (:904-967) is rebound to
    vbx.cluster on it as well (the object's threshold, Fa, Fb and plda_data are used).
    Duck-typed: nothing of the reference is imported."""
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
    if clu_session is not None:
        from . import vbx
        diarizer.clu_sess = clu_session

        def _cluster(self, all_embeddings, train_mask, segmentations, max_clusters=None):
            hard, centroids = vbx.cluster(all_embeddings, train_mask, segmentations, self.clu_sess,
                                          self.plda_data, self.threshold, self.Fa, self.Fb,
                                          max_clusters)
            if centroids is not None:
                self.speaker_centroids = centroids.copy()                   # :948
            return hard

        diarizer._cluster = types.MethodType(_cluster, diarizer)
    return diarizer
