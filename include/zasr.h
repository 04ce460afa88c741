/*
 * zasr.h — C ABI of libzasr.so, the MI355X-native offline-ASR hot path
 * (kaldi fbank -> Zipformer2 transducer encoder -> stateless decoder + joiner ->
 *  greedy / modified-beam search with Aho-Corasick hotword biasing).
 *
 * Plain C types only: caller-owned input buffers are read during the call; results are
 * library-owned until zasr_result_free (mirrors SherpaOnnxDestroyOfflineStreamResultJson,
 * offline_pwa/static/vendor/sherpa-onnx-wasm/sherpa-onnx-asr.js:1872-1878).  Every entry
 * point returns 0 on success and a nonzero code on failure; zasr_last_error() gives the
 * message of the calling thread's last failure.  One handle may be used from several
 * host threads (calls on a handle are serialised internally), matching the reference's
 * two decode workers sharing one set of sessions (core/asr_engine.py:2291-2315).
 *
 * Reference interfaces each entry point replaces:
 *   zasr_create            core/asr_engine.py:903-1020 create_recognizer (ORT sessions,
 *                          tokens, hotword ContextGraph); sherpa-onnx
 *                          SherpaOnnxCreateOfflineRecognizer (sherpa-onnx-asr.js:1782)
 *   zasr_destroy           SherpaOnnxDestroyOfflineRecognizer; core/asr_engine.py:743-773
 *                          clear_model_cache
 *   zasr_fbank             core/asr_engine.py:698-721 compute_fbank_ort (kaldi-native-fbank)
 *   zasr_decode_batch      core/asr_engine.py:1209-1226 decode_chunk (fbank + search) over a
 *                          batch of chunks; SherpaOnnxAcceptWaveformOffline +
 *                          SherpaOnnxDecodeOfflineStream (sherpa-onnx-asr.js:1799-1830)
 *   zasr_decode_features   core/asr_engine.py:1224 _ort_beam_search with precomputed
 *                          features (ROVER shares one fbank, core/asr_engine.py:2346-2350)
 *   zasr_encode_features   the encoder session run, core/asr_engine.py:1045-1049
 *   zasr_silence_flags     core/asr_engine.py:521-554 find_silent_regions (the planner's
 *                          frame energies, numpy float32 bit for bit; regions on the host)
 *   zasr_search_encoder_out  the search loop alone, core/asr_engine.py:1051-1153
 *   zasr_result_*          the (token_ids, frames, ys_log_probs, T, emit_logits) tuple of
 *                          core/asr_engine.py:1153 (entropy statistics instead of raw
 *                          logits rows, reduced on device); SherpaOnnxGetOfflineStreamResult
 *   zasr_audio_to_16k      load_audio's decode / downmix / resample, core/asr_engine.py:492-508
 *                          (ffmpeg + soxr there; sherpa-onnx's LinearResample definition here)
 *   zasr_audio_peak, zasr_audio_scale
 *                          the quiet-file boost, core/asr_engine.py:512-516, and
 *                          adaptive_peak_limit, core/audio_preprocessing.py:226-243
 *   zasr_audio_segment_sumsq, zasr_audio_apply_gain
 *                          per_segment_rms_normalize, core/audio_preprocessing.py:46-140 (the
 *                          gain plan itself stays host logic, zasr/audio.py)
 *   zasr_wpe_run_device    apply_wpe_dereverberation, core/audio_preprocessing.py:157-216, all
 *                          chunks of a file in one call (per frequency bin)
 */
#ifndef ZASR_H_
#define ZASR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zasr_recognizer zasr_recognizer;
typedef struct zasr_result zasr_result;

enum {
  ZASR_OK = 0,
  ZASR_ERR_INVALID = 1,   /* bad argument */
  ZASR_ERR_NOT_FOUND = 2, /* missing model file (reference raises FileNotFoundError) */
  ZASR_ERR_RUNTIME = 3,   /* HIP / internal failure */
};

/* FP32: exact-f32 MFMA everywhere (parity mode).  BF16: bf16 MFMA operands for the encoder
   projections / attention and the joiner, f32 accumulate, norms and search.  BF16_ENC: the
   BF16 encoder with the f32 joiner and search of FP32 (no bf16 rounding of the joiner input).
   BF16X3: f32 storage as FP32, every encoder projection product as three bf16 MFMAs over
   hi / lo operand halves (relative product error ~2^-16).  BF16X6: three bf16 pieces per
   operand, six MFMAs per product (dropped terms below 2^-24: exact-f32 quality at bf16 MFMA
   rates; token-exact against the fp32 oracle).  F16X3: two fp16 pieces
   per operand, hi = fp16(x) and lo = fp16((x - hi) * 2^11), three fp16 MFMAs per product
   (hi*hi + (hi*lo + lo*hi) * 2^-11, ~2^-22 relative: f32 quality at half the MFMAs of
   BF16X6); operands must stay below 65504 in magnitude (the 68M model's stay below 30). */
enum {
  ZASR_PRECISION_FP32 = 0,
  ZASR_PRECISION_BF16 = 1,
  ZASR_PRECISION_BF16_ENC = 2,
  ZASR_PRECISION_BF16X3 = 3,
  ZASR_PRECISION_BF16X6 = 4,
  ZASR_PRECISION_F16X3 = 5
};

typedef struct zasr_config {
  const char* model_dir;        /* config.json + model.safetensors, or the reference's
                                   encoder-/decoder-/joiner-*.onnx (+ tokens.txt for hosts) */
  const char* decoding_method;  /* "greedy_search" | "modified_beam_search" */
  int32_t max_active_paths;     /* beam for modified_beam_search, 1..16 (reference: 8) */
  float blank_penalty;          /* must be 0 (the reference applies none) */
  /* hotwords as token-id phrases (sentencepiece encoding stays on the host,
     core/hotword_context.py:234-248); may be NULL / 0 */
  const int32_t* hotword_tokens;  /* concatenated phrases */
  const int32_t* hotword_lens;    /* per-phrase token counts */
  const float* hotword_scores;    /* per-phrase score (reference default 1.5) */
  int32_t num_hotwords;
  int32_t device_id;            /* HIP device ordinal */
  int32_t precision;            /* ZASR_PRECISION_* */
} zasr_config;

int zasr_create(const zasr_config* cfg, zasr_recognizer** out);
void zasr_destroy(zasr_recognizer* h);

/* Host-only (no GPU): load a model directory the way zasr_create does -- config.json +
   model.safetensors, or the reference's encoder-/decoder-/joiner-*.onnx set chosen like
   create_recognizer (core/asr_engine.py:913-928: non-int8 preferred, int8 dequantized when it
   is the only file) with the architecture inferred from the initializer shapes -- and write
   out_dir/config.json + out_dir/model.safetensors (float32, the engine's tensor names).
   Replaces the ORT session load's file handling; ZASR_ERR_NOT_FOUND when files are missing. */
int zasr_convert_model(const char* model_dir, const char* out_dir);

/* Host-only (no GPU): the same for the single-graph models of the other stages, kind
   "silero" | "campp" | "vibert": read the file the reference opens in model_dir
   (silero_vad_16k_op15.onnx or silero_vad.onnx, core/vad_utils.py:22-24;
   campplus_cn_en_common_200k.onnx, core/speaker_diarization_senko_campp_optimized.py:324-325;
   vibert-capu.onnx or vibert-capu.int8.onnx, core/gec_model.py:133-140) -- or the engine's
   own <kind>_config.json + safetensors when present -- and write out_dir/<kind>_config.json +
   out_dir/{silero_vad,campp,vibert}.safetensors (torch state-dict names; the LSTM gates of
   the ONNX LSTM node reordered to torch's; a BatchNorm the exporter fused into its Conv kept
   as "<bn>.fused_shift").  zasr_vad_create / zasr_campp_create / zasr_vibert_create accept
   the reference's directories directly through the same reader. */
int zasr_convert_stage_model(const char* kind, const char* model_dir, const char* out_dir);

/* log-mel fbank of one waveform (f32 in [-1,1], 16 kHz).  out holds cap floats;
   *n_frames = (n + 80) / 160, output row-major [n_frames][80].  h may be NULL
   (uses device 0). */
int zasr_fbank(zasr_recognizer* h, const float* wav, int64_t n, int32_t sample_rate, float* out,
               int64_t cap, int64_t* n_frames);

/* The chunk planner's silence detector (core/asr_engine.py:521-554 find_silent_regions):
   for each of the n / frame_len frames of the HBM-resident signal d_wav (16-byte aligned),
   d_flags[f] = 1 when sqrt(mean(frame ** 2)) < threshold, evaluated exactly as numpy does
   in float32 (pairwise row sum, f32 divide, correctly rounded sqrt, f32 compare), else 0.
   frame_len: a multiple of 4, at most 256 (160 at 16 kHz).  Runs on `stream` (a hipStream_t,
   NULL = the default stream); needs no recognizer handle. */
int zasr_silence_flags(const float* d_wav, int64_t n, int32_t frame_len, float threshold,
                       uint8_t* d_flags, void* stream);

/* Decode `count` independent chunks (host buffers).  beam <= 0 uses the handle's
   configured decoding method / max_active_paths. */
int zasr_decode_batch(zasr_recognizer* h, const float* const* wav, const int64_t* n,
                      int32_t count, int32_t beam, zasr_result** out);

/* Same, from precomputed fbank features feats[i] of shape [n_frames[i]][80]. */
int zasr_decode_features(zasr_recognizer* h, const float* const* feats, const int64_t* n_frames,
                         int32_t count, int32_t beam, zasr_result** out);

/* Device-resident variant (inputs already in HBM): d_wav holds all chunks packed,
   chunk i at element offset wav_off[i] with n[i] samples (host arrays).  stream is a
   hipStream_t (NULL: the handle's stream).  Used by bench.py. */
int zasr_decode_device(zasr_recognizer* h, const float* d_wav, const int64_t* wav_off,
                       const int64_t* n, int32_t count, int32_t beam, void* stream,
                       zasr_result** out);

/* Several device-resident batches back to back: chunks as in zasr_decode_device, grouped
   into n_batches consecutive batches of batch_sizes[i] chunks (sum = count).  Batch k+1's
   fbank + encoder overlap batch k's search on the GPU; results for all count chunks, in
   chunk order, identical to decoding each batch with zasr_decode_device.  Replaces the
   reference's 2-worker chunk dispatch, whose point is that one worker's beam search runs
   while the other's encoder does (core/asr_engine.py:2250-2276). */
int zasr_decode_device_batches(zasr_recognizer* h, const float* d_wav, const int64_t* wav_off,
                               const int64_t* n, int32_t count, const int32_t* batch_sizes,
                               int32_t n_batches, int32_t beam, void* stream, zasr_result** out);

/* zasr_decode_device_batches from HOST waveforms (wav: host memory, pinned for an
   asynchronous copy, e.g. hipHostMalloc / torch pin_memory): each batch's span of samples is
   copied into the engine's device buffer for that pipeline slot on its own copy stream, and
   the batch's fbank waits for that copy alone, so batch k+1's upload runs under batch k's
   encoder and search.  Results identical to uploading the signal and calling
   zasr_decode_device_batches.  The reference's unit of work starts from the host waveform
   (core/asr_engine.py:2068). */
int zasr_decode_host_batches(zasr_recognizer* h, const float* wav, const int64_t* wav_off,
                             const int64_t* n, int32_t count, const int32_t* batch_sizes,
                             int32_t n_batches, int32_t beam, void* stream, zasr_result** out);

/* Encoder only: features -> encoder_out rows [T'_i][joiner_dim], packed in chunk order
   into out (cap floats); t_out[i] receives T'_i. */
int zasr_encode_features(zasr_recognizer* h, const float* const* feats, const int64_t* n_frames,
                         int32_t count, float* out, int64_t cap, int64_t* t_out);

/* Search only, from given encoder outputs enc[i] of shape [t_out[i]][joiner_dim]. */
int zasr_search_encoder_out(zasr_recognizer* h, const float* const* enc, const int64_t* t_out,
                            int32_t count, int32_t beam, zasr_result** out);

/* result access */
int32_t zasr_result_count(const zasr_result* r);
int32_t zasr_result_num_tokens(const zasr_result* r, int32_t i);
int32_t zasr_result_num_frames(const zasr_result* r, int32_t i); /* T' of chunk i */
const int32_t* zasr_result_tokens(const zasr_result* r, int32_t i);
const int32_t* zasr_result_frames(const zasr_result* r, int32_t i);
const double* zasr_result_log_probs(const zasr_result* r, int32_t i);
/* per token 4 floats: entropy, sum p^(1/3), top1 prob, top2 prob of the emitting row */
const float* zasr_result_token_stats(const zasr_result* r, int32_t i);
void zasr_result_free(zasr_result* r);

/* ---- offline streams: the sherpa-onnx OfflineRecognizer / OfflineStream surface ----
   The stream-shaped calls the reference's other callers bind: sherpa-onnx's C API
   (offline_pwa/static/vendor/sherpa-onnx-wasm/sherpa-onnx-asr.js:1782-1880) and its Python
   OfflineRecognizer (streaming_asr.py:224-243, core/audio_analyzer.py:345-361:
   create_stream -> accept_waveform -> decode_stream -> stream.result).  A stream holds host
   samples until decoded; zasr_decode_streams decodes several in ONE batched GPU pass (the
   zasr_decode_batch path), with the recognizer's configured method and beam.  A stream with
   fewer than 1360 samples (under 9 fbank frames) decodes to an empty result.
     zasr_create_stream            SherpaOnnxCreateOfflineStream (sherpa-onnx-asr.js:1862)
     zasr_destroy_stream           SherpaOnnxDestroyOfflineStream (:1790)
     zasr_stream_accept_waveform   SherpaOnnxAcceptWaveformOffline (:1799-1805); 16 kHz only
                                   (the reference resamples on load); appends
     zasr_decode_stream            SherpaOnnxDecodeOfflineStream (:1866-1868)
     zasr_decode_streams           SherpaOnnxDecodeMultipleOfflineStreams (one batch)
     zasr_stream_result_json       SherpaOnnxGetOfflineStreamResultAsJson (:1870-1878): keys
                                   lang, emotion, event, text, timestamps (frame x 0.04 s),
                                   tokens (tokens.txt strings, a leading U+2581 as a space, as
                                   sherpa-onnx's SymbolTable), ys_log_probs, words; *needed =
                                   bytes incl. the NUL (call with buf NULL to size it)
     zasr_stream_tokens / _frames / _log_probs / _token_stats / _num_*: the result arrays, as
                                   zasr_result_* for one chunk (valid until the stream is
                                   destroyed) */
typedef struct zasr_stream zasr_stream;
/* the symbol table zasr_stream_result_json's "tokens" / "text" use: sherpa-onnx's
   OfflineModelConfig.tokens (sherpa-onnx-asr.js:1719 tokens field; the reference passes
   tokens.txt beside its model files, core/asr_engine.py:980-986).  Default: model_dir/tokens.txt.
   ZASR_ERR_NOT_FOUND if the file does not exist. */
int zasr_set_tokens(zasr_recognizer* h, const char* tokens_path);
int zasr_create_stream(zasr_recognizer* h, zasr_stream** out);
void zasr_destroy_stream(zasr_stream* s);
int zasr_stream_accept_waveform(zasr_stream* s, int32_t sample_rate, const float* samples,
                                int64_t n);
int zasr_decode_stream(zasr_recognizer* h, zasr_stream* s);
int zasr_decode_streams(zasr_recognizer* h, zasr_stream* const* streams, int32_t n);
int32_t zasr_stream_is_decoded(const zasr_stream* s);
int32_t zasr_stream_num_tokens(const zasr_stream* s);
int32_t zasr_stream_num_frames(const zasr_stream* s);
const int32_t* zasr_stream_tokens(const zasr_stream* s);
const int32_t* zasr_stream_frames(const zasr_stream* s);
const double* zasr_stream_log_probs(const zasr_stream* s);
const float* zasr_stream_token_stats(const zasr_stream* s);
int zasr_stream_result_json(const zasr_stream* s, char* buf, int64_t cap, int64_t* needed);

/* ---- CAM++ speaker embedding ----
   Replaces the reference's onnxruntime CAM++ session and its numpy front end:
   core/speaker_diarization_senko_campp_optimized.py:86-159 (_compute_fbank_vectorized),
   :589-605 (batched emb_sess.run(['embs'], {'feats': batch})); the model is the reference's
   convert_onnx/export_campplus_onnx.py CAMPPlus (192-dim).  model_dir holds the reference's
   campplus_cn_en_common_200k.onnx (Conv+BN fused by the exporter or not) or
   campp_config.json + campp.safetensors (state-dict names); see zasr_convert_stage_model. */
typedef struct zasr_campp zasr_campp;
int zasr_campp_create(const char* model_dir, int32_t device_id, zasr_campp** out);
void zasr_campp_destroy(zasr_campp* h);
int32_t zasr_campp_embedding_dim(const zasr_campp* h);
/* fbank + per-utterance CMVN of one waveform: *n_frames = 1 + (n - 400) / 160 (0 if n < 400) */
int zasr_campp_fbank(zasr_campp* h, const float* wav, int64_t n, float* out, int64_t cap,
                     int64_t* n_frames);
/* embeddings of a feature batch [count][n_frames][80] (zero-padded like the reference's
   batch tensor) -> out [count][embedding_dim] (not L2-normalised, as the ONNX output) */
int zasr_campp_embed(zasr_campp* h, const float* feats, int32_t count, int32_t n_frames,
                     float* out);
/* same with device buffers on `stream` (NULL: the handle's stream); used by bench.py */
int zasr_campp_embed_device(zasr_campp* h, const float* d_feats, int32_t count,
                            int32_t n_frames, float* d_out, void* stream);
/* the front end of a whole file in HBM: fbank + per-region CMVN of every speech region
   [region_off[i], + region_len[i]) of d_wav, then the windows of window_frames frames every
   step_frames (tail pulled back; a region shorter than a window gives one window of all its
   frames, zero-padded; < 10 frames: none) gathered into d_feats [n][window_frames][80] on
   `stream`.  Replaces _sliding_window_embeddings' fbank-once-slice-later loop and batch
   tensor (core/speaker_diarization_senko_campp_optimized.py:540-600).  *n_windows = n;
   window_region / window_first / window_nframes (host, capacity max_windows) describe each
   window (its start time is region start + first * 10 ms, :567-577). */
int zasr_campp_windows_device(zasr_campp* h, const float* d_wav, const int64_t* region_off,
                              const int64_t* region_len, int32_t n_regions, int32_t window_frames,
                              int32_t step_frames, float* d_feats, int64_t max_windows,
                              int32_t* window_region, int32_t* window_first,
                              int32_t* window_nframes, int64_t* n_windows, void* stream);

/* ---- ViBERT-capu punctuation / capitalization ----
   Replaces the reference's onnxruntime session of vibert-capu.onnx (core/gec_model.py:
   366-412: session.run(None, {input_ids, attention_mask, token_type_ids, input_offsets}) ->
   (logits, detect_logits)); graph: convert_onnx/export_vibert_onnx.py Seq2LabelsModel.
   model_dir holds the reference's vibert-capu.onnx (or .int8.onnx, dequantized; config.json
   beside it gives the head count, else head dim 64) or vibert_config.json +
   vibert.safetensors (Hugging Face names); see zasr_convert_stage_model. */
typedef struct zasr_vibert zasr_vibert;
int zasr_vibert_create(const char* model_dir, int32_t device_id, zasr_vibert** out);
void zasr_vibert_destroy(zasr_vibert* h);
int32_t zasr_vibert_num_labels(const zasr_vibert* h);
int32_t zasr_vibert_num_detect(const zasr_vibert* h);
/* inputs int64 [batch][n_tokens] (ids, mask, token types) and [batch][n_words] offsets;
   outputs logits [batch][n_words][num_labels], detect_logits [batch][n_words][num_detect] */
int zasr_vibert_run(zasr_vibert* h, const int64_t* input_ids, const int64_t* attention_mask,
                    const int64_t* token_type_ids, const int64_t* input_offsets, int32_t batch,
                    int32_t n_tokens, int32_t n_words, float* logits, float* detect_logits);

/* ---- Silero VAD ----
   Replaces the reference's per-window onnxruntime loop over silero_vad_16k_op15.onnx
   (core/vad_utils.py:62-111: 64-sample context + 512-sample window, (2, 1, 128) LSTM state
   carried across calls).  model_dir holds the reference's silero_vad_16k_op15.onnx (or
   silero_vad.onnx; the 16 kHz branch is found by walking the graph, If branches included) or
   silero_config.json + silero_vad.safetensors (torch state-dict names of the 16 kHz model);
   see zasr_convert_stage_model. */
typedef struct zasr_vad zasr_vad;
int zasr_vad_create(const char* model_dir, int32_t device_id, zasr_vad** out);
void zasr_vad_destroy(zasr_vad* h);
/* speech probability of every full 512-sample window of n_files files (file i = audio
   [offsets[i], offsets[i] + lengths[i])), state reset per file as in _run_vad_inference;
   probs of file i start at sum_{k<i} lengths[k] / 512.  auto_boost != 0 scales a file whose
   peak is in (1e-6, 0.071) to a 0.071 peak first (get_vad_segments, vad_utils.py:203-208).
   Host buffers. */
int zasr_vad_probs(zasr_vad* h, const float* audio, const int64_t* offsets,
                   const int64_t* lengths, int32_t n_files, int32_t auto_boost, float* probs);
/* the same with device-resident audio and probs; ordered after / before `stream`
   (a hipStream_t, 0 = synchronous) */
int zasr_vad_probs_device(zasr_vad* h, const float* d_audio, const int64_t* offsets,
                          const int64_t* lengths, int32_t n_files, int32_t auto_boost,
                          float* d_probs, void* stream);
/* recurrence passes of the last probs call: a long file is decoded as parallel segments whose
   chained start states are checked against their predecessors' end states to a relative
   1e-6 per element (the rounding-noise level of two summation orders; NOT bit-exact: the
   probabilities stay within ~2.4e-7 of the sequential recurrence and give the same speech
   segments, tests/test_gpu_vad.py).  1 = every warm-up guess passed; set ZASR_VAD_PIT=0
   before create for one sequential workgroup per file */
int32_t zasr_vad_last_passes(const zasr_vad* h);
/* one session.run step for n independent streams: input [n][576], state [2][n][128] ->
   prob [n], state_out [2][n][128] (the ORT session surface, vad_utils.py:100-102) */
int zasr_vad_window(zasr_vad* h, const float* input, const float* state, int32_t n, float* prob,
                    float* state_out);

/* ---- PyanNet segmentation ----
   Replaces the reference diarizer's pyannote segmentation session
   (core/speaker_diarization_senko_campp_optimized.py:383-396, pinned there to the CPU
   provider) and the chunk batching around it (:413-437).  model_dir holds config.json +
   model.safetensors (pyannote PyanNet state-dict names, the sinc filter bank as the plain
   tensor sincnet.conv1d.0.weight [80][1][251]); reading the reference's
   segmentation-community-1.onnx is not supported.  Bad arguments (null pointers, n <= 0,
   fewer than 1261 samples per chunk) return ZASR_ERR_INVALID, missing model files
   ZASR_ERR_NOT_FOUND. */
typedef struct zasr_seg zasr_seg;
int zasr_seg_create(const char* model_dir, int32_t device_id, zasr_seg** out);
void zasr_seg_destroy(zasr_seg* h);
/* Host-only.  Output frames per chunk of chunk_samples samples (589 at 160000; the reference's
   NUM_SEG_FRAMES, core/speaker_diarization_pure_ort.py:114); 0 when chunk_samples is too short
   for a frame, and chunks need at least 2 (1261 samples). */
int32_t zasr_seg_num_frames(const zasr_seg* h, int64_t chunk_samples);
/* seg_sess.run(None, {"input_values": batch})[0] (:435): batch [n][T] -> log-probabilities
   [n][F][7], host buffers.  A chunk's result does not depend on the batch it is in. */
int zasr_seg_logits(zasr_seg* h, const float* batch, int32_t n, int32_t T, float* logits);
/* A whole file from the 16 kHz HBM signal d_audio[0, total): chunks of chunk_samples every
   step_samples, starts as in :418-424 (0, step, ... up to the first start with start + chunk >=
   total), zeros past the end of the signal (:430-434).  classes (host) [n_chunks][F] = the
   argmax over the 7 powerset classes, lowest index on ties (:443); d_logits (device,
   [n_chunks][F][7]) may be null.  Ordered after `stream` (a hipStream_t, 0 = none);
   synchronises before it returns.  Bit-identical to zasr_seg_logits on the same chunks. */
int zasr_seg_classes_device(zasr_seg* h, const float* d_audio, int64_t total,
                            int32_t chunk_samples, int32_t step_samples, uint8_t* classes,
                            float* d_logits, void* stream);
/* number of chunks zasr_seg_classes_device makes of `total` samples (host-only) */
int64_t zasr_seg_num_chunks(int64_t total, int32_t chunk_samples, int32_t step_samples);
/* diagnostics of the recurrence: sequences per workgroup of the last call, and a forced value
   (1, 2, 4, 8, 16; 0 = automatic).  Results do not depend on it. */
int32_t zasr_seg_last_group(const zasr_seg* h);
int zasr_seg_set_group(zasr_seg* h, int32_t group);
/* The handle keeps its activation workspace between calls, as large as the longest file it has
   seen (8.6 MB per 10 s chunk, at most the 8 GiB launch-group bound: 6.2 GB after an hour).
   zasr_seg_trim frees it; the next call allocates what it needs. */
int zasr_seg_trim(zasr_seg* h);
/* stage timing on HIP events (off by default): with it on, every call synchronises and leaves
   the milliseconds of its front (gather + input norm + sinc conv + pool + norm), convs,
   LSTM input projections, recurrence and head in ms5[0..4] (tools/seg_bench.py) */
int zasr_seg_set_profile(zasr_seg* h, int32_t on);
int zasr_seg_stage_ms(zasr_seg* h, float* ms5);

/* ---- Conv-TasNet overlap separation ----
   Replaces the reference's separation session (core/overlap_separator.py:45-60, an
   onnxruntime CPU session over ConvTasNet_Libri2Mix_sepclean_16k) and its per-region call
   (:281-296).  model_dir holds config.json + model.safetensors (asteroid ConvTasNet state-dict
   names); reading the reference's .onnx is not supported.  Bad arguments (null pointers,
   n <= 0, a region shorter than kernel_size = 32 samples or outside the signal) return
   ZASR_ERR_INVALID, missing model files ZASR_ERR_NOT_FOUND.  A region's result does not depend
   on the other regions of the call, on its place among them or on the workspace budget. */
typedef struct zasr_sep zasr_sep;
int zasr_sep_create(const char* model_dir, int32_t device_id, zasr_sep** out);
void zasr_sep_destroy(zasr_sep* h);
/* fewest samples of a region (the encoder's kernel_size) */
int32_t zasr_sep_min_samples(const zasr_sep* h);
/* session.run(None, {"mixture": x})[0] (core/overlap_separator.py:291) for n mixtures in one
   call: region r is samples[offsets[r], offsets[r] + lengths[r]) of the `total` host samples;
   out (host) holds [2][lengths[r]] per region, regions in order (2 * sum lengths floats): the
   raw network output, zero from the last whole frame's end to lengths[r]. */
int zasr_sep_separate(zasr_sep* h, const float* samples, int64_t total, const int64_t* offsets,
                      const int64_t* lengths, int32_t n, float* out);
/* the same for regions [starts[r], starts[r] + lengths[r]) of the 16 kHz signal
   d_audio[0, total) already in HBM (core/overlap_separator.py:283 slices the host array); out
   is device memory when out_on_device, else host.  Ordered after `stream` (a hipStream_t,
   0 = none); synchronises before it returns.  Bit-identical to zasr_sep_separate. */
int zasr_sep_separate_device(zasr_sep* h, const float* d_audio, int64_t total,
                             const int64_t* starts, const int64_t* lengths, int32_t n, float* out,
                             int32_t out_on_device, void* stream);
/* The regions of a call run in launch groups whose activations (7.4 KB per frame of 16 samples)
   stay within `bytes` (default 4 GiB; a longer region runs alone); zasr_sep_last_groups is the
   number of groups of the last call.  Not counted in the budget: the call's device copy of the
   host samples (zasr_sep_separate: 4 bytes per sample) and its output buffer when the output
   goes to the host (8 bytes per region sample), both allocated for the whole call.  zasr_sep_trim frees the workspace the handle keeps
   between calls. */
int zasr_sep_set_budget(zasr_sep* h, int64_t bytes);
int32_t zasr_sep_last_groups(const zasr_sep* h);
int zasr_sep_trim(zasr_sep* h);
/* stage timing on HIP events (off by default): the milliseconds of the last call's encoder,
   1x1 GEMMs, norms + depthwise convolution, mask + decoder in ms4[0..3] (tools/sep_bench.py) */
int zasr_sep_set_profile(zasr_sep* h, int32_t on);
int zasr_sep_stage_ms(zasr_sep* h, float* ms4);

/* ---- community-1 speaker embeddings (core/speaker_diarization_pure_ort.py) ------------------
   The embedding stage of the reference's production diarizer: WeSpeaker fbank, the ResNet34
   encoder over every 10 s chunk, masked statistics pooling per (chunk, local speaker) and the
   5120 -> 256 projection (_extract_embeddings :769-879, compute_single_embedding :681-707).
   model_dir holds config.json + model.safetensors (zasr/resnet34.py).  A chunk's embedding does
   not depend on the other chunks of the call, on its place among them or on the group size.
   Invalid arguments return ZASR_ERR_INVALID, missing model files ZASR_ERR_NOT_FOUND. */
typedef struct zasr_emb zasr_emb;
int zasr_emb_create(const char* model_dir, int32_t device_id, zasr_emb** out);  /* :417-470 */
void zasr_emb_destroy(zasr_emb* h);
int32_t zasr_emb_embedding_dim(const zasr_emb* h);                    /* 256 */
/* frames of the encoder's output for T fbank frames (:849): three stride-2 stages */
int32_t zasr_emb_num_feat_frames(const zasr_emb* h, int32_t T);
/* multiply-adds x 2 of the encoder on one input of T frames, from the model's config */
double zasr_emb_encoder_flops(const zasr_emb* h, int32_t T);
/* compute_emb_fbank's rows WITHOUT the CMVN (:271-301) of wav[0, n) followed by `tail` zero
   samples (:812; 0 for none): rows = 1 + (n + tail - 400) / 160 (0 when shorter than a frame),
   returned in *rows; out [rows][80] (cap floats). */
int zasr_emb_fbank(zasr_emb* h, const float* wav, int64_t n, int64_t tail, float* out,
                   int64_t cap, int64_t* rows);
/* the encoder session's run (:842-845): feats [n][T][80] -> out [n][2560][T'], channel
   c * 10 + f, host in / out */
int zasr_emb_encode(zasr_emb* h, const float* feats, int32_t n, int32_t T, float* out);
/* _extract_embeddings (:803-872) on the 16 kHz signal d_wav[0, total) already in HBM: the fbank
   image of the signal and 160000 zeros, per chunk c the 998 rows from starts[c] / 160 with
   CMVN, the encoder, the pooling under masks_u8 [n_chunks][3][n_seg_frames] (the used mask,
   chosen on the host) and the projection; out [n_chunks][3][256] (host).  Ordered after
   `stream` (a hipStream_t, 0 = none); synchronises before it returns. */
int zasr_emb_chunks_device(zasr_emb* h, const float* d_wav, int64_t total, const int64_t* starts,
                           int32_t n_chunks, const uint8_t* masks_u8, int32_t n_seg_frames,
                           float* out, void* stream);
/* compute_single_embedding (:681-707) of wav[0, n) (host): *ok = 0 and out untouched when the
   segment has fewer than 9 fbank frames (the reference returns None).  Any length up to 2^20
   fbank frames (2.9 h; 31 KB of activations per frame); longer returns ZASR_ERR_RUNTIME. */
int zasr_emb_segment(zasr_emb* h, const float* wav, int64_t n, float* out, int32_t* ok);
/* chunks (or encode inputs) per launch group: 0 = sized from the free memory (31 MB per 10 s
   chunk, at most 128), else forced; _last_group is the last call's.  Results do not change. */
int zasr_emb_set_group(zasr_emb* h, int32_t group);
int32_t zasr_emb_last_group(const zasr_emb* h);
int zasr_emb_trim(zasr_emb* h);
/* stage timing on HIP events (off by default): fbank + windows, stem, layer1, layer2, layer3,
   layer4, pooling, projection of the last call in ms8[0..7] (tools/emb_bench.py) */
int zasr_emb_set_profile(zasr_emb* h, int32_t on);
int zasr_emb_stage_ms(zasr_emb* h, float* ms8);

/* ---- device audio front end --------------------------------------------------------------
   Raw PCM -> the 16 kHz mono float32 HBM signal that zasr_decode_device,
   zasr_vad_probs_device and zasr_campp_windows_device read, and the reference's level
   conditioning on that signal.  The handle caches one polyphase table per input rate and owns
   the pinned staging buffers of host sources.  Every entry point with a `stream` is ordered
   after the stream's earlier work; those that return a value to the host synchronise it.
   Results are bit-identical from run to run (no floating-point atomics anywhere). */
typedef struct zasr_audio zasr_audio;
enum { ZASR_AUDIO_F32 = 0, ZASR_AUDIO_I16 = 1 };
int zasr_audio_create(int32_t device_id, zasr_audio** out);
void zasr_audio_destroy(zasr_audio* h);
/* Host-only.  Samples zasr_audio_to_16k makes of n_frames frames at `rate`:
   ceil(n_frames * 16000 / rate) in integers; -1 for a rate outside 4000..384000. */
int64_t zasr_audio_out_len(int32_t rate, int64_t n_frames);
/* Host-only (no GPU): the polyphase table of `rate`.  With g = gcd(rate, 16000), P = 16000 / g,
   Q = rate / g, output m = q P + p is sum_t x[q Q + lo[p] + t] * w[p * taps + t], t < taps,
   x = 0 outside the signal: the Hann-windowed sinc of sherpa-onnx's LinearResample (the
   resampler behind OfflineStream::AcceptWaveform, which the reference's stream callers rely on;
   its file loader resamples with ffmpeg, core/asr_engine.py:501-508) with the 1 / rate factor
   folded in.  lo [P] and w [P * taps] (cap = elements of w) may both be NULL to read the sizes
   first.  out_tile / in_tile (nullable): outputs one workgroup makes per tile, and the input
   frames that many outputs span. */
int zasr_audio_resample_taps(int32_t rate, int32_t* P, int32_t* Q, int32_t* taps,
                             int32_t* out_tile, int32_t* in_tile, int32_t* lo, float* w,
                             int64_t cap);
/* Convert (int16 -> x * 2^-15, soundfile's dtype='float32' read), downmix (the mean over
   channels in float32, audio.mean(axis=1), core/asr_engine.py:497-500) and resample to 16 kHz
   in one pass: src holds n_frames frames of `channels` interleaved samples (1..8) of `format`
   at `rate` Hz (4000..384000), on the host (src_on_device 0: uploaded in bounded pinned pieces
   under the kernel) or on the device.  d_out (device, cap samples) receives *n_out =
   zasr_audio_out_len samples.  rate 16000 runs no filter: mono float32 is copied bit for bit.
   Replaces load_audio's decode-side work, core/asr_engine.py:492-508. */
int zasr_audio_to_16k(zasr_audio* h, const void* src, int32_t format, int32_t channels,
                      int32_t rate, int64_t n_frames, int32_t src_on_device, float* d_out,
                      int64_t cap, int64_t* n_out, void* stream);
/* *peak = max |d_wav[i]| (np.max(np.abs(audio)), core/asr_engine.py:513,
   core/audio_preprocessing.py:239); 0 for n = 0. */
int zasr_audio_peak(zasr_audio* h, const float* d_wav, int64_t n, float* peak, void* stream);
/* d_wav[i] = (d_wav[i] / divisor) * multiplier, two float32 roundings: the quiet-file boost
   audio / peak * 0.95 (core/asr_engine.py:514-515) with (peak, 0.95f), and the peak limiter
   audio * (0.95 / peak) (core/audio_preprocessing.py:240-241) with (1, 0.95f / peak). */
int zasr_audio_scale(zasr_audio* h, float* d_wav, int64_t n, float divisor, float multiplier,
                     void* stream);
/* out[s] = sum of d_wav[i]^2 over [seg_begin[s], seg_end[s]) in float64 (host array), all
   segments in one launch; segments must lie inside [0, n).  The device half of
   compute_segment_rms (core/audio_preprocessing.py:39-43, :76-83). */
int zasr_audio_segment_sumsq(zasr_audio* h, const float* d_wav, int64_t n,
                             const int64_t* seg_begin, const int64_t* seg_end, int32_t n_seg,
                             double* out, void* stream);
/* d_wav[i] *= gain(i) and *peak = max |result|, one pass.  The gain is 1 except on the
   pieces [piece_begin[k], piece_end[k]) (ascending, disjoint): piece_gain[k] where
   piece_ramp[k] < 0, else ramp_values[piece_ramp[k] + i - piece_begin[k]].  Applies the sparse
   form of the reference's gain_map (core/audio_preprocessing.py:100-129) and takes the
   limiter's peak (:239); n_pieces 0 is the peak alone. */
int zasr_audio_apply_gain(zasr_audio* h, float* d_wav, int64_t n, const int64_t* piece_begin,
                          const int64_t* piece_end, const float* piece_gain,
                          const int64_t* piece_ramp, int32_t n_pieces, const float* ramp_values,
                          int64_t n_ramp_values, float* peak, void* stream);

/* ---- WPE dereverberation -----------------------------------------------------------------
   apply_wpe_dereverberation (core/audio_preprocessing.py:157-216) for a ragged batch of chunks
   of one 16 kHz signal: Blackman STFT (512 / 128, 384 zeros of fading at both ends), the
   weighted prediction error filter of each frequency bin on its own (taps K, delay, iterations;
   correlation sums and the Cholesky solve in float64), the biorthogonal inverse STFT.  The
   per-frequency algorithm the function documents, as DESIGN.md 4k defines it; the reference's
   own call stacks the bins as channels and is not reproduced.  A chunk's result depends on
   that chunk alone (bit-identical whatever shares the call); a chunk under 1024 samples comes
   back unchanged (:188-189); a chunk over 60 s is refused. */
typedef struct zasr_wpe zasr_wpe;
int zasr_wpe_create(int32_t device_id, zasr_wpe** out);      /* core/audio_preprocessing.py:157-216 */
void zasr_wpe_destroy(zasr_wpe* h);
/* Host-only.  STFT frames of a chunk of n samples (core/audio_preprocessing.py:195, nara-wpe's
   stft with fading): ceil((n + 256) / 128) + 1; -1 for n outside 0..960000. */
int64_t zasr_wpe_frames(int64_t n);
/* Chunks [offsets[c], offsets[c] + lens[c]) (host arrays; chunks may overlap) of the device
   signal d_audio[0, total) -> d_out + out_offsets[c] (device, lens[c] samples each).  taps and
   delay in 1..16, iterations in 1..8.  Ordered after `stream`'s work; synchronises before
   returning.  core/audio_preprocessing.py:157-216, once per chunk there. */
int zasr_wpe_run_device(zasr_wpe* h, const float* d_audio, int64_t total, const int64_t* offsets,
                        const int64_t* lens, int32_t count, int32_t taps, int32_t delay,
                        int32_t iterations, float* d_out, const int64_t* out_offsets, void* stream);
/* The same with audio and out in host memory (core/audio_preprocessing.py:157-216). */
int zasr_wpe_run(zasr_wpe* h, const float* audio, int64_t total, const int64_t* offsets,
                 const int64_t* lens, int32_t count, int32_t taps, int32_t delay,
                 int32_t iterations, float* out, const int64_t* out_offsets);
/* No counterpart in core/audio_preprocessing.py:157-216 (one chunk per call there): the spectrum
   bytes the chunks of one launch group may take together (about 7.7 MB per 30 s chunk; a chunk
   beyond the budget runs alone), the groups of the last call, and the release of the
   workspace between files.  Results do not depend on the grouping. */
int zasr_wpe_set_budget(zasr_wpe* h, int64_t bytes);
int32_t zasr_wpe_last_groups(const zasr_wpe* h);
int zasr_wpe_trim(zasr_wpe* h);
/* stage timing on HIP events (off by default): STFT, iterations, inverse STFT of the last call
   in ms3[0..2] (tools/wpe_bench.py) */
int zasr_wpe_set_profile(zasr_wpe* h, int32_t on);
int zasr_wpe_stage_ms(zasr_wpe* h, float* ms3);

/* model facts */
int32_t zasr_vocab_size(const zasr_recognizer* h);
int32_t zasr_joiner_dim(const zasr_recognizer* h);
/* which kernel each part of the loaded model was routed to, as JSON into buf (cap bytes):
   {"precision", "ffn_fused_h3", "ffn_gemm_pair", "gemm_h3r", "gemm_x3_range", "cnx_ffn_h3",
   "dec_table"}.  In f16x3 a layer whose weights reach 31 in magnitude keeps the
   two-accumulator GEMMs (the one-accumulator kernels scale the weight's fp16 hi piece by
   2^11); a vocabulary whose V^2 x D decoder-context table exceeds ZASR_DEC_TABLE_MAX_GB
   (default 24) runs the per-frame decoder instead (dec_table 0).  No reference counterpart:
   a diagnostic of this build's dispatch, read by the tests. */
int zasr_model_routes(zasr_recognizer* h, char* buf, int64_t cap);
/* Replace the fbank's 80 triangular filters: banks row-major [80][n_bins] (n_bins 256, or
   257 with the Nyquist column zero).  The default is knf's mel-linear triangles
   (core/asr_engine.py:698-721); the reference's browser worker computes Hz-linear triangles
   (offline_pwa/static/js/pure-ort-asr-worker.js:369-397), which lets a test hold this kernel
   to that worker's own outputs.  Applies to later zasr_fbank / decode calls on h. */
int zasr_fbank_set_mel_banks(zasr_recognizer* h, const float* banks, int32_t n_bins);
/* Launch a no-op kernel with block_threads threads per block through the library's checked
   launch path (every kernel launch is followed by the runtime's launch status): a refused
   configuration (e.g. > 1024 threads) returns ZASR_ERR_RUNTIME with the HIP error in
   zasr_last_error().  No reference counterpart: a self-test of the error path. */
int zasr_selftest_launch(int32_t block_threads);
/* Kernel self-tests of the f16x3 one-accumulator kernels on host operands (device 0,
   synchronous; no reference counterpart: test infrastructure that reaches the shapes and row
   counts the decode meets only incidentally).  gemm_h3r: C[M][N'] = epi(A[M][K] W[N][K]^T +
   bias), epi 0 (none), 3 (C += ..., C is read) or 8 (GLU over interleaved rows, N' = N / 2);
   K in {96, 192, 256, 288, 384, 512}, N >= 128, N % 16 == 0.  ffn_h3: X[R][D] += W2
   SwooshL(W1 Y + b1) + b2, then X = byp_orig + (X - byp_orig) * byp_scale when byp_orig is
   given (the bypass_mid epilogue); D in {128, 256, 384, 512} (F % 32 == 0) or 192
   (F % 64 == 0).  Every |w| must be below 31 (the kernels scale the fp16 hi piece by 2^11). */
int zasr_selftest_gemm_h3r(int32_t M, int32_t K, int32_t N, int32_t epi, const float* A,
                           const float* W, const float* bias, float* C);
int zasr_selftest_ffn_h3(int32_t R, int32_t D, int32_t F, const float* Y, const float* W1,
                         const float* b1, const float* W2, const float* b2,
                         const float* byp_orig, const float* byp_scale, float* X);
/* The general projection GEMMs alone on one dense host problem (same conventions): mode
   ZASR_PRECISION_FP32 -> gemm_f32, ZASR_PRECISION_BF16 -> gemm_bf16 (a_bf16 / c_bf16: A / C held
   in bf16 on the device, A rounded to nearest even on upload, C widened on return),
   ZASR_PRECISION_BF16X3 / BF16X6 / F16X3 -> gemm_x3 with 2 / 3 / the two fp16 pieces.  A [M][K],
   W [N][K] (prepared as the model loader prepares a weight), bias [N] or null, aux [M][N] for
   the multiply epilogues (epi 4; 5: rounded to bf16 on upload), byp_orig [M][N] + byp_scale [N]
   or both null (the bypass_mid blend after epi 3), C [M][N] in / out (epi 8, GLU: [M][N / 2]).
   epi is a GemmEpi value (csrc/gemm.h).  One call of the public entry point with lda = K,
   ldc = the C width; the kernel is the one the shape reaches in a decode.  A combination the
   entry point refuses returns ZASR_ERR_RUNTIME with its message. */
int zasr_selftest_gemm(int32_t mode, int32_t M, int32_t K, int32_t N, int32_t epi, int32_t a_bf16,
                       int32_t c_bf16, const float* A, const float* W, const float* bias,
                       const float* aux, const float* byp_orig, const float* byp_scale, float* C);
/* The general GEMMs behind their other operand loaders (same conventions; no reference
   counterpart: test infrastructure).  Every output holds its buffer's initial contents on
   entry; guard bytes lie before and behind it on the device, and a changed guard byte returns
   ZASR_ERR_RUNTIME.  Every argument is checked before a launch; a refused combination returns
   ZASR_ERR_RUNTIME with a message and leaves later calls unaffected.
   conv_gemm: conv.4 (which = 4) or conv.7 (which = 7) of Conv2dSubsampling + SwooshR for a
   ragged batch exactly as a decode runs it: the implicit-im2col loaders ALOAD_CONV2 /
   ALOAD_CONV3 over one z-slice per sequence, the slices and the GEMM (gemm_f32 / gemm_bf16 /
   gemm_x3) chosen by the functions the decode itself calls.  T[nseq] fbank frames per sequence,
   each >= 9; with l2 = (T - 3) / 2 and L = (T - 7) / 2: conv.4 reads A [sum (T - 2)][80][8],
   W [32][72], writes C [sum l2][39][32] (3x3, stride (2, 2), no padding); conv.7 reads A
   [sum l2][39][32], W [128][288], writes C [sum L][19][128] (3x3, stride (1, 2)).  W is in the
   kernels' k order, k = (kt * 3 + kf) * channels + c, and prepared on the device as the model
   loader prepares a weight.  mode / (a_bf16, c_bf16): ZASR_PRECISION_FP32 and _BF16X3 /
   _BF16X6 / _F16X3 take (0, 0); _BF16 takes (1, 1) and (0, 0) for both layers and (0, 1) for
   conv.7; everything else is refused.
   gemm_aload: one gemm_f32 problem C[:, c_col : c_col + N] = epi(A' W[N][K]^T + bias) with
   aload 4 (ALOAD_BNRELU: A'[m][k] = max(A[m * lda + k] a_scale[k] + a_shift[k], 0), A [M][lda],
   epi 0 or 6) or 5 (ALOAD_IM2COL1D: row m = n * Tout + t, column k = q * C + c reads
   A[(n * Tin + t * stride + q * dil - pad) * lda + c], zero outside [0, Tin); A [ceil(M / Tout)
   * Tin][lda]; epi 0, 6 or 4 with aux [M][ldaux]).  epi is a GemmEpi value.  C [M][ldc] is
   passed and returned whole, so what lies outside the N written columns is visible.  What
   gemm_f32 refuses (another epilogue, K % C, M % Tout, C % 4, lda % 4, K % 4) returns its
   message. */
int zasr_selftest_conv_gemm(int32_t mode, int32_t which, int32_t a_bf16, int32_t c_bf16,
                            int32_t nseq, const int32_t* T, const float* A, const float* W,
                            const float* bias, float* C);
int zasr_selftest_gemm_aload(int32_t aload, int32_t M, int32_t K, int32_t N, int32_t lda,
                             int32_t ldc, int32_t c_col, int32_t epi, const float* A,
                             const float* W, const float* bias, const float* a_scale,
                             const float* a_shift, int32_t Tin, int32_t Tout, int32_t C_in,
                             int32_t stride, int32_t dil, int32_t pad, const float* aux,
                             int32_t ldaux, float* C);
/* The joiner kernels alone on one host problem (same conventions): out[M][V] = J[M][D]
   W[V][D]^T + bias through the launcher a decode uses.  mode: ZASR_PRECISION_FP32, _BF16,
   _BF16X3, _BF16X6 or _F16X3.  layout 0: row-major J (f32; rounded to bf16 on upload in the bf16
   mode), the 32 x 32 split-K kernels, D in {64, 128, 256, 512}.  layout 1: J and W in
   MFMA-fragment order (the speculative-greedy / beam joiner; every mode but fp32, D = 256 or
   512): J is laid out on the host as the search kernels write it (rows padded to a multiple of
   64, the pad rows finite and non-zero; the split modes' bf16 / fp16 pieces one image each).  W
   is prepared as the model loader prepares the joiner weight.  live_t / live_len
   [ceil(M / live_f)] and live_f: the finished-stream filter of the greedy windows (row r
   belongs to stream r / live_f; a tile whose streams all have live_t >= live_len may be
   skipped), or null / 0 for every row.  out holds the buffer's initial contents on entry, so a
   skipped tile keeps them.  A mode / layout / D combination outside the above returns
   ZASR_ERR_INVALID. */
int zasr_selftest_joiner(int32_t mode, int32_t layout, int32_t M, int32_t V, int32_t D,
                         const float* J, const float* W, const float* bias,
                         const int32_t* live_t, const int32_t* live_len, int32_t live_f,
                         float* out);
/* The bf16 mode's fused FeedforwardModule alone on host operands (same conventions):
   X[R][D] += W2 SwooshL(W1 bf16(X) + b1) + b2 with W1 [F][D], W2 [D][F] rounded to bf16 and
   the hidden activation in bf16 (then the bypass_mid blend when byp_orig is given);
   D in {64, 96, 128, 192, 256, 384, 512}; D >= 256: F % 32 == 0, F <= 2048.  form 0: the
   decode's route; 1: the opt-in per-CU rows form at D = 384 (ZASR_FFN_ROWS=1). */
int zasr_selftest_ffn_bf16(int32_t R, int32_t D, int32_t F, const float* W1, const float* b1,
                           const float* W2, const float* b2, const float* byp_orig,
                           const float* byp_scale, float* X, int32_t form);
/* The fused FFNs out of place (a layer's feed_forward1): the kernel reads X and writes
   Xout = X + FFN(X) (then the bypass_mid blend), the same operations in the same order as the
   in-place entries above (ffn_h3 with Y = X).  Xout holds its buffer's initial contents on
   entry and the result on return; X returns what the input buffer holds afterwards. */
int zasr_selftest_ffn_bf16_oop(int32_t R, int32_t D, int32_t F, const float* W1, const float* b1,
                               const float* W2, const float* b2, const float* byp_orig,
                               const float* byp_scale, float* X, float* Xout, int32_t form);
int zasr_selftest_ffn_h3_oop(int32_t R, int32_t D, int32_t F, const float* W1, const float* b1,
                             const float* W2, const float* b2, const float* byp_orig,
                             const float* byp_scale, float* X, float* Xout);
/* The fused stack seam (seam_kernel) and the three kernels it replaces, on the same host
   operands (same conventions).  L[nseq] 50 Hz frames per sequence (>= 1), rows = sum L.  The
   stack: width d, factor ds (1, 2, 4, 8), final X xd [sum ceil(L / ds)][d] (unused when
   ds = 1), 50 Hz input orig [rows][d], bypass scale s [d].  y = orig + (xd[t / ds] - orig) s
   (ds = 1: y = orig) is written to next [rows][dn] (truncated / zero-padded; dn = 0: none),
   SimpleDownsample'd by ds_next with weights wn8 to xnext [sum ceil(L / ds_next)][dn]
   (ds_next = 1: none), and, downsampled by 2 with weights wo2, to columns [c0, d) of out
   [sum ceil(L / 2)][ldo] (c0 >= d: none).  next / xnext / out hold the buffers' initial
   contents on entry and the fused kernel's on return; *_ref receive what stack_glue ->
   downsample(next, ds_next) -> downsample(full-dim output, 2) leave in buffers with the same
   initial contents (out_ref: only columns [c0, d) are meaningful). */
int zasr_selftest_seam(int32_t nseq, const int32_t* L, int32_t d, int32_t ds, int32_t dn,
                       int32_t ds_next, int32_t c0, int32_t ldo, const float* xd,
                       const float* orig, const float* s, const float* wn8, const float* wo2,
                       float* next, float* xnext, float* out, float* next_ref, float* xnext_ref,
                       float* out_ref);
/* The convolution path's hand-written kernels and BiasNorm alone on host operands (same
   conventions; no reference counterpart: test infrastructure).  Ragged batches are given as
   per-sequence lengths; the offsets and row -> sequence maps are built as a decode builds them,
   and every entry makes exactly the launch call a decode makes.  Every output holds its
   buffer's initial contents on entry and the kernel's on return; one guard row follows each
   output on the device, and a changed guard byte returns ZASR_ERR_RUNTIME.  "bf16" operands are
   rounded to nearest even on upload and widened on return.
   dwconv1d: the ConvolutionModule core, out[rows][d] = SwooshR(b[c] + sum_k w[c][k] g[t + k -
   K / 2][c]) with zero padding per sequence, rows = sum L, d % 4 == 0, K odd <= 31, w [d][K].
   glu = 1: x [rows][2 d] and g = x[:, :d] sigmoid(x[:, d:]) (the fp32 mode); glu = 0: g = x
   [rows][d], in f32 or (bf16 = 1) with bf16 x and out (the bf16 modes); glu with bf16 is
   refused.
   conv1: conv.0 (1 -> 8, 3x3, padding (0, 1)) + SwooshR, fb [sum T][80] -> out [sum (T - 2)]
   [80][8], every T >= 3, w [8][9]; form 0 the libm SwooshR, 1 the native-exp form, 2 that form
   with bf16 out.
   convnext: x [rows][19][128], depthwise dw_w [128][7][7] (time, freq) + dw_b, pw1 w1 [384][128]
   + b1, pw2 w2 [128][384] + b2.  form 0: the f32 depthwise 7x7 alone, y = dwconv(x) + dw_b (the
   MLP's operands and out may be null).  form 1: the bf16 block, y the depthwise output and
   out = x + pw2(SwooshL(pw1(y) + b1)) + b2, x / y / out and the pw weights in bf16.  form 2:
   the f16x3 pair, the f32 depthwise then the fp16-piece MLP in place over x's buffer as a
   decode runs it (out returns that buffer; its initial contents are x, not the caller's out).
   bias_norm: x[rows][d] *= exp(log_scale) / sqrt(mean((x - bias)^2)), then, with orig and
   bscale [d] (both or neither), x = orig + (x - orig) bscale; d % 4 == 0, d <= 1024.
   copy_mode 0: no copy; 1: the result also to copy_out; 2: the result also over orig's own
   device buffer (a layer's copy for the next one).  orig returns what its buffer holds
   afterwards. */
int zasr_selftest_dwconv1d(int32_t nseq, const int32_t* L, int32_t d, int32_t K, int32_t glu,
                           int32_t bf16, const float* x, const float* w, const float* b,
                           float* out);
int zasr_selftest_conv1(int32_t nseq, const int32_t* T, int32_t form, const float* fb,
                        const float* w, const float* b, float* out);
int zasr_selftest_convnext(int32_t nseq, const int32_t* L, int32_t form, const float* x,
                           const float* dw_w, const float* dw_b, const float* w1, const float* b1,
                           const float* w2, const float* b2, float* y, float* out);
int zasr_selftest_bias_norm(int32_t rows, int32_t d, const float* bias, float log_scale,
                            float* orig, const float* bscale, int32_t copy_mode, float* x,
                            float* copy_out);
/* The attention kernels' block map alone (host only, no device call; no reference counterpart:
   test infrastructure).  lens[nseq] frames per sequence, units_per_seq heads or z-chunks;
   out[b] for block id b = sequence << 12 | unit << 8 | query tile (128 frames), or 0xffffffff
   for an id past its range's end; block id b belongs to range b % 8, the units of range x
   being contiguous in (sequence, unit) order and the 8 ranges near-equal in block-steps.
   order 0: a range's slots run sequence -> tile -> unit (the decode's), 1: sequence -> unit ->
   tile.  *grid = the launch's block count = 8 * the longest range's blocks; ZASR_ERR_INVALID
   if it exceeds cap. */
int zasr_selftest_attn_block_map(const int32_t* lens, int32_t nseq, int32_t units_per_seq,
                                 int32_t order, uint32_t* out, int64_t cap, int32_t* grid);
/* The attention kernels alone on one ragged batch of host operands (same conventions as the
   convolution entries; no reference counterpart: test infrastructure).  L[nseq] frames per
   sequence (0 allowed, at least one frame in all), R = sum L packed rows.  qkp [R][68 H]: per row
   the queries [H][32], the keys [H][32], the positional queries [H][4]; pos_tab
   [2 pmax - 1][4 H], row x + pmax - 1 for the key offset x = j - i.  mode: ZASR_PRECISION_FP32
   (attn_softmax_kernel / attn_sa_kernel) or _BF16, _BF16X3, _BF16X6, _F16X3 (attn_flash_kernel
   through launch_attn_flash with the block map in the decode's order).  In the bf16 mode qkp, v,
   h3, out and z are held in bf16 on the device (rounded to nearest even on upload, widened on
   return) and the stored query and positional-query columns carry the log2(e) factor the model
   loader folds into attn_in, so the softmax is taken in base 2 over the stored values; the
   other modes take the natural softmax.  Offsets are those a decode derives (the weight block
   of sequence b is [L_b][stride], stride = L_b rounded up to 32, to 4 in fp32; t1^T columns
   32-padded per sequence).  Every output holds its buffer's initial contents on entry; a guard
   region follows each on the device and a changed guard byte returns ZASR_ERR_RUNTIME.  Refused
   with ZASR_ERR_RUNTIME before any launch: an odd H or H > 16 outside fp32, a negative length,
   pmax below the longest sequence (fp32: below that length rounded up to 32, its kernels do not
   clamp the table rows), hid % 4 != 0, and a mode the entry's route does not have.
   attn_weights: head 0's normalised weights as a decode materialises them, A0 [sum L_b
   stride_b] f32, padding columns zero; modes fp32, bf16x3, bf16x6 (bf16 and f16x3 consume the
   weights inside the fused NonlinAttention kernel: refused).
   attn_sa: the layer's two self-attentions, out1 = softmax(S) v1 with running statistics
   (flash mode 1 / attn_sa online), which writes stats, then out2 = softmax(S) v2 from those
   stored statistics (flash mode 2 / attn_sa); v, out [R][12 H]; stats [R][H], row max +
   log2(row sum) of the base-2 scores (fp32: [R][H][2], row max and 1 / row sum, natural).
   nonlin: h3 [R][3 hid] = (s, x, y); t1t receives launch_nonlin_prep_t's image of
   t1 = tanh(s) x as stored: [pieces][hid][sum L32_b] 16-bit patterns (bf16: one bf16 plane;
   bf16x3 / bf16x6: 2 / 3 bf16 planes that sum to t1; f16x3: the fp16 planes hi and
   (t1 - hi) 2^11).  bf16 and f16x3 then run flash mode 3, z [R][hid] = (A0 t1) y; bf16x3 /
   bf16x6 stop at the image (z may be null); fp32 is refused. */
int zasr_selftest_attn_weights(int32_t mode, int32_t H, int32_t nseq, const int32_t* L,
                               int32_t pmax, const float* qkp, const float* pos_tab, float* A0);
int zasr_selftest_attn_sa(int32_t mode, int32_t H, int32_t nseq, const int32_t* L, int32_t pmax,
                          const float* qkp, const float* pos_tab, const float* v1,
                          const float* v2, float* out1, float* stats, float* out2);
int zasr_selftest_nonlin(int32_t mode, int32_t H, int32_t nseq, const int32_t* L, int32_t pmax,
                         int32_t hid, const float* qkp, const float* pos_tab, const float* h3,
                         uint16_t* t1t, float* z);

/* The transducer search kernels alone on host arrays (no reference counterpart: test
   infrastructure): one frame of launch_search_step, one super-step of launch_greedy_spec, and
   launch_search_final, through the launchers a decode calls.  Every array is uploaded, the
   call synchronises, and every array marked in / out is returned as the device holds it
   afterwards; all arrays of a call sit in one device allocation with a guard region before and
   behind each, and a changed guard byte returns ZASR_ERR_RUNTIME.  Every argument is checked
   before anything is launched (ZASR_ERR_INVALID for a null argument, ZASR_ERR_RUNTIME with a
   message otherwise).
   zasr_st_state: the SearchState of S streams x Hmax hypothesis slots (kernels.h), all in / out:
   lp, lpf, hash, len, y1, y2, hw, node [S Hmax], nh [S]; the emission node pool node_tok /
   node_frame / node_parent / node_lp [S node_cap], node_stats [S node_cap][4], node_count [S].
   hash is opaque: returned by one call and passed to the next.  Live slots (below nh) must hold
   y1, y2 in [0, V), hw a state of the automaton, node in [-1, node_count); node_cap must leave
   room for `beam` (greedy: 1) more nodes behind node_count in every stream.
   zasr_st_hotwords: n phrases as concatenated token ids (lens[n]) with their scores; the
   automaton is the engine's own build_hotword_dfa.  n = 0: no hotwords.
   zasr_st_table: the decoder-context table and the joiner input it feeds.  The entry builds
   the full table itself, table[y2][y1][:] = a[y2][:] + b[y1][:] (a, b [V][D]; V V D floats, at
   most 2^27: a small D for the large vocabularies), so no context a kernel forms can index
   outside it.  enc [enc_rows][D], stream s's frames from row enc_off[s] (enc_off[s] + enc_len[s]
   <= enc_rows).  jfmt: 0 f32 [rows][D]; 1 bf16 [rows][D]; 2 bf16 in MFMA-fragment order
   (kernels.h JoinerArgs, JOINER_PACKED; joiner_packed_rows(rows) rows); 3 / 4: 2 / 3 bf16 piece
   images in fragment order; 5: the fp16 images hi and (x - hi) 2^11 in fragment order (2 - 5:
   D = 256 or 512).  J (in / out, j_bytes = exactly the format's size) is returned whole.
   search_step: t >= 0: one frame, logits [S Hmax][V] (every row readable); tab nullable (the
   decjoin route's instantiation, no J).  t < 0: launch_search_init (and launch_table_init with a
   table) instead, logits ignored.  J rows = S Hmax.
   greedy_spec: beam 1 (Hmax = 1), window F = 4 or 8, logits [S][F][V], J rows = S F, t_cur [S]
   and active [2] in / out.  init 0: the super-step; 1: launch_search_init +
   launch_greedy_spec_init, then the super-step; 2: the two init launches alone.
   search_final: out_tok / out_frame / out_lp [S out_cap], out_stats [S out_cap][4], out_count
   [S], all in / out; node_parent[i] must be in [-1, i).
   hotword_dfa: build_hotword_dfa's tables on the host (no launch): tok2cls [V]; with
   *num_states and *num_cls set on return, next / delta [cap] and node_score [cap] receive
   [states][cls] and [states] (ZASR_ERR_RUNTIME when cap is too small). */
typedef struct zasr_st_state {
  int32_t S, Hmax, node_cap;
  double* lp;
  int32_t* lpf;
  uint64_t* hash;
  int32_t *len, *y1, *y2, *hw, *node, *nh;
  int32_t *node_tok, *node_frame, *node_parent;
  double* node_lp;
  float* node_stats;
  int32_t* node_count;
} zasr_st_state;
typedef struct zasr_st_hotwords {
  const int32_t* tokens;
  const int32_t* lens;
  const float* scores;
  int32_t n;
} zasr_st_hotwords;
typedef struct zasr_st_table {
  int32_t D, jfmt, enc_rows;
  const float *a, *b, *enc;
  const int32_t* enc_off;
  void* J;
  int64_t j_bytes;
} zasr_st_table;
int zasr_selftest_search_step(int32_t V, int32_t beam, int32_t t, const int32_t* enc_len,
                              const zasr_st_state* st, const float* logits,
                              const zasr_st_hotwords* hw, const zasr_st_table* tab);
int zasr_selftest_greedy_spec(int32_t V, int32_t F, int32_t init, int32_t parity,
                              const int32_t* enc_len, int32_t* t_cur, int32_t* active,
                              const zasr_st_state* st, const float* logits,
                              const zasr_st_hotwords* hw, const zasr_st_table* tab);
int zasr_selftest_search_final(int32_t V, const zasr_st_state* st, const zasr_st_hotwords* hw,
                               int32_t out_cap, int32_t* out_tok, int32_t* out_frame,
                               double* out_lp, float* out_stats, int32_t* out_count);
int zasr_selftest_hotword_dfa(int32_t V, const zasr_st_hotwords* hw, int32_t cap,
                              int32_t* num_states, int32_t* num_cls, int32_t* tok2cls,
                              int32_t* next, double* delta, double* node_score);

/* The CAM++, Silero VAD and ViBERT kernels alone on host arrays (no reference counterpart: test
   infrastructure; tests/test_gpu_aux_kernels.py against tests/aux_reference.py).  Each entry
   uploads its operands, runs exactly one launch function on the null stream of device 0 (vad_frames
   with `len`: launch_vad_maxabs first) and synchronises.  Every output is in / out: it starts as
   the caller's image, is returned whole, and has guard bytes behind it on the device; a changed
   guard byte returns ZASR_ERR_RUNTIME.  What a launch function refuses (Ci > 32, H > 1024,
   L > 256, a head dim outside {16, 32, 64}) and every index that would leave an array are
   ZASR_ERR_RUNTIME with a message before any launch.
   campp_conv2d: launch_campp_conv2d, kernel ks (1: pad 0, 3: pad 1), stride (sf, 1), 32 output
   channels; x [n][ci][fi][T] (in_tf: [n][T][fi], ci = 1), w [32][ci][ks][ks], scale / shift
   [32], res nullable [n][32][fo][T], fo = (fi - 1) / sf + 1; y [n][32][fo][T], or tdnn_out
   [n][T][32 fo].  use_mfma = 1 also passes the weights permuted by
   campp_conv2d_permute_weights (ci = 32), so the launcher takes the MFMA kernel when its own
   conditions hold; rb = 0: the engine's rows per block, rb > 0 (even): that many.  *route = 1
   when the MFMA kernel ran (0: the direct kernel), *rb_used its rows per block (0: direct).
   campp_cam_mask: h [n][T][128], w1 [64][128], b1 [64], w2 [32][64], b2 [32], mexp [n][T][32].
   campp_stats: x [N][T][C], s / b [C], out [N][2 C] (mean | unbiased std of relu(x s + b)).
   campp_cmvn: x [rows][80] in place, sequence i = rows [fr_off[i], fr_off[i + 1]).
   campp_gather: rows [nrows][80], window w = rows [win_row[w], + win_n[w]) zero-padded to wf
   frames, out [nwin][wf][80].
   vad_frames: frames [n_windows * 4][256].  Row mode (rows576 [n_windows][576] not null): the
   other arrays are ignored.  File mode: audio [n_samples], off / win_start [n_files] (first
   sample / first window of each file; file f has win_start[f + 1] - win_start[f] windows); len
   and maxabs [n_files] both null (no boost) or both given: launch_vad_maxabs fills a zeroed
   table, which the frames kernel reads and maxabs returns.
   vad_im2col: which 0: launch_vad_mag_im2col, in = S [N * 4][ldS] (re | im, C bins each), A
   [N * 4][Kp]; which 1: launch_vad_im2col, in = Y [N * T][C], A [N * Tout][3 C], Tout =
   (T - 1) / stride + 1.
   vad_lstm: gx [windows][512], whh [512][128], bhh [512], wd [128]; segments as VadLstmArgs
   (kernels.h): seg_start / seg_count [nseg], seg_warm nullable, init nullable [nseg][2][128];
   probs [windows], s_out / e_out nullable [nseg][2][128].
   vibert_ln: x [rows][H].  ids null: launch_vibert_layernorm in place.  Otherwise
   launch_vibert_embed: ids / tt [rows], word [V][H], pos [P][H] (P >= L), type [TT][H].
   vibert_attn: qkv [B L][3 H], mask [B L] (0 = padding), ctx [B L][H], scale 1 / sqrt(H / heads).
   vibert_gather: x [B L][H], offsets [B][W] in [0, L), g [B W][H]. */
int zasr_selftest_campp_conv2d(int32_t ks, int32_t ci, int32_t fi, int32_t sf, int32_t T, int32_t n,
                               int32_t relu, int32_t tdnn_out, int32_t in_tf, int32_t use_mfma,
                               int32_t rb, const float* x, const float* w, const float* scale,
                               const float* shift, const float* res, float* y, int32_t* route,
                               int32_t* rb_used);
int zasr_selftest_campp_cam_mask(int32_t n, int32_t T, int32_t seg_len, const float* h,
                                 const float* w1, const float* b1, const float* w2,
                                 const float* b2, float* mexp);
int zasr_selftest_campp_stats(int32_t N, int32_t T, int32_t C, const float* x, const float* s,
                              const float* b, float* out);
int zasr_selftest_campp_cmvn(int32_t nseq, int32_t rows, const int32_t* fr_off, float* x);
int zasr_selftest_campp_gather(int32_t nwin, int32_t wf, int32_t nrows, const float* rows,
                               const int32_t* win_row, const int32_t* win_n, float* out);
/* The community-1 embedding kernels, one launch each on host operands; the output keeps what the
   caller put there wherever the kernel does not write, with guard bytes before and behind it.
   emb_conv2d: x [n][Fi][Ti][Ci] (the stem, Ci = 1: [n][Ti][Fi]), w [Co][(r ks + q) Ci + ci],
   bias [Co], res (nullable) and y [n][Fo][To][Co]; ks 1 | 3, stride 1 | 2, Ci, Co in
   {32, 64, 128, 256}, or Ci = 1 (ks 3, stride 1, ReLU, no residual); route 0 = the launcher's
   pick, 1 = 32 channels per block, 2 = 64 (Co >= 64); *n_routes returns how many the layer takes.
   emb_pool: x [n][F][T][C], mask [n][S][nseg] (null with pop), stats [n S][2 C F]. */
int zasr_selftest_emb_conv2d(int32_t ks, int32_t stride, int32_t ci, int32_t co, int32_t n,
                             int32_t fi, int32_t ti, int32_t relu, int32_t route, const float* x,
                             const float* w, const float* bias, const float* res, float* y,
                             int32_t* n_routes);
int zasr_selftest_emb_pool(int32_t n, int32_t F, int32_t T, int32_t C, int32_t S, int32_t nseg,
                           int32_t pop, const float* x, const uint8_t* mask, float* stats);
int zasr_selftest_vad_frames(int32_t n_files, int64_t n_windows, int64_t n_samples,
                             const float* audio, const int64_t* off, const int64_t* win_start,
                             const int64_t* len, const float* rows576, uint32_t* maxabs,
                             float* frames);
int zasr_selftest_vad_im2col(int32_t which, int64_t N, int32_t T, int32_t C, int32_t stride,
                             int32_t ldS, int32_t Kp, const float* in, float* A);
int zasr_selftest_vad_lstm(int64_t windows, int32_t nseg, const float* gx, const float* whh,
                           const float* bhh, const float* wd, float bd, const int64_t* seg_start,
                           const int32_t* seg_count, const int32_t* seg_warm, const float* init,
                           float* probs, float* s_out, float* e_out);
int zasr_selftest_vibert_ln(int64_t rows, int32_t H, int32_t L, const int64_t* ids,
                            const int64_t* tt, int32_t V, int32_t P, int32_t TT, const float* word,
                            const float* pos, const float* type, const float* g, const float* b,
                            float eps, float* x);
int zasr_selftest_vibert_attn(int32_t B, int32_t L, int32_t heads, int32_t H, const float* qkv,
                              const int64_t* mask, float* ctx);
int zasr_selftest_vibert_gather(int32_t B, int32_t L, int32_t W, int32_t H, const float* x,
                                const int64_t* offsets, float* g);
/* The PyanNet segmentation and Conv-TasNet separation kernels other than the GEMMs, alone (test
   infrastructure; tests/test_gpu_segsep_kernels.py against tests/segsep_reference.py).  As the
   entries above, except that each runs its one launch function of seg.h / sep.h on a stream of
   its own.  Outputs are in / out with guard bytes behind them; the in-place seg_norm_act and
   every separation output (the partial sums included) also have guard bytes in front.
   float2 (mean, rstd) and double2 (sum, sum of squares) arrays are passed as [.][2].
   seg_chunk_stats: audio [total], starts [n] >= 0 (samples past `total` are zeros), stats [n][2].
   seg_front: as above plus stats [n][2] from the caller, w0t [251][80] (tap-major); out
   [n][F1][80], F1 = ((T - 251) / 10 + 1) / 3 >= 1.
   seg_pool3: x [n][L][C] -> out [n][Fp][C].  seg_norm_act: x [n][F][C] in place, stats
   [n][C][2], w / b [C].  max_blocks > 0 caps the grid of these grid-stride launches (0: the
   engine's).  seg_frame_stats: x [n][F][C] -> stats [n][C][2].
   seg_lstm: gx [n F][1024], whh [2][512][128], out [n F][256]; `group` sequences per workgroup.
   seg_head: x [rows][128], w [7][128], b [7] -> logits [rows][7], classes [rows].
   The separation entries take one call's regions as (sig_off, T) each, F = (T - win) / hop + 1
   frames, and run the launch group [r0, r0 + ng) of it on the region and tile tables the
   engine's own builder makes for the groups [0, r0) and [r0, r0 + ng); M = the group's frames,
   nt = its tiles (of at most 32 frames, none across a region edge), rows in region order.
   sep_frames: signal [n_signal] -> frames [M][win].  sep_tile_sums: x [M][C] -> partial [nt][2].
   sep_region_stats: partial [nt][2] -> stats [n_regions][2], written for the group's regions.
   sep_gln_apply: stats [n_regions][2], gamma / beta [C]; src [M][C] -> dst [M][C], or in_place:
   dst holds the input, src is ignored.  sep_mid: h [M][C], w [3][C] (tap-major), bias [C] -> y
   [M][C], partial [nt][2].  sep_prelu: x [rows][ld] in place on columns [col0, col0 + C).
   sep_overlap_add: dec0 / dec1 [M][win], out_off [n_regions] -> out [n_out], region r's two
   streams at out[out_off[r] + s T + t]. */
typedef struct zasr_sep_call {
  int32_t n_regions;
  const int64_t* sig_off; /* [n_regions] */
  const int32_t* T;       /* [n_regions] */
  int32_t r0, ng, win, hop;
} zasr_sep_call;
int zasr_selftest_seg_chunk_stats(int64_t total, int32_t n, int32_t T, const float* audio,
                                  const int64_t* starts, float* stats);
int zasr_selftest_seg_front(int64_t total, int32_t n, int32_t T, const float* audio,
                            const int64_t* starts, const float* stats, float in_w, float in_b,
                            const float* w0t, float* out);
int zasr_selftest_seg_pool3(int32_t n, int32_t L, int32_t C, int32_t Fp, int32_t max_blocks,
                            const float* x, float* out);
int zasr_selftest_seg_frame_stats(int32_t n, int32_t F, int32_t C, const float* x, float* stats);
int zasr_selftest_seg_norm_act(int32_t n, int32_t F, int32_t C, int32_t max_blocks,
                               const float* stats, const float* w, const float* b, float* x);
int zasr_selftest_seg_lstm(int32_t n, int32_t F, int32_t group, const float* gx, const float* whh,
                           float* out);
int zasr_selftest_seg_head(int64_t rows, const float* x, const float* w, const float* b,
                           float* logits, uint8_t* classes);
int zasr_selftest_sep_frames(const zasr_sep_call* call, int64_t n_signal, const float* signal,
                             float* frames);
int zasr_selftest_sep_tile_sums(const zasr_sep_call* call, int32_t C, const float* x,
                                double* partial);
int zasr_selftest_sep_region_stats(const zasr_sep_call* call, int32_t C, const double* partial,
                                   float* stats);
int zasr_selftest_sep_gln_apply(const zasr_sep_call* call, int32_t C, int32_t in_place,
                                const float* stats, const float* gamma, const float* beta,
                                const float* src, float* dst);
int zasr_selftest_sep_mid(const zasr_sep_call* call, int32_t C, int32_t dil, float slope,
                          const float* stats, const float* gamma, const float* beta, const float* w,
                          const float* bias, const float* h, float* y, double* partial);
int zasr_selftest_sep_prelu(int64_t rows, int32_t C, int32_t ld, int32_t col0, float slope,
                            int32_t max_blocks, float* x);
int zasr_selftest_sep_overlap_add(const zasr_sep_call* call, const int64_t* out_off, int64_t n_out,
                                  const float* dec0, const float* dec1, float* out);
/* The WPE kernels alone on one chunk, host operands, complex values as (re, im) pairs
   (core/audio_preprocessing.py:157-216).  wpe_stft: signal [n] -> Y [257][T]
   complex64, T = zasr_wpe_frames(n), and *max_sq = max |Y|^2.  wpe_iter: one iteration on
   Y [257][T] with the chunk maximum max_sq (epsilon = 1e-10 max_sq): x from g_prev [257][taps]
   complex128 (NULL: x = y) -> g [257][taps] complex128, and when given X [T][257] complex64 =
   y - g^H ytilde and *next_max_sq = max |X|^2.  wpe_istft: X [T][257] -> out [n],
   T = zasr_wpe_frames(n). */
int zasr_selftest_wpe_stft(zasr_wpe* h, const float* signal, int64_t n, float* Y, float* max_sq);
int zasr_selftest_wpe_iter(zasr_wpe* h, const float* Y, int32_t T, int32_t taps, int32_t delay,
                           float max_sq, const double* g_prev, double* g, float* X,
                           float* next_max_sq);
int zasr_selftest_wpe_istft(zasr_wpe* h, const float* X, int32_t T, int64_t n, float* out);

/* ---- speaker diarization: the spectral embedding of Senko's SpectralCluster on the device ----
   core/speaker_diarization_senko_campp_optimized.py:192-228 (_senko_spectral up to the
   eigenvectors; the eigengap rule, k-means and the segment logic are host code in
   zasr/diarize.py).  2 <= N <= 8192 windows, 1 <= D <= 512; anything else is
   ZASR_ERR_INVALID.  Every entry selects the handle's device first; results are bit-identical
   from run to run.  Stage entries take device pointers and are ordered on `stream`. */
typedef struct zasr_diar zasr_diar;
int zasr_diar_create(int32_t device_id, zasr_diar** out);
void zasr_diar_destroy(zasr_diar* h);
/* _cosine_similarity (:183-189): d_M [N][N] = Xn Xn^T with Xn = X / (|X|_2 + 1e-10), float32
   throughout (D % 4 == 0, which includes CAM++'s 192, takes the exact-f32 MFMA GEMM). */
int zasr_diar_similarity(zasr_diar* h, const float* d_X, int32_t N, int32_t D, float* d_M,
                         void* stream);
/* p_pruning, symmetrise and the degrees (:201-215), d_M in place: per row the
   n_elems = max(min(int((1 - pval) N), N - min_pnum), 0) smallest entries become 0 (entries
   equal to the threshold value survive from the lowest column index up; the reference's
   argsort leaves ties undefined), M <- 0.5 (M + M^T), diagonal <- 0, d_deg[i] = sum_j |M_ij|
   in float64.  0 <= pval <= 1, min_pnum >= 1. */
int zasr_diar_prune(zasr_diar* h, float* d_M, int32_t N, double pval, int32_t min_pnum,
                    double* d_deg, void* stream);
/* numpy.linalg.eigh(L)'s k smallest eigenpairs (:215-218, L = diag(deg) - M, never stored):
   lambdas [k] ascending and vecs [N][k] on the host, 1 <= k <= min(16, N), by
   Chebyshev-filtered subspace iteration in float64 until every residual |L v - lambda v|_2 is
   at most 1e-7 of the Gershgorin bound 2.02 max deg.  *passes (nullable) = outer passes run.
   ZASR_ERR_RUNTIME with a message if 200 passes do not converge.  Synchronises `stream`. */
int zasr_diar_eigs(zasr_diar* h, const float* d_M, const double* d_deg, int32_t N, int32_t k,
                   double* lambdas, double* vecs, int32_t* passes, void* stream);
/* the three stages on X [N][D] (host, or device when x_on_device) in the handle's workspace */
int zasr_diar_spectral_embed(zasr_diar* h, const float* X, int32_t x_on_device, int32_t N,
                             int32_t D, double pval, int32_t min_pnum, int32_t k,
                             double* lambdas, double* vecs, void* stream);
/* passes and block Laplacian products of the handle's last eigs / spectral_embed (no reference
   counterpart: a diagnostic read by the tests and tools/diar_bench.py) */
int zasr_diar_last_stats(zasr_diar* h, int32_t* passes, int64_t* applications);

/* ---- community-1 clustering: centroid-linkage AHC on the device ----
   core/speaker_diarization_pure_ort.py:918-921 (the linkage + fcluster of _cluster; PLDA, VBx,
   the assignment and the reconstruction are host code in zasr/vbx.py).  2 <= N <= 16384 rows,
   1 <= D <= 512, a threshold that is not NaN; anything else is ZASR_ERR_INVALID.  Rows must be
   finite.  Results are bit-identical from run to run and between the forced routes. */
typedef struct zasr_clu zasr_clu;
int zasr_clu_create(int32_t device_id, zasr_clu** out);
void zasr_clu_destroy(zasr_clu* h);
/* :918-921: labels [N] (host) = the flat clustering of
   fcluster(linkage(Xn, "centroid", "euclidean"), threshold, "distance") with
   Xn = X / (|X|_2 + 1e-10) in float32, X float32 [N][D] on the host or (x_on_device) on the
   device.  Clusters are numbered from 0 by their lowest member row (the reference's numbering is
   arbitrary and canonicalised at :640).  Synchronises `stream`. */
int zasr_clu_ahc(zasr_clu* h, const float* X, int32_t x_on_device, int32_t N, int32_t D,
                 double threshold, int32_t* labels, void* stream);
/* merges done and rows rescanned by the handle's last ahc (a diagnostic, no reference
   counterpart) */
int zasr_clu_last_stats(zasr_clu* h, int64_t* merges, int64_t* rescans);
/* HIP-event timing of the stages of the next ahc calls: ms4 = normalise (with the upload),
   pairwise, nearest neighbours, merge loop */
int zasr_clu_set_profile(zasr_clu* h, int32_t on);
int zasr_clu_stage_ms(zasr_clu* h, float* ms4);
/* test hook: force the merge loop's route on this handle (0 = a workgroup of 1024 threads, the
   default; 1 = 256 threads); *n_routes (nullable) = the number of routes */
int zasr_selftest_clu_route(zasr_clu* h, int32_t route, int32_t* n_routes);

/* profiling: per-kernel-class HIP-event timing on the handle's stream.  on = 0 off,
   1 kernel classes, 2 kernel classes with the encoder GEMMs split by shape
   ("enc_gemm|M|K|N|w16|a16|c16|epi" class names, for the per-shape roofline table) */
int zasr_profile_enable(zasr_recognizer* h, int32_t on);
int zasr_profile_reset(zasr_recognizer* h);
/* writes "name count total_ms\n" lines into buf (cap bytes) */
int zasr_profile_report(zasr_recognizer* h, char* buf, int64_t cap);

const char* zasr_last_error(void);
const char* zasr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ZASR_H_ */
