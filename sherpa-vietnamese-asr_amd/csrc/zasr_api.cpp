// C ABI of libzasr (include/zasr.h): argument checking, error capture, result objects.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/zasr.h"
#include "audio.h"
#include "campp.h"
#include "clu.h"
#include "common.h"
#include "diar.h"
#include "seg.h"
#include "emb.h"
#include "sep.h"
#include "vad.h"
#include "vibert.h"
#include "wpe.h"
#include "engine.h"
#include "host_io.h"
#include "onnx_io.h"

using zasr::Engine;
using zasr::TokenResult;

struct zasr_recognizer {
  std::unique_ptr<Engine> eng;
  std::string model_dir;
  // the symbol table (sherpa-onnx OfflineModelConfig.tokens; zasr_set_tokens, default
  // model_dir/tokens.txt), loaded on the first JSON result (sherpa-onnx SymbolTable: a
  // leading "\u2581" becomes a space)
  std::string tokens_path;
  std::mutex sym_mu;
  // immutable once published: a reader copies the pointer under sym_mu and keeps its table
  // alive across a concurrent zasr_set_tokens, which only swaps the pointer
  std::shared_ptr<const std::vector<std::string>> syms;
};

// an offline stream (sherpa-onnx OfflineStream): the samples accepted so far and, once
// decoded, its result; bound to the recognizer that created it
struct zasr_stream {
  zasr_recognizer* rec = nullptr;
  std::vector<float> samples;
  bool decoded = false;
  TokenResult res;
};

struct zasr_result {
  std::vector<TokenResult> items;
};

struct zasr_campp {
  std::unique_ptr<zasr::CamppEngine> eng;
};

struct zasr_vibert {
  std::unique_ptr<zasr::VibertEngine> eng;
};

struct zasr_vad {
  std::unique_ptr<zasr::VadEngine> eng;
};

struct zasr_seg {
  std::unique_ptr<zasr::SegEngine> eng;
};

struct zasr_sep {
  std::unique_ptr<zasr::SepEngine> eng;
};

struct zasr_emb {
  std::unique_ptr<zasr::EmbEngine> eng;
};

struct zasr_audio {
  std::unique_ptr<zasr::AudioFrontEnd> eng;
};

struct zasr_wpe {
  std::unique_ptr<zasr::WpeEngine> eng;
};

struct zasr_diar {
  std::unique_ptr<zasr::DiarEngine> eng;
  int last_passes = 0;
};

struct zasr_clu {
  std::unique_ptr<zasr::CluEngine> eng;
};

namespace {
thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const std::invalid_argument& e) {
    return fail(ZASR_ERR_NOT_FOUND, e.what());
  } catch (const std::exception& e) {
    return fail(ZASR_ERR_RUNTIME, e.what());
  } catch (...) {
    return fail(ZASR_ERR_RUNTIME, "unknown error");
  }
}

int resolve_beam(zasr_recognizer* h, int32_t beam) {
  return beam > 0 ? beam : h->eng->default_beam();
}

// fewest samples the encoder accepts: 9 fbank frames ((n + 80) / 160 >= 9); shorter streams
// decode to an empty result, as an encoder output of no frames does
constexpr long kMinStreamSamples = 9 * 160 - 80;

// Decode streams [s0, s1, ...] of one recognizer in ONE batched pass (host samples staged
// into one device buffer, the zasr_decode_batch path); results stored in the streams.
void decode_streams_impl(zasr_recognizer* h, zasr_stream* const* ss, int n) {
  Engine* e = h->eng.get();
  std::vector<int> idx;
  std::vector<long> off, len;
  long tot = 0;
  for (int i = 0; i < n; ++i) {
    const long m = (long)ss[i]->samples.size();
    if (m < kMinStreamSamples) {
      ss[i]->res = TokenResult{};
      ss[i]->decoded = true;
      continue;
    }
    idx.push_back(i);
    off.push_back(tot);
    len.push_back(m);
    tot += m;
  }
  if (idx.empty()) return;
  std::lock_guard<std::mutex> lk(e->mu);
  float* d = nullptr;
  ZASR_HIP_CHECK(hipMalloc(&d, tot * sizeof(float)));
  std::unique_ptr<float, decltype(&hipFree)> guard(d, hipFree);
  for (size_t j = 0; j < idx.size(); ++j)
    ZASR_HIP_CHECK(hipMemcpyAsync(d + off[j], ss[idx[j]]->samples.data(), len[j] * 4,
                                  hipMemcpyHostToDevice, e->stream()));
  std::vector<TokenResult> r = e->decode_device(d, off, len, e->default_beam(), e->stream());
  ZASR_HIP_CHECK(hipStreamSynchronize(e->stream()));
  for (size_t j = 0; j < idx.size(); ++j) {
    ss[idx[j]]->res = std::move(r[j]);
    ss[idx[j]]->decoded = true;
  }
}

std::shared_ptr<const std::vector<std::string>> symbols(zasr_recognizer* h) {
  std::lock_guard<std::mutex> lk(h->sym_mu);
  if (!h->syms) {
    const std::string path = h->tokens_path.empty() ? h->model_dir + "/tokens.txt" : h->tokens_path;
    std::ifstream f(path);
    if (!f) throw std::invalid_argument("symbol table not found: " + path);
    auto tab = std::make_shared<std::vector<std::string>>();
    std::string line;
    while (std::getline(f, line)) {
      std::istringstream ls(line);
      std::string sym, id_s;
      if (!(ls >> sym >> id_s)) continue;
      const long id = std::stol(id_s);
      if (id < 0) continue;
      if (sym.compare(0, 3, "\xe2\x96\x81") == 0) sym.replace(0, 3, " ");
      if ((long)tab->size() <= id) tab->resize(id + 1);
      (*tab)[id] = sym;
    }
    h->syms = std::move(tab);
  }
  return h->syms;
}

void json_string(std::ostringstream& os, const std::string& s) {
  os << '"';
  for (unsigned char c : s) {
    if (c == '"' || c == '\\') os << '\\' << c;
    else if (c < 0x20) {
      char b[8];
      std::snprintf(b, sizeof b, "\\u%04x", c);
      os << b;
    } else os << c;
  }
  os << '"';
}

}  // namespace

extern "C" {

int zasr_create(const zasr_config* cfg, zasr_recognizer** out) {
  if (!cfg || !out || !cfg->model_dir) return fail(ZASR_ERR_INVALID, "null config/model_dir/out");
  *out = nullptr;
  if (cfg->blank_penalty != 0.f) return fail(ZASR_ERR_INVALID, "blank_penalty must be 0");
  std::string method = cfg->decoding_method ? cfg->decoding_method : "modified_beam_search";
  bool greedy = (method == "greedy_search");
  if (!greedy && method != "modified_beam_search")
    return fail(ZASR_ERR_INVALID, "decoding_method must be greedy_search or modified_beam_search");
  int beam = greedy ? 1 : cfg->max_active_paths;
  if (beam < 1 || beam > 16) return fail(ZASR_ERR_INVALID, "max_active_paths must be in 1..16");
  if (cfg->num_hotwords < 0) return fail(ZASR_ERR_INVALID, "num_hotwords < 0");
  return guarded([&]() {
    std::vector<std::vector<int>> phrases;
    std::vector<float> scores;
    const int32_t* tp = cfg->hotword_tokens;
    for (int i = 0; i < cfg->num_hotwords; ++i) {
      int n = cfg->hotword_lens[i];
      if (n < 0) return fail(ZASR_ERR_INVALID, "negative hotword length");
      phrases.emplace_back(tp, tp + n);
      tp += n;
      scores.push_back(cfg->hotword_scores[i]);
    }
    auto* h = new zasr_recognizer;
    try {
      h->eng.reset(new Engine(cfg->model_dir, cfg->device_id, beam, greedy, phrases, scores,
                              cfg->precision));
    } catch (...) {
      delete h;
      throw;
    }
    h->model_dir = cfg->model_dir;
    *out = h;
    return (int)ZASR_OK;
  });
}

void zasr_destroy(zasr_recognizer* h) { delete h; }

int zasr_campp_create(const char* model_dir, int32_t device_id, zasr_campp** out) {
  if (!model_dir || !out) return fail(ZASR_ERR_INVALID, "null model_dir/out");
  *out = nullptr;
  return guarded([&]() {
    auto* h = new zasr_campp;
    try {
      h->eng.reset(new zasr::CamppEngine(model_dir, device_id));
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
    return (int)ZASR_OK;
  });
}

void zasr_campp_destroy(zasr_campp* h) { delete h; }

int32_t zasr_campp_embedding_dim(const zasr_campp* h) { return h ? h->eng->emb_dim() : 0; }

int zasr_vibert_create(const char* model_dir, int32_t device_id, zasr_vibert** out) {
  if (!model_dir || !out) return fail(ZASR_ERR_INVALID, "null model_dir/out");
  *out = nullptr;
  return guarded([&]() {
    auto* h = new zasr_vibert;
    try {
      h->eng.reset(new zasr::VibertEngine(model_dir, device_id));
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
    return (int)ZASR_OK;
  });
}

void zasr_vibert_destroy(zasr_vibert* h) { delete h; }

int32_t zasr_vibert_num_labels(const zasr_vibert* h) { return h ? h->eng->num_labels() : 0; }
int32_t zasr_vibert_num_detect(const zasr_vibert* h) { return h ? h->eng->num_detect() : 0; }

int zasr_vibert_run(zasr_vibert* h, const int64_t* input_ids, const int64_t* attention_mask,
                    const int64_t* token_type_ids, const int64_t* input_offsets, int32_t batch,
                    int32_t n_tokens, int32_t n_words, float* logits, float* detect_logits) {
  if (!h || (batch > 0 && (!input_ids || !attention_mask || !token_type_ids || !input_offsets ||
                           !logits || !detect_logits)))
    return fail(ZASR_ERR_INVALID, "null argument");
  if (batch < 0 || n_tokens < 1 || n_words < 1) return fail(ZASR_ERR_INVALID, "bad batch shape");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->run_host(reinterpret_cast<const long*>(input_ids), reinterpret_cast<const long*>(attention_mask),
                     reinterpret_cast<const long*>(token_type_ids),
                     reinterpret_cast<const long*>(input_offsets), batch, n_tokens, n_words, logits,
                     detect_logits);
    return (int)ZASR_OK;
  });
}

int zasr_vad_create(const char* model_dir, int32_t device_id, zasr_vad** out) {
  if (!model_dir || !out) return fail(ZASR_ERR_INVALID, "null model_dir/out");
  *out = nullptr;
  return guarded([&]() {
    auto* h = new zasr_vad;
    try {
      h->eng.reset(new zasr::VadEngine(model_dir, device_id));
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
    return (int)ZASR_OK;
  });
}

void zasr_vad_destroy(zasr_vad* h) { delete h; }

int32_t zasr_vad_last_passes(const zasr_vad* h) { return h ? h->eng->last_passes() : 0; }

int zasr_vad_probs(zasr_vad* h, const float* audio, const int64_t* offsets,
                   const int64_t* lengths, int32_t n_files, int32_t auto_boost, float* probs) {
  if (!h || n_files < 0 || (n_files > 0 && (!audio || !offsets || !lengths || !probs)))
    return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->probs_host(audio, reinterpret_cast<const long*>(offsets),
                       reinterpret_cast<const long*>(lengths), n_files, auto_boost != 0, probs);
    return (int)ZASR_OK;
  });
}

int zasr_vad_probs_device(zasr_vad* h, const float* d_audio, const int64_t* offsets,
                          const int64_t* lengths, int32_t n_files, int32_t auto_boost,
                          float* d_probs, void* stream) {
  if (!h || n_files < 0 || (n_files > 0 && (!d_audio || !offsets || !lengths || !d_probs)))
    return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->probs_device(d_audio, reinterpret_cast<const long*>(offsets),
                         reinterpret_cast<const long*>(lengths), n_files, auto_boost != 0, d_probs,
                         reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

int zasr_vad_window(zasr_vad* h, const float* input, const float* state, int32_t n, float* prob,
                    float* state_out) {
  if (!h || n < 0 || (n > 0 && (!input || !state || !prob || !state_out)))
    return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->window_host(input, state, n, prob, state_out);
    return (int)ZASR_OK;
  });
}

int zasr_seg_create(const char* model_dir, int32_t device_id, zasr_seg** out) {
  if (!model_dir || !out) return fail(ZASR_ERR_INVALID, "null model_dir/out");
  *out = nullptr;
  return guarded([&]() {
    auto* h = new zasr_seg;
    try {
      h->eng.reset(new zasr::SegEngine(model_dir, device_id));
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
    return (int)ZASR_OK;
  });
}

void zasr_seg_destroy(zasr_seg* h) { delete h; }

int32_t zasr_seg_num_frames(const zasr_seg*, int64_t chunk_samples) {
  return zasr::SegEngine::num_frames((long)chunk_samples);
}

int64_t zasr_seg_num_chunks(int64_t total, int32_t chunk_samples, int32_t step_samples) {
  if (total <= 0 || chunk_samples <= 0 || step_samples <= 0) return 0;
  return (int64_t)zasr::SegEngine::chunk_starts((long)total, chunk_samples, step_samples).size();
}

int32_t zasr_seg_last_group(const zasr_seg* h) { return h ? h->eng->last_group() : 0; }

int zasr_seg_set_group(zasr_seg* h, int32_t group) {
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  if (group != 0 && group != 1 && group != 2 && group != 4 && group != 8 && group != 16)
    return fail(ZASR_ERR_INVALID, "segmentation: group must be 0 (automatic), 1, 2, 4, 8 or 16");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  h->eng->set_group(group);
  return ZASR_OK;
}

int zasr_seg_trim(zasr_seg* h) {
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->trim();
    return (int)ZASR_OK;
  });
}

int zasr_seg_set_profile(zasr_seg* h, int32_t on) {
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  h->eng->set_profile(on != 0);
  return ZASR_OK;
}

int zasr_seg_stage_ms(zasr_seg* h, float* ms5) {
  if (!h || !ms5) return fail(ZASR_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  std::memcpy(ms5, h->eng->stage_ms(), sizeof(float) * zasr::SegEngine::kStages);
  return ZASR_OK;
}

int zasr_seg_logits(zasr_seg* h, const float* batch, int32_t n, int32_t T, float* logits) {
  if (n <= 0) return fail(ZASR_ERR_INVALID, "segmentation: n must be positive");
  if (T < zasr::SegEngine::kMinSamples)
    return fail(ZASR_ERR_INVALID, "segmentation: a chunk needs at least 1261 samples (2 frames)");
  if (!h || !batch || !logits) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->logits_host(batch, n, T, logits);
    return (int)ZASR_OK;
  });
}

int zasr_seg_classes_device(zasr_seg* h, const float* d_audio, int64_t total,
                            int32_t chunk_samples, int32_t step_samples, uint8_t* classes,
                            float* d_logits, void* stream) {
  if (chunk_samples < zasr::SegEngine::kMinSamples)
    return fail(ZASR_ERR_INVALID, "segmentation: a chunk needs at least 1261 samples (2 frames)");
  if (step_samples <= 0) return fail(ZASR_ERR_INVALID, "segmentation: step must be positive");
  if (!h || total < 0 || (total > 0 && (!d_audio || !classes)))
    return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->classes_device(d_audio, (long)total, chunk_samples, step_samples, classes, d_logits,
                           reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

// ---- Conv-TasNet overlap separation (core/overlap_separator.py) ----
int zasr_sep_create(const char* model_dir, int32_t device_id, zasr_sep** out) {  // :45-60
  if (!model_dir || !out) return fail(ZASR_ERR_INVALID, "null model_dir/out");
  *out = nullptr;
  return guarded([&]() {
    auto* h = new zasr_sep;
    try {
      h->eng.reset(new zasr::SepEngine(model_dir, device_id));
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
    return (int)ZASR_OK;
  });
}

void zasr_sep_destroy(zasr_sep* h) { delete h; }

// the encoder's kernel_size; core/overlap_separator.py:291 never sees less than 0.4 s (:286-292)
int32_t zasr_sep_min_samples(const zasr_sep* h) { return h ? h->eng->min_samples() : 0; }

namespace {
// region bounds of core/overlap_separator.py:283 (samples[s:e]), checked before the engine
int check_sep_regions(const zasr_sep* h, int64_t total, const int64_t* starts,
                      const int64_t* lengths, int32_t n) {
  if (n <= 0) return fail(ZASR_ERR_INVALID, "separation: n must be positive");
  if (!starts || !lengths || total < 0) return fail(ZASR_ERR_INVALID, "null argument");
  for (int32_t r = 0; r < n; ++r) {
    if (lengths[r] < h->eng->min_samples())
      return fail(ZASR_ERR_INVALID, "separation: a region needs at least " +
                                        std::to_string(h->eng->min_samples()) + " samples");
    if (starts[r] < 0 || lengths[r] > total || starts[r] > total - lengths[r])
      return fail(ZASR_ERR_INVALID, "separation: region outside the signal");
  }
  return ZASR_OK;
}
}  // namespace

int zasr_sep_separate(zasr_sep* h, const float* samples, int64_t total, const int64_t* offsets,
                      const int64_t* lengths, int32_t n, float* out) {  // :281-296
  if (!h || !samples || !out) return fail(ZASR_ERR_INVALID, "null argument");
  if (const int rc = check_sep_regions(h, total, offsets, lengths, n)) return rc;
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->separate_host(samples, (long)total, reinterpret_cast<const long*>(offsets),
                          reinterpret_cast<const long*>(lengths), n, out);
    return (int)ZASR_OK;
  });
}

int zasr_sep_separate_device(zasr_sep* h, const float* d_audio, int64_t total,
                             const int64_t* starts, const int64_t* lengths, int32_t n, float* out,
                             int32_t out_on_device, void* stream) {  // :281-296
  if (!h || !d_audio || !out) return fail(ZASR_ERR_INVALID, "null argument");
  if (const int rc = check_sep_regions(h, total, starts, lengths, n)) return rc;
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->separate_device(d_audio, (long)total, reinterpret_cast<const long*>(starts),
                            reinterpret_cast<const long*>(lengths), n, out, out_on_device != 0,
                            reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

// no counterpart in core/overlap_separator.py (one region per session call there, :297): the
// bound on what the regions of one call may allocate together
int zasr_sep_set_budget(zasr_sep* h, int64_t bytes) {
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  if (bytes <= 0) return fail(ZASR_ERR_INVALID, "separation: the budget must be positive");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  h->eng->set_budget((size_t)bytes);
  return ZASR_OK;
}

int32_t zasr_sep_last_groups(const zasr_sep* h) { return h ? h->eng->last_groups() : 0; }

// core/overlap_separator.py keeps its session for the process's life (:72-73); this frees
// the activations between files
int zasr_sep_trim(zasr_sep* h) {
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->trim();
    return (int)ZASR_OK;
  });
}

// stage times of the call that replaces core/overlap_separator.py:297 (tools/sep_bench.py)
int zasr_sep_set_profile(zasr_sep* h, int32_t on) {
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  h->eng->set_profile(on != 0);
  return ZASR_OK;
}

int zasr_sep_stage_ms(zasr_sep* h, float* ms4) {
  if (!h || !ms4) return fail(ZASR_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  std::memcpy(ms4, h->eng->stage_ms(), sizeof(float) * zasr::SepEngine::kStages);
  return ZASR_OK;
}

// ---- community-1 speaker embeddings (core/speaker_diarization_pure_ort.py) ----
int zasr_emb_create(const char* model_dir, int32_t device_id, zasr_emb** out) {  // :417-470
  if (!model_dir || !out) return fail(ZASR_ERR_INVALID, "null model_dir/out");
  *out = nullptr;
  return guarded([&]() {
    auto* h = new zasr_emb;
    try {
      h->eng.reset(new zasr::EmbEngine(model_dir, device_id));
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
    return (int)ZASR_OK;
  });
}

void zasr_emb_destroy(zasr_emb* h) { delete h; }

int32_t zasr_emb_embedding_dim(const zasr_emb* h) { return h ? h->eng->embed_dim() : 0; }

// :849 out[0].shape[1]
int32_t zasr_emb_num_feat_frames(const zasr_emb* h, int32_t T) {
  return h ? h->eng->num_feat_frames(T) : 0;
}

double zasr_emb_encoder_flops(const zasr_emb* h, int32_t T) {
  return h && T >= 1 ? h->eng->encoder_flops(T) : 0.0;
}

int zasr_emb_fbank(zasr_emb* h, const float* wav, int64_t n, int64_t tail, float* out, int64_t cap,
                   int64_t* rows) {  // :271-301, :807-817
  if (!h || !rows || n < 0 || tail < 0 || (n > 0 && !wav)) return fail(ZASR_ERR_INVALID, "null argument");
  if (n > INT32_MAX || tail > INT32_MAX) return fail(ZASR_ERR_INVALID, "embedding: signal too long");
  const int64_t r = zasr::EmbEngine::fbank_rows((long)n, (long)tail);
  *rows = r;
  if (r * 80 > cap || (r > 0 && !out)) return fail(ZASR_ERR_INVALID, "output buffer too small");
  if (r == 0) return ZASR_OK;
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->fbank_host(wav, (long)n, (long)tail, out);
    return (int)ZASR_OK;
  });
}

int zasr_emb_encode(zasr_emb* h, const float* feats, int32_t n, int32_t T, float* out) {  // :842-845
  if (!h || !feats || !out) return fail(ZASR_ERR_INVALID, "null argument");
  if (n <= 0 || T <= 0 || T > (1 << 16)) return fail(ZASR_ERR_INVALID, "embedding: n >= 1, 1 <= T <= 65536");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->encode_host(feats, n, T, out);
    return (int)ZASR_OK;
  });
}

int zasr_emb_chunks_device(zasr_emb* h, const float* d_wav, int64_t total, const int64_t* starts,
                           int32_t n_chunks, const uint8_t* masks_u8, int32_t n_seg_frames,
                           float* out, void* stream) {  // :803-872
  if (!h || !d_wav || !starts || !masks_u8 || !out) return fail(ZASR_ERR_INVALID, "null argument");
  if (n_chunks <= 0 || n_seg_frames <= 0 || total <= 0 || total > INT32_MAX - 160000)
    return fail(ZASR_ERR_INVALID, "embedding: n_chunks, n_seg_frames, total must be positive");
  for (int32_t c = 0; c < n_chunks; ++c)
    if (starts[c] < 0) return fail(ZASR_ERR_INVALID, "embedding: negative chunk start");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->chunks_device(d_wav, (long)total, reinterpret_cast<const long*>(starts), n_chunks,
                          masks_u8, n_seg_frames, out, reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

int zasr_emb_segment(zasr_emb* h, const float* wav, int64_t n, float* out, int32_t* ok) {  // :681-707
  if (!h || !out || !ok || n < 0 || (n > 0 && !wav)) return fail(ZASR_ERR_INVALID, "null argument");
  *ok = 0;
  if (n > INT32_MAX) return fail(ZASR_ERR_INVALID, "embedding: segment too long");
  if (zasr::EmbEngine::fbank_rows((long)n, 0) < 9) return ZASR_OK;  // :690 "too short"
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    *ok = h->eng->segment_host(wav, (long)n, out) ? 1 : 0;
    return (int)ZASR_OK;
  });
}

// the reference's embedding_batch_size (:822) bounds the host batch; here the launch group
int zasr_emb_set_group(zasr_emb* h, int32_t group) {
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  if (group < 0 || group > zasr::EmbEngine::kMaxGroup)
    return fail(ZASR_ERR_INVALID, "embedding: group must be 0 (automatic) or 1 .. 128");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  h->eng->set_group(group);
  return ZASR_OK;
}

int32_t zasr_emb_last_group(const zasr_emb* h) { return h ? h->eng->last_group() : 0; }

int zasr_emb_trim(zasr_emb* h) {
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->trim();
    return (int)ZASR_OK;
  });
}

int zasr_emb_set_profile(zasr_emb* h, int32_t on) {
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  h->eng->set_profile(on != 0);
  return ZASR_OK;
}

int zasr_emb_stage_ms(zasr_emb* h, float* ms8) {
  if (!h || !ms8) return fail(ZASR_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  std::memcpy(ms8, h->eng->stage_ms(), sizeof(float) * zasr::EmbEngine::kStages);
  return ZASR_OK;
}

int zasr_selftest_emb_conv2d(int32_t ks, int32_t stride, int32_t ci, int32_t co, int32_t n,
                             int32_t fi, int32_t ti, int32_t relu, int32_t route, const float* x,
                             const float* w, const float* bias, const float* res, float* y,
                             int32_t* n_routes) {
  if (!x || !w || !bias || !y) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_emb_conv2d(ks, stride, ci, co, n, fi, ti, relu, route, x, w, bias, res, y, n_routes);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_emb_pool(int32_t n, int32_t F, int32_t T, int32_t C, int32_t S, int32_t nseg,
                           int32_t pop, const float* x, const uint8_t* mask, float* stats) {
  if (!x || !stats) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_emb_pool(n, F, T, C, S, nseg, pop, x, mask, stats);
    return (int)ZASR_OK;
  });
}

int zasr_campp_fbank(zasr_campp* h, const float* wav, int64_t n, float* out, int64_t cap,
                     int64_t* n_frames) {
  if (!h || !n_frames || (n > 0 && !wav)) return fail(ZASR_ERR_INVALID, "null argument");
  const int64_t frames = n >= 400 ? 1 + (n - 400) / 160 : 0;
  *n_frames = frames;
  if (frames * 80 > cap || (frames > 0 && !out)) return fail(ZASR_ERR_INVALID, "output buffer too small");
  if (frames == 0) return ZASR_OK;
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    std::vector<float> f;
    h->eng->fbank_host(wav, (long)n, f);
    std::memcpy(out, f.data(), f.size() * sizeof(float));
    return (int)ZASR_OK;
  });
}

int zasr_campp_embed(zasr_campp* h, const float* feats, int32_t count, int32_t n_frames,
                     float* out) {
  if (!h || (count > 0 && (!feats || !out))) return fail(ZASR_ERR_INVALID, "null argument");
  if (count < 0 || n_frames < 1) return fail(ZASR_ERR_INVALID, "count >= 0 and n_frames >= 1 required");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->embed_host(feats, count, n_frames, out);
    return (int)ZASR_OK;
  });
}

int zasr_campp_embed_device(zasr_campp* h, const float* d_feats, int32_t count, int32_t n_frames,
                            float* d_out, void* stream) {
  if (!h || (count > 0 && (!d_feats || !d_out))) return fail(ZASR_ERR_INVALID, "null argument");
  if (count < 0 || n_frames < 1) return fail(ZASR_ERR_INVALID, "count >= 0 and n_frames >= 1 required");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->embed_device(d_feats, count, n_frames, d_out, reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

int zasr_campp_windows_device(zasr_campp* h, const float* d_wav, const int64_t* region_off,
                              const int64_t* region_len, int32_t n_regions, int32_t window_frames,
                              int32_t step_frames, float* d_feats, int64_t max_windows,
                              int32_t* window_region, int32_t* window_first,
                              int32_t* window_nframes, int64_t* n_windows, void* stream) {
  if (!h || !n_windows || n_regions < 0 || (n_regions > 0 && (!d_wav || !region_off || !region_len)) ||
      max_windows < 0 || (max_windows > 0 && (!d_feats || !window_region || !window_first || !window_nframes)))
    return fail(ZASR_ERR_INVALID, "null argument");
  if (window_frames < 1 || step_frames < 1)
    return fail(ZASR_ERR_INVALID, "window_frames and step_frames must be >= 1");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    *n_windows = h->eng->windows_device(d_wav, reinterpret_cast<const long*>(region_off),
                                        reinterpret_cast<const long*>(region_len), n_regions,
                                        window_frames, step_frames, d_feats, max_windows,
                                        window_region, window_first, window_nframes,
                                        reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

int zasr_convert_model(const char* model_dir, const char* out_dir) {
  if (!model_dir || !out_dir) return fail(ZASR_ERR_INVALID, "null model_dir/out_dir");
  return guarded([&]() {
    zasr::SafeTensors w;
    const std::string cfg = zasr::load_model_dir(model_dir, w);
    zasr::write_safetensors(std::string(out_dir) + "/model.safetensors", w);
    FILE* f = fopen((std::string(out_dir) + "/config.json").c_str(), "wb");
    if (!f) return fail(ZASR_ERR_RUNTIME, std::string("cannot write config.json in ") + out_dir);
    const size_t wr = fwrite(cfg.data(), 1, cfg.size(), f);
    fclose(f);
    if (wr != cfg.size()) return fail(ZASR_ERR_RUNTIME, "short write of config.json");
    return (int)ZASR_OK;
  });
}

int zasr_convert_stage_model(const char* kind, const char* model_dir, const char* out_dir) {
  if (!kind || !model_dir || !out_dir) return fail(ZASR_ERR_INVALID, "null kind/model_dir/out_dir");
  const std::string k(kind);
  if (k != "silero" && k != "campp" && k != "vibert")
    return fail(ZASR_ERR_INVALID, "kind must be silero, campp or vibert");
  return guarded([&]() {
    zasr::SafeTensors w;
    const std::string cfg = zasr::load_stage_dir(model_dir, k, w);
    zasr::write_safetensors(std::string(out_dir) + "/" + zasr::stage_safetensors_name(k), w);
    const std::string cp = std::string(out_dir) + "/" + k + "_config.json";
    FILE* f = fopen(cp.c_str(), "wb");
    if (!f) return fail(ZASR_ERR_RUNTIME, "cannot write " + cp);
    const size_t wr = fwrite(cfg.data(), 1, cfg.size(), f);
    fclose(f);
    if (wr != cfg.size()) return fail(ZASR_ERR_RUNTIME, "short write of " + cp);
    return (int)ZASR_OK;
  });
}

int zasr_fbank(zasr_recognizer* h, const float* wav, int64_t n, int32_t sr, float* out,
               int64_t cap, int64_t* n_frames) {
  if (!n_frames || (n > 0 && !wav)) return fail(ZASR_ERR_INVALID, "null argument");
  if (sr != 16000) return fail(ZASR_ERR_INVALID, "sample rate must be 16000");
  int64_t frames = n > 0 ? (n + 80) / 160 : 0;
  *n_frames = frames;
  if (frames * 80 > cap || (frames > 0 && !out)) return fail(ZASR_ERR_INVALID, "output buffer too small");
  if (frames == 0) return ZASR_OK;
  return guarded([&]() {
    Engine* e = h ? h->eng.get() : nullptr;
    if (!e) return fail(ZASR_ERR_INVALID, "zasr_fbank needs a recognizer handle");
    std::lock_guard<std::mutex> lk(e->mu);
    e->fbank_host(wav, (long)n, out);
    return (int)ZASR_OK;
  });
}

int zasr_decode_batch(zasr_recognizer* h, const float* const* wav, const int64_t* n,
                      int32_t count, int32_t beam, zasr_result** out) {
  if (!h || !out || count < 0 || (count > 0 && (!wav || !n))) return fail(ZASR_ERR_INVALID, "null argument");
  *out = nullptr;
  return guarded([&]() {
    Engine* e = h->eng.get();
    std::lock_guard<std::mutex> lk(e->mu);
    // stage host chunks into one device buffer, then run the device path
    std::vector<long> off(count), len(count);
    long tot = 0;
    for (int i = 0; i < count; ++i) {
      if (n[i] < 0) return fail(ZASR_ERR_INVALID, "negative length");
      off[i] = tot;
      len[i] = (long)n[i];
      tot += (long)n[i];
    }
    float* d = nullptr;
    ZASR_HIP_CHECK(hipMalloc(&d, std::max<long>(tot, 1) * sizeof(float)));
    std::unique_ptr<float, decltype(&hipFree)> guard(d, hipFree);
    for (int i = 0; i < count; ++i)
      if (len[i] > 0)
        ZASR_HIP_CHECK(hipMemcpyAsync(d + off[i], wav[i], len[i] * 4, hipMemcpyHostToDevice, e->stream()));
    auto r = std::make_unique<zasr_result>();
    r->items = e->decode_device(d, off, len, resolve_beam(h, beam), e->stream());
    ZASR_HIP_CHECK(hipStreamSynchronize(e->stream()));
    *out = r.release();
    return (int)ZASR_OK;
  });
}

int zasr_decode_features(zasr_recognizer* h, const float* const* feats, const int64_t* n_frames,
                         int32_t count, int32_t beam, zasr_result** out) {
  if (!h || !out || count < 0 || (count > 0 && (!feats || !n_frames))) return fail(ZASR_ERR_INVALID, "null argument");
  *out = nullptr;
  return guarded([&]() {
    Engine* e = h->eng.get();
    std::lock_guard<std::mutex> lk(e->mu);
    std::vector<const float*> f(feats, feats + count);
    std::vector<long> fr(n_frames, n_frames + count);
    auto r = std::make_unique<zasr_result>();
    r->items = e->decode_features(f, fr, resolve_beam(h, beam));
    *out = r.release();
    return (int)ZASR_OK;
  });
}

int zasr_decode_device(zasr_recognizer* h, const float* d_wav, const int64_t* wav_off,
                       const int64_t* n, int32_t count, int32_t beam, void* stream,
                       zasr_result** out) {
  if (!h || !out || count < 0 || (count > 0 && (!d_wav || !wav_off || !n))) return fail(ZASR_ERR_INVALID, "null argument");
  *out = nullptr;
  return guarded([&]() {
    Engine* e = h->eng.get();
    std::lock_guard<std::mutex> lk(e->mu);
    std::vector<long> off(wav_off, wav_off + count), len(n, n + count);
    auto r = std::make_unique<zasr_result>();
    r->items = e->decode_device(d_wav, off, len, resolve_beam(h, beam),
                                reinterpret_cast<hipStream_t>(stream));
    *out = r.release();
    return (int)ZASR_OK;
  });
}

int zasr_decode_device_batches(zasr_recognizer* h, const float* d_wav, const int64_t* wav_off,
                               const int64_t* n, int32_t count, const int32_t* batch_sizes,
                               int32_t n_batches, int32_t beam, void* stream, zasr_result** out) {
  if (!h || !out || count < 0 || n_batches < 0 || (n_batches > 0 && !batch_sizes) ||
      (count > 0 && (!d_wav || !wav_off || !n)))
    return fail(ZASR_ERR_INVALID, "null argument");
  *out = nullptr;
  long total = 0;
  for (int32_t i = 0; i < n_batches; ++i) {
    if (batch_sizes[i] < 0) return fail(ZASR_ERR_INVALID, "negative batch size");
    total += batch_sizes[i];
  }
  if (total != count) return fail(ZASR_ERR_INVALID, "batch sizes must sum to count");
  return guarded([&]() {
    Engine* e = h->eng.get();
    std::lock_guard<std::mutex> lk(e->mu);
    std::vector<long> off(wav_off, wav_off + count), len(n, n + count);
    std::vector<int> bs(batch_sizes, batch_sizes + n_batches);
    auto r = std::make_unique<zasr_result>();
    r->items = e->decode_device_batches(d_wav, off, len, bs, resolve_beam(h, beam),
                                        reinterpret_cast<hipStream_t>(stream));
    *out = r.release();
    return (int)ZASR_OK;
  });
}

int zasr_decode_host_batches(zasr_recognizer* h, const float* wav, const int64_t* wav_off,
                             const int64_t* n, int32_t count, const int32_t* batch_sizes,
                             int32_t n_batches, int32_t beam, void* stream, zasr_result** out) {
  if (!h || !out || count < 0 || n_batches < 0 || (n_batches > 0 && !batch_sizes) ||
      (count > 0 && (!wav || !wav_off || !n)))
    return fail(ZASR_ERR_INVALID, "null argument");
  *out = nullptr;
  long total = 0;
  for (int32_t i = 0; i < n_batches; ++i) {
    if (batch_sizes[i] < 0) return fail(ZASR_ERR_INVALID, "negative batch size");
    total += batch_sizes[i];
  }
  if (total != count) return fail(ZASR_ERR_INVALID, "batch sizes must sum to count");
  for (int32_t i = 0; i < count; ++i)
    if (wav_off[i] < 0 || n[i] < 0) return fail(ZASR_ERR_INVALID, "negative offset or length");
  return guarded([&]() {
    Engine* e = h->eng.get();
    std::lock_guard<std::mutex> lk(e->mu);
    std::vector<long> off(wav_off, wav_off + count), len(n, n + count);
    std::vector<int> bs(batch_sizes, batch_sizes + n_batches);
    auto r = std::make_unique<zasr_result>();
    r->items = e->decode_host_batches(wav, off, len, bs, resolve_beam(h, beam),
                                      reinterpret_cast<hipStream_t>(stream));
    *out = r.release();
    return (int)ZASR_OK;
  });
}

int zasr_encode_features(zasr_recognizer* h, const float* const* feats, const int64_t* n_frames,
                         int32_t count, float* out, int64_t cap, int64_t* t_out) {
  if (!h || !feats || !n_frames || !out || !t_out || count <= 0) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    Engine* e = h->eng.get();
    std::lock_guard<std::mutex> lk(e->mu);
    std::vector<const float*> f(feats, feats + count);
    std::vector<long> fr(n_frames, n_frames + count);
    long need = 0;
    for (int i = 0; i < count; ++i) {
      if (n_frames[i] < 9) return fail(ZASR_ERR_INVALID, "chunk shorter than 9 fbank frames");
      need += ((n_frames[i] - 7) / 2 + 1) / 2;
    }
    if (need * e->joiner_dim() > cap) return fail(ZASR_ERR_INVALID, "output buffer too small");
    std::vector<float> enc;
    std::vector<int> to;
    e->encode_host(f, fr, enc, to);
    std::memcpy(out, enc.data(), enc.size() * sizeof(float));
    for (int i = 0; i < count; ++i) t_out[i] = to[i];
    return (int)ZASR_OK;
  });
}

int zasr_search_encoder_out(zasr_recognizer* h, const float* const* enc, const int64_t* t_out,
                            int32_t count, int32_t beam, zasr_result** out) {
  if (!h || !enc || !t_out || !out || count < 0) return fail(ZASR_ERR_INVALID, "null argument");
  *out = nullptr;
  return guarded([&]() {
    Engine* e = h->eng.get();
    std::lock_guard<std::mutex> lk(e->mu);
    std::vector<const float*> p(enc, enc + count);
    std::vector<long> t(t_out, t_out + count);
    auto r = std::make_unique<zasr_result>();
    r->items = e->search_host(p, t, resolve_beam(h, beam));
    *out = r.release();
    return (int)ZASR_OK;
  });
}

int32_t zasr_result_count(const zasr_result* r) { return r ? (int32_t)r->items.size() : 0; }
static const TokenResult* item(const zasr_result* r, int32_t i) {
  return (r && i >= 0 && i < (int32_t)r->items.size()) ? &r->items[i] : nullptr;
}
int32_t zasr_result_num_tokens(const zasr_result* r, int32_t i) {
  auto* t = item(r, i);
  return t ? (int32_t)t->tok.size() : 0;
}
int32_t zasr_result_num_frames(const zasr_result* r, int32_t i) {
  auto* t = item(r, i);
  return t ? t->t_out : 0;
}
const int32_t* zasr_result_tokens(const zasr_result* r, int32_t i) {
  auto* t = item(r, i);
  return t ? t->tok.data() : nullptr;
}
const int32_t* zasr_result_frames(const zasr_result* r, int32_t i) {
  auto* t = item(r, i);
  return t ? t->frame.data() : nullptr;
}
const double* zasr_result_log_probs(const zasr_result* r, int32_t i) {
  auto* t = item(r, i);
  return t ? t->lp.data() : nullptr;
}
const float* zasr_result_token_stats(const zasr_result* r, int32_t i) {
  auto* t = item(r, i);
  return t ? t->stats.data() : nullptr;
}
void zasr_result_free(zasr_result* r) { delete r; }

int32_t zasr_vocab_size(const zasr_recognizer* h) { return h ? h->eng->vocab() : 0; }
int32_t zasr_joiner_dim(const zasr_recognizer* h) { return h ? h->eng->joiner_dim() : 0; }

int zasr_profile_enable(zasr_recognizer* h, int32_t on) {
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  if (on < 0 || on > 2) return fail(ZASR_ERR_INVALID, "profile mode must be 0, 1 or 2");
  h->eng->profile_enable((int)on);
  return ZASR_OK;
}
int zasr_profile_reset(zasr_recognizer* h) {
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  return guarded([&]() {
    h->eng->profile_reset();
    return (int)ZASR_OK;
  });
}
int zasr_profile_report(zasr_recognizer* h, char* buf, int64_t cap) {
  if (!h || !buf || cap <= 0) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    std::string s = h->eng->profile_report();
    if ((int64_t)s.size() + 1 > cap) return fail(ZASR_ERR_INVALID, "report buffer too small");
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return (int)ZASR_OK;
  });
}

int zasr_model_routes(zasr_recognizer* h, char* buf, int64_t cap) {
  if (!h || !buf || cap <= 0) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    const std::string s = h->eng->routes_json();
    if ((int64_t)s.size() + 1 > cap) return fail(ZASR_ERR_INVALID, "routes buffer too small");
    std::memcpy(buf, s.c_str(), s.size() + 1);
    return (int)ZASR_OK;
  });
}

int zasr_fbank_set_mel_banks(zasr_recognizer* h, const float* banks, int32_t n_bins) {
  if (!h || !banks) return fail(ZASR_ERR_INVALID, "null argument");
  if (n_bins != 256 && n_bins != 257) return fail(ZASR_ERR_INVALID, "n_bins must be 256 or 257");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->set_mel_banks(banks, n_bins);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_launch(int32_t block_threads) {
  if (block_threads <= 0) return fail(ZASR_ERR_INVALID, "block_threads must be positive");
  return guarded([&]() {
    zasr::launch_selftest_noop(block_threads);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_gemm_h3r(int32_t M, int32_t K, int32_t N, int32_t epi, const float* A,
                           const float* W, const float* bias, float* C) {
  if (!A || !W || !C) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_gemm_h3r(M, K, N, epi, A, W, bias, C);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_gemm(int32_t mode, int32_t M, int32_t K, int32_t N, int32_t epi, int32_t a_bf16,
                       int32_t c_bf16, const float* A, const float* W, const float* bias,
                       const float* aux, const float* byp_orig, const float* byp_scale, float* C) {
  if (!A || !W || !C) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_gemm(mode, M, K, N, epi, a_bf16 != 0, c_bf16 != 0, A, W, bias, aux, byp_orig,
                        byp_scale, C);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_conv_gemm(int32_t mode, int32_t which, int32_t a_bf16, int32_t c_bf16,
                            int32_t nseq, const int32_t* T, const float* A, const float* W,
                            const float* bias, float* C) {
  if (!T || !A || !W || !bias || !C) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_conv_gemm(mode, which, a_bf16 != 0, c_bf16 != 0, nseq, T, A, W, bias, C);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_gemm_aload(int32_t aload, int32_t M, int32_t K, int32_t N, int32_t lda,
                             int32_t ldc, int32_t c_col, int32_t epi, const float* A,
                             const float* W, const float* bias, const float* a_scale,
                             const float* a_shift, int32_t Tin, int32_t Tout, int32_t C_in,
                             int32_t stride, int32_t dil, int32_t pad, const float* aux,
                             int32_t ldaux, float* C) {
  if (!A || !W || !C) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_gemm_aload(aload, M, K, N, lda, ldc, c_col, epi, A, W, bias, a_scale, a_shift,
                              Tin, Tout, C_in, stride, dil, pad, aux, ldaux, C);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_campp_conv2d(int32_t ks, int32_t ci, int32_t fi, int32_t sf, int32_t T, int32_t n,
                               int32_t relu, int32_t tdnn_out, int32_t in_tf, int32_t use_mfma,
                               int32_t rb, const float* x, const float* w, const float* scale,
                               const float* shift, const float* res, float* y, int32_t* route,
                               int32_t* rb_used) {
  if (!x || !w || !scale || !shift || !y || !route || !rb_used)
    return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_campp_conv2d(ks, ci, fi, sf, T, n, relu, tdnn_out, in_tf, use_mfma, rb, x, w,
                                scale, shift, res, y, route, rb_used);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_campp_cam_mask(int32_t n, int32_t T, int32_t seg_len, const float* h,
                                 const float* w1, const float* b1, const float* w2,
                                 const float* b2, float* mexp) {
  if (!h || !w1 || !b1 || !w2 || !b2 || !mexp) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_campp_cam_mask(n, T, seg_len, h, w1, b1, w2, b2, mexp);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_campp_stats(int32_t N, int32_t T, int32_t C, const float* x, const float* s,
                              const float* b, float* out) {
  if (!x || !s || !b || !out) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_campp_stats(N, T, C, x, s, b, out);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_campp_cmvn(int32_t nseq, int32_t rows, const int32_t* fr_off, float* x) {
  if (!fr_off || !x) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_campp_cmvn(nseq, rows, fr_off, x);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_campp_gather(int32_t nwin, int32_t wf, int32_t nrows, const float* rows,
                               const int32_t* win_row, const int32_t* win_n, float* out) {
  if (!rows || !win_row || !win_n || !out) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_campp_gather(nwin, wf, nrows, rows, win_row, win_n, out);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_vad_frames(int32_t n_files, int64_t n_windows, int64_t n_samples,
                             const float* audio, const int64_t* off, const int64_t* win_start,
                             const int64_t* len, const float* rows576, uint32_t* maxabs,
                             float* frames) {
  if (!frames) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_vad_frames(n_files, n_windows, n_samples, audio, off, win_start, len, rows576,
                              maxabs, frames);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_vad_im2col(int32_t which, int64_t N, int32_t T, int32_t C, int32_t stride,
                             int32_t ldS, int32_t Kp, const float* in, float* A) {
  if (!in || !A) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_vad_im2col(which, N, T, C, stride, ldS, Kp, in, A);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_vad_lstm(int64_t windows, int32_t nseg, const float* gx, const float* whh,
                           const float* bhh, const float* wd, float bd, const int64_t* seg_start,
                           const int32_t* seg_count, const int32_t* seg_warm, const float* init,
                           float* probs, float* s_out, float* e_out) {
  if (!gx || !whh || !bhh || !wd || !seg_start || !seg_count || !probs)
    return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_vad_lstm(windows, nseg, gx, whh, bhh, wd, bd, seg_start, seg_count, seg_warm,
                            init, probs, s_out, e_out);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_vibert_ln(int64_t rows, int32_t H, int32_t L, const int64_t* ids,
                            const int64_t* tt, int32_t V, int32_t P, int32_t TT, const float* word,
                            const float* pos, const float* type, const float* g, const float* b,
                            float eps, float* x) {
  if (!g || !b || !x) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_vibert_ln(rows, H, L, ids, tt, V, P, TT, word, pos, type, g, b, eps, x);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_vibert_attn(int32_t B, int32_t L, int32_t heads, int32_t H, const float* qkv,
                              const int64_t* mask, float* ctx) {
  if (!qkv || !mask || !ctx) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_vibert_attn(B, L, heads, H, qkv, mask, ctx);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_vibert_gather(int32_t B, int32_t L, int32_t W, int32_t H, const float* x,
                                const int64_t* offsets, float* g) {
  if (!x || !offsets || !g) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_vibert_gather(B, L, W, H, x, offsets, g);
    return (int)ZASR_OK;
  });
}

// ---- the PyanNet and Conv-TasNet kernels alone ----
int zasr_selftest_seg_chunk_stats(int64_t total, int32_t n, int32_t T, const float* audio,
                                  const int64_t* starts, float* stats) {
  if (!audio || !starts || !stats) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_seg_chunk_stats(total, n, T, audio, reinterpret_cast<const long*>(starts), stats);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_seg_front(int64_t total, int32_t n, int32_t T, const float* audio,
                            const int64_t* starts, const float* stats, float in_w, float in_b,
                            const float* w0t, float* out) {
  if (!audio || !starts || !stats || !w0t || !out) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_seg_front(total, n, T, audio, reinterpret_cast<const long*>(starts), stats, in_w,
                             in_b, w0t, out);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_seg_pool3(int32_t n, int32_t L, int32_t C, int32_t Fp, int32_t max_blocks,
                            const float* x, float* out) {
  if (!x || !out) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_seg_pool3(n, L, C, Fp, max_blocks, x, out);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_seg_frame_stats(int32_t n, int32_t F, int32_t C, const float* x, float* stats) {
  if (!x || !stats) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_seg_frame_stats(n, F, C, x, stats);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_seg_norm_act(int32_t n, int32_t F, int32_t C, int32_t max_blocks,
                               const float* stats, const float* w, const float* b, float* x) {
  if (!stats || !w || !b || !x) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_seg_norm_act(n, F, C, max_blocks, stats, w, b, x);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_seg_lstm(int32_t n, int32_t F, int32_t group, const float* gx, const float* whh,
                           float* out) {
  if (!gx || !whh || !out) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_seg_lstm(n, F, group, gx, whh, out);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_seg_head(int64_t rows, const float* x, const float* w, const float* b,
                           float* logits, uint8_t* classes) {
  if (!x || !w || !b || !logits || !classes) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_seg_head(rows, x, w, b, logits, classes);
    return (int)ZASR_OK;
  });
}

namespace {
zasr::SepSelftestCall sep_call(const zasr_sep_call* c) {
  return zasr::SepSelftestCall{c->n_regions, reinterpret_cast<const long*>(c->sig_off), c->T, c->r0,
                               c->ng, c->win, c->hop};
}
bool sep_call_ok(const zasr_sep_call* c) { return c && c->sig_off && c->T; }
}  // namespace

int zasr_selftest_sep_frames(const zasr_sep_call* call, int64_t n_signal, const float* signal,
                             float* frames) {
  if (!sep_call_ok(call) || !signal || !frames) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_sep_frames(sep_call(call), n_signal, signal, frames);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_sep_tile_sums(const zasr_sep_call* call, int32_t C, const float* x,
                                double* partial) {
  if (!sep_call_ok(call) || !x || !partial) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_sep_tile_sums(sep_call(call), C, x, partial);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_sep_region_stats(const zasr_sep_call* call, int32_t C, const double* partial,
                                   float* stats) {
  if (!sep_call_ok(call) || !partial || !stats) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_sep_region_stats(sep_call(call), C, partial, stats);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_sep_gln_apply(const zasr_sep_call* call, int32_t C, int32_t in_place,
                                const float* stats, const float* gamma, const float* beta,
                                const float* src, float* dst) {
  if (!sep_call_ok(call) || !stats || !gamma || !beta || !dst || (!in_place && !src))
    return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_sep_gln_apply(sep_call(call), C, in_place, stats, gamma, beta, src, dst);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_sep_mid(const zasr_sep_call* call, int32_t C, int32_t dil, float slope,
                          const float* stats, const float* gamma, const float* beta, const float* w,
                          const float* bias, const float* h, float* y, double* partial) {
  if (!sep_call_ok(call) || !stats || !gamma || !beta || !w || !bias || !h || !y || !partial)
    return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_sep_mid(sep_call(call), C, dil, slope, stats, gamma, beta, w, bias, h, y, partial);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_sep_prelu(int64_t rows, int32_t C, int32_t ld, int32_t col0, float slope,
                            int32_t max_blocks, float* x) {
  if (!x) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_sep_prelu(rows, C, ld, col0, slope, max_blocks, x);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_sep_overlap_add(const zasr_sep_call* call, const int64_t* out_off, int64_t n_out,
                                  const float* dec0, const float* dec1, float* out) {
  if (!sep_call_ok(call) || !out_off || !dec0 || !dec1 || !out)
    return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_sep_overlap_add(sep_call(call), reinterpret_cast<const long*>(out_off), n_out, dec0,
                                   dec1, out);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_joiner(int32_t mode, int32_t layout, int32_t M, int32_t V, int32_t D,
                         const float* J, const float* W, const float* bias,
                         const int32_t* live_t, const int32_t* live_len, int32_t live_f,
                         float* out) {
  if (!J || !W || !bias || !out) return fail(ZASR_ERR_INVALID, "null argument");
  if (M < 1 || V < 1) return fail(ZASR_ERR_INVALID, "M and V must be positive");
  if ((live_t == nullptr) != (live_len == nullptr) || (live_t != nullptr && live_f < 1))
    return fail(ZASR_ERR_INVALID, "the live filter takes live_t, live_len and live_f >= 1");
  const bool split = mode == ZASR_PRECISION_BF16X3 || mode == ZASR_PRECISION_BF16X6 ||
                     mode == ZASR_PRECISION_F16X3;
  const bool ok0 = layout == 0 && (mode == ZASR_PRECISION_FP32 || mode == ZASR_PRECISION_BF16 || split) &&
                   (D == 64 || D == 128 || D == 256 || D == 512);
  const bool ok1 = layout == 1 && (mode == ZASR_PRECISION_BF16 || split) && (D == 256 || D == 512);
  if (!ok0 && !ok1) return fail(ZASR_ERR_INVALID, "unsupported joiner mode / layout / dim");
  return guarded([&]() {
    zasr::selftest_joiner(mode, layout, M, V, D, J, W, bias, live_t, live_len, live_f, out);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_attn_weights(int32_t mode, int32_t H, int32_t nseq, const int32_t* L,
                               int32_t pmax, const float* qkp, const float* pos_tab, float* A0) {
  if (!L || !qkp || !pos_tab || !A0) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_attn_weights(mode, H, nseq, L, pmax, qkp, pos_tab, A0);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_attn_sa(int32_t mode, int32_t H, int32_t nseq, const int32_t* L, int32_t pmax,
                          const float* qkp, const float* pos_tab, const float* v1,
                          const float* v2, float* out1, float* stats, float* out2) {
  if (!L || !qkp || !pos_tab || !v1 || !v2 || !out1 || !stats || !out2)
    return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_attn_sa(mode, H, nseq, L, pmax, qkp, pos_tab, v1, v2, out1, stats, out2);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_nonlin(int32_t mode, int32_t H, int32_t nseq, const int32_t* L, int32_t pmax,
                         int32_t hid, const float* qkp, const float* pos_tab, const float* h3,
                         uint16_t* t1t, float* z) {
  if (!L || !qkp || !pos_tab || !h3 || !t1t) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_nonlin(mode, H, nseq, L, pmax, hid, qkp, pos_tab, h3, t1t, z);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_search_step(int32_t V, int32_t beam, int32_t t, const int32_t* enc_len,
                              const zasr_st_state* st, const float* logits,
                              const zasr_st_hotwords* hw, const zasr_st_table* tab) {
  if (!enc_len || !st || !hw || (t >= 0 && !logits)) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_search_step(V, beam, t, enc_len, *st, logits, *hw, tab);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_greedy_spec(int32_t V, int32_t F, int32_t init, int32_t parity,
                              const int32_t* enc_len, int32_t* t_cur, int32_t* active,
                              const zasr_st_state* st, const float* logits,
                              const zasr_st_hotwords* hw, const zasr_st_table* tab) {
  if (!enc_len || !t_cur || !active || !st || !hw || !tab)
    return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_greedy_spec(V, F, init, parity, enc_len, t_cur, active, *st, logits, *hw, *tab);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_search_final(int32_t V, const zasr_st_state* st, const zasr_st_hotwords* hw,
                               int32_t out_cap, int32_t* out_tok, int32_t* out_frame,
                               double* out_lp, float* out_stats, int32_t* out_count) {
  if (!st || !hw || !out_tok || !out_frame || !out_lp || !out_stats || !out_count)
    return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_search_final(V, *st, *hw, out_cap, out_tok, out_frame, out_lp, out_stats,
                                out_count);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_hotword_dfa(int32_t V, const zasr_st_hotwords* hw, int32_t cap,
                              int32_t* num_states, int32_t* num_cls, int32_t* tok2cls,
                              int32_t* next, double* delta, double* node_score) {
  if (!hw || !num_states || !num_cls || !tok2cls || !next || !delta || !node_score)
    return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_hotword_dfa(V, *hw, cap, num_states, num_cls, tok2cls, next, delta, node_score);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_ffn_h3(int32_t R, int32_t D, int32_t F, const float* Y, const float* W1,
                         const float* b1, const float* W2, const float* b2,
                         const float* byp_orig, const float* byp_scale, float* X) {
  if (!Y || !W1 || !b1 || !W2 || !b2 || !X) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_ffn_h3(R, D, F, Y, W1, b1, W2, b2, byp_orig, byp_scale, X);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_ffn_bf16(int32_t R, int32_t D, int32_t F, const float* W1, const float* b1,
                           const float* W2, const float* b2, const float* byp_orig,
                           const float* byp_scale, float* X, int32_t form) {
  if (!W1 || !b1 || !W2 || !b2 || !X) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_ffn_bf16(R, D, F, W1, b1, W2, b2, byp_orig, byp_scale, X, form);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_ffn_bf16_oop(int32_t R, int32_t D, int32_t F, const float* W1, const float* b1,
                               const float* W2, const float* b2, const float* byp_orig,
                               const float* byp_scale, float* X, float* Xout, int32_t form) {
  if (!W1 || !b1 || !W2 || !b2 || !X || !Xout) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_ffn_bf16(R, D, F, W1, b1, W2, b2, byp_orig, byp_scale, X, form, Xout);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_ffn_h3_oop(int32_t R, int32_t D, int32_t F, const float* W1, const float* b1,
                             const float* W2, const float* b2, const float* byp_orig,
                             const float* byp_scale, float* X, float* Xout) {
  if (!W1 || !b1 || !W2 || !b2 || !X || !Xout) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_ffn_h3(R, D, F, nullptr, W1, b1, W2, b2, byp_orig, byp_scale, X, Xout);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_seam(int32_t nseq, const int32_t* L, int32_t d, int32_t ds, int32_t dn,
                       int32_t ds_next, int32_t c0, int32_t ldo, const float* xd,
                       const float* orig, const float* s, const float* wn8, const float* wo2,
                       float* next, float* xnext, float* out, float* next_ref, float* xnext_ref,
                       float* out_ref) {
  if (!L || !orig || !wn8 || !wo2 || !next || !xnext || !out || !next_ref || !xnext_ref ||
      !out_ref || (ds > 1 && (!xd || !s)))
    return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_seam(nseq, L, d, ds, dn, ds_next, c0, ldo, xd, orig, s, wn8, wo2, next, xnext,
                        out, next_ref, xnext_ref, out_ref);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_dwconv1d(int32_t nseq, const int32_t* L, int32_t d, int32_t K, int32_t glu,
                           int32_t bf16, const float* x, const float* w, const float* b,
                           float* out) {
  if (!L || !x || !w || !b || !out) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_dwconv1d(nseq, L, d, K, glu != 0, bf16 != 0, x, w, b, out);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_conv1(int32_t nseq, const int32_t* T, int32_t form, const float* fb,
                        const float* w, const float* b, float* out) {
  if (!T || !fb || !w || !b || !out) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_conv1(nseq, T, form, fb, w, b, out);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_convnext(int32_t nseq, const int32_t* L, int32_t form, const float* x,
                           const float* dw_w, const float* dw_b, const float* w1, const float* b1,
                           const float* w2, const float* b2, float* y, float* out) {
  if (!L || !x || !dw_w || !dw_b || !y) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_convnext(nseq, L, form, x, dw_w, dw_b, w1, b1, w2, b2, y, out);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_bias_norm(int32_t rows, int32_t d, const float* bias, float log_scale,
                            float* orig, const float* bscale, int32_t copy_mode, float* x,
                            float* copy_out) {
  if (!bias || !x) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::selftest_bias_norm(rows, d, bias, log_scale, orig, bscale, copy_mode, x, copy_out);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_attn_block_map(const int32_t* lens, int32_t nseq, int32_t units_per_seq,
                                 int32_t order, uint32_t* out, int64_t cap, int32_t* grid) {
  if (!lens || !grid || (cap > 0 && !out) || cap < 0) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    std::vector<unsigned> map;
    *grid = zasr::build_attn_block_map(lens, nseq, units_per_seq, order, map);
    if ((int64_t)map.size() > cap) return fail(ZASR_ERR_INVALID, "block map buffer too small");
    std::copy(map.begin(), map.end(), out);
    return (int)ZASR_OK;
  });
}

int zasr_silence_flags(const float* d_wav, int64_t n, int32_t frame_len, float threshold,
                       uint8_t* d_flags, void* stream) {
  if (n < 0 || (n > 0 && (!d_wav || !d_flags))) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    zasr::launch_silence_flags(d_wav, (long)n, (int)frame_len, threshold, d_flags,
                               reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

// ---- device audio front end (audio.h) ----
namespace {
int audio_source_error(int32_t format, int32_t channels, int32_t rate) {
  if (format != ZASR_AUDIO_F32 && format != ZASR_AUDIO_I16)
    return fail(ZASR_ERR_INVALID, "format must be ZASR_AUDIO_F32 or ZASR_AUDIO_I16");
  if (channels < 1 || channels > zasr::kAudioMaxChannels)
    return fail(ZASR_ERR_INVALID, "channels must be in 1..8");
  if (rate < zasr::kAudioMinRate || rate > zasr::kAudioMaxRate)
    return fail(ZASR_ERR_INVALID, "sample rate must be in 4000..384000");
  return ZASR_OK;
}
}  // namespace

int zasr_audio_create(int32_t device_id, zasr_audio** out) {
  if (!out) return fail(ZASR_ERR_INVALID, "null out");
  *out = nullptr;
  return guarded([&]() {
    auto* h = new zasr_audio;
    try {
      h->eng.reset(new zasr::AudioFrontEnd(device_id));
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
    return (int)ZASR_OK;
  });
}

void zasr_audio_destroy(zasr_audio* h) { delete h; }

int64_t zasr_audio_out_len(int32_t rate, int64_t n_frames) {
  if (rate < zasr::kAudioMinRate || rate > zasr::kAudioMaxRate || n_frames < 0 ||
      n_frames > (int64_t(1) << 40)) {
    fail(ZASR_ERR_INVALID, "sample rate must be in 4000..384000 and n_frames in 0..2^40");
    return -1;
  }
  return zasr::audio_out_len(rate, (long)n_frames);
}

int zasr_audio_resample_taps(int32_t rate, int32_t* P, int32_t* Q, int32_t* taps,
                             int32_t* out_tile, int32_t* in_tile, int32_t* lo, float* w,
                             int64_t cap) {
  if (!P || !Q || !taps) return fail(ZASR_ERR_INVALID, "null argument");
  if (rate < zasr::kAudioMinRate || rate > zasr::kAudioMaxRate)
    return fail(ZASR_ERR_INVALID, "sample rate must be in 4000..384000");
  return guarded([&]() {
    const zasr::ResampleTable t = zasr::make_resample_table(rate);
    *P = t.P;
    *Q = t.Q;
    *taps = t.taps;
    if (out_tile) *out_tile = t.out_tile;
    if (in_tile) *in_tile = t.in_tile();
    if (lo || w) {
      if (cap < (int64_t)t.w.size() || !lo || !w)
        return fail(ZASR_ERR_INVALID, "table buffers too small (lo [P], w [P * taps] = cap)");
      std::memcpy(lo, t.lo.data(), t.lo.size() * sizeof(int32_t));
      std::memcpy(w, t.w.data(), t.w.size() * sizeof(float));
    }
    return (int)ZASR_OK;
  });
}

int zasr_audio_to_16k(zasr_audio* h, const void* src, int32_t format, int32_t channels,
                      int32_t rate, int64_t n_frames, int32_t src_on_device, float* d_out,
                      int64_t cap, int64_t* n_out, void* stream) {
  if (const int rc = audio_source_error(format, channels, rate)) return rc;
  if (!h || !n_out || n_frames < 0 || (n_frames > 0 && (!src || !d_out)))
    return fail(ZASR_ERR_INVALID, "null argument");
  if (n_frames > (int64_t(1) << 40)) return fail(ZASR_ERR_INVALID, "n_frames too large");
  if (zasr::audio_out_len(rate, (long)n_frames) > cap)
    return fail(ZASR_ERR_INVALID, "output buffer too small (zasr_audio_out_len samples needed)");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    *n_out = h->eng->to_16k(src, format, channels, rate, (long)n_frames, src_on_device != 0, d_out,
                            (long)cap, reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

int zasr_audio_peak(zasr_audio* h, const float* d_wav, int64_t n, float* peak, void* stream) {
  if (!h || !peak || n < 0 || (n > 0 && !d_wav)) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    *peak = h->eng->peak(d_wav, (long)n, reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

int zasr_audio_scale(zasr_audio* h, float* d_wav, int64_t n, float divisor, float multiplier,
                     void* stream) {
  if (!h || n < 0 || (n > 0 && !d_wav)) return fail(ZASR_ERR_INVALID, "null argument");
  if (!(divisor != 0.f)) return fail(ZASR_ERR_INVALID, "divisor must not be 0");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->scale(d_wav, (long)n, divisor, multiplier, reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

int zasr_audio_segment_sumsq(zasr_audio* h, const float* d_wav, int64_t n,
                             const int64_t* seg_begin, const int64_t* seg_end, int32_t n_seg,
                             double* out, void* stream) {
  if (!h || n < 0 || n_seg < 0 || (n_seg > 0 && (!seg_begin || !seg_end || !out)) ||
      (n > 0 && !d_wav))
    return fail(ZASR_ERR_INVALID, "null argument");
  for (int32_t s = 0; s < n_seg; ++s)
    if (seg_begin[s] < 0 || seg_end[s] < seg_begin[s] || seg_end[s] > n)
      return fail(ZASR_ERR_INVALID, "segment outside the signal");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->segment_sumsq(d_wav, reinterpret_cast<const long*>(seg_begin),
                          reinterpret_cast<const long*>(seg_end), n_seg, out,
                          reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

int zasr_audio_apply_gain(zasr_audio* h, float* d_wav, int64_t n, const int64_t* piece_begin,
                          const int64_t* piece_end, const float* piece_gain,
                          const int64_t* piece_ramp, int32_t n_pieces, const float* ramp_values,
                          int64_t n_ramp_values, float* peak, void* stream) {
  if (!h || !peak || n < 0 || n_pieces < 0 || n_ramp_values < 0 || (n > 0 && !d_wav) ||
      (n_pieces > 0 && (!piece_begin || !piece_end || !piece_gain || !piece_ramp)) ||
      (n_ramp_values > 0 && !ramp_values))
    return fail(ZASR_ERR_INVALID, "null argument");
  int64_t prev = 0;
  for (int32_t k = 0; k < n_pieces; ++k) {
    if (piece_begin[k] < prev || piece_end[k] <= piece_begin[k] || piece_end[k] > n)
      return fail(ZASR_ERR_INVALID, "pieces must be non-empty, ascending, disjoint and inside the signal");
    if (piece_ramp[k] >= 0 && piece_ramp[k] + (piece_end[k] - piece_begin[k]) > n_ramp_values)
      return fail(ZASR_ERR_INVALID, "ramp piece reaches past ramp_values");
    prev = piece_end[k];
  }
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    *peak = h->eng->apply_gain(d_wav, (long)n, reinterpret_cast<const long*>(piece_begin),
                               reinterpret_cast<const long*>(piece_end), piece_gain,
                               reinterpret_cast<const long*>(piece_ramp), n_pieces, ramp_values,
                               (long)n_ramp_values, reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

// ---- WPE dereverberation (wpe.h; core/audio_preprocessing.py:157-216) ----
namespace {
int wpe_args_error(int64_t total, const int64_t* offsets, const int64_t* lens, int32_t count,
                   int32_t taps, int32_t delay, int32_t iterations, const int64_t* out_offsets) {
  if (count < 0 || total < 0 || (count > 0 && (!offsets || !lens || !out_offsets)))
    return fail(ZASR_ERR_INVALID, "null argument");
  if (taps < 1 || taps > zasr::kWpeMaxTaps) return fail(ZASR_ERR_INVALID, "WPE: taps must be in 1..16");
  if (delay < 1 || delay > zasr::kWpeMaxDelay)
    return fail(ZASR_ERR_INVALID, "WPE: delay must be in 1..16");
  if (iterations < 1 || iterations > zasr::kWpeMaxIters)
    return fail(ZASR_ERR_INVALID, "WPE: iterations must be in 1..8");
  for (int32_t c = 0; c < count; ++c) {
    if (lens[c] < 0 || offsets[c] < 0 || lens[c] > total || offsets[c] > total - lens[c])
      return fail(ZASR_ERR_INVALID, "WPE: chunk outside the signal");
    if (lens[c] > zasr::kWpeMaxSamples)
      return fail(ZASR_ERR_INVALID, "WPE: a chunk is at most 60 s (960000 samples)");
    if (out_offsets[c] < 0) return fail(ZASR_ERR_INVALID, "WPE: negative output offset");
  }
  return ZASR_OK;
}
}  // namespace

int zasr_wpe_create(int32_t device_id, zasr_wpe** out) {
  if (!out) return fail(ZASR_ERR_INVALID, "null out");
  *out = nullptr;
  return guarded([&]() {
    auto* h = new zasr_wpe;
    try {
      h->eng.reset(new zasr::WpeEngine(device_id));
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
    return (int)ZASR_OK;
  });
}

void zasr_wpe_destroy(zasr_wpe* h) { delete h; }

int64_t zasr_wpe_frames(int64_t n) {  // :195, nara-wpe's stft with fading
  if (n < 0 || n > zasr::kWpeMaxSamples) {
    fail(ZASR_ERR_INVALID, "WPE: n must be in 0..960000");
    return -1;
  }
  return zasr::wpe_frames((long)n);
}

int zasr_wpe_run_device(zasr_wpe* h, const float* d_audio, int64_t total, const int64_t* offsets,
                        const int64_t* lens, int32_t count, int32_t taps, int32_t delay,
                        int32_t iterations, float* d_out, const int64_t* out_offsets, void* stream) {
  if (!h || (count > 0 && (!d_audio || !d_out))) return fail(ZASR_ERR_INVALID, "null argument");
  if (const int rc = wpe_args_error(total, offsets, lens, count, taps, delay, iterations, out_offsets))
    return rc;
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->run_device(d_audio, (long)total, reinterpret_cast<const long*>(offsets),
                       reinterpret_cast<const long*>(lens), count, taps, delay, iterations, d_out,
                       reinterpret_cast<const long*>(out_offsets),
                       reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

int zasr_wpe_run(zasr_wpe* h, const float* audio, int64_t total, const int64_t* offsets,
                 const int64_t* lens, int32_t count, int32_t taps, int32_t delay,
                 int32_t iterations, float* out, const int64_t* out_offsets) {
  if (!h || (count > 0 && (!audio || !out))) return fail(ZASR_ERR_INVALID, "null argument");
  if (const int rc = wpe_args_error(total, offsets, lens, count, taps, delay, iterations, out_offsets))
    return rc;
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->run_host(audio, (long)total, reinterpret_cast<const long*>(offsets),
                     reinterpret_cast<const long*>(lens), count, taps, delay, iterations, out,
                     reinterpret_cast<const long*>(out_offsets));
    return (int)ZASR_OK;
  });
}

int zasr_wpe_set_budget(zasr_wpe* h, int64_t bytes) {
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  if (bytes <= 0) return fail(ZASR_ERR_INVALID, "WPE: the budget must be positive");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  h->eng->set_budget((size_t)bytes);
  return ZASR_OK;
}

int32_t zasr_wpe_last_groups(const zasr_wpe* h) { return h ? h->eng->last_groups() : 0; }

int zasr_wpe_trim(zasr_wpe* h) {
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->trim();
    return (int)ZASR_OK;
  });
}

int zasr_wpe_set_profile(zasr_wpe* h, int32_t on) {
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  h->eng->set_profile(on != 0);
  return ZASR_OK;
}

int zasr_wpe_stage_ms(zasr_wpe* h, float* ms3) {
  if (!h || !ms3) return fail(ZASR_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  std::memcpy(ms3, h->eng->stage_ms(), sizeof(float) * zasr::WpeEngine::kStages);
  return ZASR_OK;
}

int zasr_selftest_wpe_stft(zasr_wpe* h, const float* signal, int64_t n, float* Y, float* max_sq) {
  if (!h || !signal || !Y || !max_sq) return fail(ZASR_ERR_INVALID, "null argument");
  if (n < 1 || n > zasr::kWpeMaxSamples) return fail(ZASR_ERR_INVALID, "WPE: n must be in 1..960000");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->selftest_stft(signal, (long)n, Y, max_sq);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_wpe_iter(zasr_wpe* h, const float* Y, int32_t T, int32_t taps, int32_t delay,
                           float max_sq, const double* g_prev, double* g, float* X,
                           float* next_max_sq) {
  if (!h || !Y || !g) return fail(ZASR_ERR_INVALID, "null argument");
  if (T < 1 || T > zasr::wpe_frames(zasr::kWpeMaxSamples))
    return fail(ZASR_ERR_INVALID, "WPE: T out of range");
  if (taps < 1 || taps > zasr::kWpeMaxTaps || delay < 1 || delay > zasr::kWpeMaxDelay)
    return fail(ZASR_ERR_INVALID, "WPE: taps and delay must be in 1..16");
  if (!(max_sq >= 0.f)) return fail(ZASR_ERR_INVALID, "WPE: max_sq must not be negative");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->selftest_iter(Y, T, taps, delay, max_sq, g_prev, g, X, next_max_sq);
    return (int)ZASR_OK;
  });
}

int zasr_selftest_wpe_istft(zasr_wpe* h, const float* X, int32_t T, int64_t n, float* out) {
  if (!h || !X || !out) return fail(ZASR_ERR_INVALID, "null argument");
  if (n < 1 || n > zasr::kWpeMaxSamples || T != zasr::wpe_frames((long)n))
    return fail(ZASR_ERR_INVALID, "WPE: T must be zasr_wpe_frames(n), n in 1..960000");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->selftest_istft(X, T, (long)n, out);
    return (int)ZASR_OK;
  });
}

// ---- speaker diarization: spectral embedding (diar.h) ----
namespace {
int diar_shape_error(int32_t N, int32_t D) {
  if (N < zasr::kDiarMinN || N > zasr::kDiarMaxN)
    return fail(ZASR_ERR_INVALID, "N must be in 2..8192 windows");
  if (D < 1 || D > zasr::kDiarMaxD) return fail(ZASR_ERR_INVALID, "D must be in 1..512");
  return ZASR_OK;
}
int diar_prune_error(double pval, int32_t min_pnum) {
  if (!(pval >= 0.0 && pval <= 1.0)) return fail(ZASR_ERR_INVALID, "pval must be in [0, 1]");
  if (min_pnum < 1) return fail(ZASR_ERR_INVALID, "min_pnum must be at least 1");
  return ZASR_OK;
}
int diar_k_error(int32_t N, int32_t k) {
  if (k < 1 || k > zasr::kDiarMaxK || k > N)
    return fail(ZASR_ERR_INVALID, "k must be in 1..min(16, N)");
  return ZASR_OK;
}
}  // namespace

int zasr_diar_create(int32_t device_id, zasr_diar** out) {
  if (!out) return fail(ZASR_ERR_INVALID, "null out");
  *out = nullptr;
  return guarded([&]() {
    auto* h = new zasr_diar;
    try {
      h->eng.reset(new zasr::DiarEngine(device_id));
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
    return (int)ZASR_OK;
  });
}

void zasr_diar_destroy(zasr_diar* h) { delete h; }

int zasr_diar_similarity(zasr_diar* h, const float* d_X, int32_t N, int32_t D, float* d_M,
                         void* stream) {
  if (const int rc = diar_shape_error(N, D)) return rc;
  if (!h || !d_X || !d_M) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->similarity(d_X, N, D, d_M, reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

int zasr_diar_prune(zasr_diar* h, float* d_M, int32_t N, double pval, int32_t min_pnum,
                    double* d_deg, void* stream) {
  if (const int rc = diar_shape_error(N, 1)) return rc;
  if (const int rc = diar_prune_error(pval, min_pnum)) return rc;
  if (!h || !d_M || !d_deg) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->prune(d_M, N, pval, min_pnum, d_deg, reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

int zasr_diar_eigs(zasr_diar* h, const float* d_M, const double* d_deg, int32_t N, int32_t k,
                   double* lambdas, double* vecs, int32_t* passes, void* stream) {
  if (const int rc = diar_shape_error(N, 1)) return rc;
  if (const int rc = diar_k_error(N, k)) return rc;
  if (!h || !d_M || !d_deg || !lambdas || !vecs) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->last_passes = h->eng->eigs(d_M, d_deg, N, k, lambdas, vecs,
                                  reinterpret_cast<hipStream_t>(stream));
    if (passes) *passes = h->last_passes;
    return (int)ZASR_OK;
  });
}

int zasr_diar_spectral_embed(zasr_diar* h, const float* X, int32_t x_on_device, int32_t N,
                             int32_t D, double pval, int32_t min_pnum, int32_t k,
                             double* lambdas, double* vecs, void* stream) {
  if (const int rc = diar_shape_error(N, D)) return rc;
  if (const int rc = diar_prune_error(pval, min_pnum)) return rc;
  if (const int rc = diar_k_error(N, k)) return rc;
  if (!h || !X || !lambdas || !vecs) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->last_passes = h->eng->spectral_embed(X, x_on_device != 0, N, D, pval, min_pnum, k, lambdas,
                                            vecs, reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

int zasr_diar_last_stats(zasr_diar* h, int32_t* passes, int64_t* applications) {
  if (!h) return fail(ZASR_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  if (passes) *passes = h->last_passes;
  if (applications) *applications = h->eng->last_applications;
  return ZASR_OK;
}

// ---- community-1 clustering: centroid AHC (:918-921) ----
int zasr_clu_create(int32_t device_id, zasr_clu** out) {
  if (!out) return fail(ZASR_ERR_INVALID, "null out");
  *out = nullptr;
  return guarded([&]() {
    auto* h = new zasr_clu;
    try {
      h->eng.reset(new zasr::CluEngine(device_id));
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
    return (int)ZASR_OK;
  });
}

void zasr_clu_destroy(zasr_clu* h) { delete h; }

int zasr_clu_ahc(zasr_clu* h, const float* X, int32_t x_on_device, int32_t N, int32_t D,
                 double threshold, int32_t* labels, void* stream) {  // :918-921
  if (N < zasr::kCluMinN || N > zasr::kCluMaxN)
    return fail(ZASR_ERR_INVALID, "N must be in 2..16384 rows");
  if (D < 1 || D > zasr::kCluMaxD) return fail(ZASR_ERR_INVALID, "D must be in 1..512");
  if (threshold != threshold) return fail(ZASR_ERR_INVALID, "threshold is NaN");
  if (!h || !X || !labels) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    std::lock_guard<std::mutex> lk(h->eng->mu);
    h->eng->ahc(X, x_on_device != 0, N, D, threshold, labels, reinterpret_cast<hipStream_t>(stream));
    return (int)ZASR_OK;
  });
}

int zasr_clu_last_stats(zasr_clu* h, int64_t* merges, int64_t* rescans) {
  if (!h) return fail(ZASR_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  if (merges) *merges = h->eng->last_merges;
  if (rescans) *rescans = h->eng->last_rescans;
  return ZASR_OK;
}

int zasr_clu_set_profile(zasr_clu* h, int32_t on) {
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  h->eng->set_profile(on != 0);
  return ZASR_OK;
}

int zasr_clu_stage_ms(zasr_clu* h, float* ms4) {
  if (!h || !ms4) return fail(ZASR_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  std::memcpy(ms4, h->eng->stage_ms(), sizeof(float) * zasr::kCluStages);
  return ZASR_OK;
}

int zasr_selftest_clu_route(zasr_clu* h, int32_t route, int32_t* n_routes) {
  if (n_routes) *n_routes = zasr::kCluRoutes;
  if (!h) return fail(ZASR_ERR_INVALID, "null handle");
  if (route < 0 || route >= zasr::kCluRoutes) return fail(ZASR_ERR_INVALID, "unknown route");
  std::lock_guard<std::mutex> lk(h->eng->mu);
  h->eng->set_route(route);
  return ZASR_OK;
}

// ---- offline streams (sherpa-onnx OfflineStream surface) ----
int zasr_set_tokens(zasr_recognizer* h, const char* tokens_path) {
  if (!h || !tokens_path) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    std::ifstream f(tokens_path);
    if (!f) return fail(ZASR_ERR_NOT_FOUND, std::string("tokens file not found: ") + tokens_path);
    std::lock_guard<std::mutex> lk(h->sym_mu);
    h->tokens_path = tokens_path;
    h->syms.reset();  // readers holding the old table keep it alive
    return (int)ZASR_OK;
  });
}

int zasr_create_stream(zasr_recognizer* h, zasr_stream** out) {
  if (!h || !out) return fail(ZASR_ERR_INVALID, "null argument");
  return guarded([&]() {
    auto* s = new zasr_stream;
    s->rec = h;
    *out = s;
    return (int)ZASR_OK;
  });
}

void zasr_destroy_stream(zasr_stream* s) { delete s; }

int zasr_stream_accept_waveform(zasr_stream* s, int32_t sample_rate, const float* samples,
                                int64_t n) {
  if (!s || n < 0 || (n > 0 && !samples)) return fail(ZASR_ERR_INVALID, "null argument");
  if (sample_rate != 16000) return fail(ZASR_ERR_INVALID, "sample rate must be 16000");
  if (s->decoded) return fail(ZASR_ERR_INVALID, "stream already decoded");
  return guarded([&]() {
    s->samples.insert(s->samples.end(), samples, samples + n);
    return (int)ZASR_OK;
  });
}

int zasr_decode_stream(zasr_recognizer* h, zasr_stream* s) {
  return zasr_decode_streams(h, &s, 1);
}

int zasr_decode_streams(zasr_recognizer* h, zasr_stream* const* ss, int32_t n) {
  if (!h || n < 0 || (n > 0 && !ss)) return fail(ZASR_ERR_INVALID, "null argument");
  for (int32_t i = 0; i < n; ++i) {
    if (!ss[i]) return fail(ZASR_ERR_INVALID, "null stream");
    if (ss[i]->rec != h) return fail(ZASR_ERR_INVALID, "stream belongs to another recognizer");
    for (int32_t j = 0; j < i; ++j)
      if (ss[j] == ss[i]) return fail(ZASR_ERR_INVALID, "stream listed twice");
  }
  return guarded([&]() {
    decode_streams_impl(h, ss, n);
    return (int)ZASR_OK;
  });
}

int32_t zasr_stream_is_decoded(const zasr_stream* s) { return s && s->decoded ? 1 : 0; }
int32_t zasr_stream_num_tokens(const zasr_stream* s) {
  return s ? (int32_t)s->res.tok.size() : 0;
}
int32_t zasr_stream_num_frames(const zasr_stream* s) { return s ? s->res.t_out : 0; }
const int32_t* zasr_stream_tokens(const zasr_stream* s) { return s ? s->res.tok.data() : nullptr; }
const int32_t* zasr_stream_frames(const zasr_stream* s) { return s ? s->res.frame.data() : nullptr; }
const double* zasr_stream_log_probs(const zasr_stream* s) { return s ? s->res.lp.data() : nullptr; }
const float* zasr_stream_token_stats(const zasr_stream* s) {
  return s ? s->res.stats.data() : nullptr;
}

int zasr_stream_result_json(const zasr_stream* s, char* buf, int64_t cap, int64_t* needed) {
  if (!s || !needed) return fail(ZASR_ERR_INVALID, "null argument");
  if (!s->decoded) return fail(ZASR_ERR_INVALID, "stream not decoded");
  return guarded([&]() {
    const std::shared_ptr<const std::vector<std::string>> tab = symbols(s->rec);
    const std::vector<std::string>& sym = *tab;
    const TokenResult& r = s->res;
    std::ostringstream os;
    std::string text;
    std::vector<std::string> toks;
    for (int t : r.tok) {
      toks.push_back(t >= 0 && t < (int)sym.size() ? sym[t] : std::string());
      text += toks.back();
    }
    os << "{\"lang\": \"\", \"emotion\": \"\", \"event\": \"\", \"text\": ";
    json_string(os, text);
    os << ", \"timestamps\": [";
    char b[40];
    for (size_t i = 0; i < r.frame.size(); ++i) {
      // frame shift 10 ms x subsampling 4 (sherpa-onnx OfflineRecognitionResult timestamps)
      std::snprintf(b, sizeof b, "%s%.2f", i ? ", " : "", (float)(0.04f * (float)r.frame[i]));
      os << b;
    }
    os << "], \"tokens\": [";
    for (size_t i = 0; i < toks.size(); ++i) {
      if (i) os << ", ";
      json_string(os, toks[i]);
    }
    os << "], \"ys_log_probs\": [";
    for (size_t i = 0; i < r.lp.size(); ++i) {
      std::snprintf(b, sizeof b, "%s%.17g", i ? ", " : "", r.lp[i]);
      os << b;
    }
    os << "], \"words\": []}";
    const std::string js = os.str();
    *needed = (int64_t)js.size() + 1;
    if (!buf || cap < *needed) return fail(ZASR_ERR_INVALID, "result buffer too small");
    std::memcpy(buf, js.c_str(), js.size() + 1);
    return (int)ZASR_OK;
  });
}

const char* zasr_last_error(void) { return g_last_error.c_str(); }
const char* zasr_version(void) { return "zasr 0.1 (gfx950)"; }

}  // extern "C"
