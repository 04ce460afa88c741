// Host runtime of libzasr: device-resident model, per-batch workspace, and the encoder /
// search drivers that sequence the HIP kernels on one stream (engine.cpp, engine_load.cpp,
// engine_encoder.cpp, engine_search.cpp, hotword_dfa.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "device_mem.h"
#include "gemm.h"
#include "kernels.h"

namespace zasr {

class SafeTensors;

struct ModelConfig {
  std::string name;
  std::vector<int> dims, layers, ff, heads, ds, kernels;
  int qd = 32, vd = 12, pd = 4, pos_dim = 48;
  int V = 0, dec_dim = 0, joiner_dim = 0, context = 2;
  int c1 = 8, c2 = 32, c3 = 128;
  int max_dim() const {
    int m = 0;
    for (int d : dims) m = d > m ? d : m;
    return m;
  }
};

// the values of ZASR_PRECISION_* (zasr.h)
enum class Precision : int { Fp32 = 0, Bf16 = 1, Bf16Enc = 2, Bf16x3 = 3, Bf16x6 = 4, F16x3 = 5 };

// what the drivers ask about the precision mode, decided once at construction
struct PrecisionFacts {
  Precision mode = Precision::Fp32;
  bool bf16_act = false;  // bf16 weights and GEMM -> GEMM activations (Bf16, Bf16Enc)
  // the `pieces` code of the split modes: 2 / 3 bf16 pieces (bf16x3 / bf16x6), kPiecesF16 for
  // the two fp16 pieces of f16x3 (gemm.h); 0 otherwise
  int pieces = 0;
  bool f16x3 = false;
  bool flash = false;         // the flash attention kernels (every mode but fp32)
  bool nonlin_fused = false;  // NonlinAttention inside the flash kernel (bf16 modes, f16x3)
  bool f32_search = false;    // bf16 encoder with the joiner and the search in f32 (Bf16Enc)
  PrecisionFacts() = default;
  explicit PrecisionFacts(Precision m) : mode(m) {
    bf16_act = m == Precision::Bf16 || m == Precision::Bf16Enc;
    f16x3 = m == Precision::F16x3;
    pieces = m == Precision::Bf16x3 ? 2 : m == Precision::Bf16x6 ? 3 : f16x3 ? kPiecesF16 : 0;
    flash = bf16_act || pieces > 0;
    nonlin_fused = bf16_act || f16x3;
    f32_search = m == Precision::Bf16Enc;
  }
};

struct DLin {
  float* w = nullptr;  // [N][K]
  float* b = nullptr;  // [N] or null
  int N = 0, K = 0;
  void* wh = nullptr;  // bf16 copy of w (precision mode bf16)
  float* bh = nullptr; // bias of the bf16 path when it differs from b (folded row scales)
  void* wp = nullptr;  // bf16 in MFMA-fragment order (ffn_pack_host), the wide fused FFN's operand
  void* wx = nullptr;  // split bf16 of w (precision mode bf16x3): hi [N][K], then lo [N][K]
  void* wr = nullptr;  // f16x3: the two fp16 pieces in MFMA-fragment order (gemm_h3r)
  // split modes, the conv modules' in_proj: rows (and bias) interleaved so output columns
  // 2c / 2c + 1 are the GLU halves of channel c -- the GEMM epilogue applies the GLU (EPI_GLU)
  bool glu = false;
  // the host images of w and b while the model loads (the packers read them); null afterwards
  const float* hw = nullptr;
  const float* hb = nullptr;
};

// Conv2dSubsampling's conv.4 / conv.7: the general GEMMs behind the implicit-im2col loaders
// ALOAD_CONV2 / ALOAD_CONV3, one z-slice per sequence (engine_encoder.cpp; the decode and
// zasr_selftest_conv_gemm share both functions, so the self-test makes the decode's launch).
// Route: bf16 weights when the activations on either side are bf16 or the weight has no split
// image, else the split pieces, else f32.
enum ConvGemmRoute { CONV_GEMM_F32, CONV_GEMM_BF16, CONV_GEMM_X3 };
ConvGemmRoute frontend_conv_route(const DLin& l, bool a_bf16, bool c_bf16);
// fills B / bias / N / ldc of p from l and launches EPI_SWOOSHR on the route; p carries A, C,
// the slices, num_slices and max_M
void launch_frontend_conv_gemm(GemmParams& p, const DLin& l, int aload, bool a_bf16, bool c_bf16,
                               int pieces, hipStream_t st);
// The z-slices of both layers from the fbank frames per sequence T (each >= 9): conv.0 leaves
// T - 2 rows of [80][8], conv.4 l2 = (T - 3) / 2 rows of [39][32], conv.7 L = (T - 7) / 2 rows
// of [19][128], packed sequence after sequence; a slice's M is its output positions (rows x
// frequencies), K the 9 taps x input channels.
struct FrontendConvSlices {
  std::vector<GemmSlice> c2, c3;  // conv.4, conv.7
  int max_M2 = 0, max_M3 = 0;
  long rows_c1 = 0, rows_c2 = 0, rows_L = 0;  // sum of T - 2, l2, L
};
FrontendConvSlices frontend_conv_slices(const int* T, int nseq);

struct DLayer {
  DLin attn_in, sa_in[2], sa_out[2], ff_in[3], ff_out[3], na_in, na_out, cv_in[2], cv_out[2];
  float* cv_dw_w[2] = {nullptr, nullptr};
  float* cv_dw_b[2] = {nullptr, nullptr};
  float* bypass = nullptr;
  float* bypass_mid = nullptr;
  float* norm_b = nullptr;
  float norm_ls = 0.f;
  std::vector<float> pos_w;  // linear_pos weight [4h][pos_dim] (host, to rebuild tables)
  float* pos_tab = nullptr;  // [(2*pmax-1)][4h]
};

struct DStack {
  int d = 0, F = 0, h = 0, ds = 1, K = 0;
  float ds_w[8] = {0};
  float* comb = nullptr;  // out_combiner bypass scale
  std::vector<DLayer> layers;
};

struct DModel {
  ModelConfig cfg;
  float *conv0_w = nullptr, *conv0_b = nullptr;
  DLin conv4, conv7, pw1, pw2, out, enc_proj, dec_proj, joiner;
  float *dw_w = nullptr, *dw_b = nullptr;
  float* out_norm_b = nullptr;
  float out_norm_ls = 0.f;
  std::vector<DStack> stacks;
  float out_ds_w[2] = {0, 0};
  float* dec_emb = nullptr;   // [V][D]
  float* dec_conv = nullptr;  // [D][4][2]
  void* joiner_packed = nullptr;  // bf16 joiner weights in MFMA-fragment order (bf16 mode),
                                  // or their split pieces (bf16x3 / bf16x6), one image each
  long joiner_plane = 0;          // bf16 elements per packed piece image
  float* dec_table = nullptr;  // [V*V][D] decoder output per context (null: too large)
  float* dec_tap0 = nullptr;  // [V][D] conv tap 0 of each embedding row
  float* dec_tap1 = nullptr;  // [V][D] conv tap 1
  int pmax = 0;
};

struct HotwordDFA {
  int num_states = 0, num_cls = 0;
  std::vector<int> tok2cls, next;
  std::vector<double> delta, node_score;
};
HotwordDFA build_hotword_dfa(const std::vector<std::vector<int>>& phrases,
                             const std::vector<float>& scores, int V);

// 80 dense filter rows over the FFT's power bins (row stride n_bins, bins 0 .. 255 read) as the
// fbank kernel's tables: meta = start[80], len[80], woff[80]; wts = the nonzero runs
void pack_mel_banks(const float* banks, int n_bins, std::vector<int>& meta,
                    std::vector<float>& wts);

struct TokenResult {
  std::vector<int> tok, frame;
  std::vector<double> lp;
  std::vector<float> stats;  // 4 per token
  int t_out = 0;
};

class Engine {
 public:
  // model_dir: config.json + model.safetensors or the reference's ONNX files (onnx_io.h);
  // hotwords: token-id phrases + scores, compiled into the device automaton once V is known
  Engine(const std::string& model_dir, int device, int beam, bool greedy,
         const std::vector<std::vector<int>>& hotwords, const std::vector<float>& hotword_scores,
         int precision);
  ~Engine();

  int vocab() const { return model_.cfg.V; }
  int joiner_dim() const { return model_.cfg.joiner_dim; }
  int default_beam() const { return beam_; }
  hipStream_t stream() const { return stream_; }

  // full path from device waveforms (packed); results in chunk order
  std::vector<TokenResult> decode_device(const float* d_wav, const std::vector<long>& wav_off,
                                         const std::vector<long>& n, int beam, hipStream_t st);
  // several batches back to back (results in chunk order, batch_sizes[i] chunks per batch):
  // batch k+1's fbank + encoder run on the call's stream while batch k's search runs on the
  // engine's high-priority search stream -- the search loop is latency-bound on few CUs, so
  // the encoder of the next batch fills the rest of the chip
  std::vector<TokenResult> decode_device_batches(const float* d_wav, const std::vector<long>& wav_off,
                                                 const std::vector<long>& n,
                                                 const std::vector<int>& batch_sizes, int beam,
                                                 hipStream_t st);
  // the same pipeline from HOST waveforms (h_wav: pinned memory for an asynchronous copy):
  // each batch's span of samples is copied into its encoder slot's device buffer on the
  // engine's copy stream and its fbank waits on that copy only, so batch k + 1's upload runs
  // under batch k's encoder / search (the reference's unit of work starts from host audio,
  // core/asr_engine.py:2068)
  std::vector<TokenResult> decode_host_batches(const float* h_wav, const std::vector<long>& wav_off,
                                               const std::vector<long>& n,
                                               const std::vector<int>& batch_sizes, int beam,
                                               hipStream_t st);
  std::vector<TokenResult> decode_features(const std::vector<const float*>& feats,
                                           const std::vector<long>& frames, int beam);
  void fbank_host(const float* wav, long n, float* out);
  void encode_host(const std::vector<const float*>& feats, const std::vector<long>& frames,
                   std::vector<float>& out, std::vector<int>& t_out);
  std::vector<TokenResult> search_host(const std::vector<const float*>& enc,
                                       const std::vector<long>& t_out, int beam);

  // profiling
  // mode 0: off, 1: kernel classes, 2: classes with the GEMMs split by shape
  void profile_enable(int mode) {
    prof_on_ = mode > 0;
    prof_shapes_ = mode == 2;
  }
  void profile_reset();
  std::string profile_report();

  // which kernel each part of the model was routed to at load (JSON; zasr_model_routes): in
  // f16x3 a layer whose weights reach 31 in magnitude keeps the two-accumulator GEMMs
  // (ffn_h3_weights_ok), and a vocabulary whose V^2 D decoder table exceeds the size limit runs
  // the per-frame decoder (decjoin_kernel)
  std::string routes_json() const;
  // replace the fbank's 80 triangular filters (row-major [80][n_bins] weights over the FFT's
  // power bins, n_bins 256 or 257 with bin 256 zero): the reference's browser fbank uses Hz
  // triangles (offline_pwa/static/js/pure-ort-asr-worker.js:369-397) where knf uses mel ones
  void set_mel_banks(const float* banks, int n_bins);

  std::mutex mu;

 private:
  // named grow-only workspace buffer (device_mem.h); the buffers are in use on several
  // streams, so growth drains the whole device
  template <class T>
  T* ws(const std::string& name, size_t count) {
    return ws_tag_.empty() ? ws_.get<T>(name, count, nullptr)
                           : ws_.get<T>(ws_tag_ + name, count, nullptr);
  }
  void upload(void* dst, const void* src, size_t bytes);
  // host blocks (row_len[i] rows of `width` floats at rows[i]; those under min_len rows
  // skipped) packed back to back into workspace buffer `name` on st_
  float* upload_rows(const char* name, const std::vector<const float*>& rows,
                     const std::vector<long>& row_len, int width, long min_len);

  // ---- model load (engine_load.cpp) ----
  void load_model(const SafeTensors& W);
  void load_frontend(const SafeTensors& W);
  void load_stacks(const SafeTensors& W, std::vector<std::vector<float>>& host_images);
  void load_decoder(const SafeTensors& W);
  void load_split_operands();  // bf16x3 / bf16x6 / f16x3
  void load_bf16_operands();   // bf16 modes
  void build_dec_table();
  void load_fbank_tables();
  void load_hotword_tables();
  DLin load_linear(const SafeTensors& W, const std::string& prefix, int N, int K);
  // an MFMA-fragment-order weight image built on the host by `pack` into `elems` bf16-sized
  // elements, uploaded
  template <class Pack>
  void* upload_packed(size_t elems, Pack pack) {
    std::vector<__bf16> pk(elems);
    pack(pk.data());
    return store_.upload(pk);
  }

  // a batch whose encoder output is enqueued (enc_out slot `slot`), waiting for its search
  struct Pending {
    int B = 0;
    std::vector<int> valid, t_out;
    float* enc = nullptr;
    hipEvent_t ready = nullptr;
  };
  // out_slot: encoder output buffer, completion event and pinned arena (0..kMaxEnc);
  // ws_slot: encoder workspace set (0..kMaxEnc-1) -- several batches' encoders may run at
  // once on separate streams
  void encode_stage(const float* d_wav, const std::vector<long>& wav_off, const std::vector<long>& n,
                    int out_slot, int ws_slot, hipStream_t stream, Pending& p);
  std::vector<TokenResult> search_stage(Pending& p, int beam);
  // decode_device_batches for beam search: several batches' searches in flight
  std::vector<TokenResult> decode_batches_two_searches(const float* d_wav,
                                                       const std::vector<long>& wav_off,
                                                       const std::vector<long>& n,
                                                       const std::vector<int>& batch_sizes,
                                                       int beam, hipStream_t main_st);
  // pinned staging for host->device metadata uploads: one arena per encoder output slot
  // plus one for the search, so an upload never waits for the stream to drain
  struct PinArena {
    char* p = nullptr;
    size_t cap = 0, used = 0, want = 0;
  };
  static constexpr int kMaxEnc = 3;  // encoder streams of the batch pipeline
  // kMaxEnc + 1 output slots, then one per search job set (two beam searches in flight)
  static constexpr int kMaxJobs = 3;  // beam searches in flight
  PinArena pin_[kMaxEnc + 1 + kMaxJobs];
  std::string ws_tag_;  // workspace-name prefix of the encoder workspace set in use
  int pin_cur_ = 0;
  void pin_reset(int arena);

  // pipeline stages (all on st_)
  void run_fbank(const float* d_wav, const std::vector<long>& wav_off, const std::vector<long>& n,
                 float* d_feats, std::vector<int>& frames);
  void run_encoder(const float* d_feats, const std::vector<int>& T, float* d_enc,
                   std::vector<int>& t_out);
  std::vector<TokenResult> run_search(const float* d_enc, const std::vector<int>& t_out, int beam);
  // a search whose launches and result copies are enqueued; collect_search waits for it.
  // Job set `set` (0 .. kMaxJobs - 1) owns its search workspace, pinned arena, result buffers and
  // completion event, so two jobs can be in flight on the two search streams.
  struct SearchJob {
    int S_all = 0, S = 0, cap = 0, set = 0, Tmax = 0;
    std::vector<int> order, t_out;
    bool check_finite = false;  // f16x3: the encoder output's fp16-range guard
    hipStream_t stream = nullptr;
  };
  void launch_search(const float* d_enc, const std::vector<int>& t_out, int beam, int set,
                     hipStream_t stream, bool split_groups, SearchJob& job);
  std::vector<TokenResult> collect_search(SearchJob& job);
  struct ResPin {  // pinned host result buffers of one job set
    char* p = nullptr;
    size_t cap = 0;
  };
  ResPin res_pin_[kMaxJobs];

  // ---- encoder driver (engine_encoder.cpp) ----
  // what every layer of one stack shares, built once per stack in run_encoder
  struct StackCtx {
    const DStack* stk = nullptr;
    int R = 0;                         // packed rows at the stack's rate
    int B = 0;                         // sequences
    const int* off = nullptr;          // [B + 1] row offsets (device)
    const int* map = nullptr;          // row -> sequence (device)
    const long* a_off = nullptr;       // [B] head 0's weight block of each sequence
    const GemmSlice* nl_slices = nullptr;  // NonlinAttention's per-sequence GEMM slices
    int maxL = 0;
    const int* o8 = nullptr;           // [B + 1] 32-padded column offsets of t1^T
    int R8 = 0;                        // their total
    AttnBlockMaps bm{};
  };
  // the attention weights of one layer, shared by nonlin_attention, self_attn1 and self_attn2
  struct LayerAttn {
    float* qkp = nullptr;    // fp32: q / k / p projections
    float* A = nullptr;      // head 0's normalised weights (fp32, bf16x3, bf16x6)
    float* stats = nullptr;
    AttnFlashArgs fa{};      // flash modes
  };
  // X: the layer's input; Xalt: a second buffer of its size.  Returns the one that holds the
  // output: Xalt when feed_forward1 ran out of place (ff1_fused; X then stays as the input),
  // else X.  orig_ready: the previous layer wrote this layer's copy of its input (ly_orig);
  // copy_for_next: write the next layer's.
  float* layer_forward(const StackCtx& c, const DLayer& ly, float* X, float* Xalt, bool orig_ready,
                       bool copy_for_next);
  LayerAttn attention_weights(const StackCtx& c, const DLayer& ly, const float* X);
  // O: the layer's input (bypass_mid in feed_forward2's epilogue); src: out of place (fused
  // routes only)
  void feed_forward(const StackCtx& c, const DLayer& ly, int k, float* X, const float* O,
                    const float* src = nullptr);
  void nonlin_attention(const StackCtx& c, const DLayer& ly, float* X, const LayerAttn& at);
  void self_attention(const StackCtx& c, const DLayer& ly, int k, float* X, const LayerAttn& at);
  void conv_module(const StackCtx& c, const DLayer& ly, int k, float* X);
  // head 0's fused NonlinAttention pass of the flash kernel (mode 3)
  void launch_nonlin_flash(const StackCtx& c, const LayerAttn& at, const void* t1t, int hid,
                           const void* y, void* z);
  // a Conv2dSubsampling conv as an implicit-im2col GEMM (p: A, C, slices and sizes set)
  void frontend_conv_gemm(GemmParams& p, const DLin& l, int aload, bool a_bf16, bool c_bf16);
  bool ff1_fused(const DStack& stk, const DLayer& ly) const;
  // byp_orig / byp_scale (split modes, EPI_RESADD): bypass_mid in the epilogue
  void linear(const DLin& l, const float* A, int lda, int M, float* C, int ldc, int epi,
              const char* cls = "enc_gemm", const float* byp_orig = nullptr,
              const float* byp_scale = nullptr);
  // bf16 mode only: A and/or C in bf16 (GEMM -> GEMM intermediates; the GEMM rounds A to
  // bf16 on load anyway, so storing it rounded changes nothing numerically)
  void linear_h(const DLin& l, const void* A, bool a_bf16, int lda, int M, void* C, bool c_bf16,
                int ldc, int epi, const float* byp_orig = nullptr,
                const float* byp_scale = nullptr);
  // a layer projection whose intermediate side is bf16 in the bf16 modes (a16 / c16 say which
  // side that is) and f32 otherwise: linear_h or linear
  void project(const DLin& l, const void* A, bool a16, int lda, int M, void* C, bool c16, int ldc,
               int epi);
  void ensure_pos_tables(int max_len);

  // timing
  struct ProfEvent {
    std::string name;
    hipEvent_t a, b;
  };
  void prof_begin(const char* name);
  void prof_begin(const std::string& name);
  void prof_end();
  static std::string shape_key(const char* cls, int M, int K, int N, bool w16, bool a16,
                               bool c16, int epi);
  bool prof_on_ = false;
  bool prof_shapes_ = false;  // GEMM classes split by shape (profile mode 2)
  std::vector<ProfEvent> prof_pending_;
  std::map<std::string, std::pair<long, double>> prof_acc_;
  std::vector<hipEvent_t> event_pool_;
  hipEvent_t take_event();

  DModel model_;
  struct Routes {
    int ffn_fused_h3 = 0, ffn_gemm_pair = 0;  // f16x3 FFNs (d 128..512): fused / GEMM pair
    int gemm_h3r = 0, gemm_x3_range = 0;      // f16x3 layer projections the row-resident GEMM
                                              // shapes admit: taken / refused by the range check
    int cnx_ffn_h3 = -1;                      // f16x3 ConvNeXt MLP fused (1) or not (0); -1 n/a
  } routes_;
  int device_ = 0;
  int beam_ = 8;
  [[maybe_unused]] bool greedy_ = false;
  // make main_st wait for every encoder stream of a batch pipeline that is not main_st
  void order_after_encoders(const hipStream_t* enc_st, int E, hipStream_t main_st);
  PrecisionFacts prec_;
  hipStream_t stream_ = nullptr;
  hipStream_t stream2_ = nullptr;  // searches (high priority: overlaps the next batch's encoder)
  hipStream_t stream3_ = nullptr;  // the second group of a beam search (high priority)
  hipStream_t stream4_ = nullptr;  // the third beam search in flight (high priority)
  int search_cus_ = 0;             // > 0: search / encoder streams on disjoint CU sets
  hipStream_t enc_extra_[kMaxEnc - 1] = {};  // encoder streams 1.. of the batch pipeline
  // [0, kMaxEnc]: encoder output slots; kMaxEnc + 1: search done; kMaxEnc + 2: start;
  // kMaxEnc + 3: beam groups; kMaxEnc + 4 + set: search job `set` complete
  hipEvent_t part_ev_[kMaxEnc + 4 + kMaxJobs] = {};
  hipStream_t st_ = nullptr;  // stream of the current call
  // decode_host_batches: the call's waveforms are host memory; encode_stage uploads each
  // batch's span on copy_st_ (upload_ev_[slot]: that slot's copy done)
  const float* host_wav_ = nullptr;
  hipStream_t copy_st_ = nullptr;
  hipEvent_t upload_ev_[kMaxEnc + 1] = {};
  DeviceStore store_;  // weights and tables
  Workspace ws_;
  // fbank tables
  double* d_twiddle_ = nullptr;
  float* d_window_ = nullptr;
  int* d_mel_meta_ = nullptr;  // start[80], len[80], woff[80]
  float* d_mel_w_ = nullptr;
  int* h_pinned_ = nullptr;  // pinned host word (live-stream count of the greedy search)
  // hotword tables
  HotwordDFA hw_host_;
  HotwordTables hw_{};
};

}  // namespace zasr
