// libzasr search driver: greedy (speculative windows) and modified beam search over the
// encoder output, and the collection of their results.
//
// Reference mapping:
//   search loop             core/asr_engine.py:1051-1153
#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "engine.h"

namespace zasr {

namespace {

// how this engine's joiner runs, and the J buffers that go with it.  Split modes: J written
// once as `pieces` packed bf16 pieces (store_j4), the joiner on the packed W pieces; bf16: one
// packed bf16 image.  With the decoder-context table J is in fragment order for the packed
// joiner (every J writer goes through store_j4); without it decjoin writes row-major J.
struct JoinerRoute {
  const DModel& m;
  int pieces;   // the `pieces` code of the split modes, else 0
  bool bf16;    // bf16 joiner weights
  bool packed;  // the packed joiner on fragment-order J
  int images;   // packed images of J
  bool j16;     // J buffer in bf16 elements

  JoinerRoute(const DModel& model, int split_pieces)
      : m(model),
        pieces(split_pieces),
        bf16(model.joiner.wh != nullptr),
        packed((bf16 || pieces > 0) && model.joiner_packed && model.dec_table),
        images(packed && pieces > 0 ? stored_pieces(pieces) : 1),
        j16(bf16 || packed) {}

  // out[rows][V] = joiner(J), every row (kernels.h JoinerArgs)
  JoinerArgs args(const void* J, long j_plane, float* out, int rows) const {
    const void* W = packed ? m.joiner_packed : bf16 ? m.joiner.wh : pieces > 0 ? m.joiner.wx : m.joiner.w;
    JoinerArgs ja{J, W, m.joiner.b, out, rows, m.cfg.V, m.cfg.joiner_dim};
    ja.layout = packed ? JOINER_PACKED : bf16 ? JOINER_BF16 : JOINER_F32;
    ja.pieces = pieces;
    ja.j_plane = j_plane;
    ja.w_plane = packed ? m.joiner_plane : (long)m.cfg.V * m.cfg.joiner_dim;
    return ja;
  }
  // live_t / live_len / live_f: the greedy windows' live-stream filter (null / 0: every row)
  void launch(const void* J, long j_plane, float* out, int rows, const int* live_t,
              const int* live_len, int live_f, hipStream_t st) const {
    JoinerArgs ja = args(J, j_plane, out, rows);
    ja.live_t = live_t;
    ja.live_len = live_len;
    ja.live_f = live_f;
    launch_joiner(ja, st);
  }
  // the decoder-context table writing the next frame's joiner input into J (jrows packed rows)
  DecTable dec_table(const float* d_enc, const int* d_eo, const int* d_el, void* J,
                     size_t jrows) const {
    DecTable dt{m.dec_table, m.cfg.V, d_enc, d_eo, d_el, J, m.cfg.joiner_dim, bf16 ? 1 : 0};
    dt.j_packed = packed ? 1 : 0;
    dt.j_pieces = packed ? pieces : 0;
    dt.j_plane = (long)jrows * m.cfg.joiner_dim;
    return dt;
  }
};

// the search state of the streams from `first_stream` on (H hypothesis slots per stream)
SearchState slice(SearchState st, int first_stream, int H) {
  const size_t so = (size_t)first_stream * H, no = (size_t)first_stream * st.node_cap;
  for (int** p : {&st.lpf, &st.len, &st.y1, &st.y2, &st.hw, &st.node}) *p += so;
  st.lp += so;
  st.hash += so;
  st.nh += first_stream;
  for (int** p : {&st.node_tok, &st.node_frame, &st.node_parent}) *p += no;
  st.node_lp += no;
  st.node_stats += no;
  st.node_count += first_stream;
  return st;
}

}  // namespace

std::vector<TokenResult> Engine::run_search(const float* d_enc, const std::vector<int>& t_out,
                                            int beam) {
  SearchJob job;
  launch_search(d_enc, t_out, beam, 0, st_, true, job);
  return collect_search(job);
}

void Engine::launch_search(const float* d_enc, const std::vector<int>& t_out, int beam, int set,
                           hipStream_t stream, bool split_groups, SearchJob& job) {
  const ModelConfig& cfg = model_.cfg;
  const int S_all = (int)t_out.size();
  job = SearchJob{};
  job.S_all = S_all;
  job.t_out = t_out;
  job.set = set;
  job.stream = stream;
  hipStream_t caller_st = st_;
  const std::string caller_tag = ws_tag_;
  st_ = stream;
  ws_tag_ = set ? "q" + std::to_string(set) + "/" : "";  // set 0: the single-search names
  pin_reset(kMaxEnc + 1 + set);
  struct Restore {
    Engine* e;
    hipStream_t st;
    std::string tag;
    ~Restore() {
      e->st_ = st;
      e->ws_tag_ = tag;
    }
  } restore{this, caller_st, caller_tag};
  // streams with T' >= 1, sorted by T' descending so active streams form a prefix
  std::vector<int> order;
  std::vector<int> enc_off_all(S_all + 1, 0);
  for (int s = 0; s < S_all; ++s) enc_off_all[s + 1] = enc_off_all[s] + t_out[s];
  for (int s = 0; s < S_all; ++s)
    if (t_out[s] > 0) order.push_back(s);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return t_out[a] > t_out[b]; });
  const int S = (int)order.size();
  job.S = S;
  job.check_finite = prec_.f16x3;
  if (S == 0) return;
  const int H = beam;
  const int Tmax = t_out[order[0]];
  const int V = cfg.V, D = cfg.joiner_dim;
  std::vector<int> eo(S), el(S);
  for (int i = 0; i < S; ++i) {
    eo[i] = enc_off_all[order[i]];
    el[i] = t_out[order[i]];
  }
  int* d_eo = ws<int>("se_eo", S);
  int* d_el = ws<int>("se_el", S);
  upload(d_eo, eo.data(), S * sizeof(int));
  upload(d_el, el.data(), S * sizeof(int));
  const size_t slots = (size_t)S * H;
  SearchState st{};
  st.lp = ws<double>("se_lp", slots);
  st.lpf = ws<int>("se_lpf", slots);
  st.hash = ws<unsigned long long>("se_hash", slots);
  st.len = ws<int>("se_len", slots);
  st.y1 = ws<int>("se_y1", slots);
  st.y2 = ws<int>("se_y2", slots);
  st.hw = ws<int>("se_hw", slots);
  st.node = ws<int>("se_node", slots);
  st.nh = ws<int>("se_nh", S);
  st.node_cap = H * Tmax + 1;
  const size_t ncap = (size_t)S * st.node_cap;
  st.node_tok = ws<int>("se_ntok", ncap);
  st.node_frame = ws<int>("se_nfr", ncap);
  st.node_parent = ws<int>("se_npar", ncap);
  st.node_lp = ws<double>("se_nlp", ncap);
  st.node_stats = ws<float4>("se_nst", ncap);
  st.node_count = ws<int>("se_ncnt", S);
  float* logits = ws<float>("se_logits", slots * V);
  const JoinerRoute jr(model_, prec_.pieces);
  const bool j16 = jr.j16;
  const int jpc = jr.images;
  const size_t jrows = (size_t)joiner_packed_rows((long)slots);
  void* J = j16 ? (void*)ws<__bf16>("se_joinin_h", jrows * D * jpc) : (void*)ws<float>("se_joinin", slots * D);
  ZASR_HIP_CHECK(hipMemsetAsync(J, 0, (j16 ? jrows * 2 * jpc : slots * 4) * D, st_));
  DecoderW dw{model_.dec_tap0, model_.dec_tap1, model_.dec_proj.b, D};
  // greedy with the decoder-context table: speculative windows (kernels.h, greedy_spec)
  const char* spec_env = getenv("ZASR_GREEDY_WINDOW");
  const int F = spec_env ? atoi(spec_env) : 4;
  if (H == 1 && model_.dec_table && (F == 4 || F == 8)) {
    const size_t jrs = (size_t)joiner_packed_rows((long)S * F);
    void* Js = j16 ? (void*)ws<__bf16>("gs_joinin_h", jrs * D * jpc)
                   : (void*)ws<float>("gs_joinin", (size_t)S * F * D);
    // ZASR_GREEDY_FUSED=1: one launch per super-step (joiner_greedy_kernel, packed bf16 / f16x3
    // joiner, F = 4), bit-identical to the two launches but measured slower: per super-step
    // 22.8 vs 21.0 us of kernel time, and its 8-wave blocks at 219 VGPRs crowd the next batch's
    // encoder out (pipelined bf16 hour 104.7k vs 120.8k xRT, profiles/r06/fused_greedy/,
    // DESIGN.md §11) -- the write-through hand-off and the last-arriver's one wave per stream
    // cost what the launch boundary did.  Default: joiner + greedy_spec
    static const bool fused_env = getenv("ZASR_GREEDY_FUSED") && getenv("ZASR_GREEDY_FUSED")[0] == '1';
    const bool fused = fused_env && jr.packed && F == 4 && (jr.pieces == 0 || jr.pieces == kPiecesF16) &&
                       (D == 256 || D == 512) && V % 4 == 0 && V <= 2048;
    const int ldo = fused ? joiner_greedy_ldo(V) : V;
    float* lg = ws<float>("gs_logits", (size_t)S * F * ldo);
    int* d_t = ws<int>("gs_t", S);
    int* d_active = ws<int>("gs_active", 2);
    int* d_cnt = fused ? ws<int>("gs_cnt", (size_t)cdiv(S, 8)) : nullptr;
    const DecTable ds = jr.dec_table(d_enc, d_eo, d_el, Js, jrs);
    prof_begin("search");
    launch_search_init(st, S, 1, st_);
    launch_greedy_spec_init(ds, S, F, d_t, d_active, st_);
    if (fused) ZASR_HIP_CHECK(hipMemsetAsync(d_cnt, 0, (size_t)cdiv(S, 8) * sizeof(int), st_));
    prof_end();
    // every super-step advances each live stream by >= 1 frame: Tmax steps at most; the
    // host checks the live-stream count every kSync steps (one small D2H copy)
    constexpr int kSync = 16;
    int k = 0;
    hipEvent_t live_ev[2];
    for (auto& e : live_ev) ZASR_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    int slot = 0;
    bool have_prev = false;
    while (k < Tmax) {
      for (int b = 0; b < kSync && k < Tmax; ++b, ++k) {
        if (fused) {
          GreedyFusedArgs ga{};
          ga.j = jr.args(Js, ds.j_plane, lg, S * F);
          ga.ldo = ldo;
          ga.st = st;
          ga.t_cur = d_t;
          ga.enc_len = d_el;
          ga.hw = hw_;
          ga.dt = ds;
          ga.active = d_active;
          ga.parity = k & 1;
          ga.cnt = d_cnt;
          ga.S = S;
          prof_begin("joiner_search");
          launch_joiner_greedy(ga, st_);
          prof_end();
          continue;
        }
        prof_begin("joiner");
        jr.launch(Js, ds.j_plane, lg, S * F, d_t, d_el, F, st_);
        prof_end();
        prof_begin("search");
        launch_greedy_spec(st, lg, V, S, F, d_t, d_el, hw_, ds, d_active, k & 1, st_);
        prof_end();
      }
      // the live count after this batch lands in pinned slot `slot`; the host then waits only
      // for the PREVIOUS batch's count, so the GPU always has the next kSync steps queued (a
      // batch enqueued after the last stream finished exits in every kernel's first lines)
      ZASR_HIP_CHECK(hipMemcpyAsync(h_pinned_ + slot, d_active + ((k - 1) & 1), sizeof(int),
                                    hipMemcpyDeviceToHost, st_));
      ZASR_HIP_CHECK(hipEventRecord(live_ev[slot], st_));
      if (have_prev) {
        ZASR_HIP_CHECK(hipEventSynchronize(live_ev[slot ^ 1]));
        if (h_pinned_[slot ^ 1] == 0) break;
      }
      have_prev = true;
      slot ^= 1;
    }
    for (auto e : live_ev) (void)hipEventDestroy(e);
  } else {
  // beam search: the streams are split into G groups whose frame chains run concurrently on
  // the two search streams (each group's chain is latency-bound: joiner -> search step per
  // frame; two chains interleave their launch and scheduling waits).  Group g holds the
  // streams order[g], order[g + G], ... (each group sorted by T' descending, active streams
  // a prefix), laid out contiguously; the search final runs over all of them.
  const int G = split_groups ? std::min(2, S) : 1;
  if (G > 1) {
    std::vector<int> reord;
    for (int g = 0; g < G; ++g)
      for (int i = g; i < S; i += G) reord.push_back(order[i]);
    order = reord;
    for (int i = 0; i < S; ++i) {
      eo[i] = enc_off_all[order[i]];
      el[i] = t_out[order[i]];
    }
    upload(d_eo, eo.data(), S * sizeof(int));
    upload(d_el, el.data(), S * sizeof(int));
  }
  struct Group {
    int s0, n;
    SearchState st;
    DecTable dt;
    void* J;
    float* logits;
    hipStream_t stream;
    int active;
  };
  std::vector<Group> grp(G);
  for (int g = 0, s0 = 0; g < G; ++g) {
    Group& q = grp[g];
    q.s0 = s0;
    q.n = (S - g + G - 1) / G;
    s0 += q.n;
    q.st = slice(st, q.s0, H);
    q.stream = g == 0 ? st_ : stream3_;
    size_t jr_g = jrows;
    if (g == 0) {
      q.J = J;
      q.logits = logits;
    } else {
      jr_g = (size_t)joiner_packed_rows((long)q.n * H);
      q.J = j16 ? (void*)ws<__bf16>("se_joinin_h1", jr_g * D * jpc) : (void*)ws<float>("se_joinin1", (size_t)q.n * H * D);
      q.logits = ws<float>("se_logits1", (size_t)q.n * H * V);
    }
    q.dt = jr.dec_table(d_enc, d_eo + q.s0, d_el + q.s0, q.J, jr_g);
    q.active = q.n;
  }
  if (G > 1) {  // group 1 starts after the uploads / memsets / encoder-output wait on st_
    ZASR_HIP_CHECK(hipEventRecord(part_ev_[kMaxEnc + 3], st_));
    ZASR_HIP_CHECK(hipStreamWaitEvent(stream3_, part_ev_[kMaxEnc + 3], 0));
    const size_t jr1 = (size_t)joiner_packed_rows((long)grp[1].n * H);
    ZASR_HIP_CHECK(hipMemsetAsync(grp[1].J, 0, (j16 ? jr1 * 2 * jpc : (size_t)grp[1].n * H * 4) * D, stream3_));
  }
  hipStream_t home = st_;
  for (Group& q : grp) {
    st_ = q.stream;
    prof_begin("search");
    launch_search_init(q.st, q.n, H, st_);
    if (model_.dec_table) launch_table_init(q.dt, q.n, H, st_);
    prof_end();
  }
  // per frame and group: [decoder + J when there is no table] -> joiner -> search step (which
  // writes the next frame's J from the table)
  for (int t = 0; t < Tmax; ++t) {
    for (Group& q : grp) {
      const int* qel = el.data() + q.s0;
      while (q.active > 0 && qel[q.active - 1] <= t) --q.active;
      if (q.active == 0) continue;
      st_ = q.stream;
      const int rows = q.active * H;
      if (!model_.dec_table) {
        DecJoinArgs da{dw, model_.dec_proj.w, q.st.y1, q.st.y2, d_enc, d_eo + q.s0, q.J, rows, H, t, jr.bf16 ? 1 : 0};
        prof_begin("decoder");
        launch_decjoin(da, st_);
        prof_end();
      }
      prof_begin("joiner");
      jr.launch(q.J, q.dt.j_plane, q.logits, rows, nullptr, nullptr, 0, st_);
      prof_end();
      prof_begin("search");
      launch_search_step(q.st, q.logits, V, q.active, H, beam, t, d_el + q.s0, hw_,
                         model_.dec_table ? &q.dt : nullptr, st_);
      prof_end();
    }
  }
  st_ = home;
  if (G > 1) {  // the final pick on st_ reads every group's nodes
    ZASR_HIP_CHECK(hipEventRecord(part_ev_[kMaxEnc + 3], stream3_));
    ZASR_HIP_CHECK(hipStreamWaitEvent(st_, part_ev_[kMaxEnc + 3], 0));
  }
  }
  const int cap = Tmax;
  job.cap = cap;
  job.Tmax = Tmax;
  job.order = order;
  int* o_tok = ws<int>("so_tok", (size_t)S * cap);
  int* o_fr = ws<int>("so_fr", (size_t)S * cap);
  double* o_lp = ws<double>("so_lp", (size_t)S * cap);
  float4* o_st = ws<float4>("so_st", (size_t)S * cap);
  int* o_cnt = ws<int>("so_cnt", S);
  prof_begin("search");
  launch_search_final(st, S, H, hw_, cap, o_tok, o_fr, o_lp, o_st, o_cnt, st_);
  prof_end();
  // results into this set's pinned buffers (a copy into pageable memory would block the host
  // until the search is done): [cnt S][tok S cap][fr S cap][lp S cap][stats S cap]
  const size_t n = (size_t)S * cap;
  const size_t bytes = 16 * n + 8 * n + 4 * n + 4 * n + 4 * (size_t)S + 64;
  ResPin& rp = res_pin_[set];
  if (rp.cap < bytes) {  // the set's previous job was collected: its buffer is free
    if (rp.p) ZASR_HIP_CHECK(hipHostFree(rp.p));
    rp.cap = bytes + bytes / 4;
    ZASR_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&rp.p), rp.cap, hipHostMallocDefault));
  }
  char* h = rp.p;
  ZASR_HIP_CHECK(hipMemcpyAsync(h, o_st, n * 16, hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipMemcpyAsync(h + 16 * n, o_lp, n * 8, hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipMemcpyAsync(h + 24 * n, o_tok, n * 4, hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipMemcpyAsync(h + 28 * n, o_fr, n * 4, hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipMemcpyAsync(h + 32 * n, o_cnt, (size_t)S * 4, hipMemcpyDeviceToHost, st_));
  if (job.check_finite) {
    // f16x3: the encoder output this search read must be finite (fp16 range guard)
    int* d_bad = ws<int>("so_nonfinite", 1);
    launch_nonfinite_check(d_enc, (long)enc_off_all[S_all] * D, d_bad, st_);
    ZASR_HIP_CHECK(hipMemcpyAsync(h + 32 * n + 4 * (size_t)S, d_bad, 4, hipMemcpyDeviceToHost, st_));
  }
  ZASR_HIP_CHECK(hipEventRecord(part_ev_[kMaxEnc + 4 + set], st_));
}

std::vector<TokenResult> Engine::collect_search(SearchJob& job) {
  std::vector<TokenResult> res(job.S_all);
  for (int s = 0; s < job.S_all; ++s) res[s].t_out = job.t_out[s];
  if (job.S == 0) return res;
  ZASR_HIP_CHECK(hipEventSynchronize(part_ev_[kMaxEnc + 4 + job.set]));
  const int S = job.S, cap = job.cap;
  const size_t n = (size_t)S * cap;
  const char* h = res_pin_[job.set].p;
  const float* h_st = reinterpret_cast<const float*>(h);
  const double* h_lp = reinterpret_cast<const double*>(h + 16 * n);
  const int* h_tok = reinterpret_cast<const int*>(h + 24 * n);
  const int* h_fr = reinterpret_cast<const int*>(h + 28 * n);
  const int* h_cnt = reinterpret_cast<const int*>(h + 32 * n);
  if (job.check_finite && h_cnt[S] != 0) {
    // drain every engine stream (later batches' encoders, the other search job) before the
    // error leaves the pipeline: the next call reuses the workspaces and pinned arenas
    ZASR_HIP_CHECK(hipDeviceSynchronize());
    throw std::runtime_error("precision f16x3: non-finite encoder output (an activation exceeded "
                             "the fp16 range of the split operands); decode with bf16x6 or fp32");
  }
  for (int i = 0; i < S; ++i) {
    TokenResult& r = res[job.order[i]];
    const int c = h_cnt[i];
    const size_t o = (size_t)i * cap;
    r.tok.assign(h_tok + o, h_tok + o + c);
    r.frame.assign(h_fr + o, h_fr + o + c);
    r.lp.assign(h_lp + o, h_lp + o + c);
    r.stats.assign(h_st + 4 * o, h_st + 4 * (o + c));
  }
  return res;
}

}  // namespace zasr
