// hotwords: Aho-Corasick graph restated from core/hotword_context.py:46-184, flattened
// to a dense (state x trie-token) transition table of (next state, score delta)
#include <algorithm>
#include <deque>

#include "common.h"
#include "engine.h"

namespace zasr {

namespace {
struct HwNode {
  int tok = -1;
  double tok_score = 0, node_score = 0, out_score = 0;
  bool is_end = false;
  std::vector<std::pair<int, int>> kids;  // (token, node) in insertion order
  int fail = 0, out = -1;
  int child(int t) const {
    for (auto& k : kids)
      if (k.first == t) return k.second;
    return -1;
  }
};
}  // namespace

HotwordDFA build_hotword_dfa(const std::vector<std::vector<int>>& phrases,
                             const std::vector<float>& scores, int V) {
  HotwordDFA dfa;
  if (phrases.empty()) return dfa;
  std::vector<HwNode> nd(1);
  for (size_t p = 0; p < phrases.size(); ++p) {
    const auto& seq = phrases[p];
    if (seq.empty()) continue;
    double sc = (double)scores[p];
    int cur = 0;
    for (size_t j = 0; j < seq.size(); ++j) {
      int t = seq[j];
      ZASR_REQUIRE(t >= 0 && t < V, "hotword token id out of range");
      bool last = (j + 1 == seq.size());
      int c = nd[cur].child(t);
      if (c < 0) {
        HwNode n;
        n.tok = t;
        n.tok_score = sc;
        n.node_score = nd[cur].node_score + sc;
        n.out_score = last ? n.node_score : 0.0;
        n.is_end = last;
        nd.push_back(n);
        c = (int)nd.size() - 1;
        nd[cur].kids.push_back({t, c});
      } else {
        HwNode& e = nd[c];
        e.tok_score = std::max(sc, e.tok_score);
        e.node_score = nd[cur].node_score + e.tok_score;
        if (last) e.is_end = true;
        if (e.is_end) e.out_score = e.node_score;
      }
      cur = c;
    }
  }
  // BFS fail / output links
  std::deque<int> q;
  for (auto& k : nd[0].kids) {
    nd[k.second].fail = 0;
    q.push_back(k.second);
  }
  while (!q.empty()) {
    int cur = q.front();
    q.pop_front();
    for (auto& k : nd[cur].kids) {
      int t = k.first, kid = k.second;
      int f = nd[cur].fail;
      int c = nd[f].child(t);
      if (c >= 0) {
        f = c;
      } else {
        f = nd[f].fail;
        while (nd[f].child(t) < 0) {
          f = nd[f].fail;
          if (nd[f].tok == -1) break;
        }
        int c2 = nd[f].child(t);
        if (c2 >= 0) f = c2;
      }
      nd[kid].fail = f;
      int o = f;
      while (!nd[o].is_end) {
        o = nd[o].fail;
        if (nd[o].tok == -1) {
          o = -1;
          break;
        }
      }
      nd[kid].out = o;
      if (o >= 0) nd[kid].out_score += nd[o].out_score;
      q.push_back(kid);
    }
  }
  // token classes
  dfa.tok2cls.assign(V, -1);
  std::vector<int> cls_tok;
  for (size_t i = 1; i < nd.size(); ++i) {
    int t = nd[i].tok;
    if (dfa.tok2cls[t] < 0) {
      dfa.tok2cls[t] = (int)cls_tok.size();
      cls_tok.push_back(t);
    }
  }
  dfa.num_states = (int)nd.size();
  dfa.num_cls = (int)cls_tok.size();
  dfa.next.resize((size_t)dfa.num_states * dfa.num_cls);
  dfa.delta.resize((size_t)dfa.num_states * dfa.num_cls);
  dfa.node_score.resize(dfa.num_states);
  for (int s = 0; s < dfa.num_states; ++s) {
    dfa.node_score[s] = nd[s].node_score;
    for (int c = 0; c < dfa.num_cls; ++c) {
      int t = cls_tok[c];
      int n;
      double score;
      int d = nd[s].child(t);
      if (d >= 0) {
        n = d;
        score = nd[n].tok_score;
      } else {
        n = nd[s].fail;
        while (nd[n].child(t) < 0) {
          n = nd[n].fail;
          if (nd[n].tok == -1) break;
        }
        int c2 = nd[n].child(t);
        if (c2 >= 0) n = c2;
        score = nd[n].node_score - nd[s].node_score;
      }
      if (nd[n].out_score != 0) {
        double matched = nd[n].is_end ? nd[n].node_score
                                      : (nd[n].out >= 0 ? nd[nd[n].out].node_score
                                                        : nd[n].node_score);
        score = score + matched - nd[n].node_score;
        n = 0;
      }
      dfa.next[(size_t)s * dfa.num_cls + c] = n;
      dfa.delta[(size_t)s * dfa.num_cls + c] = score;
    }
  }
  return dfa;
}

}  // namespace zasr
