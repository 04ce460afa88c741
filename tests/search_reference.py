"""Cases, seeded inputs, the float64 reference, its bounds, a numpy emulation and the chain drivers
of the transducer search kernel tests (tests/test_gpu_search.py on the GPU through
zasr_selftest_search_step / _greedy_spec / _search_final; tests/test_search_reference.py without
one).

What the kernels are documented to compute (csrc/search_kernels.hip), per stream and frame t, from
the n live hypotheses (token list ys, score lp, flag lpf) and their logits rows x_h [V] as stored:

    lp_hv = (x_hv - max_h) - log sum_v exp(x_hv - max_h) + lp_h
    the k = min(beam, n V) best (h, v) by (lp descending, flat index h V + v ascending), expanded in
    that order: v = 0 (blank) keeps ys; any other v appends it and, unless v = UNK = 2, steps the
    hotword graph, whose delta is added AFTER the top-k.  Duplicates of the full token list merge
    into their first occurrence with oracle.search.log_add, one after the other in candidate order;
    lpf = 1 exactly when a merge took the non-cutoff branch (the result is then an np.float64 in the
    reference program, added in f64 on the next frame), else the flag of the larger operand (0 for a
    fresh candidate).  Every first occurrence that is an emission appends a node (tok, frame = t,
    parent = the source's node, node_lp = candidate lp - source lp, the four statistics of the
    source row = oracle.search.raw_token_stats of the row in float64).  The new hypotheses fill
    slots 0 .. nh - 1 in first-occurrence order; slots from nh on, nodes outside [old count, new
    count) and every array of a stream with t >= enc_len keep their bytes.  With the
    decoder-context table the J row of new slot j is tanh(enc[t + 1] + table[y2_j][y1_j]) when
    t + 1 < enc_len.

The reference tracks the token lists itself (the kernel's 64-bit hash is opaque) and takes every
live hypothesis's lp and lpf from the state the kernel was given -- its own previous output, already
compared -- so a chain is checked frame by frame with no drift to budget for.

Hotword states.  zasr_selftest_hotword_dfa exposes build_hotword_dfa's tables; state i of the
automaton is the i-th node oracle.search.HotwordGraph created (both builders number nodes in
insertion order), which check_dfa() proves per build by comparing node_score[i] and every
(state, token) transition's (delta, next) with HotwordGraph.step.  The kernel's `hw` is then
compared exactly as an index, and through node_score in the final pick.

The greedy window (beam 1, F rows of one context): the frame above row by row while the winner is
blank; the first non-blank row fe emits and t_new = t0 + fe + 1, else t_new = t0 + nf
(nf = min(F, enc_len - t0)); active[parity] counts streams with t_new < enc_len and
active[parity ^ 1] = 0; J row f of the next window is tanh(enc[t_new + f] + table[y2'][y1']) for
f < min(F, enc_len - t_new), every other row untouched.  Between rows the kernel carries its own
f32 score, which no output shows, so the bound of row f adds the bounds of the rows before it.

The final pick: the first maximum over the live slots of (lp - node_score(hw)) / max(len, 1) (len
counts the two context entries), its node chain walked back through the parents, oldest first; a
chain longer than out_cap keeps its newest out_cap nodes in order.

Inputs.  A row is a function of (case, stream, frame, slot, context, salt): default_rng seeded with
the crc32 of that key.  "gauss": 2 N(0, 1), blank + 4.  "peaked": 0.5 N(0, 1), blank + 6 and three
of favoured(V) -- shared by all rows of the (stream, frame) -- at + 5.5 + 0.7 U(-1, 1) per row, so
different hypotheses emit the same tokens and sequences merge.  favoured(V) holds UNK and V - 1
(the last float4 of a row).

Selection must not rest on rounding.  A frame is accepted only if every adjacent pair of the
reference's best k + 1 candidates is separated by more than 4 (B_i + B_j) or is identical (bit-equal
x in one row, or in two byte-equal rows whose hypotheses have equal (lp, lpf): the kernel's
arithmetic is then bit-equal too and the flat index decides), and if no log-add's operand
distance lies within 4 (B_i + B_j) of the -36 cutoff; otherwise the driver redraws the frame with
the next salt, at most MAX_REDRAWS times (asserted).  Which of two rounding-close candidates wins
is the hour test's audited-tie question, not this one's.

Bounds, u = 2^-24, from the float64 quantities of each element (d = x - max, S = sum exp d,
lse = log S, A1 = sum e |d| / S, A2 = sum e d^2 / S, A3 = sum e^(d/3) |d| / 3 / sum e^(d/3)):

    candidate lp  the kernel computes fl(fl(fl(x - m) - ls) + fl(score)), ls = logf(sum __expf):
                  B_lp = u (32 + 2 (|d| + |lse| + |score| + |lp|)); 32 covers __expf's ~2 ulp and
                  an f32 tree sum of <= 4096 terms (eps_S <= 16 u, |dlse| = eps_S), logf's ulp.
                  The hotword delta and the log-add are f64: a merged lp gets the largest B_lp of
                  its parts (log-add is 1-Lipschitz in the max norm) + 2^-48 (1 + |lp|).
    node_lp       (double) candidate - source lp: B_lp + u |source lp| (fl(score)'s rounding is
                  inside B_lp; the f64 subtraction sees the unrounded source).
    eps_S         u (20 + A1): 16 u the sum, 2 u __expf, u |d| the rounding of d = x - m weighted
                  by e (sum e |d| / S = A1), 2 u spare.
    top1 = 1 / S  top1 (eps_S + 2 u)
    top2          e^(m2 - m1) / S: top2 (eps_S + u (6 + |m2 - m1|)) + 2^-126 (below the smallest
                  normal f32 a result may be flushed to zero)
    entropy       ls - e1 / S, e1 = sum e d by fma in f32: u (|lse| + 2) + eps_S for ls;
                  sum e |d| (2 u + u |d| + 16 u) / S + A1 (eps_S + 2 u) for the quotient:
                  B_ent = u (24 + |lse| + |ent| + 44 A1 + A1^2 + A2)
    sum p^(1/3)   e3 exp2(-log2(S) / 3), e3 = sum __expf(d / 3):
                  B_s3 = s3 u (20 + A3 + (20 + A1) / 3 + 3 |log2 S| / 3 + 8): e3's sum and
                  __expf, the argument d / 3's rounding weighted by e^(d/3) (A3), eps_S / 3, the
                  log2 / exp2 pair (u |log2 S| / 3 in the exponent, ln 2 < 1) and their ulps.
    After test_gpu_parity._entropy_dict's normalisation these stay below the project's end-to-end
    tolerances (2e-4 on the entropy fields, 1e-5 on top-1): test_search_reference asserts it.
    J  f32 route  u (|e + d| + 4)   the f32 add, tanhf
       bf16       2^-8 |tanh| + 2^-20   fast_tanh on __expf, then RNE to bf16: 8 significant bits,
                  half an ulp is 2^-8 of the binade (a first derivation took 2^-9, which the
                  exact emulation's RNE alone reaches twice over)
       pieces     the f32-route bound + r |tanh|: r = 2^-16 for 2 bf16 pieces (2^-8 of a
                  residual that is itself <= 2^-8 |x|; not 2^-17, for the same reason), 2^-24
                  for 3, 2^-22 for fp16 hi + lo 2^-11 (11 significant bits each)
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from oracle.search import BLANK, UNK, HotwordGraph, log_add, raw_token_stats

U = 2.0 ** -24
SENT = 0x6b            # every byte of a buffer before a call
MAX_REDRAWS = 50
JFMT_NAMES = ("f32", "bf16", "bf16p", "bf16x2p", "bf16x3p", "f16hlp")
STAT_NAMES = ("entropy", "s3", "top1", "top2")
# test_gpu_parity's end-to-end tolerances: the ceiling of the normalised statistics' bounds
CEIL_ENTROPY_FIELDS, CEIL_TOP1 = 2e-4, 1e-5


def seed_of(*key) -> int:
    return zlib.crc32(repr(key).encode())


def favoured(V: int) -> List[int]:
    return [t for t in dict.fromkeys((1, 2, 3, 5, 7, V - 1)) if 0 < t < V]


# ------------------------------------------------------------------------------- hypotheses
@dataclass
class Hyp:
    ys: Tuple[int, ...]      # (-1, 0) + the emitted tokens
    lp: float
    lpf: int
    node: int
    g: object = None         # HotwordGraph node (None: no hotwords)
    B: float = 0.0

    @property
    def y1(self):
        return max(0, self.ys[-1])

    @property
    def y2(self):
        return max(0, self.ys[-2])


def init_hyps(graph: Optional[HotwordGraph]) -> List[Hyp]:
    return [Hyp((-1, BLANK), 0.0, 0, -1, graph.root if graph else None)]


def log_add_f(a, fa, b, fb):
    """oracle.search.log_add with the result-type flag; also |d + 36|, the distance of the
    operands' gap from the cutoff"""
    if a < b:
        a, b, fa, fb = b, a, fb, fa
    d = b - a
    if d < -36.0:
        return a, fa, abs(d + 36.0)
    return float(log_add(a, b)), 1, abs(d + 36.0)


def row_terms(x32: np.ndarray) -> dict:
    x = x32.astype(np.float64)
    m = float(x.max())
    d = x - m
    e = np.exp(d)
    S = float(e.sum())
    return {"d": d, "e": e, "S": S, "lse": math.log(S)}


def stats_reference(x32: np.ndarray, rt: dict):
    """(entropy, sum p^(1/3), top1, top2) = raw_token_stats in float64, and their bounds"""
    ref = raw_token_stats(x32.astype(np.float64))
    d, e, S, lse = rt["d"], rt["e"], rt["S"], rt["lse"]
    ad = np.abs(d)
    A1 = float((e * ad).sum() / S)
    A2 = float((e * d * d).sum() / S)
    e3 = np.exp(d / 3.0)
    A3 = float((e3 * ad).sum() / 3.0 / e3.sum())
    eps_S = U * (20.0 + A1)
    srt = np.sort(d)
    gap = float(srt[-1] - srt[-2]) if len(srt) > 1 else 0.0
    ent, s3, top1, top2 = ref
    B = (U * (24.0 + abs(lse) + abs(ent) + 44.0 * A1 + A1 * A1 + A2),
         s3 * U * (20.0 + A3 + (20.0 + A1) / 3.0 + abs(math.log2(S)) + 8.0),
         top1 * (eps_S + 2.0 * U),
         top2 * (eps_S + U * (6.0 + gap)) + 2.0 ** -126)
    return ref, B


def normalised_stat_bounds(B, V: int):
    """the bounds as test_gpu_parity._entropy_dict's fields see them:
    (tsallis_norm, margin, entropy_norm, top1_prob)"""
    ts_scale = 1.0 / (V ** (2.0 / 3.0) - 1.0)   # ts / ts_max = (1 - s3) / (1 - V^(2/3))
    return B[1] * ts_scale, B[2] + B[3], B[0] / math.log(V), B[2]


@dataclass
class FrameRef:
    hyps: List[Hyp]
    nodes: List[dict]
    unsafe: str                      # "" when the selection does not rest on rounding
    events: Dict[str, int] = field(default_factory=dict)
    merges: int = 0


def classify_hw(graph: HotwordGraph, state, tok: int) -> str:
    """what kind of transition graph.step(state, tok) is (for the hotword family's coverage)"""
    if tok in state.kids:
        nd = state.kids[tok]
        kind = "child"
    else:
        nd = state.fail
        while tok not in nd.kids:
            nd = nd.fail
            if nd.tok == -1:
                break
        if tok in nd.kids:
            nd = nd.kids[tok]
        if nd is graph.root:
            kind = "reset" if state is not graph.root else "miss"
        else:
            kind = "fail_link" if state is not graph.root else "child"
    if nd.out_score != 0:
        return "full_match"
    return kind


def top_candidates(flat: np.ndarray, k: int) -> np.ndarray:
    """flat indices of the best k by (value descending, index ascending)"""
    n = flat.shape[0]
    if k >= n:
        return np.argsort(-flat, kind="stable")
    thr = np.partition(flat, n - k)[n - k]
    idx = np.flatnonzero(flat >= thr)
    return idx[np.argsort(-flat[idx], kind="stable")][:k]


def frame_reference(hyps: List[Hyp], rows: np.ndarray, beam: int, t: int,
                    graph: Optional[HotwordGraph], node_base: int) -> FrameRef:
    """One frame of one stream in float64.  rows [>= n][V] float32, row h of hypothesis h."""
    n, V = len(hyps), rows.shape[1]
    terms = [row_terms(rows[h]) for h in range(n)]
    lp = np.stack([terms[h]["d"] - terms[h]["lse"] + hyps[h].lp for h in range(n)])
    flat = lp.reshape(-1)
    k = min(beam, n * V)
    top = top_candidates(flat, min(k + 1, n * V))

    def bound(idx):
        h, v = divmod(int(idx), V)
        return U * (32.0 + 2.0 * (abs(terms[h]["d"][v]) + abs(terms[h]["lse"]) + abs(hyps[h].lp)
                                  + abs(flat[idx])))

    B = [bound(i) for i in top]
    unsafe = ""
    events: Dict[str, int] = {}
    bits = rows.view(np.uint32)
    for i in range(len(top) - 1):
        a, b = int(top[i]), int(top[i + 1])
        if flat[a] - flat[b] > 4.0 * (B[i] + B[i + 1]):
            continue
        (ha, va), (hb, vb) = divmod(a, V), divmod(b, V)
        same = bits[ha, va] == bits[hb, vb] and (
            ha == hb or (np.array_equal(bits[ha], bits[hb]) and hyps[ha].lp == hyps[hb].lp
                         and hyps[ha].lpf == hyps[hb].lpf))
        if not same:
            unsafe = f"candidates {i} and {i + 1} are {flat[a] - flat[b]:.3e} apart"
            break
        tie = "tie_same_row" if ha == hb else "tie_cross_row"
        events[tie] = events.get(tie, 0) + 1
    new: Dict[tuple, Hyp] = {}
    nodes: List[dict] = []
    merges = 0
    stat_cache: Dict[int, tuple] = {}
    for rank in range(k):
        idx = int(top[rank])
        h, v = divmod(idx, V)
        src = hyps[h]
        score, g, ys = float(flat[idx]), src.g, src.ys
        if v != BLANK:
            if graph is not None and v != UNK:
                kind = classify_hw(graph, src.g, v)
                events[kind] = events.get(kind, 0) + 1
                dlt, g = graph.step(src.g, v)
                score += dlt
            ys = src.ys + (v,)
        if ys in new:
            r = new[ys]
            r.lp, r.lpf, cut = log_add_f(r.lp, r.lpf, score, 0)
            if cut <= 4.0 * (r.B + B[rank]) and not unsafe:
                unsafe = f"a log-add {cut:.3e} from the cutoff"
            r.B = max(r.B, B[rank])
            merges += 1
            continue
        node = src.node
        if v != BLANK:
            if h not in stat_cache:
                stat_cache[h] = stats_reference(rows[h], terms[h])
            node = node_base + len(nodes)
            nodes.append({"tok": v, "frame": t, "parent": src.node, "lp": float(flat[idx]) - src.lp,
                          "B": B[rank] + U * abs(src.lp), "stats": stat_cache[h][0],
                          "Bstats": stat_cache[h][1]})
        new[ys] = Hyp(ys, score, 0, node, g, B[rank])
    out = list(new.values())
    for r in out:
        r.B += 2.0 ** -48 * (1.0 + abs(r.lp))
    return FrameRef(out, nodes, unsafe, events, merges)


# ------------------------------------------------------------------------------- row generators
def gen_row(gen: str, key: tuple, V: int, fav3: Tuple[int, ...]) -> np.ndarray:
    rng = np.random.default_rng(seed_of(*key))
    if gen == "gauss":
        x = 2.0 * rng.standard_normal(V)
        x[0] += 4.0
    elif gen == "peaked":
        x = 0.5 * rng.standard_normal(V)
        x[0] += 6.0
        for tk in fav3:
            x[tk] += 5.5 + 0.7 * rng.uniform(-1.0, 1.0)
    else:
        raise ValueError(gen)
    return x.astype(np.float32)


def frame_fav(name: str, s: int, t: int, salt: int, V: int) -> Tuple[int, ...]:
    fav = favoured(V)
    rng = np.random.default_rng(seed_of(name, s, t, salt, "fav"))
    return tuple(int(x) for x in rng.choice(fav, size=min(3, len(fav)), replace=False))


# ------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class StepCase:
    name: str
    V: int
    beam: int
    Hmax: int
    gen: str
    hot: bool = False
    craft: str = ""
    enc_len: Tuple[int, ...] = (24, 1, 21, 12)
    jfmt: int = -1          # >= 0: with the decoder-context table
    D: int = 0

    @property
    def S(self):
        return len(self.enc_len)


VOCABS = (4, 8, 64, 512, 516, 2000, 2048, 2052, 4096)
BEAMS = (1, 2, 4, 5, 8, 9, 16)


def chain_cases() -> List[StepCase]:
    pairs = [(V, b) for V in VOCABS for b in (8, 16)]
    pairs += [(V, b) for V in (64, 2052) for b in BEAMS if b not in (8, 16)]
    out = []
    for V, b in pairs:
        for gen in ("gauss", "peaked"):
            out.append(StepCase(f"chain_V{V}_b{b}_{gen}", V, b, b, gen))
    for gen in ("gauss", "peaked"):
        out.append(StepCase(f"chain_V64_b5_H8_{gen}", 64, 5, 8, gen))
    return out


def hotword_cases() -> List[StepCase]:
    return [StepCase(f"hot_V{V}_b{b}", V, b, b, "peaked", hot=True)
            for V in (64, 2052) for b in (1, 4, 16)]


def hotword_phrases(V: int):
    """cut from favoured(V) = (1, 2, 3, 5, 7, V - 1): shared prefixes, a phrase that is another's
    suffix (fail and output links), one holding UNK (which never steps the graph); token 1 is
    favoured but in no phrase (the out-of-trie reset)"""
    L = V - 1
    return ([[3, 5], [5, 7, L], [3, 5, 7], [7, L], [L, 3, 3], [5, 2]],
            [2.0, 1.5, 1.0, 2.5, 0.75, 1.25])


CRAFTS = ("flat", "one_lane", "plateau", "kth_is_threshold", "equal_rows", "cutoff_merge",
          "triple_merge")


def crafted_cases() -> List[StepCase]:
    el = (4, 3)
    c = [StepCase("craft_flat_V4096_b16", 4096, 16, 16, "gauss", craft="flat", enc_len=el),
         StepCase("craft_flat_V64_b16", 64, 16, 16, "gauss", craft="flat", enc_len=el),
         StepCase("craft_one_lane_V2048_b16", 2048, 16, 16, "gauss", craft="one_lane", enc_len=el),
         StepCase("craft_one_lane_V512_b8", 512, 8, 8, "gauss", craft="one_lane", enc_len=el),
         StepCase("craft_plateau_V4096_b16", 4096, 16, 16, "gauss", craft="plateau", enc_len=el),
         StepCase("craft_plateau_V512_b8", 512, 8, 8, "gauss", craft="plateau", enc_len=el),
         StepCase("craft_plateau_V512_b4", 512, 4, 4, "gauss", craft="plateau", enc_len=el)]
    c += [StepCase(f"craft_kth_V512_b{b}", 512, b, b, "gauss", craft="kth_is_threshold", enc_len=el)
          for b in (4, 8, 16)]
    c += [StepCase("craft_equal_rows_V64_b4", 64, 4, 4, "gauss", craft="equal_rows", enc_len=el),
          StepCase("craft_equal_rows_V2052_b16", 2052, 16, 16, "gauss", craft="equal_rows", enc_len=el),
          # n V < beam on frame 0 (one hypothesis, 4 candidates) and n V = beam on frame 1
          StepCase("craft_nV_lt_beam_V4_b16", 4, 16, 16, "gauss", enc_len=el),
          StepCase("craft_cutoff_merge_V64_b2", 64, 2, 2, "gauss", craft="cutoff_merge", enc_len=el),
          StepCase("craft_triple_merge_V64_b4", 64, 4, 4, "gauss", craft="triple_merge", enc_len=el)]
    return c


def table_cases() -> List[StepCase]:
    return [StepCase(f"table_V64_b{b}_{JFMT_NAMES[f]}", 64, b, b, "peaked", enc_len=(12, 1, 9, 6),
                     jfmt=f, D=256) for b in (1, 4, 16) for f in range(6)]


def lane_cols(lane: int, V: int) -> List[int]:
    """the columns one lane holds: float4 lane + 64 q"""
    return [4 * i + c for i in range(lane, V // 4, 64) for c in range(4)]


def craft_rows(case: StepCase, s: int, t: int, hyps: List[Hyp], salt: int) -> Optional[np.ndarray]:
    """the crafted frame's rows [n][V], or None where the case's generator serves"""
    V, n = case.V, len(hyps)
    KB = 1 if case.beam == 1 else 4 if case.beam <= 4 else 8 if case.beam <= 8 else 16
    rng = np.random.default_rng(seed_of(case.name, s, t, salt, "craft"))
    cr = case.craft
    if cr in ("one_lane", "plateau", "kth_is_threshold") and t == 0:
        # one dominant hypothesis: on frame 1 the global best k are row 0's own best k
        x = -30.0 + rng.standard_normal((n, V))
        x[:, 0] = 0.0
        return x.astype(np.float32)
    if cr == "flat" and t == 1:
        return np.full((n, V), np.float32(0.125 * salt))
    if cr == "one_lane" and t == 1:
        # every other lane group's maximum is the same -50, which becomes the threshold: all V
        # elements pass it
        x = np.full((n, V), -50.0)
        cols = lane_cols(5, V)
        x[:, cols] = rng.standard_normal((n, len(cols)))
        return x.astype(np.float32)
    if cr == "plateau" and t == 1:
        x = -30.0 + rng.standard_normal((n, V))
        nhi = KB - 3                       # ranks KB - 2 .. KB + 67 are the plateau
        for h in range(n):
            cols = rng.permutation(V)[:70 + nhi]
            x[h, cols[:70]] = 1.25
            x[h, cols[70:]] = 1.75 + rng.uniform(0.0, 1.0, size=nhi)
        return x.astype(np.float32)
    if cr == "kth_is_threshold" and t == 1:
        x = -30.0 + rng.standard_normal((n, V))
        step = 64 // KB                   # one lane of each of the KB lane groups
        for h in range(n):
            vals = np.sort(rng.uniform(0.0, 8.0, size=KB))
            x[h, [4 * step * j for j in range(KB)]] = vals
        return x.astype(np.float32)
    if cr == "equal_rows":
        if t == 0:
            x = -30.0 + rng.standard_normal((n, V))
            x[:, 0] = 0.0
            x[:, 5] = x[:, V - 1] = -1.0      # two tokens with bit-equal logits
            return x.astype(np.float32)
        if t == 1:
            x = (2.0 * rng.standard_normal((n, V))).astype(np.float32)
            eq = [h for h in range(n) if hyps[h].ys[-1] in (5, V - 1) and len(hyps[h].ys) == 3]
            for h in eq[1:]:
                x[h] = x[eq[0]]
            x[eq, 9] += np.float32(12.0)       # in both rows alike: the tied pair leads
            return x
    if cr == "cutoff_merge":
        x = -100.0 + 0.01 * rng.standard_normal((n, V))
        if t == 0:
            x[:, 0], x[:, 7] = 0.0, -40.0
            return x.astype(np.float32)
        if t == 1:
            for h in range(n):
                x[h, 7 if len(hyps[h].ys) == 2 else 0] = 0.0
            return x.astype(np.float32)
    if cr == "triple_merge" and t in (0, 1):
        x = -60.0 + rng.standard_normal((n, V))
        if t == 0:
            x[:, 0], x[:, 7] = 0.0, -1.0
        else:
            for h in range(n):
                if len(hyps[h].ys) == 2:
                    x[h, 7], x[h, 0] = 0.0, -0.5
                else:
                    x[h, 0] = 0.0
        return x.astype(np.float32)
    return None


# ------------------------------------------------------------------------------- the J formats
def j_rows_packed(rows: int) -> int:
    return (rows + 63) // 64 * 64


def j_bytes(jfmt: int, rows: int, D: int) -> int:
    if jfmt == 0:
        return rows * D * 4
    if jfmt == 1:
        return rows * D * 2
    return j_rows_packed(rows) * D * 2 * (3 if jfmt == 4 else 2 if jfmt in (3, 5) else 1)


def packed_off(row, k, D):
    """element offset of J[row][k] in MFMA-fragment order (kernels.h JoinerArgs, JOINER_PACKED)"""
    return ((row // 32 * (D // 16) + k // 16) * 64 + row % 32 + 32 * (k // 8 % 2)) * 8 + k % 8


def j_element_offsets(jfmt: int, rows: int, D: int, row: int) -> List[np.ndarray]:
    """per stored image, the element offsets of J[row][0 .. D)"""
    k = np.arange(D)
    if jfmt <= 1:
        return [row * D + k]
    plane = j_rows_packed(rows) * D
    n = 3 if jfmt == 4 else 2 if jfmt in (3, 5) else 1
    return [packed_off(row, k, D) + t * plane for t in range(n)]


def bf16_to_f64(u16: np.ndarray) -> np.ndarray:
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def j_decode_row(J: np.ndarray, jfmt: int, rows: int, D: int, row: int) -> np.ndarray:
    offs = j_element_offsets(jfmt, rows, D, row)
    if jfmt == 0:
        return J.view(np.float32)[offs[0]].astype(np.float64)
    u = J.view(np.uint16)
    if jfmt == 5:
        hi, lo = (u[o].view(np.float16).astype(np.float64) for o in offs)
        return hi + lo * 2.0 ** -11
    return sum(bf16_to_f64(u[o]) for o in offs)


def j_reference(enc_row: np.ndarray, a_row: np.ndarray, b_row: np.ndarray, jfmt: int):
    """tanh(enc + table) in float64 from the f32 table entry the entry point builds, and its bound"""
    tab = (a_row.astype(np.float32) + b_row.astype(np.float32)).astype(np.float64)
    z = enc_row.astype(np.float64) + tab
    ref = np.tanh(z)
    f32b = U * (np.abs(z) + 4.0)
    if jfmt == 0:
        return ref, f32b
    if jfmt in (1, 2):
        return ref, 2.0 ** -8 * np.abs(ref) + 2.0 ** -20
    r = {3: 2.0 ** -16, 4: 2.0 ** -24, 5: 2.0 ** -22}[jfmt]
    return ref, f32b + r * np.abs(ref)


def j_encode_row(x32: np.ndarray, jfmt: int) -> List[np.ndarray]:
    """the emulation's rounding of an f32 row into the format's stored images (16-bit patterns, or
    the f32 row)"""
    def bf16(v):
        b = v.astype(np.float32).view(np.uint32).astype(np.uint64)
        return (((b + 0x7fff + ((b >> 16) & 1)) >> 16) & 0xffff).astype(np.uint16)
    if jfmt == 0:
        return [x32.astype(np.float32)]
    if jfmt in (1, 2):
        return [bf16(x32)]
    if jfmt == 5:
        hi = x32.astype(np.float16)
        lo = ((x32 - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
        return [hi.view(np.uint16), lo.view(np.uint16)]
    out, r = [], x32.astype(np.float32)
    for _ in range(3 if jfmt == 4 else 2):
        p = bf16(r)
        out.append(p)
        r = r - (p.astype(np.uint32) << 16).view(np.float32)
    return out


def table_operands(name: str, V: int, D: int, enc_len) -> dict:
    rng = np.random.default_rng(seed_of(name, "table"))
    off = np.concatenate([[0], np.cumsum(enc_len)[:-1]]).astype(np.int32)
    rows = max(int(np.sum(enc_len)), 1)
    return {"D": D, "a": (0.6 * rng.standard_normal((V, D))).astype(np.float32),
            "b": (0.6 * rng.standard_normal((V, D))).astype(np.float32),
            "enc": (0.8 * rng.standard_normal((rows, D))).astype(np.float32), "enc_off": off}


# ------------------------------------------------------------------------------- state helpers
def state_alloc(S: int, Hmax: int, node_cap: int) -> dict:
    from zasr.binding import search_state_alloc
    return search_state_alloc(S, Hmax, node_cap, SENT)


def state_copy(st: dict) -> dict:
    return {k: v.copy() for k, v in st.items()}


def state_crc(st: dict, extra=()) -> int:
    c = 0
    for k in sorted(st):
        c = zlib.crc32(st[k].tobytes(), c)
    for a in extra:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


NODE_KEYS = ("node_tok", "node_frame", "node_parent", "node_lp", "node_stats")
SLOT_KEYS = ("lp", "lpf", "hash", "len", "y1", "y2", "hw", "node")


def graph_index(graph: Optional[HotwordGraph], g) -> int:
    if graph is None:
        return 0
    for i, nd in enumerate(graph.nodes):
        if nd is g:
            return i
    raise AssertionError("graph node not in the graph")


class Worst:
    """worst |got - ref| / bound per output name"""

    def __init__(self):
        self.r: Dict[str, float] = {}

    def add(self, name: str, got, ref, bound):
        r = float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
                         / np.asarray(bound, np.float64))) if np.size(got) else 0.0
        if not r <= self.r.get(name, 0.0):     # keeps a NaN
            self.r[name] = r
        return r

    def __str__(self):
        return " ".join(f"{k} {v:.3f}" for k, v in sorted(self.r.items())) or "-"

    def bad(self):
        return [(k, v) for k, v in self.r.items() if not v <= 1.0]


def compare_stream_frame(before: dict, after: dict, s: int, ref: FrameRef,
                         graph: Optional[HotwordGraph], worst: Worst) -> List[str]:
    """the state of stream s after a frame against the reference; returns the exact-field failures"""
    bad = []
    nh = int(after["nh"][s])
    if nh != len(ref.hyps):
        return [f"nh {nh} != {len(ref.hyps)}"]
    for j, r in enumerate(ref.hyps):
        exact = {"len": len(r.ys), "y1": r.y1, "y2": r.y2, "lpf": r.lpf, "node": r.node,
                 "hw": graph_index(graph, r.g)}
        for k, v in exact.items():
            if int(after[k][s, j]) != v:
                bad.append(f"slot {j} {k} {int(after[k][s, j])} != {v}")
        worst.add("lp", after["lp"][s, j], r.lp, r.B)
    for k in SLOT_KEYS:      # slots from nh on keep their bytes
        if after[k][s, nh:].tobytes() != before[k][s, nh:].tobytes():
            bad.append(f"{k}: a slot at or above nh = {nh} changed")
    n0 = int(before["node_count"][s])
    n1 = int(after["node_count"][s])
    if n1 != n0 + len(ref.nodes):
        return bad + [f"node_count {n1} != {n0 + len(ref.nodes)}"]
    for i, nd in enumerate(ref.nodes):
        g = n0 + i
        for k, key in (("node_tok", "tok"), ("node_frame", "frame"), ("node_parent", "parent")):
            if int(after[k][s, g]) != nd[key]:
                bad.append(f"node {g} {k} {int(after[k][s, g])} != {nd[key]}")
        worst.add("node_lp", after["node_lp"][s, g], nd["lp"], nd["B"])
        for q, name in enumerate(STAT_NAMES):
            worst.add(name, after["node_stats"][s, g, q], nd["stats"][q], nd["Bstats"][q])
    for k in NODE_KEYS:      # nodes outside [n0, n1) keep their bytes
        if (after[k][s, :n0].tobytes() != before[k][s, :n0].tobytes()
                or after[k][s, n1:].tobytes() != before[k][s, n1:].tobytes()):
            bad.append(f"{k}: a node outside [{n0}, {n1}) changed")
    return bad


def stream_bytes(st: dict, s: int) -> bytes:
    return b"".join(st[k][s].tobytes() for k in sorted(st))


def compare_j(case_jfmt: int, D: int, rows: int, J_before: np.ndarray, J_after: np.ndarray,
              expect: Dict[int, Tuple[np.ndarray, np.ndarray]], worst: Worst) -> List[str]:
    """expect: J row -> (reference, bound); every element of no expected row keeps its bytes"""
    bad = []
    esz = 4 if case_jfmt == 0 else 2
    touched = np.zeros(J_after.size // esz, dtype=bool)
    for row, (ref, bound) in expect.items():
        got = j_decode_row(J_after, case_jfmt, rows, D, row)
        worst.add("J", got, ref, bound)
        for o in j_element_offsets(case_jfmt, rows, D, row):
            touched[o] = True
    view = np.uint32 if esz == 4 else np.uint16
    a, b = J_after.view(view), J_before.view(view)
    if not np.array_equal(a[~touched], b[~touched]):
        bad.append(f"J: {int(np.count_nonzero(a[~touched] != b[~touched]))} elements outside "
                   f"the live rows changed")
    return bad


# ------------------------------------------------------------------------------- step chains
StepFn = Callable[..., None]   # (V, beam, t, enc_len, st, logits, phrases, scores, tab) in place


@dataclass
class ChainResult:
    worst: Worst
    crc: int
    redraws: int
    max_redraws: int
    merges: int
    events: Dict[str, int]
    bad: List[str]
    final_state: dict = None
    final_hyps: list = None
    lpf_ones: int = 0


def case_graph(case: StepCase):
    if not case.hot:
        return None, None, None
    ph, sc = hotword_phrases(case.V)
    return HotwordGraph(ph, sc), ph, sc


def rows_for(case: StepCase, s: int, t: int, hyps: List[Hyp], salt: int) -> np.ndarray:
    x = craft_rows(case, s, t, hyps, salt)
    if x is not None:
        return x
    fav3 = frame_fav(case.name, s, t, salt, case.V)
    return np.stack([gen_row(case.gen, (case.name, s, t, j, h.y2, h.y1, salt), case.V, fav3)
                     for j, h in enumerate(hyps)])


def triple_merge_surgery(st: dict, hyps: List[Hyp], s: int):
    """after frame 0 (hypotheses [], [7] and two far below): the last slot made a second copy of
    [7], 0.25 nats lower -- a state no decode reaches, which makes three duplicates of one
    sequence on the next frame"""
    j = next(i for i, h in enumerate(hyps) if h.ys[-1] == 7)
    n = len(hyps) - 1
    assert j != n
    for k in SLOT_KEYS:
        st[k][s, n] = st[k][s, j]
    st["lp"][s, n] -= 0.25
    h = hyps[j]
    hyps[n] = Hyp(h.ys, float(st["lp"][s, n]), h.lpf, h.node, h.g)


def run_step_chain(case: StepCase, step: StepFn, stop_on_bad: bool = True) -> ChainResult:
    """The chain of one case from the init state, every frame compared with the reference applied
    to the state the step function was given."""
    S, H, V = case.S, case.Hmax, case.V
    el = np.asarray(case.enc_len, np.int32)
    T = int(el.max())
    graph, phrases, scores = case_graph(case)
    st = state_alloc(S, H, case.beam * T + 1)
    tab = None
    rows_j = S * H
    if case.jfmt >= 0:
        tab = table_operands(case.name, V, case.D, el)
        tab["jfmt"] = case.jfmt
        tab["J"] = np.full(j_bytes(case.jfmt, rows_j, case.D), SENT, np.uint8)
    step(V, case.beam, -1, el, st, None, phrases, scores, tab)
    worst, bad = Worst(), []
    for s in range(S):     # the init state, exactly
        want = {"lp": 0.0, "lpf": 0, "len": 2, "y1": 0, "y2": 0, "hw": 0, "node": -1}
        for k, v in want.items():
            if not np.all(st[k][s] == v):
                bad.append(f"init s{s} {k}")
        if st["nh"][s] != 1 or st["node_count"][s] != 0:
            bad.append(f"init s{s} nh / node_count")
    if tab is not None:
        expect = {s * H: j_reference(tab["enc"][tab["enc_off"][s]], tab["a"][0], tab["b"][0], case.jfmt)
                  for s in range(S) if el[s] > 0}
        bad += [f"init {m}" for m in compare_j(case.jfmt, case.D, rows_j,
                                               np.full_like(tab["J"], SENT), tab["J"], expect, worst)]
    hyps = [init_hyps(graph) for _ in range(S)]
    crc, redraws, max_red, merges, lpf_ones = state_crc(st), 0, 0, 0, 0
    events: Dict[str, int] = {}
    for t in range(T):
        if bad and stop_on_bad:
            break
        if case.craft == "triple_merge" and t == 1:
            for s in range(S):
                if t < el[s]:
                    triple_merge_surgery(st, hyps[s], s)
        logits = np.zeros((S, H, V), np.float32)
        refs: List[Optional[FrameRef]] = [None] * S
        for s in range(S):
            if t >= el[s]:
                continue
            for j, h in enumerate(hyps[s]):     # the scores the step is given
                h.lp, h.lpf = float(st["lp"][s, j]), int(st["lpf"][s, j])
            n = len(hyps[s])
            for salt in range(MAX_REDRAWS + 1):
                rows = rows_for(case, s, t, hyps[s], salt)
                ref = frame_reference(hyps[s], rows, case.beam, t, graph, int(st["node_count"][s]))
                if not ref.unsafe:
                    break
            else:
                bad.append(f"t{t} s{s}: more than {MAX_REDRAWS} redraws ({ref.unsafe})")
                break
            redraws += salt
            max_red = max(max_red, salt)
            logits[s, :n] = rows
            if n < H:   # rows of dead slots: the kernel loads them
                logits[s, n:] = np.random.default_rng(seed_of(case.name, s, t, "dead")) \
                    .standard_normal((H - n, V)).astype(np.float32)
            refs[s] = ref
        before = state_copy(st)
        if tab is not None:
            tab["J"][:] = SENT
        step(V, case.beam, t, el, st, logits, phrases, scores, tab)
        crc = zlib.crc32(stream_bytes(st, 0), crc)
        expect = {}
        for s in range(S):
            if refs[s] is None:    # t >= enc_len: byte-identical
                if stream_bytes(st, s) != stream_bytes(before, s):
                    bad.append(f"t{t} s{s}: a finished stream changed")
                continue
            ref = refs[s]
            msgs = compare_stream_frame(before, st, s, ref, graph, worst)
            bad += [f"t{t} s{s}: {m}" for m in msgs]
            merges += ref.merges
            lpf_ones += sum(h.lpf for h in ref.hyps)
            for k, v in ref.events.items():
                events[k] = events.get(k, 0) + v
            hyps[s] = ref.hyps
            if tab is not None and t + 1 < el[s]:
                e = tab["enc"][tab["enc_off"][s] + t + 1]
                for j, h in enumerate(ref.hyps):
                    expect[s * H + j] = j_reference(e, tab["a"][h.y2], tab["b"][h.y1], case.jfmt)
        if tab is not None:
            bad += [f"t{t}: {m}" for m in compare_j(case.jfmt, case.D, rows_j,
                                                    np.full_like(tab["J"], SENT), tab["J"], expect, worst)]
            crc = zlib.crc32(tab["J"].tobytes(), crc)
    bad += [f"{k} ratio {v:.3f}" for k, v in worst.bad()]
    return ChainResult(worst, state_crc(st, [np.uint32(crc)]), redraws, max_red, merges, events, bad,
                       st, hyps, lpf_ones)


def check_case_claims(case: StepCase, r: ChainResult, bad: list):
    """a case reached what it was built to reach (counted by the reference)"""
    ev, miss = r.events, []
    live = sum(1 for n in case.enc_len if n > 1)
    if case.craft == "flat" and ev.get("tie_same_row", 0) < live * case.beam:
        miss.append("the best k + 1 of the flat frame are not one row's equal candidates")
    if case.craft == "plateau" and ev.get("tie_same_row", 0) < live * 3:
        miss.append("the plateau does not straddle the k-th rank")
    if case.craft == "equal_rows" and not ev.get("tie_cross_row"):
        miss.append("no tie across two rows")
    if case.craft == "cutoff_merge" and (r.merges < live or r.lpf_ones):
        miss.append("no merge in the cutoff branch")
    if case.craft == "triple_merge" and r.merges < 2 * live:
        miss.append("no merge of three duplicates")
    if case.craft == "" and case.gen == "peaked" and case.beam >= 8 and not (r.merges and r.lpf_ones):
        miss.append("a peaked chain without a merge")
    if miss:
        bad.append((case.name, miss))


def check_greedy_claims(case, r: GreedyResult, bad: list):
    want = ["all_blank", "emit_row0", "emit_last_row", "ends_inside_window", "winner_last_float4"]
    if case.F == 8:
        want.append("emit_second_row_of_wave")
    miss = [k for k in want if not r.seen.get(k)]
    if not r.events.get("tie_same_row"):
        miss.append("tie at the top value")
    if miss:
        bad.append((case.name, "never reached: " + ", ".join(miss)))


# ------------------------------------------------------------------------------- greedy windows
@dataclass(frozen=True)
class GreedyCase:
    name: str
    V: int
    F: int
    D: int
    jfmt: int
    hot: bool = False
    gen: str = "peaked"

    @property
    def enc_len(self):
        return (30, 1, 3, self.F, self.F + 1)

    @property
    def S(self):
        return 5


def greedy_cases() -> List[GreedyCase]:
    out = []
    for F in (4, 8):
        for f in range(6):
            out.append(GreedyCase(f"greedy_V64_F{F}_{JFMT_NAMES[f]}", 64, F, 256, f))
        out.append(GreedyCase(f"greedy_V64_F{F}_hot", 64, F, 256, 0, hot=True))
        for V in (516, 2052, 4096):
            out.append(GreedyCase(f"greedy_V{V}_F{F}", V, F, 4, 0, gen="gauss" if V == 516 else "peaked"))
    return out


def greedy_row(case: GreedyCase, s: int, t: int, h: Hyp, salt: int) -> np.ndarray:
    """the logits row of frame t under context h: the step chains' generator at slot 0, with the
    crafted frames of stream 0 -- t = 5: the top value twice, the smaller index wins; t = 9: the
    winner in the last float4; then a window whose last row emits, an all-blank window and a
    window whose row 0 emits"""
    V, F = case.V, case.F
    x = gen_row(case.gen, (case.name, s, t, 0, h.y2, h.y1, salt), V, frame_fav(case.name, s, t, salt, V))
    if s != 0:
        return x
    if t == 5:
        x[V - 2] = x[7] = np.float32(x.max() + 1.0)
    elif t == 9:                               # the next window starts at frame 10
        x[V - 1] = np.float32(x.max() + 2.0)
    elif t in (10 + F - 1, 10 + 2 * F):        # its last row emits; after the blank window, row 0
        x[3] = np.float32(x.max() + 3.0)
    elif 10 <= t < 10 + 2 * F:                 # blank rows: F - 1 of them, then a whole window
        x[0] = np.float32(x.max() + 12.0)
    return x


@dataclass
class GreedyResult:
    worst: Worst
    crc: int
    bad: List[str]
    redraws: int
    max_redraws: int
    seen: Dict[str, int]
    salts: Dict[tuple, int]
    final_state: dict
    events: Dict[str, int]
    steps: int


def run_greedy_chain(case, step: Callable[..., None]) -> GreedyResult:
    """Super-steps until active == 0, each compared with the reference window applied to the state
    the step was given.  step(V, F, init, parity, enc_len, t_cur, active, st, logits, tab, phrases,
    scores) updates st, t_cur, active and tab["J"] in place."""
    S, F, V, D = case.S, case.F, case.V, case.D
    el = np.asarray(case.enc_len, np.int32)
    graph, phrases, scores = case_graph(case)
    st = state_alloc(S, 1, int(el.max()) + 1)
    tab = table_operands(case.name, V, D, el)
    tab["jfmt"] = case.jfmt
    rows_j = S * F
    tab["J"] = np.full(j_bytes(case.jfmt, rows_j, D), SENT, np.uint8)
    t_cur = np.full(S, 0x6b6b6b6b, np.int32)
    active = np.full(2, 0x6b6b6b6b, np.int32)
    worst, bad = Worst(), []
    step(V, F, 2, 0, el, t_cur, active, st, None, tab, phrases, scores)
    if not (np.all(t_cur == 0) and np.all(active == 0)):
        bad.append(f"init: t_cur {t_cur} active {active}")
    expect = {}
    for s in range(S):
        for f in range(min(F, int(el[s]))):
            expect[s * F + f] = j_reference(tab["enc"][tab["enc_off"][s] + f], tab["a"][0],
                                            tab["b"][0], case.jfmt)
    bad += [f"init {m}" for m in compare_j(case.jfmt, D, rows_j, np.full_like(tab["J"], SENT),
                                           tab["J"], expect, worst)]
    hyps = [init_hyps(graph)[0] for _ in range(S)]
    crc, redraws, max_red, k = state_crc(st), 0, 0, 0
    seen: Dict[str, int] = {}
    events: Dict[str, int] = {}
    salts: Dict[tuple, int] = {}

    def note(name):
        seen[name] = seen.get(name, 0) + 1

    while True:
        if bad or k > int(el.max()):
            break
        live = [s for s in range(S) if t_cur[s] < el[s]]
        if not live:
            break
        logits = np.zeros((S, F, V), np.float32)
        plan = {}
        for s in live:
            t0 = int(t_cur[s])
            nf = min(F, int(el[s]) - t0)
            if nf < F:
                note("ends_inside_window")
            h = hyps[s]
            h.lp, h.lpf = float(st["lp"][s, 0]), int(st["lpf"][s, 0])
            cur = Hyp(h.ys, h.lp, h.lpf, h.node, h.g)
            E = 0.0                       # the bound carried from the rows before
            out = None
            for f in range(nf):
                key = (s, t0 + f, cur.y2, cur.y1)
                for salt in range(MAX_REDRAWS + 1):
                    row = greedy_row(case, s, t0 + f, cur, salt)
                    ref = frame_reference([cur], row[None, :], 1, t0 + f, graph,
                                          int(st["node_count"][s]))
                    if not ref.unsafe:
                        break
                else:
                    bad.append(f"k{k} s{s} f{f}: more than {MAX_REDRAWS} redraws ({ref.unsafe})")
                    break
                redraws += salt
                max_red = max(max_red, salt)
                salts[key] = salt
                logits[s, f] = row
                if out is not None:
                    continue              # rows behind the emission: read, never used
                nh = ref.hyps[0]
                nh.B += E
                if ref.nodes:
                    nd = ref.nodes[0]
                    nd["B"] += 2.0 * E
                    out = (f, nh, nd)
                    for kk, v in ref.events.items():
                        events[kk] = events.get(kk, 0) + v
                else:
                    E = nh.B
                    cur = Hyp(cur.ys, nh.lp, 0, cur.node, cur.g, nh.B)
            if out is None:
                note("all_blank")
                plan[s] = (t0 + nf, cur, None, cur.B if nf else 0.0)
            else:
                f, nh, nd = out
                note("emit_row0" if f == 0 else "emit_last_row" if f == F - 1 else "emit_mid")
                if f >= 4:
                    note("emit_second_row_of_wave")
                if nd["tok"] >= V - 4:
                    note("winner_last_float4")
                plan[s] = (t0 + f + 1, nh, nd, nh.B)
        if bad:
            break
        before = state_copy(st)
        t_before = t_cur.copy()
        tab["J"][:] = SENT
        parity = k & 1
        step(V, F, 0, parity, el, t_cur, active, st, logits, tab, phrases, scores)
        crc = zlib.crc32(stream_bytes(st, 0) + t_cur.tobytes(), crc)
        expect = {}
        n_active = 0
        for s in range(S):
            if s not in plan:
                if stream_bytes(st, s) != stream_bytes(before, s) or t_cur[s] != t_before[s]:
                    bad.append(f"k{k} s{s}: a finished stream changed")
                continue
            t_new, nh, nd, B = plan[s]
            if int(t_cur[s]) != t_new:
                bad.append(f"k{k} s{s}: t_cur {int(t_cur[s])} != {t_new}")
            fr = FrameRef([Hyp(nh.ys, nh.lp, 0, nh.node, nh.g, B)], [nd] if nd else [], "")
            bad += [f"k{k} s{s}: {m}" for m in compare_stream_frame(before, st, s, fr, graph, worst)]
            hyps[s] = fr.hyps[0]
            if t_new < el[s]:
                n_active += 1
                for f in range(min(F, int(el[s]) - t_new)):
                    expect[s * F + f] = j_reference(tab["enc"][tab["enc_off"][s] + t_new + f],
                                                    tab["a"][nh.y2], tab["b"][nh.y1], case.jfmt)
        if int(active[parity]) != n_active or int(active[parity ^ 1]) != 0:
            bad.append(f"k{k}: active {active} != {n_active} at parity {parity}")
        bad += [f"k{k}: {m}" for m in compare_j(case.jfmt, D, rows_j, np.full_like(tab["J"], SENT),
                                                tab["J"], expect, worst)]
        crc = zlib.crc32(tab["J"].tobytes(), crc)
        active[parity] = 0       # the next step adds to the counter the one after zeroes
        k += 1
        if n_active == 0:
            break
    if not bad and any(t_cur[s] < el[s] for s in range(S)):
        bad.append("the chain did not finish")
    bad += [f"{kk} ratio {v:.3f}" for kk, v in worst.bad()]
    return GreedyResult(worst, state_crc(st, [np.uint32(crc)]), bad, redraws, max_red, seen, salts,
                        st, events, k)


def run_greedy_as_steps(case, salts: Dict[tuple, int], step: StepFn) -> dict:
    """the greedy case's frames through the beam-1 step function, with the rows (and salts) the
    window chain used: the state it ends in"""
    S, V = case.S, case.V
    el = np.asarray(case.enc_len, np.int32)
    graph, phrases, scores = case_graph(case)
    st = state_alloc(S, 1, int(el.max()) + 1)
    step(V, 1, -1, el, st, None, phrases, scores, None)
    ys = [(0, 0)] * S
    for t in range(int(el.max())):
        logits = np.zeros((S, 1, V), np.float32)
        for s in range(S):
            if t >= el[s]:
                continue
            y2, y1 = int(st["y2"][s, 0]), int(st["y1"][s, 0])
            h = Hyp((y2, y1), 0.0, 0, -1)
            logits[s, 0] = greedy_row(case, s, t, h, salts[(s, t, y2, y1)])
        step(V, 1, t, el, st, logits, phrases, scores, None)
    return st


# ------------------------------------------------------------------------------- the final pick
def final_reference(st: dict, s: int, graph: Optional[HotwordGraph], out_cap: int,
                    length_norm: bool = True, keep_newest: bool = True):
    n = int(st["nh"][s])
    best, best_v = 0, -math.inf
    for h in range(n):
        lp = float(st["lp"][s, h])
        if graph is not None:
            lp += -graph.nodes[int(st["hw"][s, h])].node_score
        v = lp / float(max(int(st["len"][s, h]), 1)) if length_norm else lp
        if h == 0 or v > best_v:
            best, best_v = h, v
    chain = []
    nd = int(st["node"][s, best])
    while nd >= 0:
        chain.append(nd)
        nd = int(st["node_parent"][s, nd])
    chain.reverse()
    if len(chain) > out_cap:
        chain = chain[-out_cap:] if keep_newest else chain[:out_cap]
    return best, chain


@dataclass(frozen=True)
class FinalCase:
    name: str
    nodes: int
    chain: int
    out_cap: int
    kind: str = "chain"


def final_cases() -> List[FinalCase]:
    return [FinalCase("final_5_of_40", 40, 5, 16),
            FinalCase("final_2049_of_8192_cap4096", 8192, 2049, 4096),
            FinalCase("final_8193_global", 8193, 37, 64),
            FinalCase("final_300_cap100_staged", 600, 300, 100),
            FinalCase("final_300_cap100_global", 8200, 300, 100),
            FinalCase("final_no_emission", 12, 0, 8),
            FinalCase("final_length_norm", 40, 5, 16, "length_norm"),
            FinalCase("final_hotword_finalize", 40, 5, 16, "hotword"),
            FinalCase("final_equal_scores", 40, 5, 16, "equal")]


def final_state(case: FinalCase):
    """a crafted state of 3 streams x 4 slots: the case's stream in the middle, between a stream
    with its own small pool and one with no emission"""
    rng = np.random.default_rng(seed_of(case.name))
    S, H, cap = 3, 4, case.nodes + 3
    st = state_alloc(S, H, cap)
    for k in SLOT_KEYS:
        st[k][...] = 0
    st["node"][...] = -1
    st["len"][...] = 2
    st["nh"][:] = (2, 3, 1)
    st["node_count"][:] = (3, case.nodes, 0)
    for s in range(S):
        n = int(st["node_count"][s])
        st["node_tok"][s, :n] = rng.integers(1, 60, n)
        st["node_frame"][s, :n] = np.arange(n)
        st["node_lp"][s, :n] = -rng.uniform(0.1, 3.0, n)
        st["node_stats"][s, :n] = rng.uniform(0.0, 1.0, (n, 4)).astype(np.float32)
        st["node_parent"][s, :n] = -1
    # stream 0: slot 1 wins with a chain 0 <- 2
    st["node_parent"][0, 2] = 0
    st["lp"][0, :2] = (-9.0, -4.0)
    st["len"][0, :2] = (4, 4)
    st["node"][0, :2] = (1, 2)
    # stream 1: the winning chain of `chain` nodes spread over the pool, every other node on
    # side branches hanging off it
    n = case.nodes
    if case.chain:
        ids = np.sort(rng.choice(n, case.chain, replace=False))
        on = np.zeros(n, bool)
        on[ids] = True
        prev = -1
        for i in range(n):
            if on[i]:
                st["node_parent"][1, i] = prev
                prev = i
            else:
                st["node_parent"][1, i] = int(rng.integers(-1, i)) if i else -1
        tip = int(ids[-1])
    else:
        for i in range(n):
            st["node_parent"][1, i] = int(rng.integers(-1, i)) if i else -1
        tip = -1
    other = int(rng.integers(0, n))
    st["lp"][1, :3] = (-30.0, -12.0, -20.0)
    st["len"][1, :3] = (case.chain + 2, case.chain + 2, case.chain + 2)
    st["node"][1, :3] = (other, tip, other)
    phrases = scores = None
    if case.kind == "length_norm":
        # slot 0: lp -10 over 10 entries (-1.0); slot 1: lp -8 over 4 entries (-2.0): the
        # normalised pick is slot 0, the raw one slot 1
        st["lp"][1, :3] = (-10.0, -8.0, -50.0)
        st["len"][1, :3] = (10, 4, 4)
        st["node"][1, :3] = (tip, other, other)
    if case.kind == "hotword":
        # slot 0 sits inside an unfinished phrase: finalize takes its 4.5 back and slot 1 wins
        phrases, scores = [[3, 5, 7]], [2.25]
        st["lp"][1, :3] = (-6.0, -8.0, -50.0)
        st["len"][1, :3] = (4, 4, 4)
        st["hw"][1, :3] = (2, 0, 0)
        st["node"][1, :3] = (other, tip, other)
    if case.kind == "equal":
        st["lp"][1, :3] = (-12.0, -12.0, -12.0)
        st["len"][1, :3] = (6, 6, 6)
        st["node"][1, :3] = (tip, other, other)
    return st, phrases, scores


def check_final(case: FinalCase, st: dict, out: dict, graph) -> List[str]:
    bad = []
    for s in range(st["lp"].shape[0]):
        best, chain = final_reference(st, s, graph, case.out_cap)
        c = len(chain)
        if int(out["count"][s]) != c:
            bad.append(f"s{s} count {int(out['count'][s])} != {c}")
            continue
        for ok, sk in (("tok", "node_tok"), ("frame", "node_frame"), ("lp", "node_lp"),
                       ("stats", "node_stats")):
            if out[ok][s, :c].tobytes() != st[sk][s, chain].tobytes():
                bad.append(f"s{s} {ok} is not the chain's {sk}")
            if not np.all(out[ok][s, c:].view(np.uint8) == SENT):
                bad.append(f"s{s} {ok}: written beyond count")
    return bad


# ------------------------------------------------------------------------------- the DFA
def check_dfa(dfa: dict, graph: HotwordGraph, V: int) -> List[str]:
    """build_hotword_dfa's tables against HotwordGraph, state i = the i-th node created"""
    bad = []
    ns = len(graph.nodes)
    if dfa["node_score"].shape[0] != ns:
        return [f"{dfa['node_score'].shape[0]} states != {ns}"]
    trie = sorted({nd.tok for nd in graph.nodes if nd.tok >= 0})
    for v in range(V):
        if (dfa["tok2cls"][v] >= 0) != (v in trie):
            bad.append(f"tok2cls[{v}]")
    for i, nd in enumerate(graph.nodes):
        if dfa["node_score"][i] != nd.node_score:
            bad.append(f"node_score[{i}]")
        for v in trie:
            d, nx = graph.step(nd, v)
            c = int(dfa["tok2cls"][v])
            if dfa["delta"][i, c] != d or graph.nodes[int(dfa["next"][i, c])] is not nx:
                bad.append(f"transition ({i}, {v})")
    return bad


# ------------------------------------------------------------------------------- the emulation
M64 = (1 << 64) - 1
HASH0 = 0x6a09e667f3bcc908


def hash_push(h: int, tok: int) -> int:
    x = h ^ ((0x9e3779b97f4a7c15 + tok + (h << 6) + (h >> 2)) & M64)
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


DEFECTS = ("tie_larger_index", "no_second_row", "delta_before_topk", "unk_steps", "merge_last",
           "lpf_never", "node_lp_merged", "j_candidate_index", "greedy_j_from_t0",
           "final_no_length_norm", "final_keep_oldest")


def emu_row(x: np.ndarray, lp: float, lpf: int):
    """one row as the kernels compute it, in numpy f32 with numpy's own summation order:
    (candidate scores f32 [V], the four statistics f32)"""
    f = np.float32
    m1 = x.max()
    d = x - m1
    e = np.exp(d)
    se = f(np.sum(e[::-1]))
    ls = f(np.log(se))
    lpv = (d - ls).astype(f)
    cand = (lpv.astype(np.float64) + lp).astype(f) if lpf else lpv + f(lp)
    e1 = f(np.sum((e * d)[::-1]))
    e3 = f(np.sum(np.exp(d * f(1.0 / 3.0))[::-1]))
    m2 = np.partition(x, -2)[-2] if x.size > 1 else f(-np.inf)
    stats = np.array([ls - e1 / se, e3 * np.exp2(-np.log2(se) * f(1.0 / 3.0)), f(1.0) / se,
                      np.exp(f(m2 - m1)) / se], dtype=f)
    return cand, stats


def emu_j_write(tab: dict, rows: int, row: int, enc_row: np.ndarray, y2: int, y1: int):
    f = np.float32
    z = enc_row.astype(f) + (tab["a"][y2].astype(f) + tab["b"][y1].astype(f))
    x = np.tanh(z).astype(f)
    imgs = j_encode_row(x, tab["jfmt"])
    offs = j_element_offsets(tab["jfmt"], rows, tab["D"], row)
    view = tab["J"].view(np.float32 if tab["jfmt"] == 0 else np.uint16)
    for img, o in zip(imgs, offs):
        view[o] = img


def make_emu_step(defect: str = "") -> StepFn:
    """The step entry point's behaviour in numpy (f32 where the kernel is f32), optionally with one
    defect.  `hw` is the index of the HotwordGraph node."""
    assert defect == "" or defect in DEFECTS

    def step(V, beam, t, enc_len, st, logits, phrases, scores, tab):
        S, H = st["lp"].shape
        graph = HotwordGraph(phrases, scores) if phrases else None
        if t < 0:
            st["lp"][...] = 0.0
            for k in ("lpf", "len", "y1", "y2", "hw", "node"):
                st[k][...] = {"len": 2, "node": -1}.get(k, 0)
            st["hash"][...] = HASH0
            st["nh"][...] = 1
            st["node_count"][...] = 0
            if tab is not None:
                for s in range(S):
                    if enc_len[s] > 0:
                        emu_j_write(tab, S * H, s * H, tab["enc"][tab["enc_off"][s]], 0, 0)
            return
        for s in range(S):
            if t >= enc_len[s]:
                continue
            n = int(st["nh"][s])
            cands, stats = [], []
            for h in range(n):
                hs = h - 8 if defect == "no_second_row" and h >= 8 else h
                c, q = emu_row(logits[s, hs], float(st["lp"][s, hs]), int(st["lpf"][s, hs]))
                if defect == "delta_before_topk" and graph is not None:
                    g = graph.nodes[int(st["hw"][s, h])]
                    c = c.astype(np.float64)
                    for v in range(1, V):
                        if v != UNK:
                            c[v] += graph.step(g, v)[0]
                cands.append(c)
                stats.append(q)
            flat = np.concatenate(cands)
            k = min(beam, n * V)
            if defect == "tie_larger_index":
                order = np.lexsort((-np.arange(flat.size), -flat))[:k]
            else:
                order = top_candidates(flat, k)
            recs = []   # [hash, len, lp, lpf, y1, y2, hw, node, emit-dict or None, cand index]
            by_key: Dict[tuple, int] = {}
            for c, idx in enumerate(order):
                h, v = divmod(int(idx), V)
                score = float(flat[idx])
                hh, ln = int(st["hash"][s, h]), int(st["len"][s, h])
                y1, y2, hw = int(st["y1"][s, h]), int(st["y2"][s, h]), int(st["hw"][s, h])
                emit = None
                if v != BLANK:
                    if graph is not None and (v != UNK or defect == "unk_steps"):
                        dlt, g = graph.step(graph.nodes[hw], v)
                        if defect != "delta_before_topk":
                            score += dlt
                        hw = graph_index(graph, g)
                    hh, ln, y2, y1 = hash_push(hh, v), ln + 1, y1, v
                    cand_lp = float(cands[h][v]) if defect != "delta_before_topk" else \
                        float(emu_row(logits[s, h], float(st["lp"][s, h]), int(st["lpf"][s, h]))[0][v])
                    emit = {"tok": v, "parent": int(st["node"][s, h]),
                            "lp": cand_lp - float(st["lp"][s, h]), "stats": stats[h], "cand_lp": cand_lp,
                            "plp": float(st["lp"][s, h])}
                key = (ln, hh)
                rec = [hh, ln, score, 0, y1, y2, hw, int(st["node"][s, h]), emit, c]
                if key in by_key:
                    j = by_key[key]
                    r = recs[j]
                    lp, lpf, _ = log_add_f(r[2], r[3], score, 0)
                    if defect == "merge_last":
                        rec[2], rec[3] = lp, lpf
                        recs[j] = rec
                    else:
                        r[2], r[3] = lp, lpf
                else:
                    by_key[key] = len(recs)
                    recs.append(rec)
            if defect == "merge_last":
                recs.sort(key=lambda r: r[9])
            base = int(st["node_count"][s])
            ne = 0
            for j, r in enumerate(recs):
                node = r[7]
                if r[8] is not None:
                    g = base + ne
                    ne += 1
                    e = r[8]
                    st["node_tok"][s, g], st["node_frame"][s, g] = e["tok"], t
                    st["node_parent"][s, g] = e["parent"]
                    st["node_lp"][s, g] = (r[2] - e["plp"]) if defect == "node_lp_merged" else e["lp"]
                    st["node_stats"][s, g] = e["stats"]
                    node = g
                st["hash"][s, j], st["len"][s, j], st["lp"][s, j] = r[0], r[1], r[2]
                st["lpf"][s, j] = 0 if defect == "lpf_never" else r[3]
                st["y1"][s, j], st["y2"][s, j], st["hw"][s, j], st["node"][s, j] = r[4], r[5], r[6], node
                if tab is not None and t + 1 < enc_len[s]:
                    row = s * H + (r[9] if defect == "j_candidate_index" else j)
                    emu_j_write(tab, S * H, row, tab["enc"][tab["enc_off"][s] + t + 1], r[5], r[4])
            st["nh"][s] = len(recs)
            st["node_count"][s] = base + ne
    return step


def make_emu_greedy(defect: str = ""):
    estep = make_emu_step(defect)

    def step(V, F, init, parity, enc_len, t_cur, active, st, logits, tab, phrases, scores):
        S = st["lp"].shape[0]
        if init:
            estep(V, 1, -1, enc_len, st, None, phrases, scores, None)
            t_cur[:] = 0
            active[:] = 0
            for s in range(S):
                for f in range(min(F, int(enc_len[s]))):
                    emu_j_write(tab, S * F, s * F + f, tab["enc"][tab["enc_off"][s] + f], 0, 0)
            if init == 2:
                return
        active[parity ^ 1] = 0
        for s in range(S):
            t0, T = int(t_cur[s]), int(enc_len[s])
            if t0 >= T:
                continue
            nf = min(F, T - t0)
            one = {k: v[s:s + 1].copy() for k, v in st.items()}
            t_new = t0 + nf
            for f in range(nf):
                nc = int(one["node_count"][0])
                # between rows the kernel carries the f32 score
                one["lp"][0, 0] = float(np.float32(one["lp"][0, 0])) if f else one["lp"][0, 0]
                estep(V, 1, t0 + f, np.array([T], np.int32), one, logits[s:s + 1, f:f + 1],
                      phrases, scores, None)
                if int(one["node_count"][0]) != nc:
                    t_new = t0 + f + 1
                    break
            one["lpf"][0, 0] = 0
            for k in st:
                st[k][s] = one[k][0]
            t_cur[s] = t_new
            if t_new < T:
                active[parity] += 1
                src = t0 if defect == "greedy_j_from_t0" else t_new
                for f in range(min(F, T - t_new)):
                    e = tab["enc"][tab["enc_off"][s] + min(src + f, T - 1)]
                    emu_j_write(tab, S * F, s * F + f, e, int(st["y2"][s, 0]), int(st["y1"][s, 0]))
    return step


def emu_final(st: dict, graph, out_cap: int, defect: str = "") -> dict:
    S = st["lp"].shape[0]
    out = {"tok": np.empty((S, out_cap), np.int32), "frame": np.empty((S, out_cap), np.int32),
           "lp": np.empty((S, out_cap), np.float64), "stats": np.empty((S, out_cap, 4), np.float32),
           "count": np.empty((S,), np.int32)}
    for a in out.values():
        a.view(np.uint8)[...] = SENT
    for s in range(S):
        _, chain = final_reference(st, s, graph, out_cap, defect != "final_no_length_norm",
                                   defect != "final_keep_oldest")
        c = len(chain)
        out["count"][s] = c
        for ok, sk in (("tok", "node_tok"), ("frame", "node_frame"), ("lp", "node_lp"),
                       ("stats", "node_stats")):
            out[ok][s, :c] = st[sk][s, chain]
    return out
