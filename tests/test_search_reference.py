"""tests/search_reference.py without a GPU.

(a) the float64 one-frame reference, chained from the initial hypothesis over the committed search
    goldens, and the final pick give the reference program's tokens, frames and log-probs;
(b) a numpy emulation of the kernels' arithmetic (f32 log-softmax in numpy's summation order, f32
    score add, f64 add when lpf, f32 statistics, tanh in f32, the J formats' rounding) stays inside
    every bound on every GPU case, every exact field equal, the redraw cap held on every chain;
(c) eleven single-defect emulations each leave a bound or fail an exact field in every case family
    they apply to.
"""
import glob
import json
import os

import numpy as np
import pytest

import search_reference as sr
from oracle.search import HotwordGraph, beam_search
from synth_case import case_config, dec_joiner_weights, enc_out_for, np_decoder, np_joiner

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GOLDENS = sorted(glob.glob(os.path.join(GOLD, "search_*.json")))


# ------------------------------------------------------------------ (a) reference = oracle
def chain_reference(enc, w, beam, graph):
    """frame_reference from the initial hypothesis, its own float64 scores carried; returns the
    state and node pool the final pick reads"""
    hyps = sr.init_hyps(graph)
    pool = []
    for t in range(enc.shape[0]):
        ctx = np.array([[h.y2, h.y1] for h in hyps], dtype=np.int64)
        rows = np_joiner(w, np.repeat(enc[t:t + 1], len(hyps), axis=0), np_decoder(w, ctx))
        ref = sr.frame_reference(hyps, rows.astype(np.float32), beam, t, graph, len(pool))
        pool += ref.nodes
        hyps = ref.hyps
    n = len(hyps)
    st = {"nh": np.array([n]), "lp": np.array([[h.lp for h in hyps]]),
          "hw": np.array([[sr.graph_index(graph, h.g) for h in hyps]]),
          "len": np.array([[len(h.ys) for h in hyps]]), "node": np.array([[h.node for h in hyps]]),
          "node_parent": np.array([[nd["parent"] for nd in pool] + [-1]])}
    return st, pool


def test_reference_chain_and_final_pick_give_the_goldens():
    frames_total, ties_total = 0, 0
    for path in GOLDENS:
        with open(path) as f:
            g = json.load(f)
        cfg = case_config(g["kind"])
        w = dec_joiner_weights(g["kind"], g["seed"])
        enc = enc_out_for(g["kind"], g["seed"], g["T"], cfg.joiner_dim)
        graph = HotwordGraph(g["phrases"], g["scores"]) if g["hotwords"] else None
        ties = []
        beam_search(enc, lambda y: np_decoder(w, y), lambda e, d: np_joiner(w, e, d), g["beam"],
                    graph, ties=ties)
        frames_total += g["T"]
        ties_total += len(ties)
        if ties:   # the kept set of such a frame is introselect's, not a stable order: skipped
            continue
        st, pool = chain_reference(enc, w, g["beam"], graph)
        _, chain = sr.final_reference(st, 0, graph, g["T"])
        name = os.path.basename(path)
        assert [pool[i]["tok"] for i in chain] == g["token_ids"], name
        assert [pool[i]["frame"] for i in chain] == g["frames"], name
        np.testing.assert_allclose([pool[i]["lp"] for i in chain], g["ys_log_probs"], rtol=0,
                                   atol=5e-4, err_msg=name)
    assert ties_total * 100 < frames_total, (ties_total, frames_total)


# ------------------------------------------------------------------ (b) the bounds hold
STEP_GROUPS = {"chains": sr.chain_cases, "hotwords": sr.hotword_cases, "crafted": sr.crafted_cases,
               "table": sr.table_cases}


@pytest.mark.parametrize("group", sorted(STEP_GROUPS))
def test_emulated_step_chains_stay_inside_the_bounds(group):
    bad, events = [], {}
    for c in STEP_GROUPS[group]():
        r = sr.run_step_chain(c, sr.make_emu_step())
        print(f"{c.name}: {r.worst} redraws {r.redraws} (max {r.max_redraws}) merges {r.merges}")
        assert r.max_redraws <= sr.MAX_REDRAWS
        if r.bad:
            bad.append((c.name, r.bad[:4]))
        for k, v in r.events.items():
            events[k] = events.get(k, 0) + v
        sr.check_case_claims(c, r, bad)
    assert not bad, bad
    if group == "hotwords":
        for kind in ("child", "fail_link", "reset", "full_match"):
            assert events.get(kind, 0) > 0, (kind, events)


def test_emulated_greedy_windows_stay_inside_the_bounds():
    bad, seen = [], {}
    for c in sr.greedy_cases():
        r = sr.run_greedy_chain(c, sr.make_emu_greedy())
        print(f"{c.name}: {r.worst} redraws {r.redraws} steps {r.steps} {r.seen}")
        assert r.max_redraws <= sr.MAX_REDRAWS
        if r.bad:
            bad.append((c.name, r.bad[:4]))
        st2 = sr.run_greedy_as_steps(c, r.salts, sr.make_emu_step())
        diff = [k for k in st2 if st2[k].tobytes() != r.final_state[k].tobytes()]
        if diff:
            bad.append((c.name, "windows != frame-by-frame steps", diff))
        sr.check_greedy_claims(c, r, bad)
        for k, v in r.seen.items():
            seen[k] = seen.get(k, 0) + v
    assert not bad, bad


def test_emulated_final_pick_is_exact():
    for c in sr.final_cases():
        st, ph, sc = sr.final_state(c)
        graph = HotwordGraph(ph, sc) if ph else None
        assert not sr.check_final(c, st, sr.emu_final(st, graph, c.out_cap), graph), c.name


def test_statistics_bounds_stay_below_the_end_to_end_tolerances():
    worst = np.zeros(4)
    for V in sr.VOCABS:
        for gen in ("gauss", "peaked"):
            for i in range(6):
                x = sr.gen_row(gen, ("ceiling", V, i), V, tuple(sr.favoured(V)[:3]))
                _, B = sr.stats_reference(x, sr.row_terms(x))
                worst = np.maximum(worst, sr.normalised_stat_bounds(B, V))
        for x in (np.zeros(V, np.float32), np.r_[0.0, np.full(V - 1, -100.0)].astype(np.float32)):
            _, B = sr.stats_reference(x, sr.row_terms(x))
            worst = np.maximum(worst, sr.normalised_stat_bounds(B, V))
    print("normalised bounds (tsallis, margin, entropy, top1):", worst)
    assert np.all(worst[:3] <= sr.CEIL_ENTROPY_FIELDS) and worst[3] <= sr.CEIL_TOP1


# ------------------------------------------------------------------ (c) defects are caught
STEP_DEFECTS = {
    # defect: the case families it can show in
    "tie_larger_index": {"crafted": ("flat", "plateau", "equal_rows")},
    "no_second_row": {"chains": None, "hotwords": None, "crafted": None, "table": None},
    "delta_before_topk": {"hotwords": None},
    "unk_steps": {"hotwords": None},
    "merge_last": {"chains": None, "hotwords": None, "crafted": ("triple_merge", "cutoff_merge"),
                   "table": None},
    "lpf_never": {"chains": None, "hotwords": None, "crafted": ("triple_merge",), "table": None},
    "node_lp_merged": {"chains": None, "hotwords": None, "crafted": ("triple_merge",), "table": None},
    "j_candidate_index": {"table": None},
}


def family_cases(group, crafts, defect):
    cases = STEP_GROUPS[group]()
    if crafts is not None:
        cases = [c for c in cases if c.craft in crafts]
    if defect == "no_second_row":
        cases = [c for c in cases if c.beam > 8]
    if defect in ("merge_last", "lpf_never", "node_lp_merged", "j_candidate_index") and crafts is None:
        cases = [c for c in cases if c.gen == "peaked" and c.beam >= 4]
    return sorted(cases, key=lambda c: c.V * c.beam)   # the cheap ones first


@pytest.mark.parametrize("defect", sorted(STEP_DEFECTS))
def test_step_defect_is_caught_in_every_family_it_applies_to(defect):
    for group, crafts in STEP_DEFECTS[defect].items():
        cases = family_cases(group, crafts, defect)
        assert cases, (defect, group)
        caught = None
        for c in cases:
            r = sr.run_step_chain(c, sr.make_emu_step(defect))
            if r.bad:
                caught = (c.name, r.bad[0])
                break
        print(defect, group, "->", caught)
        assert caught, (defect, group, [c.name for c in cases])


def test_greedy_defects_are_caught():
    for defect in ("greedy_j_from_t0", "unk_steps"):
        cases = [c for c in sr.greedy_cases() if c.hot or defect == "greedy_j_from_t0"]
        caught = []
        for c in cases:
            r = sr.run_greedy_chain(c, sr.make_emu_greedy(defect))
            if r.bad:
                caught.append(c.name)
        print(defect, "->", caught)
        # the J defect shows in every case (every J format, every vocabulary)
        assert caught == [c.name for c in cases] if defect == "greedy_j_from_t0" else caught


def test_final_defects_are_caught():
    hit = {"final_no_length_norm": [], "final_keep_oldest": []}
    for c in sr.final_cases():
        st, ph, sc = sr.final_state(c)
        graph = HotwordGraph(ph, sc) if ph else None
        for d in hit:
            if sr.check_final(c, st, sr.emu_final(st, graph, c.out_cap, d), graph):
                hit[d].append(c.name)
    assert hit["final_no_length_norm"] == ["final_length_norm"], hit
    assert hit["final_keep_oldest"] == ["final_300_cap100_staged", "final_300_cap100_global"], hit
    # the hotword finalize and the first-maximum rule decide their cases' picks
    for name, alt in (("final_hotword_finalize", "no_graph"), ("final_equal_scores", "last_max")):
        c = next(c for c in sr.final_cases() if c.name == name)
        st, ph, sc = sr.final_state(c)
        graph = HotwordGraph(ph, sc) if ph else None
        best, _ = sr.final_reference(st, 1, graph, c.out_cap)
        if alt == "no_graph":
            assert sr.final_reference(st, 1, None, c.out_cap)[0] != best
        else:
            v = [st["lp"][1, h] / st["len"][1, h] for h in range(int(st["nh"][1]))]
            assert best == 0 and v[0] == v[1] == v[2]
