"""The transducer search kernels alone, frame by frame, against a float64 reference.

search_step_kernel (every KB / Q instantiation, with and without the decoder-context table),
greedy_spec_kernel and search_final_kernel run through zasr_selftest_search_step / _greedy_spec /
_search_final on host arrays: the launchers a decode calls, the hotword tables from the engine's
build_hotword_dfa (held to oracle.search.HotwordGraph through zasr_selftest_hotword_dfa), the
decoder-context table built in full by the entry point.  Cases, inputs, reference, bounds and the
chain drivers: tests/search_reference.py (checked without a GPU by tests/test_search_reference.py).
A chain starts from the engine's own init state and every frame is compared with the reference
applied to the state the kernel was given, so a failure names its frame.  The entry points keep
guard regions around every array and refuse a run that wrote into one.

Each case prints its worst |got - ref| / bound per output and the zlib.crc32 of the returned
bytes; the CRCs of two builds of the library compare the kernels bit for bit.
"""
import numpy as np
import pytest

import search_reference as sr
from conftest import gpu_available
from oracle.search import HotwordGraph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def need_gpu():
    if not gpu_available():
        pytest.skip("no GPU")


def gpu_step(V, beam, t, enc_len, st, logits, phrases, scores, tab):
    from zasr.binding import selftest_search_step
    selftest_search_step(V, beam, t, enc_len, st, logits, phrases, scores, tab)


def gpu_greedy(V, F, init, parity, enc_len, t_cur, active, st, logits, tab, phrases, scores):
    from zasr.binding import selftest_greedy_spec
    selftest_greedy_spec(V, F, init, parity, enc_len, t_cur, active, st, logits, tab, phrases, scores)


def run_group(cases):
    bad, events = [], {}
    for c in cases:
        r = sr.run_step_chain(c, gpu_step)
        print(f"{c.name}: {r.worst} redraws {r.redraws} merges {r.merges} crc32 = {r.crc:08x}")
        if r.bad:
            bad.append((c.name, r.bad[:6]))
        sr.check_case_claims(c, r, bad)
        for k, v in r.events.items():
            events[k] = events.get(k, 0) + v
    return bad, events


def test_step_chains_match_f64_frame_by_frame(need_gpu):
    bad, _ = run_group(sr.chain_cases())
    assert not bad, bad


def test_hotword_dfa_is_the_oracle_graph(need_gpu):
    from zasr.binding import selftest_hotword_dfa
    for V in (64, 2052):
        ph, sc = sr.hotword_phrases(V)
        assert not sr.check_dfa(selftest_hotword_dfa(V, ph, sc), HotwordGraph(ph, sc), V)
    # shared prefixes with different scores, a phrase inside another, a repeated phrase
    ph = [[4, 9, 4], [4, 9], [9, 4, 9, 11], [4], [11, 4, 9], [4, 9]]
    sc = [1.0, 3.0, 0.5, 0.25, 2.0, 1.5]
    assert not sr.check_dfa(selftest_hotword_dfa(16, ph, sc), HotwordGraph(ph, sc), 16)


def test_hotword_step_chains_match_f64(need_gpu):
    bad, events = run_group(sr.hotword_cases())
    assert not bad, bad
    print("hotword transitions:", events)
    for kind in ("child", "fail_link", "reset", "full_match"):   # they all occurred
        assert events.get(kind, 0) > 0, (kind, events)


def test_crafted_frames_match_f64(need_gpu):
    bad, _ = run_group(sr.crafted_cases())
    assert not bad, bad


def test_step_with_table_writes_every_j_format(need_gpu):
    bad, _ = run_group(sr.table_cases())
    assert not bad, bad


def test_greedy_windows_match_f64_and_the_beam1_step(need_gpu):
    bad = []
    for c in sr.greedy_cases():
        r = sr.run_greedy_chain(c, gpu_greedy)
        print(f"{c.name}: {r.worst} redraws {r.redraws} super-steps {r.steps} crc32 = {r.crc:08x}")
        if r.bad:
            bad.append((c.name, r.bad[:6]))
            continue
        sr.check_greedy_claims(c, r, bad)
        # the project's contract at these shapes: the windows and the frame-by-frame beam-1 step
        # end in the same bytes
        st2 = sr.run_greedy_as_steps(c, r.salts, gpu_step)
        diff = [k for k in st2 if st2[k].tobytes() != r.final_state[k].tobytes()]
        if diff:
            bad.append((c.name, "windows != frame-by-frame steps", diff))
    assert not bad, bad


def test_final_pick_and_backtrack_are_exact(need_gpu):
    from zasr.binding import selftest_search_final
    bad = []
    for c in sr.final_cases():
        st, ph, sc = sr.final_state(c)
        before = sr.state_copy(st)
        out = selftest_search_final(64, st, c.out_cap, ph, sc, fill=sr.SENT)
        graph = HotwordGraph(ph, sc) if ph else None
        msgs = sr.check_final(c, st, out, graph)
        if any(st[k].tobytes() != before[k].tobytes() for k in st):
            msgs.append("the state changed")
        print(f"{c.name}: count {out['count'].tolist()} crc32 = {sr.state_crc(out):08x}")
        if msgs:
            bad.append((c.name, msgs))
    assert not bad, bad


def _ok_step_args():
    c = sr.StepCase("refuse", 64, 4, 4, "gauss", enc_len=(3, 2))
    st = sr.state_alloc(c.S, c.Hmax, 16)
    gpu_step(64, 4, -1, c.enc_len, st, None, None, None, None)
    return c, st


def test_refusals_launch_nothing(need_gpu):
    from zasr.binding import ZasrError, selftest_search_final
    c, st0 = _ok_step_args()
    el = np.asarray(c.enc_len, np.int32)

    def step(V=64, beam=4, Hmax=4, enc_len=el, node_cap=16, D=None):
        st = sr.state_alloc(2, Hmax, node_cap)
        n = min(Hmax, 4)
        for k in st:
            if st[k].ndim >= 2 and st[k].shape[1] == Hmax and k in sr.SLOT_KEYS:
                st[k][:, :n] = st0[k][:, :n]
        st["nh"][:] = 1
        st["node_count"][:] = 0
        tab = None
        if D is not None:
            tab = sr.table_operands("refuse", V, D, enc_len)
            tab.update(jfmt=0, J=np.full(sr.j_bytes(0, 2 * Hmax, D), sr.SENT, np.uint8))
        before = sr.state_copy(st)
        with pytest.raises(ZasrError):
            gpu_step(V, beam, 0, enc_len, st, np.zeros((2, Hmax, V), np.float32), None, None, tab)
        assert all(st[k].tobytes() == before[k].tobytes() for k in st)
        if tab is not None:
            assert np.all(tab["J"] == sr.SENT)

    step(V=66)
    step(V=4100)
    step(beam=0)
    step(beam=17, Hmax=16)
    step(beam=4, Hmax=2)
    step(D=6)
    step(D=516)
    step(node_cap=3)                                   # node_count + beam > node_cap
    step(enc_len=np.array([3, -1], np.int32))
    # the greedy window: F = 6, node_cap without room for one more node
    g = sr.GreedyCase("refuse_greedy", 64, 4, 256, 0)
    for F, cap in ((6, 32), (4, 0)):
        S = g.S
        st = sr.state_alloc(S, 1, max(cap, 1))
        for k in sr.SLOT_KEYS:
            st[k][...] = 0
        st["nh"][:] = 1
        st["node_count"][:] = 1 if cap == 0 else 0
        tab = sr.table_operands(g.name, 64, 256, g.enc_len)
        tab.update(jfmt=0, J=np.full(sr.j_bytes(0, S * F, 256), sr.SENT, np.uint8))
        t_cur, active = np.zeros(S, np.int32), np.zeros(2, np.int32)
        with pytest.raises(ZasrError):
            gpu_greedy(64, F, 0, 0, g.enc_len, t_cur, active, st, np.zeros((S, F, 64), np.float32),
                       tab, None, None)
        assert np.all(tab["J"] == sr.SENT) and not t_cur.any()
    # the final pick: a parent that does not precede its node
    fc = sr.final_cases()[0]
    st, ph, sc = sr.final_state(fc)
    st["node_parent"][1, 5] = 5
    with pytest.raises(ZasrError):
        selftest_search_final(64, st, fc.out_cap, ph, sc)
