"""The attention kernels' block map (csrc/kernels.h build_attn_block_map), host only, through
zasr_selftest_attn_block_map: which (sequence, head or z-chunk, query tile) every block id of
the 1-D launch serves.

Properties held for every case and both slot orders:
  - every (sequence, unit, tile) with tile * 128 < L appears exactly once, and nothing else;
  - range x's entries sit at block ids = x (mod 8), and the units of the ranges are contiguous
    runs of the sequence-major unit list, in range order;
  - the grid is 8 * the longest range's blocks, every range filled from slot 0 without holes;
  - the heaviest range weighs at most the mean plus one unit's largest weight, a unit weighing
    cdiv(L, 128) * cdiv(L, 32) block-steps (the property of a contiguous cut);
  - a range's slots run in the stated order.
"""
import numpy as np
import pytest

from zasr.binding import ZasrError, selftest_attn_block_map

NONE = 0xFFFFFFFF
XCDS = 8

_rng = np.random.RandomState(7)
HOUR = _rng.randint(1350, 1751, size=121).tolist()
EDGES = [1, 127, 128, 129, 255, 256, 257, 383, 384, 385, 31, 32, 33, 511, 512, 513, 640, 1000, 2]

CASES = {
    "one_L1": ([1], 4),
    "one_L128": ([128], 4),
    "one_L129": ([129], 4),
    "one_L129_head0": ([129], 1),
    "three_by_two": ([200, 129, 40], 2),
    "empty_between": ([300, 0, 257], 4),
    "empty_ends": ([0, 130, 0], 2),
    "edges_19x4": (EDGES, 4),
    "hour_x4": (HOUR, 4),
    "hour_x8": (HOUR, 8),
    "hour_x2_chunks": (HOUR, 2),
    "hour_x1": (HOUR, 1),
}
assert len(EDGES) == 19


def _tiles(L):
    return (L + 127) // 128


def _weight(L):
    return _tiles(L) * ((L + 31) // 32)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_block_map(name, order):
    lens, units = CASES[name]
    m = selftest_attn_block_map(lens, units, order)
    grid = len(m)
    assert grid % XCDS == 0
    want = {(b, u, t) for b, L in enumerate(lens) for u in range(units) for t in range(_tiles(L))}
    ranges = []
    for x in range(XCDS):
        col = m[x::XCDS]
        live = col != NONE
        n = int(live.sum())
        assert live[:n].all() and not live[n:].any(), f"range {x} has a hole"
        e = col[:n].astype(np.int64)
        ranges.append(list(zip((e >> 12).tolist(), ((e >> 8) & 15).tolist(), (e & 255).tolist())))
    got = [e for r in ranges for e in r]
    assert len(got) == len(set(got)), "an entry appears twice"
    assert set(got) == want
    assert grid == XCDS * max(len(r) for r in ranges)
    # contiguous ranges of the sequence-major unit list, in range order
    last = (-1, -1)
    for r in ranges:
        us = sorted({(b, u) for b, u, _ in r})
        if us:
            assert us[0] > last, "ranges overlap or run backwards"
            last = us[-1]
            # every tile of a unit sits in the unit's range
            assert len(r) == sum(_tiles(lens[b]) for b, _ in us)
    # balance: heaviest range <= mean + one unit's largest weight
    wr = [sum(_weight(lens[b]) for b, _ in {(b, u) for b, u, _ in r}) for r in ranges]
    total = sum(_weight(L) for L in lens) * units
    assert sum(wr) == total
    assert max(wr) <= total / XCDS + max(_weight(L) for L in lens)
    # slot order inside a range: sequence, then (tile, unit) or (unit, tile)
    for r in ranges:
        key = (lambda e: (e[0], e[2], e[1])) if order == 0 else (lambda e: e)
        assert r == sorted(r, key=key)


def test_all_empty_and_limits():
    assert len(selftest_attn_block_map([0, 0], 4)) == 0
    assert len(selftest_attn_block_map([], 4)) == 0
    with pytest.raises(ZasrError):
        selftest_attn_block_map([10], 17)  # units over the entry's 4-bit field
    with pytest.raises(ZasrError):
        selftest_attn_block_map([128 * 256 + 1], 1)  # tiles over the entry's 8-bit field
    with pytest.raises(ZasrError):
        selftest_attn_block_map([10], 2, order=2)
