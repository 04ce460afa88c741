"""Cases, seeded operands and the float64 reference of the joiner kernel tests
(tests/test_gpu_joiner.py on the GPU, tests/test_joiner_reference.py without one).

One problem per case: out[M][V] = J[M][D] W[V][D]^T + bias through zasr_selftest_joiner.

    layout 0  row-major J: joiner_kernel (fp32), joiner_bf16_kernel (bf16), joiner_split_kernel
              (bf16x3 / bf16x6 / f16x3).  32 x 32 tiles, four waves splitting K.  Every D in
              {64, 128, 256, 512} in all five modes over (M, V) = (1, 5) one partial tile,
              (31, 32) a row tail under a full column tile, (33, 68) and (65, 68) two / three row
              tiles and three column tiles, the last of each partial.
    layout 1  fragment-packed J and W: joiner_reg_kernel (bf16), joiner_split_packed_kernel (the
              split modes).  64 x 64 blocks, wave = (row tile, column group); D in {256, 512}
              over (1, 5) one partial tile, the block's second row tile past M and its second
              column group past V; (33, 68) a partial second row tile, a partial column group
              and one that starts past V; (65, 100) a second block whose second row tile starts
              past M; (97, 36) a partial second column group under two blocks of rows.
    live      the finished-stream filter in both layouts, bf16 and f16x3, D = 256: 24 streams of
              live_f = 4 rows (M = 96), V = 68; finished = streams 0-15 (layout 0 skips two row
              tiles, layout 1 one block), 8-15 (layout 0 skips one row tile, layout 1 none: the
              block's other row tile is live) or 17 alone (no tile is all finished).

Inputs: J = tanh(N(0, 1)), what decjoin_kernel / store_j4 write; W = N(0, 1) / sqrt(D) and
bias = 0.1 N(0, 1) as in tests/test_gpu_gemm.py; seeded per case.  `out` enters as SENTINEL, so
what a kernel leaves alone shows.

Bound per element, the pre-activation row of tests/test_gpu_gemm.py's table (derived there):

    |got - ref| <= (u_op + 2 D u) S,   S = |J'| |W'|^T + |bias|,   u = 2^-24

with the reference a float64 product of the operands as the kernel sees them: both rounded to
bf16 (nearest even) in the bf16 mode, the f32 values otherwise.
"""
import math
import zlib
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
# tests/test_gpu_gemm.py U_OP (test_joiner_reference.py holds the two equal)
U_OP = {"fp32": 0.0, "bf16": 0.0, "bf16x3": 2.0 ** -15, "bf16x6": 2.0 ** -22, "f16x3": 2.0 ** -21}
SENTINEL = np.float32(-7777.0)

# live: None, or the name of a LIVE_PATTERNS entry
Case = namedtuple("Case", "layout mode D M V live")

MODES0 = ["fp32", "bf16", "bf16x3", "bf16x6", "f16x3"]
MODES1 = ["bf16", "bf16x3", "bf16x6", "f16x3"]
SHAPES0 = [(1, 5), (31, 32), (33, 68), (65, 68)]
SHAPES1 = [(1, 5), (33, 68), (65, 100), (97, 36)]
EDGE_GROUPS = [(0, m, d) for m in MODES0 for d in (64, 128, 256, 512)] + \
              [(1, m, d) for m in MODES1 for d in (256, 512)]

LIVE_F, LIVE_STREAMS, LIVE_V, LIVE_D = 4, 24, 68, 256
LIVE_PATTERNS = {"s0_15": range(0, 16), "s8_15": range(8, 16), "s17": [17]}
LIVE_GROUPS = [(layout, mode) for layout in (0, 1) for mode in ("bf16", "f16x3")]


def group_cases(layout, mode, D):
    return [Case(layout, mode, D, M, V, None) for M, V in (SHAPES1 if layout else SHAPES0)]


def live_cases(layout, mode):
    return [Case(layout, mode, LIVE_D, LIVE_STREAMS * LIVE_F, LIVE_V, p) for p in LIVE_PATTERNS]


def all_cases():
    return [c for g in EDGE_GROUPS for c in group_cases(*g)] + \
           [c for g in LIVE_GROUPS for c in live_cases(*g)]


def case_id(c):
    return f"l{c.layout}_{c.mode}_D{c.D}_M{c.M}_V{c.V}" + (f"_{c.live}" if c.live else "")


def rne_bf16(x):
    """float32 -> the nearest-even bfloat16, returned as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def operands(c):
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    return dict(J=np.tanh(f(c.M, c.D)), W=f(c.V, c.D) / np.float32(math.sqrt(c.D)),
                bias=f(c.V) * np.float32(0.1), out0=np.full((c.M, c.V), SENTINEL, np.float32))


def seen(c, o):
    """J and W as the kernel sees them (float32)."""
    return (rne_bf16(o["J"]), rne_bf16(o["W"])) if c.mode == "bf16" else (o["J"], o["W"])


def reference(c, o):
    """(float64 reference, per-element bound): the module docstring's formula."""
    J, W = (x.astype(np.float64) for x in seen(c, o))
    b = o["bias"].astype(np.float64)
    return J @ W.T + b, (U_OP[c.mode] + 2 * c.D * U) * (np.abs(J) @ np.abs(W).T + np.abs(b))


def live_arrays(c):
    """(live_t, live_len, finished streams): a finished stream has live_t >= live_len."""
    done = np.zeros(LIVE_STREAMS, bool)
    done[list(LIVE_PATTERNS[c.live])] = True
    live_len = np.full(LIVE_STREAMS, 10, np.int32)
    return np.where(done, 10, 3).astype(np.int32), live_len, done
