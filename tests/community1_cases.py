"""Seeded synthetic files for the community-1 back-end tests: a turn-taking timeline of a few
global speakers, cut into the diarizer's 10 s / 1 s chunks as powerset class maps [C][589], and
embeddings [C][3][256] that follow the speaker of each local slot.  Shared by
tests/golden/make_golden_community1_cluster.py (which feeds the reference's own functions) and
test_vbx_reference.py; the stub sessions stand where the segmentation and embedding models are.

The audio of a file is a staircase, sample t holds (t // 16000) / 64, so a stub segmenter can
tell which chunk it was handed from the chunk's first sample."""
import numpy as np

F = 589
DIM = 256
CHUNK, STEP, SR = 160000, 16000, 16000
PAIR_CLASS = {(0, 1): 4, (0, 2): 5, (1, 2): 6}

# name -> (seed, samples, global speakers)
FILES = {"f7_3": (11, 116800, 2), "f10_0": (12, 160000, 2), "f26": (13, 416000, 4)}
CLUSTER_CASE = ("cluster24", 21, 24 * 16000 + 9 * 16000 + 4000, 4)   # 25 chunks


def staircase(samples):
    return (np.arange(samples) // STEP).astype(np.float32) / np.float32(64.0)


def chunk_starts(samples):
    starts, s = [], 0
    while True:
        starts.append(s)
        if s + CHUNK > samples:
            return starts
        s += STEP


def scenario(seed, samples, n_spk):
    """dict(classes uint8 [C][F], embeddings float32 [C][3][DIM], starts)."""
    rng = np.random.default_rng(seed)
    starts = chunk_starts(samples)
    C = len(starts)
    fd = 10.0 / F
    n_glob = int((starts[-1] / SR + 10.0) / fd) + 2
    active = np.zeros((n_glob, n_spk), bool)       # global timeline, at most 2 at once
    t, cur = 0, 0
    while t < n_glob:
        length = int(rng.integers(60, 260))
        nxt = int((cur + rng.integers(1, n_spk)) % n_spk) if n_spk > 1 else 0
        active[t:t + length, cur] = True
        if rng.random() < 0.5:                      # the next speaker starts early: overlap
            active[max(t + length - int(rng.integers(20, 50)), 0):t + length, nxt] = True
        else:                                       # or after a pause
            t += int(rng.integers(0, 30))
        t += length
        cur = nxt
    end_frame = int(samples / SR / fd)
    active[end_frame:] = False                      # nobody speaks in the zero padding
    q, _ = np.linalg.qr(rng.standard_normal((DIM, n_spk)))
    classes = np.zeros((C, F), np.uint8)
    emb = np.empty((C, 3, DIM), np.float32)
    for c, s in enumerate(starts):
        f0 = int(round(s / SR / fd))
        win = active[f0:f0 + F]
        order = [g for g in np.argsort([np.argmax(win[:, g]) if win[:, g].any() else 10 ** 6
                                        for g in range(n_spk)], kind="stable")
                 if win[:, g].any()][:3]
        local = np.zeros((F, 3), bool)
        for slot, g in enumerate(order):
            local[:, slot] = win[:, g]
        for f in range(F):
            on = tuple(np.flatnonzero(local[f])[:2])
            classes[c, f] = 0 if not on else on[0] + 1 if len(on) == 1 else PAIR_CLASS[on]
        for slot in range(3):
            if slot < len(order):
                v = q.T[order[slot]] + 0.25 * rng.standard_normal(DIM) / np.sqrt(DIM)
            else:
                v = rng.standard_normal(DIM) / np.sqrt(DIM)
            emb[c, slot] = (v * rng.uniform(0.5, 2.0)).astype(np.float32)
    return {"classes": classes, "embeddings": emb, "starts": starts}


def synthetic_plda_files(seed=5, dim=DIM, lda_dim=128):
    """(xvec_transform.npz contents, plda.npz contents) of a seeded synthetic PLDA."""
    rng = np.random.default_rng(seed)
    tr = np.linalg.qr(rng.standard_normal((lda_dim, lda_dim)))[0] * rng.uniform(0.5, 2.0, (lda_dim, 1))
    return ({"mean1": 0.05 * rng.standard_normal(dim), "mean2": 0.05 * rng.standard_normal(lda_dim),
             "lda": rng.standard_normal((dim, lda_dim)) / np.sqrt(dim)},
            {"mu": 0.05 * rng.standard_normal(lda_dim), "tr": tr,
             "psi": np.sort(rng.uniform(0.05, 8.0, lda_dim))[::-1].copy()})


class StubSegmenter:
    """seg_sess of the reference / SegSession's run(): one-hot log-probabilities of the
    scenario's class map, the chunk recognised by its first sample."""

    def __init__(self, classes):
        self.classes = classes

    def run(self, output_names, feeds):
        batch = np.asarray(feeds["input_values"])
        batch = batch[:, 0, :] if batch.ndim == 3 else batch
        out = np.full((batch.shape[0], F, 7), -10.0, np.float32)
        for i in range(batch.shape[0]):
            c = int(round(float(batch[i, 0]) * 64.0))
            out[i, np.arange(F), self.classes[c]] = 0.0
        return [out]


class StubEmbedder:
    """EmbSession's chunk_embeddings(): the scenario's embeddings."""

    def __init__(self, embeddings):
        self.embeddings = embeddings

    def chunk_embeddings(self, audio, chunk_starts, masks):
        idx = [int(s) // STEP for s in chunk_starts]
        return self.embeddings[idx].copy()
