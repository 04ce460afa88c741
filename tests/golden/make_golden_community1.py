"""Writes tests/golden/community1_pool_cases.json: the reference's own
PureOrtDiarizer._masked_stats_pool (core/speaker_diarization_pure_ort.py:756-767) on the 16 x 125
feature block and the six masks of tests/resnet34_reference.py, for
tests/test_resnet34_reference.py.

    python tests/golden/make_golden_community1.py /path/to/reference

The reference is imported here only (its module needs numpy and scipy at import).  The method
does not touch `self`, so it is called unbound.  Only data is recorded: per mask the active
frames of the weights it was given and the 32 float32 statistics it returned, and the sha256 of
the seeded feature block.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), REPO, os.path.join(REPO, "sherpa-vietnamese-asr_amd")):
    sys.path.insert(0, p)
import resnet34_reference as R  # noqa: E402


def main(ref_root: str) -> None:
    sys.path.insert(0, ref_root)
    from core.speaker_diarization_pure_ort import PureOrtDiarizer

    block = R.pool_block(16)
    idx = R.feat_idx(block.shape[1], R.NSEG)
    out = {"numpy": np.__version__, "block_shape": list(block.shape),
           "block_sha256": hashlib.sha256(block.tobytes()).hexdigest(),
           "min_seg_frames": R.MIN_SEG_FRAMES, "cases": {}}
    for name, (full, clean) in R.pool_masks().items():
        weights = R.used_mask(full, clean, R.MIN_SEG_FRAMES)[idx].astype(np.float32)
        stats = PureOrtDiarizer._masked_stats_pool(None, block, weights)
        assert stats.dtype == np.float32 and stats.shape == (32,), (stats.dtype, stats.shape)
        out["cases"][name] = {"weights_on": np.flatnonzero(weights).tolist(),
                              "stats": [float(v) for v in stats]}
    path = os.path.join(HERE, "community1_pool_cases.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
