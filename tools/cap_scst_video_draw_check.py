"""CPU check behind the token cap of tests/test_gpu_cap_scst_video.py: for every multi-row case of tests/cap_scst_video_oracle.py, at
dropout p 0 and 0.5 and at temperature 1.0 and 0.7, the composed oracle draws its tokens in float32 and in float64 from the same
uniforms; prints the rows whose tokens differ per setting (docs/CAPTION_SCST_PER_VIDEO.md records the result).  No GPU.

  usage: cap_scst_video_draw_check.py [case ...]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import cap_scst_video_oracle as svo  # noqa: E402


def main(argv):
    names = argv or svo.MULTI_ROW
    worst = 0
    for name in names:
        for p in (0.0, 0.5):
            for temp in (1.0, 0.7):
                a, _ = svo.draw(name, True, p, 123457, temp, torch.float32)
                b, _ = svo.draw(name, True, p, 123457, temp, torch.float64)
                n = max(a.shape[1], b.shape[1])
                pad = lambda s: np.concatenate([s, np.zeros((s.shape[0], n - s.shape[1]), s.dtype)], 1)      # noqa: E731
                rows = np.flatnonzero((pad(a) != pad(b)).any(1))
                worst = max(worst, rows.size)
                print("%-10s p %.1f temperature %.1f: width %d / %d, rows that differ %s" % (name, p, temp, a.shape[1], b.shape[1], rows.tolist()),
                      flush=True)
    print("most differing rows in one setting: %d" % worst)


if __name__ == "__main__":
    main(sys.argv[1:])
