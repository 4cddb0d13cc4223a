"""The workload of the per-tile CRC kernel's trace: a C3-size volume (512^3 uint16, MeanPredictor
p = 0, levels='auto') written with ``tile_crc=True`` and read back partially, so that one kernel
trace holds ``tile_crc_kernel`` (write mode over the whole bundle, check mode over a selection's
windows) and the unchanged ``crc32_kernel`` over the same bundle bytes.

    rocprofv3 --kernel-trace --stats -d OUT -o tile_crc --output-format csv -- \\
        python tools/tile_crc_trace.py [--size 512] [--reps 3]
"""

import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import kompressor_amd as kom  # noqa: E402
from region_time import volume  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    n = a.size
    arr = volume(n).reshape(1, n, n, n, 1)
    mid = n // 2
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'v.kmp')
        for _ in range(a.reps):
            info = kom.container.compress(path, arr, kom.MeanPredictor(0, 3), levels='auto', tile_crc=True)
            for planes in ((mid, mid + 1), (mid, mid + 64)):
                got = kom.container.read_region(path, planes=planes)
                assert kom.container.last_timing['tile_crc'] and np.array_equal(got, arr[:, planes[0]:planes[1]])
        tiles = kom.container.info(path)['tile_crc']
        print(f'tile_crc_trace: {n}^3 uint16, {info["bytes"]} bytes, {tiles} tiles, reps {a.reps}')


if __name__ == '__main__':
    main()
