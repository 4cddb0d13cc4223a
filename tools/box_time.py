"""Box and level reads against the routes to the same samples without them (container.read_region
with rows / cols / level vs its planes-only form plus a slice, and vs decompress plus a stride).

One volume ``[1, n, n, n, 1]`` uint16 (a smooth field plus noise, as tools/region_time.py makes it)
is compressed once -- MeanPredictor p = 0, levels='auto', tile_crc=True -- and read in one process,
its pages warm:

  (a) a box of ``--box``^3 samples at the centre: ``read_region(planes, rows, cols)`` alternating with
      ``read_region(planes)[..., y0:y1, x0:x1]``, ``--reps`` rounds each; medians with the min .. max
      spread, the payload bytes read, the tiles decoded and the read / device / d2h split of both;
  (b) ``read_region(level=k)`` for k = 1, 2 and L alternating with ``decompress`` plus the stride.

Times are host-clock around calls that end in a synchronise.

    python tools/box_time.py [--size 512] [--box 64] [--reps 9] [--log profiles/box/box_time.log]
"""

import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import kompressor_amd as kom  # noqa: E402


def volume(n, seed=0):
    """A smooth uint16 field with noise (residuals of a few bits, like a tomogram)."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float32)] * 3, indexing='ij', sparse=True)
    f = 9000 * np.sin(z / 37) * np.cos(y / 29) + 7000 * np.sin(x / 41 + y / 53) + 30000
    f = f + rng.normal(0, 12, (n, n, n)).astype(np.float32)
    return np.clip(np.rint(f), 0, 65535).astype(np.uint16)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def alternate(fns, reps):
    """``reps`` rounds of every callable in turn: per callable its times and its last ``last_timing``."""
    ts, tms = [[] for _ in fns], [None] * len(fns)
    for _ in range(reps):
        for q, fn in enumerate(fns):
            ts[q].append(timed(fn)[0])
            tms[q] = dict(kom.container.last_timing)
    return ts, tms


def ms(t):
    return f'{1e3 * statistics.median(t):.2f} ({1e3 * min(t):.2f} .. {1e3 * max(t):.2f})'


def split(tm):
    return ' '.join(f'{k} {1e3 * tm[k]:.2f}' for k in ('read', 'device', 'd2h') if k in tm)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--box', type=int, default=64)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--log', default=None)
    ap.add_argument('--dir', default=None, help='where the file goes (default: a temporary directory)')
    a = ap.parse_args()
    n, C = a.size, kom.container
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    arr = volume(n).reshape(1, n, n, n, 1)
    lo = (n - a.box) // 2
    sel = (lo, lo + a.box)
    say(f'# box_time: {n}^3 uint16, mean-p0, levels auto, tile_crc, reps {a.reps}, {torch.cuda.get_device_name(0)}')
    say('# times: median ms (min .. max)')
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        path = os.path.join(d, 'volume.kmp')
        made = C.compress(path, arr, kom.MeanPredictor(0, 3), levels='auto', tile_crc=True)
        L = made['levels']
        say(f'# file: {made["bytes"]} bytes, ratio {made["ratio"]:.3f}, levels {L}, shapes {C.level_shapes(path)}')
        full = C.decompress(path)  # warm-up of the file's pages and of every kernel family
        assert np.array_equal(full, arr)

        def box():
            return C.read_region(path, planes=sel, rows=sel, cols=sel)

        def slab():
            return np.ascontiguousarray(C.read_region(path, planes=sel)[:, :, sel[0]:sel[1], sel[0]:sel[1]])

        want = arr[:, sel[0]:sel[1], sel[0]:sel[1], sel[0]:sel[1]]
        assert np.array_equal(box(), want) and np.array_equal(slab(), want)
        ts, tms = alternate([box, slab], a.reps)
        say(f'# (a) {a.box}^3 box at {sel}: route | ms | payload bytes read | tiles decoded / total | split ms')
        for name, t, tm in zip(('box', 'planes + slice'), ts, tms):
            say(f'a | {name} | {ms(t)} | {tm["payload_bytes_read"]} | {tm["tiles_decoded"]}/{tm["tiles_total"]} | '
                f'{split(tm)}')
        say(f'a | box / planes + slice: time {statistics.median(ts[0]) / statistics.median(ts[1]):.3f}, payload '
            f'{tms[0]["payload_bytes_read"] / tms[1]["payload_bytes_read"]:.3f}')
        say('# (b) a whole level: level | read_region(level) ms | decompress + stride ms | ratio | payload bytes read '
            '| tiles decoded / total | split ms')
        for k in sorted({1, 2, L}):
            def level():
                return C.read_region(path, level=k)

            def stride():
                return np.ascontiguousarray(C.decompress(path)[:, ::2 ** k, ::2 ** k, ::2 ** k])

            assert np.array_equal(level(), stride())
            ts, tms = alternate([level, stride], a.reps)
            r, f = statistics.median(ts[0]), statistics.median(ts[1])
            say(f'b | level {k}{" (= L)" if k == L else ""} | {ms(ts[0])} | {ms(ts[1])} | {f / r:.1f}x | '
                f'{tms[0]["payload_bytes_read"]} | {tms[0]["tiles_decoded"]}/{tms[0]["tiles_total"]} | {split(tms[0])}')
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
