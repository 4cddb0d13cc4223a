"""Partial reads against full reads of the same file (container.read_region vs container.decompress).

A C3-size volume (512^3 uint16) is compressed twice -- MeanPredictor p = 0 and LinearPredictor
p = 1, levels='auto' -- as ONE volume [1, 512, 512, 512, 1] and as 512 tiles of 64^3
[512, 64, 64, 64, 1].  Per file: ``read_region`` of 1, 16 and 64 planes (the volume) or of 1 and 32
tiles (the tiled file), alternating with ``decompress`` of the same file in the same process,
after a warm-up; the median of ``--reps`` host-clock times around calls that end in a
synchronise, the tiles decoded of the tiles in the file, the payload bytes read and the peak
``torch.cuda.max_memory_allocated`` of each call.

    python tools/region_time.py [--size 512] [--reps 11] [--log profiles/region/region_time.log]

``--tile-crc`` adds the Mean p = 0 volume written with the per-tile CRC table beside the one without
(``--only-tile-crc``: those rows alone): read_region of 1, 16 and 64 planes, decompress and compress.
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


def linear(p):
    n = (2 * p + 2) ** 3
    w = (np.full((n, 19), 1.0 / n) + np.random.default_rng(p).standard_normal((n, 19)) * 0.01).astype(np.float32)
    return kom.LinearPredictor(w, np.zeros(19, np.float32), p, 3)


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, torch.cuda.max_memory_allocated(), out


def tile_crc_rows(a, arr, mid, d, say):
    """``--tile-crc``: the Mean p = 0 volume written without and with the per-tile CRC table; per
    selection the two files' ``read_region`` alternate in one process (median of ``--reps``), then
    ``compress`` and ``decompress`` of both, host-inclusive.  A build whose ``compress`` has no
    ``tile_crc`` keyword (the baseline) alternates two files without a table, so that its rows carry
    the same alternation between two files."""
    import inspect
    pred = kom.MeanPredictor(0, 3)
    has = 'tile_crc' in inspect.signature(kom.container.compress).parameters
    files = [('no table', os.path.join(d, 'crc_plain.kmp'), {}),
             ('table', os.path.join(d, 'crc_table.kmp'), {'tile_crc': True}) if has else
             ('no table (2nd file)', os.path.join(d, 'crc_plain2.kmp'), {})]
    say(f'# tile_crc rows: volume mean-p0, files {[f[0] for f in files]}; columns: median ms (min .. max)')
    for _, path, ckw in files:
        kom.container.compress(path, arr, pred, levels='auto', **ckw)

    def row(name, fns):
        ts = [[] for _ in fns]
        for _ in range(a.reps):
            for q, fn in enumerate(fns):
                ts[q].append(timed(fn)[0])
        say(f'tile_crc | {name} | ' + ' | '.join(
            f'{files[q][0]} {1e3 * statistics.median(t):.3f} ({1e3 * min(t):.3f} .. {1e3 * max(t):.3f})'
            for q, t in enumerate(ts)))

    for sname, kw in (('1 plane', {'planes': (mid, mid + 1)}), ('16 planes', {'planes': (mid, mid + 16)}),
                      ('64 planes', {'planes': (mid, mid + 64)})):
        for _, path, _ in files:
            assert np.array_equal(kom.container.read_region(path, **kw), arr[:, kw['planes'][0]:kw['planes'][1]])
        row(f'read_region {sname}', [lambda p=path: kom.container.read_region(p, **kw) for _, path, _ in files])
        if has:
            say(f'tile_crc | read_region {sname} | ran {kom.container.last_timing.get("tile_crc")} tiles '
                f'{kom.container.last_timing["tiles_decoded"]}/{kom.container.last_timing["tiles_total"]}')
    row('decompress', [lambda p=path: kom.container.decompress(p) for _, path, _ in files])
    row('compress', [lambda p=path, c=ckw: kom.container.compress(p, arr, pred, levels='auto', **c)
                     for _, path, ckw in files])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--tile-crc', action='store_true',
                    help='also time a file with the per-tile CRC table beside one without (mean-p0 volume)')
    ap.add_argument('--only-tile-crc', action='store_true', help='the --tile-crc rows alone')
    ap.add_argument('--log', default=None)
    ap.add_argument('--dir', default=None, help='where the files go (default: a temporary directory)')
    a = ap.parse_args()
    n = a.size
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    vol = volume(n)
    t = 64
    tiles = vol.reshape(n // t, t, n // t, t, n // t, t).transpose(0, 2, 4, 1, 3, 5).reshape(-1, t, t, t, 1)
    tiles = np.ascontiguousarray(tiles)
    mid = n // 2
    say(f'# region_time: {n}^3 uint16, reps {a.reps} (median), {torch.cuda.get_device_name(0)}')
    say('# file | selection | read_region ms | decompress ms | ratio | tiles decoded/total | payload read / bundle bytes '
        '| peak MiB region / full')
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        for pname, pred in (() if a.only_tile_crc else (('mean-p0', kom.MeanPredictor(0, 3)), ('linear-p1', linear(1)))):
            for fname, arr, sels in (
                    ('volume', vol.reshape(1, n, n, n, 1),
                     [('1 plane', {'planes': (mid, mid + 1)}), ('16 planes', {'planes': (mid, mid + 16)}),
                      ('64 planes', {'planes': (mid, mid + 64)})]),
                    ('tiles', tiles, [('1 tile', {'batch': (37, 38)}), ('32 tiles', {'batch': (37, 69)})])):
                path = os.path.join(d, f'{fname}_{pname}.kmp')
                info = kom.container.compress(path, arr, pred, levels='auto')
                say(f'# {fname} {pname}: {info["bytes"]} bytes, ratio {info["ratio"]:.3f}, levels {info["levels"]}')
                for sname, kw in sels:
                    want = arr[slice(*kw.get('batch', (None, None))), slice(*kw.get('planes', (None, None)))]
                    got = kom.container.read_region(path, **kw)
                    assert np.array_equal(got, want), (fname, pname, sname)
                    kom.container.decompress(path)  # warm-up of both
                    tr, tf, mr, mf = [], [], 0, 0
                    for _ in range(a.reps):
                        dt, m, _ = timed(lambda: kom.container.read_region(path, **kw))
                        tm = dict(kom.container.last_timing)
                        tr.append(dt)
                        mr = max(mr, m)
                        dt, m, _ = timed(lambda: kom.container.decompress(path))
                        tf.append(dt)
                        mf = max(mf, m)
                    r, f = statistics.median(tr), statistics.median(tf)
                    say(f'{fname} {pname} | {sname} | {1e3 * r:.2f} | {1e3 * f:.2f} | {f / r:.1f}x | '
                        f'{tm["tiles_decoded"]}/{tm["tiles_total"]} | {tm["payload_bytes_read"]}/{tm["bundle_bytes"]} | '
                        f'{mr / 2**20:.1f} / {mf / 2**20:.1f} | split read {1e3 * tm["read"]:.2f} device '
                        f'{1e3 * tm["device"]:.2f} d2h {1e3 * tm["d2h"]:.2f} ms')
        if a.tile_crc or a.only_tile_crc:
            tile_crc_rows(a, vol.reshape(1, n, n, n, 1), mid, d, say)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
