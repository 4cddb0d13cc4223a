"""The per-tile CRC table of a v2 Rice bundle, restated from the bundle's BYTES with ``zlib.crc32``
and the documented layout (oracle/rice.py "Bundle format v2") -- the independent
reference the kernel (``kmp_rice_tile_crc``), ``packing.tile_crcs`` and the container's trailer are
compared against.  Pure Python / numpy; knows nothing of the product.

    tile_crc(a, t) = zlib.crc32(params[256 t : 256 t + nbk] || bw[256 t : 256 t + nbk]
                                || payload words [toff[t], closing) as little-endian bytes)

with nbk = min(256, ceil(n_a / 64) - 256 t) and closing = toff[t + 1], or the array's end word after
its last tile; the table lists the arrays in bundle order, each array's tiles in order.
"""

import struct
import zlib

import numpy as np

TILE_BLOCKS = 256
BLOCK = 64


def tiles_of(n):
    """Tiles of an array of ``n`` samples."""
    return -(-(-(-n // BLOCK)) // TILE_BLOCKS) if n > 0 else 0


def bundle_arrays(b):
    """Per array of the bundle bytes ``b``: ``{'n', 'nb', 'nt', 'side', 'bw', 'toff', 'first', 'end'}``
    (byte offsets into the bundle; ``first`` / ``end`` in payload words), and the payload offset."""
    b = bytes(b)
    magic, version, count = struct.unpack('<4sHH', b[:8])
    assert magic == b'KMPB' and version == 2
    poff = struct.unpack('<Q', b[48:56])[0]
    out = []
    for i in range(count):
        n, nb, nt, side, toff, first, end = struct.unpack('<5q2Q', b[80 + 128 * i + 72:80 + 128 * (i + 1)])
        assert nb == -(-n // BLOCK) and nt == tiles_of(n)
        out.append({'n': n, 'nb': nb, 'nt': nt, 'side': side, 'bw': side + (nb + 7) // 8 * 8, 'toff': toff,
                    'first': first, 'end': end})
    return out, poff


def tile_bytes(b, a, t, arrays=None, poff=None):
    """The bytes tile ``t`` of array ``a`` is checksummed over."""
    b = bytes(b)
    if arrays is None:
        arrays, poff = bundle_arrays(b)
    r = arrays[a]
    nbk = min(TILE_BLOCKS, r['nb'] - TILE_BLOCKS * t)
    assert nbk >= 1
    tab = struct.unpack(f'<{r["nt"]}Q', b[r['toff']:r['toff'] + 8 * r['nt']])
    start = tab[t]
    closing = tab[t + 1] if t + 1 < r['nt'] else r['end']
    return (b[r['side'] + TILE_BLOCKS * t:r['side'] + TILE_BLOCKS * t + nbk]
            + b[r['bw'] + TILE_BLOCKS * t:r['bw'] + TILE_BLOCKS * t + nbk]
            + b[poff + 4 * start:poff + 4 * closing])


def tile_crc_table(b):
    """The uint32 table of the bundle bytes ``b`` in global tile order."""
    b = bytes(b)
    arrays, poff = bundle_arrays(b)
    return np.array([zlib.crc32(tile_bytes(b, a, t, arrays, poff)) & 0xffffffff
                     for a, r in enumerate(arrays) for t in range(r['nt'])], dtype=np.uint32)


def tile_begin(b):
    """The global index of every array's first tile (prefix sum of the arrays' tile counts)."""
    arrays, _ = bundle_arrays(b)
    return [int(v) for v in np.concatenate([[0], np.cumsum([r['nt'] for r in arrays])])[:-1]]


def crc32_bitwise(data):
    """CRC-32 one bit at a time (reflected 0xEDB88320, init and final xor 0xFFFFFFFF)."""
    c = 0xffffffff
    for byte in bytes(data):
        c ^= byte
        for _ in range(8):
            c = (c >> 1) ^ (0xEDB88320 if c & 1 else 0)
    return c ^ 0xffffffff
