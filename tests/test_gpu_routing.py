"""Which kernel family serves which request: one table for the fused codec's dispatch.

Each row is a configuration with the launch names ``kmp_last_launch()`` reports after its encode and
its decode.  The expected names are literals recorded from the library as it was before the
dispatch moved into one table (kmp_codec.hip), so a reordered or dropped table entry shows
up here as a changed name.  Every row also checks that one family serves both directions and that
the round trip is lossless."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U8, U16, I32 = np.uint8, np.uint16, np.int32

# (id, shape, dtype, predictor, padding, options, chunk, encode launch, decode launch)
#   predictor: 'mean', 'f32' (LinearPredictor, the fma chain) or 'bf16x2' (the matrix cores)
#   chunk: None = whole-array encode / decode; an int = encode_chunks / decode_chunks regions
ROWS = [
    # ---- volumes ----
    ('vol-u8-p0', (2, 12, 16, 64, 1), U8, 'mean', 0, {}, None, 'wave3d_encode', 'wave3d_decode'),
    ('vol-u8-p1', (2, 12, 16, 64, 1), U8, 'mean', 1, {}, None, 'wave3dp_encode', 'wave3dp_decode'),
    ('vol-u8-p2', (2, 12, 16, 64, 1), U8, 'mean', 2, {}, None, 'wave3dp_encode', 'wave3dp_decode'),
    ('vol-u16-p0', (2, 12, 16, 64, 1), U16, 'mean', 0, {}, None, 'wave3d_encode', 'wave3d_decode'),
    ('vol-u16-p1', (2, 12, 16, 64, 1), U16, 'mean', 1, {}, None, 'wave3dp_encode', 'wave3dp_decode'),
    ('vol-u16-p2', (2, 12, 16, 64, 1), U16, 'mean', 2, {}, None, 'wave3dr_encode', 'wave3dr_decode'),
    ('vol-i32-p0', (2, 8, 10, 32, 1), I32, 'mean', 0, {}, None, 'wave3d32_encode', 'wave3d32_decode'),
    # 6 lanes per row is not a power of two: no wave kernel, the LDS kernel
    ('vol-u16-w48-p1', (2, 9, 12, 48, 1), U16, 'mean', 1, {}, None, 'fast3d_encode', 'fast3d_decode'),
    ('vol-u8-c3', (1, 8, 16, 32, 3), U8, 'mean', 0, {}, None, 'encode_generic', 'decode_generic'),
    ('vol-lin-f32-p0', (1, 6, 32, 32, 1), U16, 'f32', 0, {}, None, 'linear3y_encode', 'linear3y_decode'),
    ('vol-lin-f32-p0-oddh', (2, 9, 15, 32, 1), U16, 'f32', 0, {}, None, 'linear3d_encode', 'linear3d_decode'),
    ('vol-lin-f32-p1', (2, 9, 14, 32, 1), U16, 'f32', 1, {}, None, 'linear3dp_encode', 'linear3dp_decode'),
    ('vol-lin-mfma-p0', (2, 16, 32, 32, 1), U16, 'bf16x2', 0, {}, None, 'linear3m_encode', 'linear3m_decode'),
    ('vol-lin-mfma-p1', (1, 8, 32, 64, 1), U16, 'bf16x2', 1, {}, None, 'linear3pm_encode', 'linear3pm_decode'),
    # ---- images ----
    ('img-u8-p0', (2, 32, 64, 1), U8, 'mean', 0, {}, None, 'wave2d_encode', 'wave2d_decode'),
    ('img-u8-p1', (2, 32, 64, 1), U8, 'mean', 1, {}, None, 'wave2dr_encode', 'wave2dr_decode'),
    ('img-u8-p2', (2, 32, 64, 1), U8, 'mean', 2, {}, None, 'wave2dr_encode', 'wave2dr_decode'),
    ('img-u16-p0', (2, 32, 64, 1), U16, 'mean', 0, {}, None, 'wave2d_encode', 'wave2d_decode'),
    ('img-u16-p1', (2, 32, 64, 1), U16, 'mean', 1, {}, None, 'wave2dr_encode', 'wave2dr_decode'),
    ('img-u16-p2', (2, 32, 64, 1), U16, 'mean', 2, {}, None, 'wave2dr_encode', 'wave2dr_decode'),
    ('img-lin-f32-p0', (3, 64, 64, 1), U16, 'f32', 0, {}, None, 'wave2d_encode', 'wave2d_decode'),
    ('img-u16-w48-p2', (2, 31, 48, 1), U16, 'mean', 2, {}, None, 'fast2d_encode', 'fast2d_decode'),
    ('img-u8-c3', (2, 16, 32, 3), U8, 'mean', 0, {}, None, 'encode_generic', 'decode_generic'),
    # ---- dispatch options ----
    ('opt-wave-vol', (2, 12, 16, 64, 1), U16, 'mean', 1, {'KMP_DISABLE_WAVE': 1}, None,
     'fast3d_encode', 'fast3d_decode'),
    ('opt-wave-img', (2, 32, 64, 1), U8, 'mean', 0, {'KMP_DISABLE_WAVE': 1}, None, 'fast2d_encode', 'fast2d_decode'),
    ('opt-fast-vol', (2, 9, 12, 48, 1), U16, 'mean', 1, {'KMP_DISABLE_FAST': 1}, None,
     'encode_generic', 'decode_generic'),
    ('opt-fast-img', (2, 31, 48, 1), U16, 'mean', 2, {'KMP_DISABLE_FAST': 1}, None,
     'encode_generic', 'decode_generic'),
    ('opt-linfused-vol', (1, 6, 32, 32, 1), U16, 'f32', 0, {'KMP_DISABLE_LINEAR_FUSED': 1}, None,
     'encode_generic', 'decode_generic'),
    ('opt-linfused-img', (3, 64, 64, 1), U16, 'f32', 0, {'KMP_DISABLE_LINEAR_FUSED': 1}, None,
     'encode_generic', 'decode_generic'),
    # ---- regions (the chunked drivers' z slabs / row ranges) ----
    ('region-vol-z', (2, 12, 16, 64, 1), U16, 'mean', 1, {}, 5, 'wave3dp_encode', 'wave3dp_decode'),
    ('region-img-rows', (2, 32, 64, 1), U8, 'mean', 2, {}, 5, 'wave2dr_encode', 'wave2dr_decode'),
]


def _family(name):
    """'wave3dr_encode' -> 'wave3dr', 'decode_generic' -> 'generic'."""
    parts = [s for s in name.split('_') if s not in ('encode', 'decode')]
    assert len(parts) + 1 == len(name.split('_')), name
    return '_'.join(parts)


def _predictor(kom, kind, p, ndim, dtype):
    if kind == 'mean':
        return kom.MeanPredictor(p, ndim)
    n, k = (2 * p + 2) ** ndim, 19 if ndim == 3 else 5
    rng = np.random.default_rng(41)
    w = (1.0 / n + rng.standard_normal((n, k)) * (0.3 / n)).astype(np.float32)
    b = (rng.standard_normal(k) * 50.0).astype(np.float32)
    return kom.LinearPredictor(w, b, p, ndim, arith=kind)


def run_row(kom, set_option, row):
    """Runs one row; returns the launch names of its encode and decode (asserts the round trip)."""
    _, shape, dtype, kind, p, options, chunk, _, _ = row
    for name, value in options.items():
        set_option(name, value)
    ndim = len(shape) - 2
    ns = kom.volume if ndim == 3 else kom.image
    coder = {U8: 'uint8', U16: 'uint16', I32: 'raw'}[dtype]
    enc, dec = getattr(ns, 'encode_values_' + coder), getattr(ns, 'decode_values_' + coder)
    info = np.iinfo(dtype)
    x = np.random.default_rng(40).integers(info.min, info.max + 1, size=shape, dtype=np.int64).astype(dtype)
    pred = _predictor(kom, kind, p, ndim, dtype)
    last = lambda: kom._lib.lib.kmp_last_launch().decode()  # noqa: E731
    if chunk is None:
        lo, encoded = ns.encode(pred, enc, x, padding=p)
        got_enc = last()
        back = ns.decode(pred, dec, lo, encoded, padding=p)
        got_dec = last()
    else:
        lo, encoded = ns.encode_chunks(pred, enc, x, chunk=chunk, padding=p)
        got_enc = last()
        back = ns.decode_chunks(pred, dec, lo, encoded, chunk=chunk, padding=p)
        got_dec = last()
    assert np.array_equal(back, x), 'round trip is not lossless'
    return got_enc, got_dec


@pytest.mark.parametrize('row', ROWS, ids=[r[0] for r in ROWS])
def test_routing(kom, kmp_opt, row):
    got_enc, got_dec = run_row(kom, kmp_opt, row)
    print(row[0], got_enc, got_dec)
    assert (got_enc, got_dec) == (row[7], row[8])
    assert got_enc.count('encode') == 1 and got_dec.count('decode') == 1
    assert _family(got_enc) == _family(got_dec)
