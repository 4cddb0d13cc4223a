"""compress / decompress of a 512^3 uint16 smooth-plus-noise volume at max_error 0, 1, 2, 4: file size,
bits per sample and the last_timing splits; three rounds, the deltas alternated within each."""
import json, os, sys, tempfile
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kompressor_amd as kom
from kompressor_amd import container

rng = np.random.default_rng(0)
n = 512
ax = np.linspace(0, 1, n, dtype=np.float32)
f = np.zeros((n, n, n), np.float32)
for _ in range(4):
    k = rng.uniform(0.5, 2.5, 3).astype(np.float32); ph = np.float32(rng.uniform(0, 2 * np.pi))
    f += np.sin(2 * np.pi * (k[0] * ax[:, None, None] + k[1] * ax[None, :, None] + k[2] * ax[None, None, :]) + ph)
f /= np.abs(f).max()
x = np.clip(np.round(2000 + 300 * f + 20 * rng.standard_normal((n, n, n), dtype=np.float32)), 0, 65535).astype(np.uint16)
x = x.reshape(1, n, n, n, 1)
xt = torch.from_numpy(x).cuda()
pred = kom.MeanPredictor(0, 3)
d = tempfile.mkdtemp(dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
out = {}
for rnd in range(4):
    for delta in (0, 1, 2, 4):
        path = os.path.join(d, f'v{delta}.kmp')
        res = container.compress(path, xt, pred, levels=3, max_error=delta)
        tc = dict(container.last_timing)
        torch.cuda.synchronize()
        y = container.decompress(path, as_numpy=False)
        td = dict(container.last_timing)
        err = kom.near.d_max_abs_error(y, xt)
        assert err == delta, (delta, err)
        if rnd:  # round 0 warms up
            out.setdefault(delta, []).append((res, tc, td))
        os.remove(path)
for delta, runs in out.items():
    med = lambda xs: float(np.median(xs))
    res = runs[0][0]
    line = {'max_error': delta, 'bytes': res['bytes'], 'bits_per_sample': round(res['bits_per_sample'], 4),
            'max_abs_error': res['max_abs_error'],
            'compress_ms': {k: [round(1e3 * f([r[1][k] for r in runs]), 2) for f in (med, min, max)] for k in runs[0][1]},
            'decompress_ms': {k: [round(1e3 * f([r[2][k] for r in runs]), 2) for f in (med, min, max)]
                              for k in runs[0][2] if isinstance(runs[0][2][k], float)}}
    print(json.dumps(line), flush=True)
