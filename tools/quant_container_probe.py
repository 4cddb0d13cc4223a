"""compress / decompress of a 512^3 float32 smooth-plus-noise field at abs_error None, 1e-1, 1e-2, 1e-3:
file size, bits per sample and the last_timing splits; three timed rounds, the bounds alternated within
each.  ``--nan`` turns about 10 % of the volume (a slab of planes) into NaN: the cost of the exception
path; ``--runs`` next to it stores the exceptions as runs over hold-filled integers (DESIGN.md §21:
``exceptions='runs'`` at every bound).  ``--lossless-only`` runs the ``None`` row alone and passes no keyword, so the same script
measures a build from before error-bounded coding.  ``--rel`` measures the relative mode instead
(DESIGN.md §18): the field becomes ``10 ** (2 f)`` -- four decades -- times ``1 + noise / 15``, and the
bounds are ``rel_error`` None, 1e-1, 1e-2, 1e-3.  ``--target`` measures rate control instead (DESIGN.md
§19): ``compress(target_bits=4 / 8)`` against ``compress(abs_error=the chosen bound)``, the probes it
made and the time of one probe.  ``--psnr`` measures quality targets:
``compress(target_psnr=60 / 90)`` against ``compress(abs_error=the chosen bound)``, the probes, and the
time of the quality pass every lossy ``compress`` now holds.  ``--ssim`` measures structural targets (DESIGN.md
§23): ``compress(target_ssim=0.99)`` against ``compress(abs_error=the chosen bound)``, the probes and the time
of one probe."""
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
x = (f + rng.standard_normal((n, n, n), dtype=np.float32) / 15).astype(np.float32)  # noise 1/15 of the amplitude
REL = '--rel' in sys.argv
RUNS = {'exceptions': 'runs'} if '--runs' in sys.argv else {}
KEY, MAX = ('rel_error', 'max_rel_error') if REL else ('abs_error', 'max_abs_error')
if REL:  # multiplicative noise on a field that spans four decades
    x = (np.power(np.float32(10), 2 * f) * (1 + rng.standard_normal((n, n, n), dtype=np.float32) / 15)).astype(np.float32)
if '--nan' in sys.argv:
    x[200:251] = np.nan
x = x.reshape(1, n, n, n, 1)
xt = torch.from_numpy(x).cuda()
pred = kom.MeanPredictor(0, 3)
d = tempfile.mkdtemp(dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
bounds = (None,) if '--lossless-only' in sys.argv else (None, 1e-1, 1e-2, 1e-3)
out = {}
if '--target' in sys.argv:
    # rate control: compress(target_bits=b) against compress(abs_error=chosen) on the same
    # field, alternated over three timed rounds; the probe count and the device time of one probe
    # (compressed_size at the chosen rung, synchronised)
    import time
    path = os.path.join(d, 'v.kmp')
    for bits in (4.0, 8.0):
        rows = {'target': [], 'explicit': [], 'probe': []}
        for rnd in range(4):
            res = container.compress(path, xt, pred, levels=3, target_bits=bits)
            tt = dict(container.last_timing)
            target_bytes = open(path, 'rb').read()
            ex = container.compress(path, xt, pred, levels=3, abs_error=res['abs_error'])
            te = dict(container.last_timing)
            assert open(path, 'rb').read() == target_bytes and res['bits_per_sample'] <= bits
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sized = container.compressed_size(xt, pred, levels=3, abs_error=res['abs_error'])
            torch.cuda.synchronize()
            tp = time.perf_counter() - t0
            assert sized['bound_bytes'] == res['bound_bytes']
            if rnd:
                rows['target'].append(tt['total']); rows['explicit'].append(te['total']); rows['probe'].append(tp)
        stat = lambda xs: [round(1e3 * f(xs), 2) for f in (lambda v: float(np.median(v)), min, max)]
        print(json.dumps({'target_bits': bits, 'abs_error': res['abs_error'], 'bits_per_sample': round(res['bits_per_sample'], 4),
                          'bytes': res['bytes'], 'target_bytes': res['target_bytes'], 'bound_bytes': res['bound_bytes'],
                          'probes': len(res['probes']), 'probe_rungs': [p[0] for p in res['probes']],
                          'target_total_ms': stat(rows['target']), 'explicit_total_ms': stat(rows['explicit']),
                          'one_probe_ms': stat(rows['probe'])}), flush=True)
    os.remove(path)
    sys.exit(0)
if '--psnr' in sys.argv:
    # quality targets: compress(target_psnr=dB) against compress(abs_error=chosen) on the same
    # field, alternated over three timed rounds; the probes it made, and the device time of the quality
    # pass the explicit call now holds (restore and compare in slabs, one read-back; synchronised)
    import time
    from kompressor_amd import quant, _lib
    path = os.path.join(d, 'v.kmp')
    for db in (60.0, 90.0):
        rows = {'target': [], 'explicit': [], 'quality': []}
        for rnd in range(4):
            res = container.compress(path, xt, pred, levels=3, target_psnr=db)
            tt = dict(container.last_timing)
            target_bytes = open(path, 'rb').read()
            ex = container.compress(path, xt, pred, levels=3, abs_error=res['abs_error'])
            te = dict(container.last_timing)
            assert open(path, 'rb').read() == target_bytes and res['psnr'] >= db and ex['psnr'] == res['psnr']
            e = quant.exponent(res['abs_error'])
            nq, exc = quant.d_quantise(xt, e)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q = container._quality(container._restored_record(xt, nq, lambda s: quant.d_code(_lib.DECODE, nq.dtype, e, s), exc),
                                   xt.dtype)
            tq = time.perf_counter() - t0
            assert q['psnr'] == res['psnr']
            del nq
            if rnd:
                rows['target'].append(tt['total']); rows['explicit'].append(te['total']); rows['quality'].append(tq)
        stat = lambda xs: [round(1e3 * f(xs), 2) for f in (lambda v: float(np.median(v)), min, max)]
        print(json.dumps({'target_psnr': db, 'abs_error': res['abs_error'], 'psnr': res['psnr'],
                          'bits_per_sample': round(res['bits_per_sample'], 4), 'bytes': res['bytes'],
                          'probes': len(res['probes']), 'probe_rungs': [p[0] for p in res['probes']],
                          'target_total_ms': stat(rows['target']), 'explicit_total_ms': stat(rows['explicit']),
                          'quality_pass_ms': stat(rows['quality'])}), flush=True)
    os.remove(path)
    sys.exit(0)
if '--ssim' in sys.argv:
    # structural targets: compress(target_ssim=0.99) against compress(abs_error=chosen) on the same
    # field, alternated over three timed rounds; the probes it made, and the time of one probe (the quantiser,
    # the whole array restored, one SSIM call and its read-back; synchronised)
    import time
    from kompressor_amd import metrics, quant, _lib
    path = os.path.join(d, 'v.kmp')
    rows = {'target': [], 'explicit': [], 'probe': []}
    for rnd in range(4):
        res = container.compress(path, xt, pred, levels=3, target_ssim=0.99)
        tt = dict(container.last_timing)
        target_bytes = open(path, 'rb').read()
        ex = container.compress(path, xt, pred, levels=3, abs_error=res['abs_error'])
        te = dict(container.last_timing)
        assert open(path, 'rb').read() == target_bytes and res['ssim'] >= 0.99
        e = quant.exponent(res['abs_error'])
        frame = metrics.ssim(xt, xt)  # peak and base, outside the timed probe
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nq, exc = quant.d_quantise(xt, e)
        r = container._restored_whole(nq, lambda s: quant.d_code(_lib.DECODE, nq.dtype, e, s), exc)
        words = metrics.record_words(metrics.d_ssim(metrics._items(xt), metrics._items(r), metrics.ssim_dims(xt.shape)[1:],
                                                    *metrics.ssim_constants(frame['peak']), frame['base']))
        tp = time.perf_counter() - t0
        assert metrics.ssim_summary(words)['ssim'] == res['ssim']
        del nq, r
        if rnd:
            rows['target'].append(tt['total']); rows['explicit'].append(te['total']); rows['probe'].append(tp)
    stat = lambda xs: [round(1e3 * f(xs), 2) for f in (lambda v: float(np.median(v)), min, max)]
    print(json.dumps({'target_ssim': 0.99, 'abs_error': res['abs_error'], 'ssim': res['ssim'], 'psnr': res['psnr'],
                      'bits_per_sample': round(res['bits_per_sample'], 4), 'bytes': res['bytes'],
                      'probes': len(res['probes']), 'probe_rungs': [p[0] for p in res['probes']],
                      'target_total_ms': stat(rows['target']), 'explicit_total_ms': stat(rows['explicit']),
                      'one_probe_ms': stat(rows['probe'])}), flush=True)
    os.remove(path)
    sys.exit(0)
for rnd in range(4):
    for a in bounds:
        path = os.path.join(d, 'v.kmp')
        res = container.compress(path, xt, pred, levels=3, **({} if a is None else {KEY: a, **RUNS}))
        tc = dict(container.last_timing)
        torch.cuda.synchronize()
        y = container.decompress(path, as_numpy=False)
        td = dict(container.last_timing)
        if a is None:
            assert torch.equal(y.view(torch.int32), xt.view(torch.int32))
        else:
            err = (y.double() - xt.double()).abs()
            if REL:
                err /= xt.double().abs().clamp_min(2.0 ** -126)
            assert float(err[torch.isfinite(xt)].max().item()) == res[MAX] <= res[KEY]
            assert torch.equal(y.view(torch.int32)[~torch.isfinite(xt)], xt.view(torch.int32)[~torch.isfinite(xt)])
            del err
        del y
        if rnd:  # round 0 warms up
            out.setdefault(a, []).append((res, tc, td))
        os.remove(path)
for a, runs in out.items():
    med = lambda xs: float(np.median(xs))
    res = runs[0][0]
    line = {KEY: a, 'nan_slab': '--nan' in sys.argv, 'runs': bool(RUNS), 'bytes': res['bytes'],
            'bits_per_sample': round(res['bits_per_sample'], 4),
            **{k: res[k] for k in (KEY, MAX, 'exceptions', 'exception_runs', 'quant_dtype') if k in res and a is not None},
            KEY + '_asked': a,
            'compress_ms': {k: [round(1e3 * f([r[1][k] for r in runs]), 2) for f in (med, min, max)] for k in runs[0][1]},
            'decompress_ms': {k: [round(1e3 * f([r[2][k] for r in runs]), 2) for f in (med, min, max)]
                              for k in runs[0][2] if isinstance(runs[0][2][k], float)}}
    print(json.dumps(line), flush=True)
