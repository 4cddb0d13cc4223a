#!/usr/bin/env python3
"""Store policy and block order of the one-pass codec, measured on the pipelines that follow an
encode.

    python tools/pipeline_rows.py [--reps N] [--workload volume|image] [--padding P] [--tiles T]
                                  [--cand parent,0:0,1:0,1:65536,...] [--tag NAME]
    python tools/pipeline_rows.py --summarize LOG [LOG ...]

Without --cand: the encode's lowres / map stores either allocate in the MALL (default policy,
knob = 1) or stream past it (non-temporal, 0).  Volume: C3, 512 x 64^3 uint16 (KMP_W3_ST_ENC for
p = 0, KMP_W3P_ST_ENC for p = 1, 2); image: C2, 1024 x 256^2 uint8 (KMP_W2_ST_ENC / KMP_W2P_ST_ENC).

With --cand (volume, p = 0): each candidate is ``rev:tail`` = KMP_W3_DEC_REV : KMP_W3_ST_TAIL in
KiB (decode order and the cached tail of the encode's output, kmp_codec_wave3d.hip), or ``parent``:
no option is touched, for a run against another build of the library (KOMPRESSOR_HIP_LIB).  One
process measures all its candidates in turn; alternate processes to alternate libraries.
--tiles takes the first T tiles of the volume (128: a working set that fits the MALL).

Rows (one JSON line each, per candidate; device time from HIP events over ``reps`` iterations):
  bench      encode -> decode alternating (bench.py's timed loop)
  enc_stream encode back to back with itself (a producer that only encodes)
  compress   encode -> Rice bundle encode of its 8 outputs (the file path: container.compress)
  decompress Rice bundle decode -> decode (container.decompress)
The Rice launches are kompressor_amd.packing's own (no host synchronisation inside the loop).

--summarize reads such logs and applies the rule for a default: per (tiles, row) the
noise is the spread (max - min) of the parent's runs; a candidate qualifies if its bench row at 512
tiles gains more than twice that noise and no row at any tile count loses more than its noise.
"""
import argparse
import collections
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summarize(paths):
    runs = collections.defaultdict(list)  # (tiles, row, cand) -> [us]
    for p in paths:
        for line in open(p):
            if not line.startswith('{'):
                continue
            d = json.loads(line)
            if 'cand' in d:
                runs[(d['tiles'], d['row'].rsplit(':', 1)[1], d['cand'])].append(d['us_per_iter'])
    keys = sorted({(t, r) for t, r, _ in runs})
    cands = sorted({c for _, _, c in runs if c != 'parent'})
    verdict = {c: {'gain': None, 'lost': []} for c in cands}
    for t, r in keys:
        par = runs.get((t, r, 'parent'))
        if not par:
            continue
        noise, pmean = max(par) - min(par), sum(par) / len(par)
        print(f'tiles={t:<4} {r:<11} parent mean {pmean:7.1f} us  min {min(par):7.1f}  max {max(par):7.1f}  '
              f'noise {noise:5.1f}  (n={len(par)})')
        for c in cands:
            v = runs.get((t, r, c))
            if not v:
                continue
            mean = sum(v) / len(v)
            d = mean - pmean
            print(f'           {"":<11} {c:<9} mean {mean:7.1f} us  delta {d:+6.1f}  (n={len(v)})')
            if r == 'bench' and t == 512:
                verdict[c]['gain'] = (-d, noise)
            elif d > noise:
                verdict[c]['lost'].append(f'{r}@{t} {d:+.1f} > {noise:.1f}')
    for c in cands:
        g = verdict[c]['gain']
        ok = g is not None and g[0] > 2 * g[1] and not verdict[c]['lost']
        print(f'candidate {c:<9} bench@512 gain {g[0] if g else float("nan"):+6.1f} us vs 2 x noise '
              f'{2 * g[1] if g else float("nan"):5.1f}; rows lost: {verdict[c]["lost"] or "none"} -> '
              f'{"QUALIFIES" if ok else "does not qualify"}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--workload', default='volume')
    ap.add_argument('--padding', type=int, default=0)
    ap.add_argument('--tiles', type=int, default=512)
    ap.add_argument('--cand', default='')
    ap.add_argument('--tag', default='')
    ap.add_argument('--summarize', nargs='+')
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    vol3 = args.workload == 'volume'
    knob = ('KMP_W3_ST_ENC' if args.padding == 0 else 'KMP_W3P_ST_ENC') if vol3 else \
           ('KMP_W2_ST_ENC' if args.padding == 0 else 'KMP_W2P_ST_ENC')
    if args.cand:
        assert vol3 and args.padding == 0, '--cand: the volume p = 0 kernel'
        cands = []
        for c in args.cand.split(','):
            cands.append((c, {} if c == 'parent' else dict(zip(('KMP_W3_DEC_REV', 'KMP_W3_ST_TAIL'), map(int, c.split(':'))))))
    else:
        cands = [(None, {knob: 1}), (None, {knob: 0})]
    import torch
    import kompressor_amd as kom
    from kompressor_amd import _lib, _nd, packing as kpk
    torch.cuda.set_device(0)
    # a structured volume / image set (the Rice stage's cost depends on the residuals): smooth field + noise
    gen = torch.Generator(device='cuda').manual_seed(0)
    if vol3:
        zz, yy, xx = torch.meshgrid(*[torch.arange(512, device='cuda', dtype=torch.float32)] * 3, indexing='ij')
        f = torch.sin(xx / 41.0) * torch.cos(yy / 29.0) + torch.sin(zz / 53.0 + xx / 97.0)
        f = 4000 + 9000 * (f - f.min()) / (f.max() - f.min())
        del zz, yy, xx
        vol = (f + 4 * torch.randn(f.shape, device='cuda', generator=gen)).round().clamp(0, 65535).to(torch.int32)
        hi = vol.to(torch.uint16).view(8, 64, 8, 64, 8, 64).permute(0, 2, 4, 1, 3, 5).reshape(512, 64, 64, 64, 1)
        hi = hi[:args.tiles].contiguous()
        del f, vol
    else:
        yy, xx = torch.meshgrid(*[torch.arange(256, device='cuda', dtype=torch.float32)] * 2, indexing='ij')
        ph = torch.rand((1024, 1, 1), device='cuda', generator=gen) * 6.28
        f = 128 + 80 * torch.sin(xx / 23.0 + ph) * torch.cos(yy / 31.0 - ph)
        hi = (f + 2 * torch.randn(f.shape, device='cuda', generator=gen)).round().clamp(0, 255).to(torch.uint8)
        hi = hi.reshape(1024, 256, 256, 1).contiguous()
        del f
    torch.cuda.empty_cache()
    ndim = 3 if vol3 else 2
    pred = kom.MeanPredictor(args.padding, ndim)
    coder = _nd.NATURAL_CODER[hi.dtype]
    lo, maps, dims = _nd._alloc_encoded(hi, coder, ndim)
    rec = torch.empty_like(hi)
    ws = torch.empty(max(1, _nd.workspace_bytes(hi, pred, ndim)), dtype=torch.uint8, device='cuda')
    enc = lambda: _nd.fused_encode_into(hi, pred, coder, lo, maps, ndim, workspace=ws)  # noqa: E731
    dec = lambda: _nd.fused_decode_into(lo, maps, dims, pred, coder, rec, ndim, workspace=ws)  # noqa: E731
    enc()
    blob = kpk.pack_encoded(lo, (maps, dims))
    hb = blob[:4096].cpu().numpy().tobytes()
    raw = hi.numel() * hi.element_size()

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(50_000_000)  # keep the GPU busy while the host enqueues (no host-bound intervals)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps / 1e3

    pipes = {
        'bench': lambda: (enc(), dec()),
        'enc_stream': enc,
        'compress': lambda: (enc(), kpk._rice_encode_launch((lo, *maps), dims)),
        'decompress': lambda: (kpk._rice_decode_launch(blob, hb), dec()),
    }
    for rep in range(2):
        for name, fn in pipes.items():
            for cand, opts in cands:
                # the library reads its environment once, at load: options go through its table
                for k, v in opts.items():
                    _lib.set_option(k, v)
                t = timed(fn)
                for k in opts:
                    _lib.set_option(k, None)
                row = {'row': f'pipeline:{args.workload}_p{args.padding}:{name}', **opts,
                       'us_per_iter': round(t * 1e6, 1), 'raw_GBps': round(raw / t / 1e9, 1), 'rep': rep}
                if cand is not None:
                    row.update(cand=cand, tiles=args.tiles, tag=args.tag)
                print(json.dumps(row), flush=True)
    enc()
    dec()
    torch.cuda.synchronize()
    assert torch.equal(rec, hi)


if __name__ == '__main__':
    main()
