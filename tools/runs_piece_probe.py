"""RUNS on the 10 % slab of 512 x 64^3 float32 for several piece sizes of the table (device-event time)."""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # the repository root
from kompressor_amd import quant

n = 512 * 64 ** 3
f32 = torch.zeros(n, dtype=torch.float32, device='cuda')
starts = torch.tensor([n // 3], device='cuda')
lengths = torch.tensor([n // 10], device='cuda')
bits = torch.tensor([0x7fc00000], device='cuda')


def gpu_time(fn, reps=10):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


tables = {p: quant.d_table(starts, lengths, bits, p) for p in (16384, 2048, 1024, 512, 256, 128, 64, 32)}
samples = {p: [] for p in tables}
for _ in range(7):
    for p, t in tables.items():
        samples[p].append(gpu_time(lambda t=t: quant.d_patch_runs(f32, t)))
for p, v in samples.items():
    print(json.dumps({'piece': p, 'records': int(tables[p].shape[0]), 'us': round(float(np.median(v)), 1),
                      'us_min': round(min(v), 1), 'us_max': round(max(v), 1)}), flush=True)
assert int((f32.view(torch.int32) == 0x7fc00000).sum().item()) == n // 10
