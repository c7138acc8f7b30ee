#!/usr/bin/env python
"""Times the model regulariser (sepfwi.regularize.Regularizer) on the GPU: the value-and-gradient launch and the product launch for
three fields of nz x nx cells, against the same expressions in eager torch on the same device (regularize.USE_FUSED = False).
Device events around windows of `--reps` calls, after a warm-up of each path; the two paths alternate, `--windows` times each, and
every window is printed (the spread is the noise).  Recorded, not asserted: profiles/r22_model_regularisation.txt.

    python scripts/regularizer_bench.py [--nz 1000 --nx 2000 --reps 200 --windows 5]

Bytes per call, counted from the shapes: the launches read p, p0 (v for the product) and W and write g (Hv) once per field,
12 arrays of 4 nz nx bytes (the shifted re-reads of p hit the caches)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sep-2023_amd")]
from sepfwi import regularize  # noqa: E402


class _Fields(torch.nn.Module):
    NAMES = ("Vp", "Vs", "Den")
    para_fname = None

    def __init__(self, nz, nx):
        super().__init__()
        g = torch.Generator(device="cuda").manual_seed(1)
        for n, b in zip(self.NAMES, (3000.0, 1700.0, 2400.0)):
            setattr(self, n, torch.nn.Parameter(b * (1.0 + 0.05 * torch.randn(nz, nx, device="cuda", generator=g))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nz", type=int, default=1000)
    ap.add_argument("--nx", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    mod = _Fields(a.nz, a.nx)
    prior = [1.01 * getattr(mod, n).detach() for n in mod.NAMES]
    W = (torch.rand(a.nz, a.nx, device="cuda") > 0.2).float()
    reg = regularize.Regularizer(mod, alpha=0.5, beta=0.3, gamma=1.0, eps=2e-3, prior=prior, weight=W, dx=10.0, dz=7.5)
    v = tuple(0.02 * getattr(mod, n).detach() * torch.randn(a.nz, a.nx, device="cuda") for n in mod.NAMES)
    calls = {"value_and_grad": reg.value_and_grad, "hvp": lambda: reg.hvp(v)}

    def window(fn, reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / reps      # microseconds per call

    out = {"nz": a.nz, "nx": a.nx, "reps": a.reps, "bytes_per_call": 12 * 4 * a.nz * a.nx}
    for what, fn in calls.items():
        for fused in (True, False):      # warm-up of both paths
            regularize.USE_FUSED = fused
            window(fn, 5)
        t = {True: [], False: []}
        for _ in range(a.windows):
            for fused in (True, False):
                regularize.USE_FUSED = fused
                t[fused].append(window(fn, a.reps if fused else max(a.reps // 10, 5)))
        regularize.USE_FUSED = True
        med = lambda x: sorted(x)[len(x) // 2]
        out[what] = {"fused_us": [round(x, 2) for x in t[True]], "torch_us": [round(x, 1) for x in t[False]],
                     "fused_us_median": round(med(t[True]), 2), "torch_us_median": round(med(t[False]), 1),
                     "fused_gbytes_per_s": round(out["bytes_per_call"] / med(t[True]) / 1e3, 1)}
        print("%s: fused %s us per call (median %.2f, %.0f GB/s of the counted bytes), eager torch %s us (median %.1f): %.0f x" % (
            what, out[what]["fused_us"], out[what]["fused_us_median"], out[what]["fused_gbytes_per_s"], out[what]["torch_us"],
            out[what]["torch_us_median"], out[what]["torch_us_median"] / out[what]["fused_us_median"]), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
