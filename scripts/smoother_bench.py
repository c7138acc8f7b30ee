#!/usr/bin/env python
"""Times the smoothing operator (sepfwi.smooth.Smoother) on the GPU: one application of S to three fields of nz x nx cells (two
launches: the z pass, then the x pass) at constant widths of `--sigmas` cells (radius 3 sigma), against two device-to-device copies of
the same three fields in the same process -- the least traffic two passes can have, a yardstick that is none of this code.  Device
events around windows of `--reps` calls after a warm-up of each; `--windows` windows each, alternating; every window is printed (the
spread is the noise) and the median is the figure.  Recorded, not asserted: profiles/r26_smoother.txt.

    python scripts/smoother_bench.py [--nz 1000 --nx 2000 --sigmas 4 12 --reps 20 --windows 20]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sep-2023_amd")]
from sepfwi.smooth import Smoother  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nz", type=int, default=1000)
    ap.add_argument("--nx", type=int, default=2000)
    ap.add_argument("--sigmas", type=float, nargs="+", default=[4.0, 12.0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    g = torch.Generator(device="cuda").manual_seed(1)
    u = tuple(b * torch.randn(a.nz, a.nx, device="cuda", generator=g) for b in (300.0, 170.0, 24.0))
    mid, dst = [torch.empty_like(t) for t in u], [torch.empty_like(t) for t in u]

    def copies():
        for s, m, d in zip(u, mid, dst):
            m.copy_(s)
            d.copy_(m)

    def window(fn, reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / reps      # microseconds per call

    med = lambda x: sorted(x)[len(x) // 2]
    out = {"nz": a.nz, "nx": a.nx, "reps": a.reps, "windows": a.windows}
    for sigma in a.sigmas:
        sm = Smoother((a.nz, a.nx), sigma, sigma, unit="cells")
        apply = lambda: sm.apply(u)
        window(apply, 3), window(copies, 3)
        t_s, t_c = [], []
        for _ in range(a.windows):
            t_s.append(window(apply, a.reps))
            t_c.append(window(copies, a.reps))
        key = "sigma_%g" % sigma
        out[key] = {"radius": sm.radius, "apply_us": [round(x, 1) for x in t_s], "copies_us": [round(x, 1) for x in t_c],
                    "apply_us_median": round(med(t_s), 1), "copies_us_median": round(med(t_c), 1), "ratio": round(med(t_s) / med(t_c), 2)}
        print("sigma %g cells (radii %s): S of three fields %.1f us (median of %d windows, min %.1f max %.1f), two copies of them %.1f us: ratio %.2f" % (
            sigma, sm.radius, med(t_s), a.windows, min(t_s), max(t_s), med(t_c), med(t_s) / med(t_c)), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
