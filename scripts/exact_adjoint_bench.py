#!/usr/bin/env python
"""Cost of the exact discrete adjoint (csrc/exact_adjoint.hip) per backward time step on the headline model.

    python scripts/exact_adjoint_bench.py [--nz 1000 --nx 2000 --nsteps 400 --calls 4] [--parent-lib PATH]

One shot through the C ABI; `sepfwi_stats.bwd_ms` per time step (HIP events around the backward loop of the call's shot):
  * exact      sepfwi_adjoint_exact in its gradient mode: k_exact_a, injection, k_exact_b per step
  * two_launch sepfwi_cufd(calc_id 1) with option bwd_fuse = 2: k_bwd_a, k_bwd_b (+ injection) per step -- on this build and, with
               --parent-lib, on a library built from the parent commit
  * loop       sepfwi_cufd(calc_id 1) with the default bwd_fuse = 4 (the persistent loop), for scale
Calls are interleaved, two series per variant; the spread between the two series of one variant is the noise.  The exact step streams the
same arrays as the two-launch step and adds tap loads of media: anything beyond about 1.3 x wants an explanation.  Nothing is
asserted.  Prints one line per figure and a last line of JSON."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sep-2023_amd")]
import bench                                            # noqa: E402
from sepfwi import _native                              # noqa: E402


class Lib:
    def __init__(self, path, pb):
        L = C.CDLL(path)
        L.sepfwi_cufd.argtypes = [C.c_void_p] * 9 + [C.c_int] * 3 + [C.c_void_p, C.c_char_p]
        L.sepfwi_get_stats.argtypes = [C.c_char_p, C.c_int, C.POINTER(_native.Stats)]
        L.sepfwi_set_option.argtypes = [C.c_char_p, C.c_int]
        L.sepfwi_last_error.restype = C.c_char_p
        if hasattr(L, "sepfwi_adjoint_exact"):
            L.sepfwi_adjoint_exact.argtypes = [C.c_void_p] * 14 + [C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_void_p]
        self.L, self.pb, self.fn = L, pb, pb["para_fname"].encode()
        self.m = [t.cuda() for t in pb["lame_init"]]
        self.mt = [t.cuda() for t in pb["lame_true"]]
        self.g = [torch.zeros_like(self.m[0]) for _ in range(3)]
        self.gs = torch.zeros((1, pb["Stf"].shape[1]), dtype=torch.float32)
        self.misfit = torch.zeros(1, dtype=torch.float32)
        self.ids = np.zeros(1, np.int32)

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.sepfwi_last_error().decode(errors="replace"))

    def cufd(self, calc_id, true_model=False):
        p = lambda t: C.c_void_p(t.data_ptr())
        m = self.mt if true_model else self.m
        torch.cuda.synchronize()
        self._check(self.L.sepfwi_cufd(p(self.misfit), p(self.g[0]), p(self.g[1]), p(self.g[2]), p(self.gs), p(m[0]), p(m[1]), p(m[2]),
                                       C.c_void_p(self.pb["Stf"].data_ptr()), calc_id, 0, 1, C.c_void_p(self.ids.ctypes.data), self.fn))

    def exact(self):
        p = lambda t: C.c_void_p(t.data_ptr())
        torch.cuda.synchronize()
        self._check(self.L.sepfwi_adjoint_exact(p(self.misfit), p(self.g[0]), p(self.g[1]), p(self.g[2]), None, None, None, None, None, None,
                                                p(self.m[0]), p(self.m[1]), p(self.m[2]), C.c_void_p(self.pb["Stf"].data_ptr()), 0, 1,
                                                C.c_void_p(self.ids.ctypes.data), self.fn, None))

    def bwd_us(self):
        st = _native.Stats()
        self._check(self.L.sepfwi_get_stats(self.fn, 0, C.byref(st)))
        return 1e3 * st.bwd_ms / max(st.bwd_steps, 1), int(st.launches), int(st.persist_steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nz", type=int, default=1000)
    ap.add_argument("--nx", type=int, default=2000)
    ap.add_argument("--nsteps", type=int, default=400)
    ap.add_argument("--calls", type=int, default=4, help="calls per series (two series per variant)")
    ap.add_argument("--parent-lib", default=None, help="libsepfwi.so built from the parent commit, for the two-launch step there")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exact_adjoint_bench.py needs a HIP device")
    out = {"nz": a.nz, "nx": a.nx, "nsteps": a.nsteps, "calls_per_series": a.calls}
    with tempfile.TemporaryDirectory(prefix="sepfwi_exbench_") as work:
        def make(path, sub):
            d = os.path.join(work, sub)
            os.makedirs(d)
            lib = Lib(path, bench.setup_problem(d, a.nz, a.nx, a.nsteps, 1))
            lib.cufd(3, true_model=True)                    # observed data of the true model into the session's store
            return lib

        new = make(_native.LIB_PATH, "new")

        def fused(lib, fuse):
            def run():
                lib._check(lib.L.sepfwi_set_option(b"bwd_fuse", fuse))
                try:
                    lib.cufd(1)
                finally:
                    lib.L.sepfwi_set_option(b"bwd_fuse", 4)
                return lib.bwd_us()
            return run

        def exact():
            new.exact()
            return new.bwd_us()

        variants = [("exact", exact), ("two_launch", fused(new, 2)), ("loop", fused(new, 4))]
        if a.parent_lib:
            variants.append(("parent_two_launch", fused(make(a.parent_lib, "parent"), 2)))
        series = {name: [[], []] for name, _ in variants}
        info = {}
        for name, run in variants:      # warm-up, not counted
            run()
        for s in range(2):
            for _ in range(a.calls):
                for name, run in variants:
                    us, launches, persist = run()
                    series[name][s].append(us)
                    info[name] = (launches, persist)
        mean = {}
        for name, _ in variants:
            m = [float(np.mean(x)) for x in series[name]]
            mean[name] = float(np.mean(m))
            out[name] = {"bwd_us_per_step": m, "spread": abs(m[0] - m[1]), "launches": info[name][0], "persist_steps": info[name][1]}
            print("%-18s bwd %.2f / %.2f us per time step (two series of %d calls; spread %.2f), %d launches per call, %d steps in the loop"
                  % (name, m[0], m[1], a.calls, abs(m[0] - m[1]), info[name][0], info[name][1]))
        out["exact_over_two_launch"] = mean["exact"] / mean["two_launch"]
        print("exact / two-launch step = %.3f" % out["exact_over_two_launch"])
        if a.parent_lib:
            out["exact_over_parent_two_launch"] = mean["exact"] / mean["parent_two_launch"]
            print("exact / two-launch step of the parent build = %.3f" % out["exact_over_parent_two_launch"])
        new.L.sepfwi_release_all()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
