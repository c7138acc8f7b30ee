#!/usr/bin/env python
"""Cost and large-size consistency of the diagonal pseudo-Hessian (csrc/pseudo_hessian.hip) on the headline model.

    python scripts/pseudo_hessian_bench.py [--nz 1000 --nx 2000 --nsteps 300 --shots 3 --calls 6] [--parent-lib PATH]

Misfit calls (calc_id 0: the forward time loops and the residual) through the C ABI, `sepfwi_stats.fwd_ms` per time step and shot
(HIP events around the forward loops of the call's shots, which run side by side in the session's forward lanes):
  * cost: disarmed, every = 1, every = 4 -- each variant measured twice (two series of --calls calls each, the variants interleaved
    call by call); the spread of the two series of one variant is the noise;
  * the added time per accumulating launch against its algorithmic bytes: 48 B per interior cell (5 fields x 4 B, rho 4 B, three
    accumulators read and written 24 B);
  * disarmed cost: with --parent-lib, the same measurement on a library built from the parent commit, interleaved with the others;
  * forward lanes: every = 1 with 3 lanes against 2 (option fwd_lanes, which only the -DSEPFWI_PROBES build exposes);
  * consistency where no oracle can go: two armed calls bit for bit; H(all shots) against the sum of the one-shot results; every = 4
    against every = 1.
Prints one line per figure and a last line of JSON."""
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

HBM_PEAK = 8.0e12
BYTES_PER_CELL = 48.0


class Lib:
    """One build of the library driven through the C ABI alone (a parent-commit build has no pseudo-Hessian entry points)."""

    def __init__(self, L, pb, dev_tensors):
        self.L, self.pb, self.fn = L, pb, pb["para_fname"].encode()
        self.lam, self.mu, self.den, self.lam_t, self.mu_t, self.den_t = dev_tensors
        self.misfit = torch.zeros(1, dtype=torch.float32, device="cuda")
        L.sepfwi_last_error.restype = C.c_char_p

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.sepfwi_last_error().decode(errors="replace"))

    def cufd(self, calc_id, ids, true_model=False):
        p = lambda t: C.c_void_p(t.data_ptr())
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        m = (self.lam_t, self.mu_t, self.den_t) if true_model else (self.lam, self.mu, self.den)
        torch.cuda.synchronize()
        self._check(self.L.sepfwi_cufd(p(self.misfit), None, None, None, None, p(m[0]), p(m[1]), p(m[2]), C.c_void_p(self.pb["Stf"].data_ptr()),
                                       C.c_int(calc_id), C.c_int(0), C.c_int(ids.size), C.c_void_p(ids.ctypes.data), self.fn))

    def fwd_us(self, nshots, nsteps):
        st = _native.Stats()
        self._check(self.L.sepfwi_get_stats(self.fn, 0, C.byref(st)))
        return 1e3 * st.fwd_ms / (nshots * (nsteps - 1)), st.launches

    def arm(self, every):
        self._check(self.L.sepfwi_pseudo_hessian_arm(self.fn, 0, every))

    def get(self):
        shape = (self.pb["nz_pad"], self.pb["nx_pad"])
        out = [np.empty(shape, np.float32) for _ in range(3)]
        self._check(self.L.sepfwi_get_pseudo_hessian(self.fn, 0, *[C.c_void_p(a.ctypes.data) for a in out]))
        return out


def load(path):
    L = C.CDLL(path)
    L.sepfwi_cufd.argtypes = [C.c_void_p] * 9 + [C.c_int] * 3 + [C.c_void_p, C.c_char_p]
    L.sepfwi_get_stats.argtypes = [C.c_char_p, C.c_int, C.POINTER(_native.Stats)]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nz", type=int, default=1000)
    ap.add_argument("--nx", type=int, default=2000)
    ap.add_argument("--nsteps", type=int, default=300)
    ap.add_argument("--shots", type=int, default=3)
    ap.add_argument("--calls", type=int, default=6, help="calls per series (two series per variant)")
    ap.add_argument("--parent-lib", default=None, help="libsepfwi.so built from the parent commit, for the disarmed comparison")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pseudo_hessian_bench.py needs a HIP device")
    ids = np.arange(a.shots, dtype=np.int32)
    nsh, nst = a.shots, a.nsteps
    cells = a.nz * a.nx                                   # interior cells: one accumulating launch touches 48 B of each
    out = {"nz": a.nz, "nx": a.nx, "nsteps": nst, "shots": nsh, "calls_per_series": a.calls, "interior_cells": cells}
    with tempfile.TemporaryDirectory(prefix="sepfwi_phbench_") as work:
        libs = {}

        def make(name, path, sub):
            d = os.path.join(work, sub)
            os.makedirs(d)
            pb = bench.setup_problem(d, a.nz, a.nx, nst, nsh)
            tens = [t.cuda() for t in pb["lame_init"]] + [t.cuda() for t in pb["lame_true"]]
            lib = Lib(load(path), pb, tens)
            lib.cufd(3, ids, true_model=True)              # observed data of the true model into the session's store
            libs[name] = lib
            return lib

        new = make("new", _native.LIB_PATH, "new")
        variants = [("disarmed", new, 0), ("every1", new, 1), ("every4", new, 4)]
        if a.parent_lib:
            variants.append(("parent", make("parent", a.parent_lib, "parent"), None))

        def call(lib, every):
            if every:
                lib.arm(every)
            try:
                lib.cufd(0, ids)
            finally:
                if every:
                    lib.arm(0)
            return lib.fwd_us(nsh, nst)

        # ---- cost: two series per variant, interleaved call by call (first round: warm-up, not counted)
        series = {name: [[], []] for name, _, _ in variants}
        launches = {}
        for name, lib, every in variants:
            call(lib, every)
        for s in range(2):
            for _ in range(a.calls):
                for name, lib, every in variants:
                    us, launches[name] = call(lib, every)
                    series[name][s].append(us)
        mean = {}
        for name, _, _ in variants:
            m = [float(np.mean(x)) for x in series[name]]
            mean[name] = float(np.mean(m))
            out[name] = {"fwd_us_per_step_and_shot": m, "spread": abs(m[0] - m[1]), "launches": int(launches[name])}
            print("%-9s fwd %.3f / %.3f us per time step and shot (two series of %d calls; spread %.3f), %d launches per call" %
                  (name, m[0], m[1], a.calls, abs(m[0] - m[1]), launches[name]))
        noise = max(v["spread"] for k, v in out.items() if isinstance(v, dict) and "spread" in v)
        out["noise_us"] = noise
        for name, every in (("every1", 1), ("every4", 4)):
            n_acc = -(-(nst - 1) // every)                  # accumulating launches per shot: it = 0, every, ... <= nSteps - 2
            add = (mean[name] - mean["disarmed"]) * (nst - 1) / n_acc   # added time per ACCUMULATING launch (shots side by side in the lanes)
            tbs = BYTES_PER_CELL * cells / (add * 1e-6) / 1e12 if add > 0 else float("nan")
            out[name].update(added_us_per_launch=add, tb_per_s=tbs, frac_of_8tbs=tbs * 1e12 / HBM_PEAK)
            print("%-9s adds %.3f us per accumulating launch: %.0f MB algorithmic -> %.2f TB/s, %.3f of 8 TB/s "
                  "(forward kernels: k_stress 42.1 of 40 B/cell, fwd_step_frac 0.731)" % (name, add, BYTES_PER_CELL * cells / 1e6, tbs, tbs * 1e12 / HBM_PEAK))
        if a.parent_lib:
            d = mean["disarmed"] - mean["parent"]
            out["disarmed_minus_parent_us"] = d
            print("disarmed - parent = %+.3f us per time step and shot; noise (largest spread of two identical series) %.3f -> %s" %
                  (d, noise, "within the noise" if abs(d) <= noise else "OUTSIDE the noise"))
            assert out["disarmed"]["launches"] == out["parent"]["launches"], "a disarmed call must issue the parent's launches"

        # ---- consistency at this size
        new.arm(1)
        try:
            new.cufd(0, ids)
            h_a = new.get()
            new.cufd(0, ids)
            h_b = new.get()
            parts = []
            for k in range(nsh):
                new.cufd(0, ids[k:k + 1])
                parts.append(new.get())
            new.arm(4)
            new.cufd(0, ids)
            h_4 = new.get()
        finally:
            new.arm(0)
        out["repeat_bit_identical"] = bool(all(np.array_equal(x, y) for x, y in zip(h_a, h_b)))
        print("two armed calls bit-identical: %s" % out["repeat_bit_identical"])
        rel = lambda x, y: float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y))
        out["additivity"], out["every4_vs_1"] = [], []
        for k, name in enumerate(("hLambda", "hMu", "hDen")):
            want = sum(p[k].astype(np.float64) for p in parts)
            dmax, l2 = float(np.abs(h_a[k] - want).max() / want.max()), rel(h_a[k], want)
            out["additivity"].append({"max": dmax, "rel_l2": l2})
            e4 = rel(h_4[k], h_a[k].astype(np.float64))
            out["every4_vs_1"].append(e4)
            inside = h_a[k][new.pb["nPml"]:new.pb["nPml"] + a.nz, new.pb["nPml"]:-new.pb["nPml"]]
            print("%-8s H(%d shots) vs sum of one-shot results: max-norm %.2e of the maximum, rel-L2 %.2e (tolerance 1e-4); every 4 vs 1 rel-L2 %.2e; "
                  "max %.3e, interior min / max %.2e" % (name, nsh, dmax, l2, e4, h_a[k].max(), inside.min() / inside.max()))
        out["additivity_ok"] = bool(all(v["max"] <= 1e-4 and v["rel_l2"] <= 1e-4 for v in out["additivity"]))
        for lib in libs.values():
            lib.L.sepfwi_release_all()

        # ---- forward lanes: three more arrays per lane in a working set sized to the Infinity Cache
        with _native.use_variant("probes") as LP:
            try:
                pl = make("probes", _native.PROBES_LIB_PATH, "probes")
                lanes = {3: [[], []], 2: [[], []]}
                for n_l in (3, 2):                          # warm-up of both lane counts
                    _native.check(LP.sepfwi_set_option(b"fwd_lanes", n_l))
                    call(pl, 1)
                for s in range(2):
                    for _ in range(a.calls):
                        for n_l in (3, 2):
                            _native.check(LP.sepfwi_set_option(b"fwd_lanes", n_l))
                            lanes[n_l][s].append(call(pl, 1)[0])
                for n_l in (3, 2):
                    m = [float(np.mean(x)) for x in lanes[n_l]]
                    out["lanes%d_every1" % n_l] = m
                    print("every = 1 with %d forward lanes: fwd %.3f / %.3f us per time step and shot" % (n_l, m[0], m[1]))
            finally:
                LP.sepfwi_set_option(b"fwd_lanes", 3)
                LP.sepfwi_release_all()
    print(json.dumps(out))
    if not (out["repeat_bit_identical"] and out["additivity_ok"]):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
