#!/usr/bin/env python
"""SHA-256 of every output of the model-space operators of one build of the library, for comparing two builds bit for bit: the
four parameterisation maps (sepfwi_param_forward / _backward / _jvp / _diag), the regulariser (sepfwi_regularizer / _hvp) and the
smoother (sepfwi_smooth_plan / _apply), driven through the C ABI with fixed seeded inputs on shapes of a few hundred cells that
reach every branch of the kernels and of the host call path (device and host pointers, NULL tangents, in place).

    python scripts/model_ops_digest.py --lib sep-2023_amd/libsepfwi.so --out new.json
    python scripts/model_ops_digest.py --lib /somewhere/else/libsepfwi.so --out old.json      # each in a process of its own

Two builds compute the same bits exactly when the two files are equal entry for entry.  Nothing of this is a golden file: the bits
of expf and of the divisions belong to the ROCm version, not to the project."""
import argparse
import ctypes as C
import hashlib
import json

import numpy as np
import torch

# (nz, nx, nPml, nPad): one row, one column, rim rectangles of more than 64 replicas (33 x 33 and 33 x 36 cells in the last)
PARAM_SHAPES = [(1, 70, 3, 2), (5, 1, 4, 0), (2, 65, 33, 1), (37, 131, 32, 3)]
REG_SHAPES = [(5, 63), (33, 129)]
SMOOTH_SHAPES = [(5, 65, 32, 7), (67, 9, 3, 32)]      # (nz, nx, rx, rz)


def sha(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def ptr(a):
    if a is None:
        return None
    return C.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a.ctypes.data_as(C.c_void_p)


def triple(arrs):
    return (C.c_void_p * 3)(*[None if a is None else ptr(a).value for a in arrs])


def cuda(a):
    return None if a is None else torch.tensor(a).cuda()


class Run(object):
    def __init__(self, lib):
        self.L = C.CDLL(lib)
        self.L.sepfwi_last_error.restype = C.c_char_p
        self.out = {}

    def call(self, name, *args):
        rc = getattr(self.L, name)(*args)
        torch.cuda.synchronize()
        assert rc == 0, "%s: %s" % (name, self.L.sepfwi_last_error().decode())

    def put(self, key, arrs):
        for k, a in enumerate(arrs):
            assert key + "/%d" % k not in self.out
            self.out[key + "/%d" % k] = sha(a)


def param_maps(run):
    for nz, nx, nPml, nPad in PARAM_SHAPES:
        nzp, nxp = nz + 2 * nPml + nPad, nx + 2 * nPml
        for kind in range(7):
            rng = np.random.default_rng(100 * kind + nz + 1000 * nx)
            f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
            base = (0.25, 0.4, 0.6) if kind >= 5 else (3000.0, 1700.0, 2400.0)      # rock physics: porosity, clay, saturation
            phys = [cuda(f32(b * (1.0 + 0.1 * rng.uniform(-1, 1, (nz, nx))))) for b in base]
            ref = [cuda(f32(b * (1.0 + 0.1 * rng.uniform(-1, 1, (nzp, nxp))))) for b in base]
            mask = rng.uniform(0.0, 1.0, (nzp, nxp)) * (rng.uniform(size=(nzp, nxp)) > 0.15)      # fractional in the padding, some exact 0
            mask[nPml:nPml + nz, nPml:nPml + nx] = 1.0
            mask = cuda(f32(mask))
            padded = [cuda(f32(rng.standard_normal((nzp, nxp)))) for _ in range(3)]                # g or h (h non-negative)
            h = [t.abs() for t in padded]
            tang = [cuda(f32(b * 0.01 * rng.standard_normal((nz, nx)))) for b in base]
            head = [C.c_int(x) for x in (kind, nz, nx, nPml, nPad)] + [ptr(t) for t in phys + ref + [mask]]
            key = "param/kind%d/%dx%d_pml%d_pad%d/" % (kind, nz, nx, nPml, nPad)
            on_padded = lambda: [torch.full((nzp, nxp), -7.0, device="cuda") for _ in range(3)]
            on_phys = lambda: [torch.full((nz, nx), -7.0, device="cuda") for _ in range(3)]
            o = on_padded()
            run.call("sepfwi_param_forward", *head, *[ptr(t) for t in o], None)
            run.put(key + "forward", o)
            o = on_phys()
            run.call("sepfwi_param_backward", *head, *[ptr(t) for t in padded + o], None)
            run.put(key + "backward", o)
            for what, v in (("jvp", tang), ("jvp_null_b", [tang[0], None, tang[2]]), ("jvp_null_all", [None, None, None])):
                o = on_padded()
                run.call("sepfwi_param_jvp", *head, *[ptr(t) for t in v + o], None)
                run.put(key + what, o)
            o = on_phys()
            run.call("sepfwi_param_diag", *head, *[ptr(t) for t in h + o], None)
            run.put(key + "diag", o)


def regulariser(run):
    for nz, nx in REG_SHAPES:
        rng = np.random.default_rng(1000 * nz + nx)
        grid = (nz, nx)
        p, p0, v = [], [], []
        for b in (3000.0, 1700.0, 2400.0):
            a = b * (1.0 + 0.05 * rng.standard_normal(grid))
            a[nz // 2:, nx // 3:] += 0.08 * b
            p.append(a.astype(np.float32))
            p0.append((a + 0.03 * b * rng.standard_normal(grid)).astype(np.float32))
            v.append((0.02 * b * rng.standard_normal(grid)).astype(np.float32))
        W = (rng.uniform(0.5, 1.5, grid) * (rng.uniform(size=grid) > 0.2)).astype(np.float32)
        f3 = lambda *x: (C.c_float * 3)(*x)
        for where, put in (("device", cuda), ("host", np.ascontiguousarray)):
            keep = [[put(a) for a in p], [put(a) for a in p0], put(W), [put(a) for a in v]]
            args = [C.c_int(nz), C.c_int(nx), C.c_float(10.0), C.c_float(7.5), triple(keep[0]), triple(keep[1]), ptr(keep[2]),
                    f3(0.7, 0.0, 1.3), f3(0.4, 0.9, 0.0), f3(0.0, 0.6, 1.1), f3(3100.0, 1650.0, 2500.0), C.c_float(2e-3)]
            empty = lambda: [put(np.full(grid, -7.0, np.float32)) for _ in range(3)]
            key = "regularizer/%dx%d/%s/" % (nz, nx, where)
            g, val = empty(), C.c_double(-1.0)
            run.call("sepfwi_regularizer", *args, C.cast(C.byref(val), C.c_void_p), triple(g), None)
            run.put(key + "gradient", g)
            run.put(key + "value", [np.float64(val.value)])
            hv = empty()
            run.call("sepfwi_regularizer_hvp", *args, triple(keep[3]), triple(hv), None)
            run.put(key + "product", hv)


def smoother(run):
    for nz, nx, rx, rz in SMOOTH_SHAPES:
        rng = np.random.default_rng(10 * nz + nx)
        grid = (nz, nx)
        sig = [(rng.uniform(0.0, r / 2.5, grid) * (rng.uniform(size=grid) > 0.1)).astype(np.float32) for r in (rx, rz)]
        u = [rng.standard_normal(grid).astype(np.float32) for _ in range(3)]
        dims = [C.c_int(x) for x in (nz, nx, rx, rz)]
        for where, put in (("device", cuda), ("host", np.ascontiguousarray)):
            key = "smoother/%dx%d_rx%d_rz%d/%s/" % (nz, nx, rx, rz, where)
            s = [put(a) for a in sig]
            inv = [put(np.full(grid, -7.0, np.float32)) for _ in range(2)]
            run.call("sepfwi_smooth_plan", *dims, ptr(s[0]), ptr(s[1]), ptr(inv[0]), ptr(inv[1]), None)
            run.put(key + "plan", inv)
            for transpose in (0, 1):
                src = [put(a) for a in u]
                dst = [put(np.full(grid, -7.0, np.float32)) for _ in range(3)]
                run.call("sepfwi_smooth_apply", *dims, ptr(s[0]), ptr(s[1]), ptr(inv[0]), ptr(inv[1]), C.c_int(transpose), triple(src), triple(dst), None)
                run.put(key + ("S^T" if transpose else "S"), dst)
                same = [put(a.copy()) for a in u]
                run.call("sepfwi_smooth_apply", *dims, ptr(s[0]), ptr(s[1]), ptr(inv[0]), ptr(inv[1]), C.c_int(transpose), triple(same), triple(same), None)
                run.put(key + ("S^T" if transpose else "S") + "_in_place", same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="the build of libsepfwi.so to drive")
    ap.add_argument("--out", required=True, help="the JSON file of digests to write")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.zeros(1, device="cuda")      # torch first: the library and torch share one HIP runtime
    run = Run(a.lib)
    param_maps(run)
    regulariser(run)
    smoother(run)
    run.L.sepfwi_release_all()
    with open(a.out, "w") as f:
        json.dump(run.out, f, indent=0, sort_keys=True)
    print("%d digests of %s -> %s" % (len(run.out), a.lib, a.out))


if __name__ == "__main__":
    main()
