#!/usr/bin/env python3
"""Digests of everything the data-conditioning chain hands out, for comparing two builds of the library bit for bit (needs a GPU).

    python scripts/conditioning_bits.py --lib PATH/libsepfwi.so --out A.txt      one line per output: "<case> <what> <sha256 | scalar>"
    python scripts/conditioning_bits.py --compare OLD1.txt OLD2.txt NEW.txt      the table: OLD run twice, NEW once

Cases, with no time loop (tests/data_entry_common.py: problem and traces): every NSTEPS value with the layouts five and ragged, the wide
layouts at nSteps 65 and 257, the four key sets, the misfits L2, if_cross_misfit, if_envelope_misfit and if_src_update (with L2); a
combination the parameter check refuses is listed as refused.  Per case: data_misfit (misfit scalar and adjoint source), data_gn (L2 and
envelope), condition with and without transpose.  Then two calls through the time loop on the problem of tests/test_gpu_envelope_misfit.py
under `both`: backward, and gauss_newton without the exact adjoint.

Arrays are compared by digest.  The misfit's sum has a fixed order under if_cross_misfit and if_envelope_misfit: the scalar must be the
same.  The L2 sum is one double atomicAdd per trace: where the two OLD runs agree NEW must agree with them, where they differ NEW must lie
within their spread."""
import argparse
import hashlib
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sep-2023_amd"), os.path.join(ROOT, "tests")]

LAYOUTS = {"five": (5,), "ragged": (5, 3)}
WIDE = {"w64": (64,), "w65": (65,), "w257": (257,), "w513_2": (513, 2)}
FILTER = [25.0, 60.0, 260.0, 400.0]      # tests/test_gpu_cross_data.py's
KEYSETS = {"alone": {}, "filter": {"filter": FILTER}, "window": {"if_win": True}, "both": {"filter": FILTER, "if_win": True}}
MISFITS = {"l2": {}, "cross": {"if_cross_misfit": True}, "envelope": {"if_envelope_misfit": True}, "srcupd": {"if_src_update": True}}
FIXED_ORDER = ("cross", "envelope")


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def produce(lib, out):
    import data_entry_common as DE
    import envelope_ref as E
    from sepfwi import _native
    if lib:
        _native.VARIANTS["default"] = (os.path.abspath(lib), [])
    from sepfwi import fwi_ops
    lines = []
    emit = lambda case, what, v: lines.append("%s %s %s" % (case, what, v))
    geoms = [(nt, n, LAYOUTS[n], 48) for n in LAYOUTS for nt in DE.NSTEPS] + [(nt, n, WIDE[n], 560) for n in WIDE for nt in (65, 257)]
    with tempfile.TemporaryDirectory() as tmp:
        for nt, layout, nrec, nx in geoms:
            for keys in KEYSETS:
                for mf, mkey in MISFITS.items():
                    case = "nt%d/%s/%s/%s" % (nt, layout, keys, mf)
                    fwi_ops.release()
                    pb = DE.problem(pathlib.Path(tmp) / case.replace("/", "_"), nt, nrec, dict(KEYSETS[keys], **mkey), "bits", misfit_key=None, nx=nx)
                    obs, syn, d = (DE.flat(DE.traces(pb, s)).cuda() for s in (1, 2, 3))
                    ids, fn = pb["Shot_ids"], pb["para_fname"]
                    try:
                        f, a = fwi_ops.data_misfit(obs, syn, ids, fn)
                    except _native.SepFwiError as e:
                        emit(case, "refused", hashlib.sha256(str(e).encode()).hexdigest())
                        continue
                    emit(case, "misfit", "%s:%s" % ("fixed" if mf in FIXED_ORDER else "atomic", float(f).hex()))
                    emit(case, "adjoint_source", sha(a))
                    if mf in ("l2", "envelope"):
                        emit(case, "data_gn", sha(fwi_ops.data_gn(syn, d, ids, fn)))
                    emit(case, "condition", sha(fwi_ops.condition(syn, ids, fn)))
                    emit(case, "condition_t", sha(fwi_ops.condition(syn, ids, fn, transpose=True)))
        # through the time loop: residual_conditioned and adjoint_source_conditioned
        pb = E.gpu_problem(pathlib.Path(tmp) / "loop", "both")
        m = [t.cuda() for t in pb["lame_init"]]
        fwi_ops.release()
        fwi_ops.obscalc(*[t.cuda() for t in pb["lame_true"]], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])      # the observed files
        res = fwi_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
        emit("loop/backward", "misfit", "fixed:%s" % float(res[0]).hex())
        for name, t in zip(("gLambda", "gMu", "gDen", "gStf"), res[1:5]):
            emit("loop/backward", name, sha(t))
        hv = fwi_ops.gauss_newton(*m, *[1e-3 * t for t in m], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact=False)
        for name, t in zip(("hvLambda", "hvMu", "hvDen"), hv):
            emit("loop/gauss_newton", name, sha(t))
        fwi_ops.release()
    text = "\n".join(lines) + "\n"
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        open(out, "w").write(text)
    print("%d lines, digest of all of them %s" % (len(lines), hashlib.sha256(text.encode()).hexdigest()))


def compare(old1, old2, new):
    read = lambda fn: {tuple(ln.split()[:2]): ln.split()[2] for ln in open(fn) if ln.strip()}
    a, b, n = read(old1), read(old2), read(new)
    bad, spread = [], []
    if not (a.keys() == b.keys() == n.keys()):
        bad.append("the three runs list different outputs")
    for k in sorted(set(a) & set(b) & set(n)):
        if a[k].startswith("atomic:") and a[k] != b[k]:
            va, vb, vn = (float.fromhex(x.split(":")[1]) for x in (a[k], b[k], n[k]))
            spread.append("%s %s: old %r / %r, new %r" % (k[0], k[1], va, vb, vn))
            if not min(va, vb) <= vn <= max(va, vb):
                bad.append("%s %s: new %r outside the old runs' spread [%r, %r]" % (k[0], k[1], vn, min(va, vb), max(va, vb)))
        elif not (a[k] == b[k] == n[k]):
            bad.append("%s %s: old %s / %s, new %s" % (k[0], k[1], a[k], b[k], n[k]))
    cases = {k[0] for k in n}
    print("cases %d (refused by the parameter check: %d), outputs compared %d, mismatches %d" % (len(cases), sum(1 for k in n if k[1] == "refused"), len(n), len(bad)))
    print("L2 misfits on which the two old runs differed: %d" % len(spread))
    for ln in spread + bad:
        print("  " + ln)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="the libsepfwi.so to load in the place of the tree's own")
    ap.add_argument("--out", help="file to write the lines to")
    ap.add_argument("--compare", nargs=3, metavar=("OLD1", "OLD2", "NEW"))
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else produce(args.lib, args.out))
