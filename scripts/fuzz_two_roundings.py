#!/usr/bin/env python
"""How well-conditioned is a fuzz draw?  Runs tests/test_gpu_fuzz.py's draw(s) (tests/fuzz_sides.py) with the PRODUCT replaced by a second build of the oracle
(gcc -O3 -march=native -ffp-contract=fast: the same algorithm with other round-off) against the regular oracle build, on the CPU.
A draw on which the reference algorithm differs from ITSELF by 1e-3 is no 1e-3 parity target for anybody.
    python scripts/fuzz_two_roundings.py 25550,167        (prints the test's diagnostics: rel-L2 per gradient, in / below a water layer)"""
import os, sys, importlib.util, tempfile, pathlib
os.environ["SEPFWI_FUZZ_SEEDS"] = sys.argv[1]
os.environ["SEPFWI_FUZZ_DIAG"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'sep-2023_amd'), os.path.join(ROOT, 'tests')]
from oracle import oracle as O
O.build()
spec = importlib.util.spec_from_file_location("oracle_alt", os.path.join(ROOT, "oracle", "oracle.py"))
OA = importlib.util.module_from_spec(spec); spec.loader.exec_module(OA)
OA._LIB_PATH = "/tmp/liboracle_fast.so"
import subprocess
subprocess.check_call("gcc -O3 -march=native -ffp-contract=fast -fopenmp -fPIC -shared -o /tmp/liboracle_fast.so /root/repo/oracle/torchfwi_oracle.c "
                      "/root/repo/oracle/numba_oracle.c -lm".replace("/root/repo", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), shell=True)
import fuzz_common as C
from fuzz_sides import plain_oracle_side
alt_oracle = OA.TorchFWIOracle()
for seed in C.seeds("SEPFWI_FUZZ"):
    o, scale = C.settle(plain_oracle_side, pathlib.Path(tempfile.mkdtemp()), O, O.load_variant("nvfma"), seed)
    if o is None:
        print("seed", seed, "the wave does not reach the channels even with a record four times as long")
        continue
    pb, w = o["d"]["pb"], o["d"]["water"]
    for i, sid in enumerate(pb["Shot_ids"].tolist()):      # the observed data of the oracle's side, as the test installs them
        os.makedirs(pb["data_dir"], exist_ok=True)
        for k, c in enumerate(("pr", "vx", "vz", "ett")):
            o["obs"][i, k].tofile(os.path.join(pb["data_dir"], "Shot_%s%d.bin" % (c, sid)))
    got = alt_oracle.backward(*[t.numpy() for t in pb["lame_init"]], pb["Stf"].numpy(), 1, pb["Shot_ids"].numpy(), pb["para_fname"])
    print("seed %d scale %d: misfit second build %.9e, oracle %.9e, nvcc-FMA oracle %.9e, target %r" % (seed, scale, float(got[0]), o["ref"]["misfit"], o["alt"]["misfit"], o["target"]))
    for name, g in zip(("gLambda", "gMu", "gDen"), got[1:4]):
        r, a = o["ref"][name], o["alt"][name]
        miss = C.gradient_miss(g, r, a, C.GRAD_TOL, o["cond_g"], w, C.d_own)
        print("seed %d %s: second build vs oracle %.2e, oracle vs its nvcc-FMA build %.2e (rel-L2), water rows %d: %s"
              % (seed, name, C.rel(C.d_own(g, r), r), C.rel(C.d_own(a, r), r), w, "misses " + miss if miss else "held"))
