"""examples/gauss_newton_fwi.py keeps running (-m gpu): the 101 x 201 anomaly problem of the reference's experiment 001 with a reduced
record and every third shot, two Gauss-Newton iterations of three conjugate-gradient iterations each -- the CG residual decreases and
the misfit after the step is below the initial misfit."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_gauss_newton_example_reduces_the_misfit(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "gauss_newton_fwi.py"), "--device", "cuda", "--outer", "2", "--inner", "3",
                          "--nsteps", "700", "--shot-stride", "3", "--rtol", "1e-6", "--workdir", str(tmp_path)], capture_output=True, text=True,
                         timeout=300, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    lines = out.stdout.splitlines()
    f = [float(ln.split("misfit")[1].split()[0]) for ln in lines if ln.startswith("iterate ") and "misfit" in ln]
    assert len(f) == 3 and f[1] < f[0] and f[2] < f[1], out.stdout[-2000:]
    for k in (1, 2):
        r = [float(ln.split("residual")[1]) for ln in lines if ln.startswith("  outer %d cg" % k)]
        assert len(r) == 3 and r[-1] < 1.0 and r[-1] < r[0], (k, r)
    assert any(ln.startswith("done: ") for ln in lines)
