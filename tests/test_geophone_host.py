"""Joint DAS + geophone misfit (parameter keys "misfit_w_*", csrc/geophone.cpp) on the CPU: the concatenated channel list and its
adjoint plan against the dense transpose, the keys' parsing with every refusal -- under AddressSanitizer / UBSan -- and the
parameter-file writer."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from sepfwi import utils as ft


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_geophone_plan_and_keys_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "geophone_check")
    csrc = os.path.join(ROOT, "sep-2023_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "geophone_check.cpp")] + [os.path.join(csrc, f) for f in ("geophone.cpp", "das_gauge.cpp", "config.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for seed in (1, 2):
        out = subprocess.run([exe, str(seed), "8"], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


def _para(tmp_path, **kw):
    fn = str(tmp_path / "para.json")
    ft.paraGen(60, 80, 10.0, 10.0, 100, 1e-3, 10.0, 10, 2, fn, str(tmp_path / "survey.json"), str(tmp_path / "Data"), **kw)
    with open(fn) as fp:
        return fp.read()


def test_paragen_misfit_weight_keys(tmp_path):
    plain = _para(tmp_path)
    assert not any(k.startswith("misfit_w_") for k in json.loads(plain))
    assert _para(tmp_path, misfit_weights=None) == plain              # default files stay byte-identical
    assert _para(tmp_path, misfit_weights={}) == plain
    j = json.loads(_para(tmp_path, misfit_weights=dict(ett=1, vx=0.5, vz=2)))
    assert (j["misfit_w_ett"], j["misfit_w_vx"], j["misfit_w_vz"]) == (1.0, 0.5, 2.0)
    j = json.loads(_para(tmp_path, misfit_weights=dict(vz=1)))
    assert j["misfit_w_vz"] == 1.0 and "misfit_w_ett" not in j and "misfit_w_vx" not in j     # only the keys given
    for bad in (dict(vx=-1.0), dict(ett=float("nan")), dict(vz=float("inf")), dict(pr=1.0)):
        with pytest.raises(ValueError):
            _para(tmp_path, misfit_weights=bad)
