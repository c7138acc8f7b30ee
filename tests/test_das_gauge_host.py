"""DAS gauge length (parameter key "das_gauge_length", csrc/das_gauge.cpp) on the CPU: the taps of gauge channels against their
definition, their adjoint plan against the exact transpose, the member bounds and the key's parsing -- under AddressSanitizer /
UBSan -- and the parameter-file writer."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from sepfwi import utils as ft


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_gauge_taps_and_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "das_gauge_check")
    csrc = os.path.join(ROOT, "sep-2023_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "das_gauge_check.cpp"), os.path.join(csrc, "das_gauge.cpp"), os.path.join(csrc, "config.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for seed in (1, 2):
        out = subprocess.run([exe, str(seed), "60"], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


def _para(tmp_path, **kw):
    fn = str(tmp_path / "para.json")
    ft.paraGen(60, 80, 10.0, 10.0, 100, 1e-3, 10.0, 10, 2, fn, str(tmp_path / "survey.json"), str(tmp_path / "Data"), **kw)
    with open(fn) as fp:
        return fp.read()


def test_paragen_gauge_length_key(tmp_path):
    plain = _para(tmp_path)
    assert "das_gauge_length" not in json.loads(plain)
    assert _para(tmp_path, das_gauge_length=None) == plain            # default files stay byte-identical
    assert json.loads(_para(tmp_path, das_gauge_length=30.0))["das_gauge_length"] == 30.0
    assert json.loads(_para(tmp_path, das_gauge_length=20, das_fiber="vertical"))["das_gauge_length"] == 20.0
    for bad in (0, 0.0, -10.0):
        with pytest.raises(ValueError):
            _para(tmp_path, das_gauge_length=bad)
