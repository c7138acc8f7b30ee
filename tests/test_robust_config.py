"""The parameter keys robust_misfit / robust_delta / robust_quantile in the host-side parser (csrc/config.cpp) and in utils.paraGen,
without a GPU: a stand-alone program over config.cpp built with AddressSanitizer + UndefinedBehaviorSanitizer, as tests/test_w2_config.py
builds the W2 misfit's."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_robust_keys_in_the_parser_under_asan_ubsan(tmp_path):
    """parsed; the kind ignored (but validated) in reference mode; another kind, a missing or bad robust_delta, a robust_quantile outside
    (0, 1], a stray robust_delta / robust_quantile, the four refused pairs and the joint-weights refusal name their keys, all as
    std::invalid_argument (SEPFWI_EINVAL at the C ABI); what the parser accepted and refused before, it still does."""
    exe = str(tmp_path / "robust_config_check")
    src = [os.path.join(ROOT, "tests", "native", "robust_config_check.cpp"), os.path.join(ROOT, "sep-2023_amd", "csrc", "config.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


def test_paragen_writes_the_keys_only_when_set(tmp_path):
    from sepfwi import utils as ft
    args = (64, 80, 10.0, 10.0, 100, 1e-3, 10.0, 10, 4)
    plain, keyed, D = str(tmp_path / "plain.json"), str(tmp_path / "keyed.json"), str(tmp_path / "D")
    ft.paraGen(*args, plain, "s.json", D)
    ft.paraGen(*args, keyed, "s.json", D, robust_misfit="huber", robust_delta=2, filter_para=[1.0, 2.0, 8.0, 10.0])
    a, b = json.load(open(plain)), json.load(open(keyed))
    assert not any(k.startswith("robust_") for k in a)
    assert b["robust_misfit"] == "huber" and b["robust_delta"] == 2.0 and "robust_quantile" not in b and b["filter"] == [1.0, 2.0, 8.0, 10.0]
    ft.paraGen(*args, keyed, "s.json", D, robust_misfit="cauchy", robust_delta=0.5, robust_quantile=1)
    b = json.load(open(keyed))
    assert b["robust_misfit"] == "cauchy" and b["robust_delta"] == 0.5 and b["robust_quantile"] == 1.0
    ft.paraGen(*args, keyed, "s.json", D, robust_misfit=None)
    assert open(keyed).read() == open(plain).read()      # absent: the file of before, byte for byte
    with pytest.raises(ValueError, match="robust_misfit"):
        ft.paraGen(*args, keyed, "s.json", D, robust_misfit="l1", robust_delta=1.0)
    with pytest.raises(ValueError, match="robust_delta"):                      # required with the key: no default
        ft.paraGen(*args, keyed, "s.json", D, robust_misfit="huber")
    for bad in (0, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="robust_delta"):
            ft.paraGen(*args, keyed, "s.json", D, robust_misfit="huber", robust_delta=bad)
    for bad in (0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="robust_quantile"):
            ft.paraGen(*args, keyed, "s.json", D, robust_misfit="huber", robust_delta=1.0, robust_quantile=bad)
    with pytest.raises(ValueError, match="robust_delta without robust_misfit"):
        ft.paraGen(*args, keyed, "s.json", D, robust_delta=1.0)
    with pytest.raises(ValueError, match="robust_quantile without robust_misfit"):
        ft.paraGen(*args, keyed, "s.json", D, robust_quantile=0.5)
