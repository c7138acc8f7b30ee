"""The parameter keys fk_slowness / fk_mode in the host-side parser (csrc/config.cpp), the channel spacing the session derives from the survey
under them (csrc/host_checks.cpp: fk_channel_spacing) and utils.paraGen, without a GPU: a stand-alone program over the two sources built
with AddressSanitizer + UndefinedBehaviorSanitizer and run directly, in the pattern of tests/test_envelope_config.py.

Without the feature the program does not compile (Params has no has_fk, host_checks.hpp no fk_channel_spacing) and paraGen refuses the
arguments."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_fk_keys_in_the_parser_and_the_channel_spacing_under_asan_ubsan(tmp_path):
    """parsed; validated and ignored in reference mode; every refusal (four finite ascending numbers, the two mode strings, fk_mode without
    fk_slowness, joint weights) a std::invalid_argument naming its keys; the spacing of horizontal, vertical, strided and diagonal lines with
    dz != dx; one-channel, non-uniform and zero-step shots refused naming the shot and the first offending channel; what the parser accepted
    and refused before, it still does."""
    exe = str(tmp_path / "fk_config_check")
    csrc = os.path.join(ROOT, "sep-2023_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "fk_config_check.cpp"), os.path.join(csrc, "config.cpp"), os.path.join(csrc, "host_checks.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


def test_paragen_writes_the_keys_only_when_set(tmp_path):
    from sepfwi import utils as ft
    args = (64, 80, 10.0, 10.0, 100, 1e-3, 10.0, 10, 4)
    plain, keyed = str(tmp_path / "plain.json"), str(tmp_path / "keyed.json")
    ft.paraGen(*args, plain, "s.json", str(tmp_path / "D"))
    before = open(plain).read()
    assert before == json.dumps({"nz": 64, "nx": 80, "dz": 10.0, "dx": 10.0, "nSteps": 100, "dt": 1e-3, "f0": 10.0, "nPoints_pml": 10, "nPad": 4,
                                 "survey_fname": "s.json", "data_dir_name": str(tmp_path / "D")})      # the file of before, byte for byte
    ft.paraGen(*args, keyed, "s.json", str(tmp_path / "D"), fk_slowness=None, fk_mode=None)
    assert open(keyed).read() == before
    ft.paraGen(*args, keyed, "s.json", str(tmp_path / "D"), fk_slowness=(1e-4, 2e-4, 6e-4, 8e-4))
    a = json.load(open(keyed))
    assert a["fk_slowness"] == [1e-4, 2e-4, 6e-4, 8e-4] and "fk_mode" not in a
    ft.paraGen(*args, keyed, "s.json", str(tmp_path / "D"), fk_slowness=[-8e-4, -2e-4, -2e-4, -1e-4], fk_mode="reject", filter_para=[1.0, 2.0, 8.0, 10.0])
    a = json.load(open(keyed))
    assert a["fk_slowness"] == [-8e-4, -2e-4, -2e-4, -1e-4] and a["fk_mode"] == "reject" and a["filter"] == [1.0, 2.0, 8.0, 10.0]
    assert {k: v for k, v in a.items() if k not in ("fk_slowness", "fk_mode", "filter")} == json.loads(before)
    for bad in ([1e-4, 2e-4, 3e-4], [2e-4, 2e-4, 3e-4, 4e-4], [1e-4, 3e-4, 2e-4, 4e-4], [1e-4, 2e-4, 4e-4, 4e-4], [1e-4, 2e-4, 3e-4, float("inf")], [1e-4, float("nan"), 3e-4, 4e-4]):
        with pytest.raises(ValueError, match="fk_slowness"):
            ft.paraGen(*args, keyed, "s.json", str(tmp_path / "D"), fk_slowness=bad)
    with pytest.raises(ValueError, match="fk_mode"):
        ft.paraGen(*args, keyed, "s.json", str(tmp_path / "D"), fk_slowness=[1e-4, 2e-4, 3e-4, 4e-4], fk_mode="keep")
    with pytest.raises(ValueError, match="fk_mode without fk_slowness"):
        ft.paraGen(*args, keyed, "s.json", str(tmp_path / "D"), fk_mode="pass")
