"""The parameter keys if_w2_misfit / w2_beta in the host-side parser (csrc/config.cpp) and in utils.paraGen, without a GPU: a stand-alone
program over config.cpp built with AddressSanitizer + UndefinedBehaviorSanitizer, as tests/test_envelope_config.py builds the envelope's."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_w2_keys_in_the_parser_under_asan_ubsan(tmp_path):
    """parsed; the flag ignored in reference mode; the three refused pairs and the joint-weights refusal name both keys, a w2_beta outside
    (0, 16] names the key, all as std::invalid_argument (SEPFWI_EINVAL at the C ABI); what the parser accepted and refused before, it
    still does."""
    exe = str(tmp_path / "w2_config_check")
    src = [os.path.join(ROOT, "tests", "native", "w2_config_check.cpp"), os.path.join(ROOT, "sep-2023_amd", "csrc", "config.cpp")]
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
    ft.paraGen(*args, keyed, "s.json", str(tmp_path / "D"), if_w2_misfit=True, filter_para=[1.0, 2.0, 8.0, 10.0])
    a, b = json.load(open(plain)), json.load(open(keyed))
    assert "if_w2_misfit" not in a and "w2_beta" not in a
    assert b["if_w2_misfit"] is True and "w2_beta" not in b and b["filter"] == [1.0, 2.0, 8.0, 10.0]
    ft.paraGen(*args, keyed, "s.json", str(tmp_path / "D"), if_w2_misfit=True, w2_beta=5)
    b = json.load(open(keyed))
    assert b["if_w2_misfit"] is True and b["w2_beta"] == 5.0
    ft.paraGen(*args, keyed, "s.json", str(tmp_path / "D"), if_w2_misfit=False)
    assert open(keyed).read() == open(plain).read()      # false: the file of before, byte for byte
    for bad in (0, -1, 17, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="w2_beta"):
            ft.paraGen(*args, keyed, "s.json", str(tmp_path / "D"), if_w2_misfit=True, w2_beta=bad)
