"""Which combinations of the misfit-kind keys, if_src_update and the other live conditioning keys the host-side parser (csrc/config.cpp)
accepts, and the exact text of every refusal, without a GPU: a stand-alone program over config.cpp built with AddressSanitizer +
UndefinedBehaviorSanitizer, as tests/test_robust_config.py builds the robust misfit's."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_every_subset_of_the_misfit_keys_under_asan_ubsan(tmp_path):
    """the 32 subsets of {if_cross_misfit, if_envelope_misfit, if_w2_misfit, robust_misfit, if_src_update} are accepted or refused with the
    message recorded from the parser of before the misfit kind was one enum; the 256 subsets of the eight live keys under misfit_w_vx get
    that message, else the joint-weights refusal naming the first live key; every refusal is std::invalid_argument."""
    exe = str(tmp_path / "misfit_keys_check")
    src = [os.path.join(ROOT, "tests", "native", "misfit_keys_check.cpp"), os.path.join(ROOT, "sep-2023_amd", "csrc", "config.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
