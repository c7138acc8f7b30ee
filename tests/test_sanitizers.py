"""AddressSanitizer + UndefinedBehaviorSanitizer run of the device-free host code of libsepfwi (JSON reader, parameter /
survey parsers, C-PML profiles, source taper, shot split) on well-formed and randomly damaged documents.  GPU sanitizers
are not available on the target pool; this is the CPU build the sanitizers can see."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_parsers_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "config_sanitize")
    src = [os.path.join(ROOT, "tests", "native", "config_sanitize.cpp"), os.path.join(ROOT, "sep-2023_amd", "csrc", "config.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for seed in (1, 2, 3):
        out = subprocess.run([exe, str(seed), "3000"], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.startswith("OK"), out.stdout + out.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_pack_index_and_survey_checks_under_asan_ubsan(tmp_path):
    """The validation code session.cpp / obs_store.cpp rely on (csrc/host_checks.cpp): index of the packed observed-data file
    (flipped bytes, truncation, a lying file size) and the survey geometry against the stored grid (receivers and sources on and
    beyond every edge, coordinate lists shorter than nrec) -- accepted input stays inside the file / grid, everything else throws."""
    exe = str(tmp_path / "host_checks_sanitize")
    src = [os.path.join(ROOT, "tests", "native", "host_checks_sanitize.cpp"), os.path.join(ROOT, "sep-2023_amd", "csrc", "host_checks.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for seed in (1, 2, 3):
        out = subprocess.run([exe, str(seed), "1500", str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.startswith("OK"), out.stdout + out.stderr
        acc = [int(w) for w in out.stdout.split() if w.isdigit()]
        assert min(acc) > 0, out.stdout          # every branch (accepted and refused) was exercised


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_persistent_loop_tiling_under_asan_ubsan(tmp_path):
    """The host-built tiling of the persistent backward loop (csrc/persist_plan.cpp): every row segment owned once, tiles balanced to
    +- 1, edge / cross-band flags exactly where a stencil leaves the tile / the band, edge segments first, neighbour lists complete
    and symmetric -- on the shipped headline plan and on random grids, band counts, workgroup counts and strip widths."""
    exe = str(tmp_path / "persist_plan_check")
    src = [os.path.join(ROOT, "tests", "native", "persist_plan_check.cpp"), os.path.join(ROOT, "sep-2023_amd", "csrc", "persist_plan.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for seed in (1, 2):
        out = subprocess.run([exe, str(seed), "300"], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_injection_plan_under_asan_ubsan(tmp_path):
    """The host-built adjoint-source plan of the persistent loop's general receivers (csrc/inject_plan.cpp): for random scattered,
    repeated, strided, vertical and directional channel sets, folding the residual per target cell and adding it through lookup /
    lane mask / popcount leaves exactly what the channel-by-channel adds of res_injection_exx / _ezz (Src/utilities.cu:605-641) leave."""
    exe = str(tmp_path / "inject_plan_check")
    src = [os.path.join(ROOT, "tests", "native", "inject_plan_check.cpp"), os.path.join(ROOT, "sep-2023_amd", "csrc", "inject_plan.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for seed in (1, 2):
        out = subprocess.run([exe, str(seed), "400"], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_owning_buffers_under_asan_ubsan(tmp_path):
    """The owners of every device and pinned allocation, stream and event of the library (csrc/device_alloc.hpp), on a malloc-backed
    stub of the two raw functions: moves, the tally and the process-wide counters against the bytes really held, ensure (free before
    allocate; a failed allocation leaves an empty buffer of capacity 0), constructors that throw after every j-th allocation, maps
    of move-only structs of buffers -- and a clean leak report."""
    exe = str(tmp_path / "device_buffer_check")
    src = [os.path.join(ROOT, "tests", "native", "device_buffer_check.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_schedule_and_lane_layouts_under_asan_ubsan(tmp_path):
    """The schedule of a call, the sub-batches of a batch and the lane layouts (csrc/schedule.cpp): over a dense sweep of array sizes,
    group sizes, call kinds, options and store caps the schedule is the one Session::run used to work out in place (kept in the check
    word for word); the grids that the comment in Session::run names get the backward batch sizes it states, the notebook problem all
    its 19 shots at once; the sub-batches of every batch of 1 ... 64 shots are non-empty, contiguous, cover it and carry the facts of
    exactly their shots; the layout views give the offsets they replace."""
    exe = str(tmp_path / "schedule_check")
    src = [os.path.join(ROOT, "tests", "native", "schedule_check.cpp"), os.path.join(ROOT, "sep-2023_amd", "csrc", "schedule.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe, "1"], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 10 ** 7, out.stdout      # the sweep ran in full
