"""csrc/knn_tile_schedule.h on the host: which candidate tile every call of a sweep of the second kNN filter form loads,
and which operand set and key block a tile uses -- the definition the kernel (csrc/knn_filter.h f2_sweep4, f2_sweep)
uses.  tests/knn_tile_schedule_host.cpp is a stand-alone program that walks the schedule like the kernel does, for
candidate ranges that start at tile 0 and 41 and hold 0-9, 25-28, 32, 33, 37, 41 and 109 tiles, as a deferred / main /
revisit triple (with 32, 8 and 2 deferred tiles; every sweep starts on its own) and as a lone second-attempt sweep, the
recording sweeps with four operand sets and the deferred pass with two, and checks that

  * every tile's operands are loaded exactly once before the call that issues its matrix products; only the last
    four (two) loads of a sweep re-read its clamped last tile,
  * a load never goes to a set whose operands still wait to be used,
  * every tile index lies inside the sweep's range,
  * consecutive tiles use different key blocks and the threshold is converted on the odd calls of a sweep, as in the
    loop of two calls per trip.

It is built twice: plainly, and with -fsanitize=address,undefined (run directly, no preload)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "asan_ubsan"])
def test_tile_schedule(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "knn_tile_schedule_host")
    subprocess.check_call([cxx, *flags, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "deepmetv2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "knn_tile_schedule_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok"), r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
