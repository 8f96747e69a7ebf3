"""The trip arithmetic of csrc/knn_tile_schedule.h on the host: a four-set sweep of the second kNN filter form runs as
whole trips of four calls in a loop with no exit inside, then its zero to three remaining calls written out
(csrc/knn_filter.h f2_sweep4 uses f2_whole_trips, f2_remainder_calls, f2_remainder_trip_call, f2_trip_load_set and
f2_trip_use_set).  tests/knn_trip_schedule_host.cpp is a stand-alone program that walks those functions like the kernel
does for every sweep length from 1 to 200 tiles, from tile 0 and from tile 41, and checks that

  * every tile is visited once and in order,
  * no set is loaded before the call that issued its products, every tile is loaded once before its products, and
    only the last four loads re-read the clamped last tile,
  * the remainder calls continue the set, key-block and CONV rotation of the trips.

It is built twice: plainly, and with -fsanitize=address,undefined (run directly, no preload)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "asan_ubsan"])
def test_trip_schedule(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "knn_trip_schedule_host")
    subprocess.check_call([cxx, *flags, "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "deepmetv2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "knn_trip_schedule_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 400 sweeps"), r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
