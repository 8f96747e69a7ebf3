"""csrc/knn_key64.h on the host: the kNN re-rank's sorted insertion as f64 min / max (new[p] = max(old[p-1], min(old[p],
nk)) on the (distance bits << 32 | id) words read as doubles, high word clamped to the sentinel's bits) against the
compare / select insertion on unsigned 64-bit words that it replaces.  tests/knn_key64_host.cpp is a stand-alone
program built with the host compiler; it takes the header's host path (bit casts + fmin / fmax) and fuzzes lists of
8 / 16 / 20 slots, empty to full, with random words, repeated words, and the edge patterns: high word 0 with
id 0 / 1 / 0xFFFFFFFF (+0.0 and subnormal doubles), the sentinel with id 0 and above, +inf, -inf, 0x7FC00000, 0xFFC00000,
0x7FFFFFFF, 0x80000000 and the ~0 of an exhausted lane.  Every list must equal the reference word for word after every
insertion.  This proves the clamp and the min / max network, not the GPU instruction (tests/test_gpu_knn_rerank_keys.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_key64_insertion_matches_compare_select(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "knn_key64_host")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "deepmetv2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "knn_key64_host.cpp"), "-o", exe])
    r = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok"), r.stdout
