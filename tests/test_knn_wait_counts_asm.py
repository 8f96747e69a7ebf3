"""The waits hipcc places in the tile blocks of knn_filter12_kernel<16,1>, read from the device assembly.

The recording sweeps of the second filter form at 32 features keep four operand tiles in flight (csrc/knn_filter.h
f2_sweep4).  That holds only while the compiler's own wait insertion answers every tile block with a COUNTED s_waitcnt
vmcnt(N) that leaves the younger tiles' loads outstanding.  Where paths with different numbers of loads in flight join
-- a loop with an exit after every call was such a join -- it answers with vmcnt(0), a full drain, and the pipeline is
one tile deep again without a single source line saying so.  This test is the guard: it compiles csrc/knn.hip to
gfx950 assembly with the build's flags, runs tools/knn_tile_counts.py on it, and asserts for <16,1>

  * every tile block of the main sweep, the revisit and the second attempt (30 v_alignbit on the hot path) that issues
    MFMAs waits on its hot path with vmcnt(N), N >= 3, only: no vmcnt(0), no smaller count, and at least one wait per
    block (a block that issues products must wait for operands);
  * the trip blocks are there: 3 x 4 recording blocks whose only wait is vmcnt(9) -- three tiles of three loads in
    flight -- and 3 x 2 remainder blocks with vmcnt(6) and vmcnt(3) (the third remainder call issues no products);
  * no scratch, and two wavefronts per SIMD (at most 256 VGPRs), in all six instances;
  * in all six instances no inline-asm vector instruction is the first to touch an MFMA's result within 12 wait
    states: hipcc pads those states for its own instructions only, and the deferred pass as a four-call trip once had
    a v_min3 statement directly behind its MFMA (wrong thresholds: other flagged-query counts, right tables).

The deferred pass is NOT held to counted waits: on the four-set trip its block of four tiles had them (vmcnt
6, 9, 11, 10, 9, 6) and was slower in every measured run, so it keeps its two-set loop, whose block of two tiles waits
with vmcnt 0, 5, 4, 3 (profiles/r10_knn_counted_waits.md).  Its waits are printed, not asserted.

CPU only; skipped where hipcc is absent."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-DNDEBUG", "--cuda-device-only", "-S"]
INSTANCES = ((8, 1), (16, 1), (20, 1), (8, 2), (16, 2), (20, 2))


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return exe if os.path.exists(exe) else None


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    path = str(tmp_path_factory.mktemp("knn_asm") / "knn.s")
    subprocess.check_call([hipcc, *FLAGS, os.path.join(ROOT, "deepmetv2_amd", "csrc", "knn.hip"), "-o", path])
    return path


def _rows(asm_path):
    """tools/knn_tile_counts.py's table for <16,1>: one dict per block that issues MFMAs"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "knn_tile_counts.py"), asm_path, "16", "1"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    head = lines[0].split()
    assert head[0] == "block" and head[-1] == "vmcnt", lines[0]
    rows = []
    for ln in lines[1:]:
        f = ln.split()
        row = {h: (v if h in ("block", "vmcnt") else int(v)) for h, v in zip(head, f)}
        row["waits"] = [] if row["vmcnt"] == "-" else [int(v) for v in row["vmcnt"].split(",")]
        rows.append(row)
    return rows


def test_recording_tile_blocks_wait_with_counts_only(asm):
    rows = _rows(asm)
    rec = [r for r in rows if r["mfma"] > 0 and r["alignbit"] == 30]
    # (a deferred tile inserts into the threshold list: M - 1 = 21 v_med3 at k = 16, and two start its minimum trees;
    # the blocks that open a recording sweep hold two v_med3)
    deferred = [r for r in rows if r["mfma"] > 0 and r["alignbit"] == 0 and r["med3"] >= 21]
    for r in rec + deferred:
        print(r["block"], "VALU", r["VALU"], "med3", r["med3"], "loads", r["loads"], "vmcnt", r["vmcnt"])
    assert rec and deferred, rows
    for r in rec:
        assert r["waits"], f"{r['block']} issues MFMAs and waits for nothing: {r}"
        assert min(r["waits"]) >= 3, f"{r['block']} drains its operand loads: vmcnt {r['vmcnt']}"
    # three recording sweeps (main, revisit, second attempt): four trip blocks each, three tiles in flight at the wait,
    # and the first two remainder calls
    assert len(rec) == 18, [(r["block"], r["vmcnt"]) for r in rec]
    assert sum(1 for r in rec if r["loads"] == 3 and r["waits"] == [9]) == 12, [(r["block"], r["vmcnt"]) for r in rec]
    assert sum(1 for r in rec if r["waits"] == [6]) == 3 and sum(1 for r in rec if r["waits"] == [3]) == 3, \
        [(r["block"], r["vmcnt"]) for r in rec]


def test_no_scratch_and_two_waves_per_simd(asm):
    text = open(asm).read()
    for kp, nh in INSTANCES:
        m = re.search(rf"\.amdhsa_kernel \S*knn_filter12_kernelILi{kp}ELi{nh}E\S*\n(.*?)\.end_amdhsa_kernel", text, re.S)
        assert m, (kp, nh)
        body = m.group(1)
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        print(f"<{kp},{nh}>: {vgprs} VGPRs, {scratch} bytes of scratch")
        assert scratch == 0, (kp, nh, scratch)
        assert vgprs <= 256, (kp, nh, vgprs)     # 512 per SIMD lane: two wavefronts


@pytest.mark.parametrize("kp,nh", INSTANCES)
def test_no_asm_statement_reads_a_fresh_mfma_result(asm, kp, nh):
    """hipcc pads the wait states after an MFMA only for readers of its own: the v_min3 statements of f2_tile must come
    behind one (tools/knn_mfma_asm_distance.py; 12 wait states after an 8-pass MFMA otherwise)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "knn_mfma_asm_distance.py"), asm, str(kp), str(nh)],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wait states to their MFMA: 0" in r.stdout, r.stdout
