"""Vector instructions per tile visit of knn_filter12_kernel<KP, NH>, counted in the device assembly.

    FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -DNDEBUG --cuda-device-only -S"
    hipcc $FLAGS deepmetv2_amd/csrc/knn.hip -o knn.s
    python tools/knn_tile_counts.py knn.s 16 1

Counting rule (profiles/r06_knn_operands.md): every basic block of the instance that issues MFMAs is listed; its hot path
runs from the block label to the first s_cbranch_vccz -- the branch that guards the rare f2_compact -- or to the end of
the block where there is none.  VALU = instructions that start with v_ except the MFMAs.  The tile blocks of the second
form are the ones with 30 v_alignbit (hit masks: revisit and second attempt without v_med3, main sweep with) and the
block with 2 x (M + 1) v_med3 and no v_alignbit (two tiles of the deferred pass: M - 1 of the list insertion and two
that start the minimum trees per tile; four tiles in a -DDMET_F2_DEFER_FOUR build).  The last column lists the N of
every s_waitcnt vmcnt(N) on the hot path, in order: a 0 is a full drain of the operand loads in flight
(profiles/r10_knn_counted_waits.md)."""
import re
import sys


def blocks_of(path, kp, nh):
    sym = f"knn_filter12_kernelILi{kp}ELi{nh}E"
    lines = open(path).read().split("\n")
    start = next(i for i, ln in enumerate(lines) if re.match(rf"^_Z\S*{sym}\S*:", ln))
    end = next(i for i in range(start, len(lines)) if ".Lfunc_end" in lines[i])
    out, cur = [], ["entry", []]
    for ln in lines[start + 1:end]:
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            out.append(cur)
            cur = [m.group(1), []]
            continue
        s = ln.strip()
        if s and not s.startswith((";", ".")):
            cur[1].append(re.sub(r"\s*;.*$", "", s))
    out.append(cur)
    return out


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    print(f"{'block':12s} {'hot':>4s} {'mfma':>4s} {'VALU':>4s} {'v_mov':>5s} {'swap':>4s} {'mad_u64':>7s} {'med3':>4s} "
          f"{'alignbit':>8s} {'loads':>5s}  vmcnt")
    for name, ins in blocks_of(*argv):
        if not any(i.startswith("v_mfma") for i in ins):
            continue
        cut = next((n for n, i in enumerate(ins) if i.startswith("s_cbranch_vccz")), len(ins) - 1)
        hot = ins[:cut + 1]
        valu = [i for i in hot if i.startswith("v_") and not i.startswith("v_mfma")]
        waits = [m.group(1) for i in hot if i.startswith("s_waitcnt") for m in [re.search(r"vmcnt\((\d+)\)", i)] if m]

        def n(*prefix):
            return sum(1 for i in valu if i.startswith(prefix))
        print(f"{name:12s} {len(hot):4d} {sum(1 for i in hot if i.startswith('v_mfma')):4d} {len(valu):4d} "
              f"{n('v_mov_b32', 'v_mov_b64'):5d} {n('v_permlane32_swap'):4d} {n('v_mad_u64_u32'):7d} {n('v_med3'):4d} "
              f"{n('v_alignbit'):8d} {sum(1 for i in hot if i.startswith(('global_load', 'flat_load'))):5d}  "
              f"{','.join(waits) or '-'}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
