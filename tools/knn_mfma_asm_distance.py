"""Wait states between an MFMA and the first inline-asm vector instruction that touches its result, per basic block of
knn_filter12_kernel<KP, NH>, counted in the device assembly.

    hipcc $FLAGS deepmetv2_amd/csrc/knn.hip -o knn.s          (FLAGS as in tools/knn_tile_counts.py)
    python tools/knn_mfma_asm_distance.py knn.s 16 1

hipcc pads the wait states an MFMA's result needs before its first reader or writer (12 after an 8-pass MFMA such as
v_mfma_f32_32x32x16_f16) only for instructions it knows; nothing is padded for the text between ;;#ASMSTART and
;;#ASMEND.  The tile code of the second filter form takes its minima with v_min3_f32 statements (csrc/knn_filter.h
f2_tile), each made to depend on an instruction of hipcc's own that reads the same accumulator block first.  This tool
shows that it came out so: for every block, the smallest number of wait states between an MFMA and an asm vector
instruction that reads or writes a register of its destination with no hipcc instruction reading that register in
between ("asm"), and the same figure for hipcc's own first readers for comparison ("hipcc": padded by the compiler).
A wait state is counted per instruction in between, N + 1 for an s_nop N: a lower bound of the cycles.
Prints the ten smallest distances of each kind; exit status 1 if an "asm" distance is below 12."""
import re
import sys

NEEDED = 12


def regs(tok):
    m = re.match(r"^([va])\[(\d+):(\d+)\]$", tok)
    if m:
        return {(m.group(1), r) for r in range(int(m.group(2)), int(m.group(3)) + 1)}
    m = re.match(r"^([va])(\d+)$", tok)
    return {(m.group(1), int(m.group(2)))} if m else set()


def distances(path, kp, nh):
    """{(block, 'asm' | 'hipcc'): (wait states, instruction)}: the smallest per block and kind"""
    sym = f"knn_filter12_kernelILi{kp}ELi{nh}E"
    lines = open(path).read().split("\n")
    start = next(i for i, ln in enumerate(lines) if re.match(rf"^_Z\S*{sym}\S*:", ln))
    end = next(i for i in range(start, len(lines)) if ".Lfunc_end" in lines[i])
    block, inasm, now, fresh, worst = "entry", False, 0, {}, {}
    for ln in lines[start + 1:end]:
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            block, now, fresh = m.group(1), 0, {}
            continue
        s = ln.strip()
        if s.startswith(";;#ASMSTART"):
            inasm = True
            continue
        if s.startswith(";;#ASMEND"):
            inasm = False
            continue
        if not s or s.startswith((";", ".")):
            continue
        s = re.sub(r"\s*;.*$", "", s)
        parts = s.replace(",", " ").split()
        op, ops = parts[0], parts[1:]
        if op.startswith("v_mfma"):
            now += 1
            for r in regs(ops[0]):
                fresh[r] = now       # the state after which the MFMA was issued
            continue
        if op.startswith("v_") and ops:
            touched = set()
            for t in ops:
                touched |= regs(t)
            hit = [now - fresh[r] for r in touched if r in fresh]
            if hit:
                key = (block, "asm" if inasm else "hipcc")
                if key not in worst or min(hit) < worst[key][0]:
                    worst[key] = (min(hit), s)
                if not inasm:
                    # hipcc has padded for this MFMA: every register it wrote is safe from here on
                    at = {fresh[r] for r in touched if r in fresh}
                    fresh = {r: v for r, v in fresh.items() if v not in at}
        now += int(ops[0], 0) + 1 if op == "s_nop" else 1
    return worst


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    worst = distances(*argv)
    bad = 0
    for kind in ("asm", "hipcc"):
        rows = sorted((v[0], k[0], v[1]) for k, v in worst.items() if k[1] == kind)
        for d, block, ins in rows[:10]:
            print(f"{kind:5s} {block:12s} {d:4d}  {ins}")
        if kind == "asm":
            bad = sum(1 for d, _b, _i in rows if d < NEEDED)
    print(f"asm readers closer than {NEEDED} wait states to their MFMA: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
