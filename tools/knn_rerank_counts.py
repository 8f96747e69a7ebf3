"""Instructions of the exact re-rank's sorted insertion in knn_filter12_kernel<KP, NH>, counted in the device assembly.

    FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -DNDEBUG --cuda-device-only -S"
    hipcc $FLAGS deepmetv2_amd/csrc/knn.hip -o knn.s
    python tools/knn_rerank_counts.py knn.s 16 1 [more.s ...]

Every basic block of the instance that holds a piece of the insertion -- a 64-bit unsigned compare (the compare / select
form) or a v_min_f64 / v_max_f64 (csrc/knn_key64.h) -- is listed with its totals by mnemonic class.  The round block of
the 32-feature re-rank is the one with the 32 v_sub_f32 + 32 v_fmac_f32 of the R1 chain (64 + 64 at 64 features, the
loop of one row per lane); the split-item merge is the block with KP insertions and no chain.  The tool counts and
classifies; it asserts nothing (profiles/r07_knn_rerank.md reads the tables)."""
import re
import sys

from knn_tile_counts import blocks_of

CLASSES = (
    ("total", lambda i: True),
    ("VALU", lambda i: i.startswith("v_") and not i.startswith("v_mfma")),
    ("cndmask", lambda i: i.startswith("v_cndmask")),
    ("cmp_u64", lambda i: re.match(r"v_cmpx?_\w+_u64", i) is not None),
    ("cmp_oth", lambda i: i.startswith("v_cmp") and re.match(r"v_cmpx?_\w+_u64", i) is None),
    ("minmax64", lambda i: i.startswith(("v_min_f64", "v_max_f64"))),
    ("sub_f32", lambda i: i.startswith("v_sub_f32")),
    ("fma_f32", lambda i: i.startswith(("v_fmac_f32", "v_fma_f32"))),
    ("addr64", lambda i: i.startswith(("v_ashrrev_i32", "v_lshlrev_b64", "v_lshl_add_u64", "v_mad_u64_u32", "v_mad_i64_i32"))),
    ("v_mov", lambda i: i.startswith("v_mov_b")),
    ("s_nop", lambda i: i.startswith("s_nop")),
    ("waitcnt", lambda i: i.startswith("s_waitcnt")),
    ("saveexec", lambda i: "saveexec" in i),
    ("gload", lambda i: i.startswith(("global_load", "flat_load"))),
    ("ds_rd", lambda i: i.startswith("ds_read")),
    ("ds_wr", lambda i: i.startswith("ds_write")),
    ("bperm", lambda i: i.startswith("ds_bpermute")),
)


def table(path, kp, nh):
    print(f"{path}  knn_filter12_kernel<{kp},{nh}>")
    print(f"{'block':12s} " + " ".join(f"{name:>8s}" for name, _ in CLASSES))
    for name, ins in blocks_of(path, kp, nh):
        if not any(re.match(r"v_cmpx?_\w+_u64|v_min_f64|v_max_f64", i) for i in ins):
            continue
        print(f"{name:12s} " + " ".join(f"{sum(1 for i in ins if f(i)):8d}" for _, f in CLASSES))


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    for path in [argv[0]] + argv[3:]:
        table(path, argv[1], argv[2])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
