"""Micro-benchmark of the fused EdgeConv pieces on BASELINE configs[1] shapes (real kNN table).

`python tools/gather_micro.py --forms LABEL` instead times every forward form one launch at a time (HIP events, 200 launches
after 20 warm-up ones) and prints ONE JSON line: per form [median, 10th, 90th percentile] in us.  For an A/B of two builds of
the library run it in alternation, `DMET_HIP_LIB=<other build> python tools/gather_micro.py --forms parent` and
`python tools/gather_micro.py --forms new`, a few processes each, and compare the medians with the spread between the
processes of one build (profiles/NOTES.md, "K3 empty-row rule").  Forms: the LDS kNN gather at 64 x 4500 nodes for k = 16 and
32 in both table layouts and id widths, with and without arg; the fused kernel; a batch with one 5200-node event among 4500-node
ones (the LDS kernel's own L2 path, and the mixed entry); the counted gather out of the radius kernel's uint16 rows."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from deepmetv2_amd import _native, _lib


def time_forms(label):
    import json
    import deepmetv2_amd as dm
    dev = torch.device("cuda:0"); torch.manual_seed(0)
    B, n, H = 64, 4500, 32
    res = {"lib": label}

    def measure(name, f):
        for _ in range(20): f()
        torch.cuda.synchronize()
        ts = []
        for _ in range(200):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); f(); e.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(e) * 1e3)
        ts.sort()
        res[name] = [round(ts[len(ts) // 2], 2), round(ts[len(ts) // 10], 2), round(ts[9 * len(ts) // 10], 2)]

    W = torch.randn(H, 2 * H, device=dev) * 0.1; b = torch.randn(H, device=dev)
    for k in (16, 32):
        x = torch.randn(B * n, H, device=dev)
        ptr = torch.arange(0, (B + 1) * n, n, dtype=torch.int64, device=dev)
        nbr, _, loc = _native.knn_local(x, ptr, k)
        P, Q = _native.node_linear_split(x, W, b)
        Ps, Qs = _native.node_linear_split(x, W, b, sliced=True)
        measure(f"k{k}_sliced_u16_arg", lambda: _native.gather_max(Ps, Qs, nbr, ptr, True, lds=True, nbr_local=loc, sliced=True))
        measure(f"k{k}_sliced_u16_noarg", lambda: _native.gather_max(Ps, Qs, nbr, ptr, False, lds=True, nbr_local=loc, sliced=True))
        measure(f"k{k}_sliced_i32_arg", lambda: _native.gather_max(Ps, Qs, nbr, ptr, True, lds=True, sliced=True))
        measure(f"k{k}_row_u16_arg", lambda: _native.gather_max(P, Q, nbr, ptr, True, lds=True, nbr_local=loc))
        measure(f"k{k}_row_i32_arg", lambda: _native.gather_max(P, Q, nbr, ptr, True, lds=True))
        measure(f"k{k}_row_i32_noarg", lambda: _native.gather_max(P, Q, nbr, ptr, False, lds=True))
        measure(f"k{k}_fused_arg", lambda: _native.edgeconv_fused_lds(x, W, b, nbr, ptr, True))
    # one event beyond the LDS image: the LDS kernel's in-kernel L2 path, and the mixed entry
    sizes = [4500] * 31 + [5200]
    x = torch.randn(sum(sizes), H, device=dev)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)]).to(dev)
    nbr, _, loc = _native.knn_local(x, ptr, 16)
    P, Q = _native.node_linear_split(x, W, b)
    measure("big_event_lds_u16_arg", lambda: _native.gather_max(P, Q, nbr, ptr, True, lds=True, nbr_local=loc))
    measure("big_event_mixed_u16_arg", lambda: _native.gather_max(P, Q, nbr, ptr, True, nbr_local=loc, mixed=True))
    # the radius table of the static flow: counted rows read as event-local uint16 rows
    N = B * n
    etaphi = torch.stack([(torch.rand(N, device=dev) - 0.5) * 5, (torch.rand(N, device=dev) - 0.5) * 6.28], 1)
    batch = torch.repeat_interleave(torch.arange(B, device=dev), n)
    t = dm.radius_table(etaphi, 0.4, batch, loop=True, max_num_neighbors=255)
    x = torch.randn(N, H, device=dev)
    Ps, Qs = _native.node_linear_split(x, W, b, sliced=True)
    if t.rows16 is not None:
        order = t.order_by_count()
        measure("local_j16_sliced_arg", lambda: _native.gather_max_local_j16(Ps, Qs, t.rows16, t.cnt, order, t.ptr, t.k, True))
        measure("local_j16_sliced_noarg", lambda: _native.gather_max_local_j16(Ps, Qs, t.rows16, t.cnt, order, t.ptr, t.k, True,
                                                                                want_arg=False))
    print(json.dumps(res))


if "--forms" in sys.argv:
    time_forms(sys.argv[sys.argv.index("--forms") + 1])
    sys.exit(0)
B, n, H, k = int(sys.argv[1]) if len(sys.argv) > 1 else 64, 4500, 32, 16
dev = torch.device("cuda:0"); torch.manual_seed(0)
x = torch.randn(B * n, H, device=dev)
ptr = torch.arange(0, (B + 1) * n, n, dtype=torch.int64, device=dev)
nbr, _, loc = _native.knn_local(x, ptr, k)
W = torch.randn(H, 2 * H, device=dev) * 0.1; b = torch.randn(H, device=dev)
P, Q = _native.node_linear_split(x, W, b)
def timeit(f, reps=30):
    for _ in range(3): f()
    torch.cuda.synchronize()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): f()
    e.record(); torch.cuda.synchronize()
    return a.elapsed_time(e) / reps * 1e3
res = {}
for form in ("l2-only", "lds"):
    _native.GATHER_MAX_FORM = form
    for arg in (False, True):
        us = timeit(lambda: _native.gather_max(P, Q, nbr, ptr, arg))
        byts = B * n * (128 + 64 + 128 + (32 if arg else 0))
        print(f"gather_max[{form}] arg={arg}: {us:7.2f} us  -> {byts/us/1e3:7.1f} GB/s algorithmic = {byts/us/1e3/8000*100:5.1f}% of 8 TB/s")
    res[form] = _native.gather_max(P, Q, nbr, ptr, True)
for arg in (False, True):
    us = timeit(lambda: _native.gather_max(P, Q, nbr, ptr, arg, lds=True, nbr_local=loc))
    byts = B * n * (128 + 64 + 128 + (32 if arg else 0))
    print(f"gather_max[lds, uint16 local ids] arg={arg}: {us:7.2f} us  -> {byts/us/1e3:7.1f} GB/s algorithmic = {byts/us/1e3/8000*100:5.1f}% of 8 TB/s")
r16 = _native.gather_max(P, Q, nbr, ptr, True, lds=True, nbr_local=loc)
print("uint16 ids agree:", torch.equal(r16[0], res["lds"][0]), torch.equal(r16[1], res["lds"][1]))
print("forms agree:", torch.equal(res["l2-only"][0], res["lds"][0]), torch.equal(res["l2-only"][1], res["lds"][1]))
for arg in (False, True):
    us = timeit(lambda: _native.edgeconv_fused_lds(x, W, b, nbr, ptr, arg))
    byts = B * n * (128 + 64 + 128 + (32 if arg else 0))
    print(f"edgeconv_fused_lds arg={arg}: {us:7.2f} us -> {byts/us/1e3:7.1f} GB/s algorithmic = {byts/us/1e3/8000*100:5.1f}% of 8 TB/s")
ref = _native.gather_max(P, Q, nbr, ptr, True)
fo = _native.edgeconv_fused_lds(x, W, b, nbr, ptr, True)
print("fused vs split max|d|:", float((fo[0]-ref[0]).abs().max()), "arg mismatches:", int((fo[1]!=ref[1]).sum()))
print(f"node_linear_split: {timeit(lambda: _native.node_linear_split(x, W, b)):.2f} us")
