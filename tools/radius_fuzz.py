"""Randomised cross-check of the windowed radius graph against the all-pairs sweep: ids, order and counts must agree
(plain coordinates, then periodic ones)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from deepmetv2_amd import _native

dev = torch.device("cuda:0")
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 60
g = torch.Generator().manual_seed(77)
bad = 0
for it in range(rounds):
    B = int(torch.randint(1, 50, (1,), generator=g))
    hi = [3000, 100, 6000, 20, 800][it % 5]
    sizes = [int(v) for v in torch.randint(0, hi, (B,), generator=g)]
    N = sum(sizes)
    if N == 0:
        continue
    D = [2, 1, 3, 8, 2][it % 5]
    x = torch.randn(N, D, generator=g) * torch.tensor([3.0, 2.0, 1.0, 0.5, 0.5, 0.2, 0.2, 0.1][:D])
    mode = it % 4
    if mode == 1:      # dense blobs: rows overflow max_nbr
        c = torch.randn(5, D, generator=g) * 2
        x = c[torch.randint(0, 5, (N,), generator=g)] + 0.05 * torch.randn(N, D, generator=g)
    elif mode == 2:    # lattice: exact ties at the radius
        x = torch.round(x * 4) / 4
    elif mode == 3:    # constant first coordinate: the window keeps everything
        x[:, 0] = 0.25
    r = [0.4, 0.25, 1.0, 0.05][it % 4]
    mx = [255, 32, 7, 64][(it // 4) % 4]
    skip = bool(it % 2)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)]).to(dev)
    xd = x.to(dev)
    _native.RADIUS_FORM = "sweep"
    n0, c0 = _native.radius(xd, ptr, r, mx, skip_self=skip, pad=True)
    _native.RADIUS_FORM = "windowed"
    n1, c1 = _native.radius(xd, ptr, r, mx, skip_self=skip, pad=True)
    ok = torch.equal(n0, n1) and torch.equal(c0, c1)
    bad += 0 if ok else 1
    print(f"round {it:3d}: B={B:2d} N={N:6d} D={D} r={r} max={mx:3d} mode={mode} mean_cnt={float(c0.float().mean()):6.1f} {'ok' if ok else 'MISMATCH'}")
print("mismatching rounds:", bad)

# periodic rounds (radius_graph(..., period=)): the windowed periodic build against the all-pairs one.  Coordinate 0 stays
# plain (the window's coordinate); one or two later coordinates are periodic, their values atan2-like in one period
# or, every third round, spread over three periods (the formula still defines the bits there)
bad_p = 0
for it in range(rounds):
    B = int(torch.randint(1, 50, (1,), generator=g))
    hi = [3000, 100, 6000, 20, 800][it % 5]
    sizes = [int(v) for v in torch.randint(0, hi, (B,), generator=g)]
    N = sum(sizes)
    if N == 0:
        continue
    D = [2, 3, 2, 8, 4][it % 5]
    x = torch.randn(N, D, generator=g) * torch.tensor([3.0, 2.0, 1.0, 0.5, 0.5, 0.2, 0.2, 0.1][:D])
    period = [0.0] * D
    period[1] = 2 * 3.14159265358979
    if D > 2 and it % 2:
        period[D - 1] = 1.5
    for c in range(1, D):
        if period[c] > 0:
            L = period[c]
            span = 3.0 if it % 3 == 0 else 1.0
            x[:, c] = (torch.rand(N, generator=g) - 0.5) * L * span
    mode = it % 4
    if mode == 1:      # dense blobs across the seam: rows overflow max_nbr on wrapped hits
        x[: N // 2, 1] = torch.where(torch.rand(N // 2, generator=g) < 0.5, -3.1, 3.1)
        x[: N // 2, 0] = 0.1 * torch.randn(N // 2, generator=g)
    elif mode == 2:    # lattice: exact ties at the radius
        x = torch.round(x * 4) / 4
    elif mode == 3:    # constant first coordinate: the window keeps everything
        x[:, 0] = 0.25
    r = [0.4, 0.25, 1.0, 3.3][it % 4]
    mx = [255, 32, 7, 64][(it // 4) % 4]
    skip = bool(it % 2)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(sizes).cumsum(0)]).to(dev)
    xd = x.to(dev)
    _native.RADIUS_FORM = "sweep"
    n0, c0 = _native.radius_periodic(xd, ptr, r, mx, period, skip_self=skip, pad=True)
    _native.RADIUS_FORM = "windowed"
    n1, c1 = _native.radius_periodic(xd, ptr, r, mx, period, skip_self=skip, pad=True)
    ok = torch.equal(n0, n1) and torch.equal(c0, c1)
    bad_p += 0 if ok else 1
    print(f"periodic round {it:3d}: B={B:2d} N={N:6d} D={D} period={[round(p, 3) for p in period]} r={r} max={mx:3d} "
          f"mode={mode} mean_cnt={float(c0.float().mean()):6.1f} {'ok' if ok else 'MISMATCH'}")
print("mismatching periodic rounds:", bad_p)
sys.exit(1 if bad or bad_p else 0)
