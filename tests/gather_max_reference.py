"""K3, out = P + max_j Q[nbr[i, j]]: a plain CPU reference of the contract every gather-max form is held to (include/dmet.h,
DESIGN.md R3 / R4).  The operation is one exact maximum followed by one fp32 add, so the reference is bit-exact: the GPU
tests compare with torch.equal, no tolerance.

  row i uses slots 0 .. m-1, m = min(k, cnt[i]) (k without cnt); a slot with nbr < 0 is empty;
  per channel best = -inf, winner = 255; slots in ascending order, best replaced on strict `>` only: the lowest slot wins
  exact ties (R4), +0 == -0, NaN and -inf never win, +inf wins (ties among +inf to the lowest slot);
  a row with a non-empty slot: out = fl32(P + best), arg = winner (255 for a channel nothing beat);
  a row without one: out = 0, arg = 255, whatever P holds (R3).

numpy, not torch: numpy's float32 compare and add keep subnormals whatever the thread's flush-to-zero state."""
import numpy as np
import torch

_ROWS = 8192        # rows gathered at a time: the largest intermediate is _ROWS x H floats


def _np(t, dtype):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=dtype)


def gather_max_ref(P, Q, nbr, cnt=None):
    """(out float32 [N, H], arg uint8 [N, H]) as torch CPU tensors."""
    P, Q, nbr = _np(P, np.float32), _np(Q, np.float32), _np(nbr, np.int64)
    N, H = P.shape
    k = nbr.shape[1]
    m = np.full(N, k, np.int64) if cnt is None else np.minimum(k, _np(cnt, np.int64))
    out = np.zeros((N, H), np.float32)
    arg = np.full((N, H), 255, np.uint8)
    with np.errstate(invalid="ignore"):
        for r0 in range(0, N, _ROWS):
            r1 = min(N, r0 + _ROWS)
            best = np.full((r1 - r0, H), -np.inf, np.float32)
            win = np.full((r1 - r0, H), 255, np.uint8)
            some = np.zeros(r1 - r0, bool)
            for s in range(k):
                j = nbr[r0:r1, s]
                used = (j >= 0) & (s < m[r0:r1])
                if not used.any():
                    continue
                v = Q[np.where(used, j, 0)]
                better = used[:, None] & (v > best)          # False for NaN, for -inf and for an exact tie
                best = np.where(better, v, best)
                win = np.where(better, np.uint8(s), win)
                some |= used
            out[r0:r1] = np.where(some[:, None], P[r0:r1] + best, np.float32(0))
            arg[r0:r1] = np.where(some[:, None], win, np.uint8(255))
    return torch.from_numpy(out), torch.from_numpy(arg)


def gather_max_loops(P, Q, nbr, cnt=None):
    """The same contract as a literal triple loop (rows, channels, slots): what gather_max_ref is checked against."""
    P, Q, nbr = _np(P, np.float32), _np(Q, np.float32), _np(nbr, np.int64)
    N, H = P.shape
    k = nbr.shape[1]
    out = np.zeros((N, H), np.float32)
    arg = np.full((N, H), 255, np.uint8)
    ninf = np.float32(-np.inf)
    for i in range(N):
        m = k if cnt is None else min(k, int(cnt[i]))
        if not any(nbr[i, s] >= 0 for s in range(m)):
            continue
        for c in range(H):
            best, win = ninf, 255
            for s in range(m):
                if nbr[i, s] >= 0 and Q[nbr[i, s], c] > best:
                    best, win = Q[nbr[i, s], c], s
            out[i, c] = np.float32(P[i, c]) + np.float32(best)
            arg[i, c] = win
    return torch.from_numpy(out), torch.from_numpy(arg)


def winner_ids16(arg, nbr, ptr):
    """The uint16 event-local winner ids of the `j16` forms, as int64 [N, H]: nbr[i, arg[i, c]] - ptr[event of i], and
    0xFFFF where arg is 255.  Compare with `argj.long() & 0xFFFF`."""
    arg, nbr, ptr = arg.cpu().long(), nbr.cpu().long(), ptr.cpu().long()
    lo = torch.repeat_interleave(ptr[:-1], ptr.diff()).view(-1, 1)
    none = arg == 255
    j = torch.gather(nbr, 1, arg.masked_fill(none, 0))
    return torch.where(none, torch.full_like(j, 0xFFFF), j - lo)


# ---------------------------------------------------------------------------------------------------------------------
# The inputs of the tests: one ragged batch whose rows and columns carry every input class, so that one call covers them.
# A node's classes go by its event-local index l and a channel's by c % 8 (H is a multiple of 8):
#   Q columns  c % 8 in {2, 3}: multiples of 0.25 in [-1, 1], most candidates tie (c);  {4, 5}: +inf in the rows of the
#              nodes l % 16 == 10 (e);  everything else random floats (a)
#   Q rows     l % 16 in {7, 8}: +-0 and the fp32 subnormals +-1e-40, +-1e-45 in every channel (d)
#   table rows l % 16 ==  1: a duplicated id (a);  2 / 3 / 4: -1 holes leading / in the middle / trailing, 5: the whole row,
#              6: holes at random (b);  9: candidates from the (d) nodes alone, P = 0 in every other such row;
#              11: two +inf nodes, in the middle and in the last slot (e)
# variant "fh":  Q rows l % 16 == 12 hold -inf (c % 8 in {0, 1}) and NaN (c % 8 in {6, 7}) among finite values (f); the
#              empty rows have NaN / +inf / -inf in P (h)
# variant "g1" / "g2" / "g3": Q rows l % 16 == 13 hold -inf and l % 16 == 14 NaN in the channels c % 4 == 0 / c % 4 != 0 /
#              all; table rows l % 16 == 13 take every candidate from those nodes (l % 64 == 13: the -inf nodes alone,
#              29: the NaN nodes alone, else both), with a hole in slot 0 when l % 128 >= 64 (g)
# counted: cnt[i] uniform in 0 .. k; the slots from cnt[i] on keep valid ids, which a form that reads them would gather.
# ---------------------------------------------------------------------------------------------------------------------
VARIANTS = ("finite", "fh", "g1", "g2", "g3")


def make_inputs(sizes, k, H, variant="finite", counted=False, seed=0):
    """dict of CPU tensors: P, Q float32 [N, H]; local int64 [N, k] event-local ids (-1 = empty); nbr int32 [N, k] global
    ids; cnt int32 [N] or None; ptr int64 [B + 1]."""
    assert H % 8 == 0 and variant in VARIANTS
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    N = int(ptr[-1])
    ev = np.repeat(np.arange(len(sizes)), sizes)
    lo, n = ptr[ev], sizes[ev]
    l = np.arange(N) - lo
    c8 = np.arange(H) % 8
    P = rng.standard_normal((N, H)).astype(np.float32)
    Q = rng.standard_normal((N, H)).astype(np.float32)
    quant = np.isin(c8, (2, 3))
    Q[:, quant] = rng.integers(-4, 5, (N, int(quant.sum()))).astype(np.float32) * np.float32(0.25)
    tiny = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-45, -1e-45], np.float32)
    rows = np.isin(l % 16, (7, 8))
    Q[rows] = tiny[rng.integers(0, len(tiny), (int(rows.sum()), H))]
    Q[np.ix_(l % 16 == 10, np.isin(c8, (4, 5)))] = np.inf
    if variant == "fh":
        Q[np.ix_(l % 16 == 12, np.isin(c8, (0, 1)))] = -np.inf
        Q[np.ix_(l % 16 == 12, np.isin(c8, (6, 7)))] = np.nan
    if variant in ("g1", "g2", "g3"):
        c4 = np.arange(H) % 4
        chans = {"g1": c4 == 0, "g2": c4 != 0, "g3": c4 >= 0}[variant]
        Q[np.ix_(l % 16 == 13, chans)] = -np.inf
        Q[np.ix_(l % 16 == 14, chans)] = np.nan

    local = rng.integers(0, np.maximum(n, 1)[:, None], (N, k))
    slot = np.arange(k)[None, :]
    rc = (l % 16)[:, None]

    def pool(first, span):
        """per row and slot, a random event-local id among the nodes l' % 16 in [first, first + span) (needs n > first)"""
        q = rng.integers(0, np.maximum((n - first - 1) // 16 + 1, 1)[:, None], (N, k))
        ids = 16 * q + first + rng.integers(0, span, (N, k))
        return np.where(ids < n[:, None], ids, 16 * q + first)

    if k >= 2:
        local[:, 1] = np.where(l % 16 == 1, local[:, 0], local[:, 1])
    third = max(1, k // 3)
    local = np.where((rc == 2) & (slot < third), -1, local)
    local = np.where((rc == 3) & (slot >= third) & (slot < max(third + 1, 2 * k // 3)) & (k >= 3), -1, local)
    local = np.where((rc == 4) & (slot >= k - third), -1, local)
    local = np.where(rc == 5, -1, local)
    local = np.where((rc == 6) & (rng.random((N, k)) < 0.3), -1, local)
    has = lambda first: (n > first)[:, None]
    local = np.where((rc == 9) & has(7), pool(7, 2), local)
    P[(l % 32 == 9) & (n > 7)] = 0
    local = np.where((rc == 11) & has(10) & ((slot == k - 1) | (slot == k // 2)), pool(10, 1), local)
    if variant in ("g1", "g2", "g3"):
        both, neg, nan = pool(13, 2), pool(13, 1), pool(14, 1)
        l64 = (l % 64)[:, None]
        cand = np.where((l64 == 13), neg, np.where((l64 == 29) & has(14), nan, both))
        local = np.where((rc == 13) & has(13), cand, local)
        local = np.where((rc == 13) & ((l % 128) >= 64)[:, None] & (slot == 0) & (k >= 2), -1, local)
    cnt = rng.integers(0, k + 1, N).astype(np.int32) if counted else None
    if variant == "fh":
        m = np.full(N, k) if cnt is None else cnt
        empty = ~((local >= 0) & (slot < m[:, None])).any(1)
        P[empty] = np.array([np.nan, np.inf, -np.inf, 1.0], np.float32)[np.arange(H) % 4]
    nbr = np.where(local >= 0, local + lo[:, None], -1).astype(np.int32)
    t = torch.from_numpy
    return {"P": t(P), "Q": t(Q), "local": t(local), "nbr": t(nbr), "cnt": None if cnt is None else t(cnt),
            "ptr": t(ptr.astype(np.int64))}
