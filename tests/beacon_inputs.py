"""Position-sensitive ("beacon") inputs for the decode, varlen and dense masked forward tests.

On N(0, 1) inputs every key weighs about 1 / n in its row, so a key lost or counted twice at a seam moves o and lse by about
1 / n, far inside the absolute tolerances.  Here every query row has a designated TARGET key that carries about half of the
row's probability, and every key position a kernel treats specially (a tile, unit, page or split boundary, the ragged end,
the diagonal) is the target of some row, so each such key is visible in o and lse on its own.

Construction, for one K / V head (d_head 128): u[j] is a seeded sign vector of norm 1 per key position and k[j] = a u[j] with
a^2 / sqrt(128) = beta_k = ln(max(n_k, 2)) + 1; v is N(0, 1).  A query row r with target t and diagonal d (the last key it
sees: r + n_k - n_q under the causal mask, n_k - 1 without a mask) is

    q[r] = b_r (u[t] + LEAK w) + NOISE z,    w = u[d + 1] and z ~ N(0, 1), both made orthogonal to u[t],

so its score on the target is beta_r = a b_r / sqrt(128) exactly (before rounding to 16 bit), on the first key it must NOT see
about LEAK beta_r -- that key, if it leaks, dominates the row -- and on every other key N(0, sigma_r^2) with
sigma_r^2 = beta_r^2 (1 + LEAK^2) / 128 + NOISE^2 beta_k / sqrt(128).  beta_r solves beta = ln(max(d, 1)) + sigma^2(beta) / 2,
which makes the target's weight e^beta equal to the expected total weight of the row's d other keys: probability about 1 / 2.
(The per-row beta is the tuning the probability condition needs under a causal mask, where rows of one sequence see from 1 to
n_k keys; the two projections keep the target's score from moving with u[t] . u[d + 1], which would alone be +- 1.5 nats.)
tests/test_beacon_cpu.py asserts the outcome: every target's fp32 probability lies in [0.25, 0.75] wherever the row sees at
least two keys.  A row that sees no key gets plain noise.  u is drawn for positions up to n_k INCLUSIVE (and further, for a
cache with capacity behind its length), so the key behind the last one exists and holds the beacon the last rows' queries point at.

Two-sided windows (forward_kvcache(window_size=(left, right))): row r at position p = n_k - n_q + r sees lo_r .. hi_r with
lo_r = max(0, p - left) (0 for left < 0) and hi_r = min(n_k - 1, p + right) (n_k - 1 for right < 0; causal means right = 0),
and is live iff hi_r >= lo_r.  The query leaks in both directions, q[r] = b_r (u[t] + LEAK w_hi + LEAK w_lo) + NOISE z with
w_hi = u[hi_r + 1] and w_lo = u[lo_r - 1] (absent when lo_r = 0), each made orthogonal to u[t], and beta_r is the smaller root of
beta = L + kappa beta^2 with L = ln(max(hi_r - lo_r, 1)) + NOISE^2 beta_k / (2 sqrt(128)) and kappa = (1 + LEAK^2 n_leaks) / 256,
n_leaks = 2 when lo_r >= 1, else 1: with lo_r = 0 the one-sided formula above.  window_positions lists what the window moves:
every row's two edges, lo_min = max(0, n_k - n_q - left) and the key above it, the unit, tile, page and split boundaries counted
from lo_min's tile; assign_window_targets gives a position only to a row whose window holds it.

Nothing here reads the code under test: the positions come from the sizes the kernels are documented to use (64-key tiles,
32-key units, 128-row blocks, pages, the split rule 64 floor(n_tiles s / num_splits), under a window
64 (tl + floor((n_tiles - tl) s / num_splits)) with tl = lo_min / 64).  Plain helper module: no tests, no
fixtures; runs on the CPU or the GPU with a seed.
"""
import math

import torch

D = 128
LEAK = 1.5
NOISE = 0.25
O_TOL = {torch.bfloat16: 2.0 ** -6, torch.float16: 2.0 ** -9}
LSE_TOL = 1e-3
P_LO, P_HI = 0.25, 0.75
NEG_INF = float("-inf")

# the launches of tests/test_beacon_gpu.py; tests/test_beacon_cpu.py holds the same inputs to its mutants
DECODE_LENGTHS = [1, 2, 33, 64, 65, 130, 1000, 4097, 33000]
DECODE_CACHE_LEN = 33024                         # a multiple of both page sizes, and one row at least behind the longest entry
DECODE_SHAPES = [(8, 2, 4), (8, 1, 8), (8, 8, 16)]   # (H, Hkv, Sq)
DECODE_SPLITS = [1, 3, 8, 0]                     # 0: the rule's (fa_decode_num_splits)
VARLEN_HEADS = [(4, 4), (8, 2), (4, 1)]
VARLEN_FAMILIES = {   # name -> ((len_q, len_k) pairs, loose (max_seqlen_q, max_seqlen_k) or None)
    "pairs": ([(37, 1000), (300, 4096), (128, 192), (129, 257), (1, 777), (65, 63), (512, 4096)], None),
    "equal": ([(n, n) for n in (63, 64, 65, 257, 1000, 2500)], None),
    "loose": ([(37, 1000), (128, 192), (65, 63)], (1024, 2048)),
}
DENSE_CASES = [(1000, True), (1024, True), (4096, False)]   # (seq_len, causal): forward_ex on the default configuration
# the windowed decode launches of tests/test_window_beacon_gpu.py (the shapes are DECODE_SHAPES): one batch of all lengths.  136 and
# 143 put lo_min on a tile boundary and on a tile's middle (lo_min % 64 = 0 and 32) at every seqlen_q of DECODE_SHAPES: 136 - 4 - 100
# = 32, 136 - 8 - 0 = 128 and 136 - 8 - 64 = 64, 143 - 16 - 63 = 64 and 143 - 16 - 31 = 96, beside 1000 - 4 - 100 = 896 and 1000 - 8 - 0 = 992
WINDOW_LENGTHS = [1, 2, 33, 64, 65, 130, 136, 143, 1000, 4097]
WINDOW_CACHE_LEN = 4352                          # a multiple of both page sizes, and rows behind the longest entry
WINDOWS = [(0, -1, True), (1, -1, True), (31, -1, True), (63, 0, False), (64, -1, True), (100, -1, True), (200, 3, False),
           (3, 2, False), (-1, 3, False), (1000, -1, True), (5000, -1, True)]   # (left, right, causal); causal: right = 0
WINDOW_SPLITS = [1, 3, 16, 0]                    # 0: the rule's (fa_decode_window_num_splits)


# ---- the inputs -------------------------------------------------------------------------------------------------------------

def _beta_k(n_k):
    return math.log(max(n_k, 2)) + 1.0


def beacon_kv(n_k, dtype, n_alloc=None, seed=0, device="cpu"):
    """-> k, v of shape (n_alloc, 128), n_alloc >= n_k + 1 (default n_k + 1): every row a beacon, the rows behind n_k too."""
    n_alloc = max(n_alloc or 0, n_k + 1)
    gen = torch.Generator(device=device).manual_seed(seed)
    sign = torch.randint(0, 2, (n_alloc, D), generator=gen, device=device).float() * 2 - 1
    a = math.sqrt(_beta_k(n_k) * math.sqrt(D))
    v = torch.randn((n_alloc, D), generator=gen, device=device)
    return (sign * (a / math.sqrt(D))).to(dtype), v.to(dtype)


def beacon_q(k, n_k, targets, diag, dtype, seed=0, lo=None):
    """Query rows for one K / V head's beacons: k (>= n_k + 1, 128) from beacon_kv; targets and diag int64 (n_q,) on k's
    device, targets[r] in [0, diag[r]] or -1, diag[r] in [-inf, n_k - 1] (< 0: the row sees no key).  lo: int64 (n_q,), the
    first key each row sees (a two-sided window: targets[r] in [lo[r], diag[r]], and a second leak towards key lo[r] - 1)."""
    device = k.device
    gen = torch.Generator(device=device).manual_seed(seed)
    n_q = targets.numel()
    z = torch.randn((n_q, D), generator=gen, device=device)
    live = (diag >= 0) & (targets >= 0)
    assert bool((targets[live] <= diag[live]).all()) and bool((diag < n_k).all())
    u = torch.sign(k.float())                                  # (entries +- a / sqrt(128): the signs are u sqrt(128))
    ut = u[targets.clamp_min(0)] / math.sqrt(D)
    w = u[(diag + 1).clamp_min(0)] / math.sqrt(D)
    w = w - (w * ut).sum(-1, keepdim=True) * ut
    z_perp = z - (z * ut).sum(-1, keepdim=True) * ut
    beta_k = _beta_k(n_k)
    if lo is None:
        big_l = torch.log(diag.clamp_min(1).double()) + 0.5 * NOISE ** 2 * beta_k / math.sqrt(D)
        kappa = (1.0 + LEAK ** 2) / (2.0 * D)                  # beta = L + kappa beta^2, the smaller root
    else:
        assert bool((targets[live] >= lo[live]).all()) and bool((lo >= 0).all())
        below = (lo >= 1)[:, None]
        w_lo = u[(lo - 1).clamp_min(0)] / math.sqrt(D)
        w = w + torch.where(below, w_lo - (w_lo * ut).sum(-1, keepdim=True) * ut, torch.zeros_like(w_lo))
        big_l = torch.log((diag - lo).clamp_min(1).double()) + 0.5 * NOISE ** 2 * beta_k / math.sqrt(D)
        kappa = (1.0 + LEAK ** 2 * (1 + below[:, 0].double())) / (2.0 * D)
    beta = (1.0 - torch.sqrt(1.0 - 4.0 * kappa * big_l)) / (2.0 * kappa)
    b = (beta * math.sqrt(D) / math.sqrt(beta_k * math.sqrt(D))).float()[:, None]
    q = torch.where(live[:, None], b * (ut + LEAK * w) + NOISE * z_perp, NOISE * z)
    return q.to(dtype)


def beacon_qkv(n_q, n_k, targets, dtype, causal=False, n_alloc=None, seed=0, device="cpu"):
    """One sequence (or one batch entry) for one K / V head: -> q (n_q, 128), k, v (max(n_alloc, n_k + 1), 128).  targets: n_q
    key positions (a list or tensor; -1: no target).  causal: row r's diagonal is r + n_k - n_q."""
    k, v = beacon_kv(n_k, dtype, n_alloc, seed, device)
    targets = torch.as_tensor(targets, dtype=torch.int64, device=device)
    return beacon_q(k, n_k, targets, diagonals(n_q, n_k, causal, device), dtype, seed + 1), k, v


def diagonals(n_q, n_k, causal, device="cpu"):
    """The last key each of n_q rows sees (negative: none)."""
    if causal:
        return torch.arange(n_q, device=device) + (n_k - n_q)
    return torch.full((n_q,), n_k - 1, dtype=torch.int64, device=device)


def window_sides(left, right, causal):
    """(left, right, causal) as forward_kvcache takes them -> the (left, right) the mask uses: causal means right = 0"""
    assert not causal or right in (-1, 0)
    return left, (0 if causal else right)


def window_bounds(n_q, n_k, left, right, device="cpu"):
    """The first and the last key each of n_q rows sees under window (left, right), -1 = unbounded -> lo, hi int64 (n_q,);
    lo >= 0 always, and a row is live iff hi >= lo (a dead row has hi < 0: its position lies more than `right` below key 0)."""
    p = torch.arange(n_q, device=device) + (n_k - n_q)
    lo = torch.zeros_like(p) if left < 0 else (p - left).clamp_min(0)
    hi = torch.full_like(p, n_k - 1) if right < 0 else (p + right).clamp_max(n_k - 1)
    return lo, hi


def window_lo_min(n, seqlen_q, left):
    """the lowest key any row of the entry sees"""
    return 0 if left < 0 else max(0, n - seqlen_q - left)


# ---- the positions that matter ------------------------------------------------------------------------------------------------

def _unique_inside(positions, n):
    out, seen = [], set()
    for p in positions:
        if 0 <= p < n and p not in seen:
            seen.add(p)
            out.append(p)
    return out


def _both_sides(boundaries):
    return [p for b in boundaries for p in (b - 1, b)]


def decode_positions(n, seqlen_q, num_splits, page_sizes=(64, 256)):
    """forward_kvcache, one entry of length n: the ends, both sides of the 32-key unit and 64-key tile boundaries inside the
    first two tiles (32, 64, 96 and the second tile's end, 128), of the page boundaries that end the first two pages of each
    page size (P and 2 P), of every split boundary 64 floor(n_tiles s / num_splits), the last key of a ragged unit (n - 1),
    and every row's diagonal key."""
    n_tiles = (n + 63) // 64
    pos = [0, n - 2, n - 1] + _both_sides([32, 64, 96, 128]) + _both_sides(m * p for p in page_sizes for m in (1, 2))
    pos += _both_sides(64 * (n_tiles * s // num_splits) for s in range(1, num_splits))
    pos += [n - seqlen_q + qi for qi in range(seqlen_q)]
    return _unique_inside(pos, n)


def varlen_positions(n_q, n_k):
    """forward_varlen, one sequence: the ends (n_k - 1 is the last key of a ragged range), both sides of the 64-key tile
    boundaries inside the first two and the last two tiles, and both sides of both ends of the last tile each 128-row block
    visits under the shifted diagonal."""
    n_tiles = (n_k + 63) // 64
    pos = [0, n_k - 2, n_k - 1] + _both_sides(64 * t for t in (1, 2, n_tiles - 2, n_tiles - 1))
    for qb in range((n_q + 127) // 128):
        last_row = min(n_q, 128 * (qb + 1)) - 1
        tile = min(max((last_row + n_k - n_q) // 64, 0), n_tiles - 1)
        pos += _both_sides([64 * tile, 64 * tile + 64])
    return _unique_inside(pos, n_k)


def dense_positions(n, diagonals=True):
    """forward_ex: the ends, both sides of every 64-key tile boundary inside the first two and the last two tiles, and (unless
    diagonals=False) every row's diagonal key: all of 0 .. n - 1."""
    n_tiles = (n + 63) // 64
    pos = [0, n - 2, n - 1] + _both_sides(64 * t for t in (1, 2, n_tiles - 2, n_tiles - 1))
    return _unique_inside(pos + (list(range(n)) if diagonals else []), n)


def window_positions(n, seqlen_q, left, right, num_splits, page_sizes=(64, 256)):
    """forward_kvcache with window_size, one entry of length n: every live row's first and last key, lo_min and the key above
    it, n - 2 and n - 1, both sides of the 32-key unit and 64-key tile boundaries in the tile that holds lo_min and in the tile
    after it, of the first page boundary above lo_min for each page size, and of every windowed split boundary
    64 (tl + floor((n_tiles - tl) s / num_splits)), tl = lo_min / 64; all inside [lo_min, n)."""
    lo, hi = window_bounds(seqlen_q, n, left, right)
    live = hi >= lo
    lo_min = window_lo_min(n, seqlen_q, left)
    n_tiles, tl = (n + 63) // 64, lo_min // 64
    pos = [p for pair in zip(lo[live].tolist(), hi[live].tolist()) for p in pair] + [lo_min, lo_min + 1, n - 2, n - 1]
    pos += _both_sides(64 * tl + off for off in (32, 64, 96, 128))
    pos += _both_sides(p * (lo_min // p + 1) for p in page_sizes)
    pos += _both_sides(64 * (tl + (n_tiles - tl) * s // num_splits) for s in range(1, num_splits))
    return [p for p in _unique_inside(pos, n) if p >= lo_min]


def assign_targets(n_q, n_heads, n_k, listed, causal, phase=0):
    """Spread `listed` over the n_q x n_heads rows of one sequence -> (targets int64 (n_heads, n_q), -1 on rows that see no key;
    n_phases).  Without a mask the first row of head 0 targets the last key (every row's diagonal) and the other rows take the
    other listed positions in turn.  Under the causal mask head 0 of every row targets
    the row's diagonal, and the other heads take in turn the listed positions that are no live row's diagonal (those lie below
    every live diagonal, so every live row sees them); where none is left they target the diagonal too.  So in every phase
    some row targets its own diagonal.  A list longer than the
    rows that can hold it is cut into n_phases chunks: the caller repeats the sequence (or the launch), one phase each."""
    diag = diagonals(n_q, n_k, causal)
    live = diag >= 0
    n_live = int(live.sum())
    targets = torch.where(live, diag, torch.full_like(diag, -1)).repeat(n_heads, 1)
    if n_live == 0 or n_k == 0:
        return targets, 1
    if causal:
        diags = set(diag[live].tolist())
        rest = [p for p in listed if p not in diags]
        rows = [(h, r) for r in range(n_q) if live[r] for h in range(1, n_heads)]
    else:
        rest = [p for p in listed if p != n_k - 1]
        rows = [(h, r) for r in range(n_q) for h in range(n_heads)][1:]
    if not rest or not rows:
        return targets, 1
    n_phases = (len(rest) + len(rows) - 1) // len(rows)
    chunk = rest[phase * len(rows):(phase + 1) * len(rows)] or rest[:len(rows)]
    hs, rs = (torch.tensor(x) for x in zip(*rows))
    targets[hs, rs] = torch.tensor([chunk[i % len(chunk)] for i in range(len(rows))])
    return targets, n_phases


def build_sequence(n_q, n_k, n_heads, n_kv_heads, listed, dtype, causal, phase=0, n_alloc=None, seed=0, device="cpu", kv=None):
    """One sequence with all its heads -> dict: q (n_q, n_heads, 128), k, v (n_alloc, n_kv_heads, 128) (row n_k and beyond hold
    beacons: slice [:n_k] for a packed layout), targets (n_heads, n_q) on the CPU, diag (n_q,), n_phases.  kv: a (k, v) pair of
    an earlier call for the same keys, reused (only q depends on the targets)."""
    targets, n_phases = assign_targets(n_q, n_heads, n_k, listed, causal, phase)
    group = n_heads // n_kv_heads
    if kv is None:
        pairs = [beacon_kv(n_k, dtype, n_alloc, seed * 1000 + 2 * h, device) for h in range(n_kv_heads)]
        kv = torch.stack([p[0] for p in pairs], dim=1), torch.stack([p[1] for p in pairs], dim=1)
    k, v = kv
    diag = diagonals(n_q, n_k, causal, device)
    q = torch.stack([beacon_q(k[:, h // group], n_k, targets[h].to(device), diag, dtype, seed * 1000 + 2 * h + 1 + 7919 * phase)
                     for h in range(n_heads)], dim=1) if n_q else torch.zeros((0, n_heads, D), dtype=dtype, device=device)
    return dict(q=q, k=k, v=v, targets=targets, diag=diag.cpu(), n_phases=n_phases, n_q=n_q, n_k=n_k, listed=list(listed))


def assign_window_targets(n_heads, lo, hi, listed, phase=0):
    """Spread `listed` over the rows of one windowed entry -> (targets int64 (n_heads, n_q), -1 on rows that see no key;
    n_phases).  lo, hi: window_bounds.  Head 0 of every live row targets the row's own last key and head 1 its own first key, in
    every phase; the other heads take the listed positions that are no live row's edge, each given only to a row whose
    [lo, hi] holds it -- the positions fewest rows can hold first, each to the holding row with most heads left -- and a
    position that finds no head waits for the next phase.  A head left over targets an edge of its row (even heads the last
    key, odd heads the first).  An entry with fewer phases than its launch repeats them in turn."""
    assert n_heads >= 2
    lo, hi = lo.tolist(), hi.tolist()
    n_q = len(lo)
    live = [r for r in range(n_q) if hi[r] >= lo[r]]
    targets = torch.full((n_heads, n_q), -1, dtype=torch.int64)
    for r in live:
        targets[0::2, r], targets[1::2, r] = hi[r], lo[r]
    edges = {e for r in live for e in (lo[r], hi[r])}
    holders = {p: [r for r in live if lo[r] <= p <= hi[r]] for p in listed if p not in edges}
    rest = sorted(holders, key=lambda p: len(holders[p]))          # (stable: the list's order among equals)
    phases = []
    while rest:
        free = {r: list(range(2, n_heads)) for r in live}
        placed, waiting = {}, []
        for p in rest:
            rows = [r for r in holders[p] if free[r]]
            if rows:
                r = max(rows, key=lambda r: len(free[r]))
                placed[free[r].pop(0), r] = p
            else:
                waiting.append(p)
        assert placed, ("no live row sees", rest)
        phases.append(placed)
        rest = waiting
    if phases:
        for (h, r), p in phases[phase % len(phases)].items():
            targets[h, r] = p
    return targets, max(len(phases), 1)


def build_window_sequence(n_q, n_k, n_heads, n_kv_heads, listed, dtype, left, right, phase=0, n_alloc=None, seed=0, device="cpu",
                          kv=None):
    """build_sequence under window (left, right) (causal: pass right = 0) -> the same dict with lo (n_q,) beside diag, which
    holds hi; eager, references and target_probabilities read both."""
    lo, hi = window_bounds(n_q, n_k, left, right)
    targets, n_phases = assign_window_targets(n_heads, lo, hi, listed, phase)
    group = n_heads // n_kv_heads
    if kv is None:
        pairs = [beacon_kv(n_k, dtype, n_alloc, seed * 1000 + 2 * h, device) for h in range(n_kv_heads)]
        kv = torch.stack([p[0] for p in pairs], dim=1), torch.stack([p[1] for p in pairs], dim=1)
    k, v = kv
    q = torch.stack([beacon_q(k[:, h // group], n_k, targets[h].to(device), hi.to(device), dtype, seed * 1000 + 2 * h + 1 + 7919 * phase,
                              lo=lo.to(device)) for h in range(n_heads)], dim=1)
    return dict(q=q, k=k, v=v, targets=targets, diag=hi, lo=lo, n_phases=n_phases, n_q=n_q, n_k=n_k, listed=list(listed))


def cpu_cap(n, limit=1100):
    """A length the CPU tests can afford: lengths beyond `limit` keep their remainder by 64 on top of 1024 keys."""
    return n if n <= limit else 1024 + n % 64


def varlen_family(name, n_heads, n_kv_heads, dtype, causal, device="cpu", seed=0, cap=None):
    """The sequences of one packed launch -> (list of build_sequence dicts, (max_seqlen_q, max_seqlen_k)).  A pair whose rows
    cannot hold its list -- (1, 777) -- is repeated, one copy per phase, so that every listed position has its row.
    cap: a function applied to every length (the CPU tests')."""
    pairs, loose = VARLEN_FAMILIES[name]
    if cap:
        pairs = [(cap(a), cap(b)) for a, b in pairs]
    seqs = []
    for i, (n_q, n_k) in enumerate(pairs):
        listed, phase, n_phases = varlen_positions(n_q, n_k), 0, 1
        while phase < n_phases:
            seqs.append(build_sequence(n_q, n_k, n_heads, n_kv_heads, listed, dtype, causal, phase, seed=seed + 10 * i + phase, device=device))
            n_phases, phase = seqs[-1]["n_phases"], phase + 1
    return seqs, loose or (max(s["n_q"] for s in seqs), max(s["n_k"] for s in seqs))


def pack(seqs):
    """-> packed q (total_q, H, 128), k, v (total_k, Hkv, 128) and the two offset lists"""
    cuq, cuk = [0], [0]
    for s in seqs:
        cuq.append(cuq[-1] + s["n_q"])
        cuk.append(cuk[-1] + s["n_k"])
    q = torch.cat([s["q"] for s in seqs])
    k, v = (torch.cat([s[name][:s["n_k"]] for s in seqs]) for name in ("k", "v"))
    return q, k, v, cuq, cuk


# ---- the reference and the comparison -----------------------------------------------------------------------------------------

def eager(q, k, v, diag, dtype, delta=0, want_p=False, lo=None, delta_lo=0):
    """Eager attention of one sequence in `dtype` arithmetic: q (n_q, H, 128), k / v (n_keys, Hkv, 128), row r sees keys
    j <= diag[r] + delta (delta != 0: a deliberately wrong mask) and, with lo (n_q,), j >= lo[r] + delta_lo
    -> o (n_q, H, 128) in dtype, lse fp32 (H, n_q)[, p].  A row that sees no key: o = 0, lse = -inf."""
    group = q.shape[1] // k.shape[1]
    kk, vv = k.to(dtype).repeat_interleave(group, dim=1), v.to(dtype).repeat_interleave(group, dim=1)
    s = torch.einsum("qhd,khd->hqk", q.to(dtype), kk) * (1.0 / math.sqrt(D))
    hidden = torch.arange(k.shape[0], device=q.device)[None, :] > (diag.to(q.device)[:, None] + delta)
    if lo is not None:
        hidden = hidden | (torch.arange(k.shape[0], device=q.device)[None, :] < (lo.to(q.device)[:, None] + delta_lo))
    s = s.masked_fill(hidden[None], NEG_INF)
    dead = hidden.all(dim=1)[None, :, None]
    lse = torch.logsumexp(s.float().masked_fill(dead, 0.0), dim=-1).masked_fill(dead[..., 0], NEG_INF)
    p = torch.softmax(s.masked_fill(dead, 0.0), dim=-1).masked_fill(dead, 0.0)
    o = torch.einsum("hqk,khd->qhd", p, vv)
    return (o, lse, p) if want_p else (o, lse)


def references(seq):
    """-> (o32, lse32, o16) of a build_sequence dict, on its device; fp32 eager and the same eager in the 16-bit type"""
    n_k, dtype = seq["n_k"], seq["q"].dtype
    if seq["n_q"] == 0 or n_k == 0:
        o = torch.zeros(seq["q"].shape, dtype=torch.float32, device=seq["q"].device)
        return o, torch.full((seq["q"].shape[1], seq["n_q"]), NEG_INF, device=o.device), o.to(dtype)
    o32, lse32 = eager(seq["q"], seq["k"][:n_k], seq["v"][:n_k], seq["diag"], torch.float32, lo=seq.get("lo"))
    o16, _ = eager(seq["q"], seq["k"][:n_k], seq["v"][:n_k], seq["diag"], dtype, lo=seq.get("lo"))
    return o32, lse32, o16


def target_probabilities(seq, lse32):
    """fp32 probability of every row's target, exp(q . k[target] / sqrt(128) - lse32) -> (H, n_q) and the mask of the rows
    the [P_LO, P_HI] condition holds for: live rows that see at least two keys (diag + 1, under a window diag + 1 - lo)."""
    q, k, targets = seq["q"].float(), seq["k"].float(), seq["targets"].to(seq["q"].device)
    group = q.shape[1] // k.shape[1]
    kt = torch.stack([k[targets[h].clamp_min(0), h // group] for h in range(q.shape[1])])          # (H, n_q, 128)
    p = torch.exp((q.transpose(0, 1) * kt).sum(-1) * (1.0 / math.sqrt(D)) - lse32)
    sees = seq["diag"] + 1 if seq.get("lo") is None else seq["diag"] + 1 - seq["lo"]
    several = ((targets >= 0) & (sees.to(p.device) >= 2)[None, :])
    return p, several


def compare(o, lse, o32, lse32, o16, dtype):
    """The decode tests' rule for ONE sequence or batch entry: max|O - O32| <= max(O_TOL, 2 max|O_eager16 - O32|), lse within
    1e-3 on live rows, -inf rows exact (lse may be None).  -> dict(ok, err, bound, lse_err, inf_ok)"""
    o = o.float()
    ref_err = (o16.float() - o32).abs().max().item() if o32.numel() else 0.0
    bound = max(O_TOL[dtype], 2.0 * ref_err)
    err = (o - o32).abs().max().item() if o32.numel() else 0.0
    finite = bool(torch.isfinite(o).all())
    inf_ok, lse_err = True, 0.0
    if lse is not None:
        inf = lse32 == NEG_INF
        inf_ok = bool(torch.equal(lse == NEG_INF, inf)) and not bool(torch.isnan(lse).any())
        if inf_ok and bool((~inf).any()):
            lse_err = (lse[~inf] - lse32[~inf]).abs().max().item()
    ok = finite and err <= bound and inf_ok and lse_err <= LSE_TOL
    return dict(ok=ok, err=err, bound=bound, lse_err=lse_err, inf_ok=inf_ok)
