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

The backward's inputs (the section "the backward's cells" at the end; tests/test_backward_beacon_gpu.py): the backward works in
(row range x key range) pairs, so assign_cell_targets puts a target into every live (32-row band, 32-key cell) pair under the
shifted diagonal (backward_cells), neighbouring rows' target scores lie BETA_STEP above and below the balanced beta_r, so that a
row's lse differs from its neighbour's, and beacon_dout adds to seeded noise a component along v[t_r] - o32_r, so that
|dS32[r, t_r]| >= DS_FLOOR on every targeted row (target_ds).  reference_backward is the explicit fp32 backward with hooks for
the CPU proof's mutants, and grad_rule the gradient rule of tests/test_backward_gpu.py for one sequence.

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


def beacon_q(k, n_k, targets, diag, dtype, seed=0, lo=None, beta_shift=None):
    """Query rows for one K / V head's beacons: k (>= n_k + 1, 128) from beacon_kv; targets and diag int64 (n_q,) on k's
    device, targets[r] in [0, diag[r]] or -1, diag[r] in [-inf, n_k - 1] (< 0: the row sees no key).  lo: int64 (n_q,), the
    first key each row sees (a two-sided window: targets[r] in [lo[r], diag[r]], and a second leak towards key lo[r] - 1).
    beta_shift: (n_q,), added to the balanced beta_r (the backward's inputs: neighbouring rows with different lse)."""
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
    if beta_shift is not None:
        beta = beta + beta_shift.to(device).double()
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


# ---- the backward's cells ("Backward cells") ---------------------------------------------------------------------
#
# The backward kernels work in (row range x key range) pairs: a dK / dV workgroup owns a 128-key block, 32 keys per wave, and
# sweeps 64-row Q / dO tiles in two 32-row halves; a dQ workgroup owns 128 rows, 32 per wave, and sweeps 64-key tiles in 32-key
# halves.  A 32 x 32 product left out of one accumulator, a diagonal flag wrong for one tile, a delta or lse row
# read from its neighbour touch only the rows and keys of that cell, so the targets below cover every live (32-row band,
# 32-key cell) pair, and dout is constructed so that every targeted row carries |dS| >= DS_FLOOR on its target.

CELL = 32                     # rows per wave (dQ) and keys per wave (dK / dV): the accumulator a product can be missing from
BWD_TILE = 64                 # rows per Q / dO tile of a dK / dV sweep, keys per tile of a dQ sweep
BWD_BLOCK = 128               # keys per dK / dV workgroup, rows per dQ workgroup
BETA_STEP = 0.4               # even rows' target scores lie BETA_STEP above the balanced beta_r, odd rows' below: lse differs by about it
DOUT_ALONG = 0.25             # dout's component along v[t_r] - o32_r, in units of the noise's standard deviation
DS_FLOOR = 0.375              # |dS32[r, t_r]| of every targeted row that sees two keys or more
BACKWARD_HEADS = [(4, 4), (8, 2)]
BACKWARD_VARLEN_PAIRS = [(512, 512), (300, 300), (129, 300), (64, 1)]


def backward_cells(n_q, n_k, causal):
    """The live 32-row x 32-key cells of one sequence under the shifted diagonal -> [(row band i, key cell j, on_diagonal)]:
    band i holds rows 32 i .. 32 i + 31 (clipped to n_q), cell j keys 32 j .. 32 j + 31 (clipped to n_k); a cell is live when
    some row of the band sees some key of the cell, and on a diagonal when it holds some live row's last key (without a mask
    that is key n_k - 1 for every row: the last key cell of every band)."""
    diag = diagonals(n_q, n_k, causal).tolist()
    cells = []
    for i in range((n_q + CELL - 1) // CELL):
        last = [d for d in diag[CELL * i:CELL * (i + 1)] if d >= 0]
        if last and n_k:
            on = {d // CELL for d in last}
            cells += [(i, j, j in on) for j in range(max(last) // CELL + 1)]
    return cells


def assign_cell_targets(n_q, n_heads, n_k, causal, phase=0):
    """Targets that cover every live cell -> (targets int64 (n_heads, n_q), -1 on rows that see no key; n_phases).  Under the
    causal mask head 0 of every live row targets its own diagonal, so every diagonal cell is hit and every key that is some
    row's diagonal is a target; the (row, head) slots of the other heads are dealt in turn over the key cells of their row band
    (a slot dealt a cell its row does not see whole -- the band's upper diagonal cell -- takes what it sees of it, or keeps the
    diagonal).  Without a mask every row's last key is n_k - 1: one slot per band takes it and all heads are dealt.  Inside its
    cell a slot takes a key still NEEDED -- the keys of the diagonal cells that are no row's diagonal, and keys 0, n_k - 2,
    n_k - 1 -- if it sees one, else a key that moves with the row and the head.  A band with fewer slots than key cells (a ragged
    last band) needs several phases: the caller repeats the sequence, one phase each, as for assign_targets.  A causal sequence
    whose diagonals reach no key of some 128-key block gets one phase more, in which head 1 holds the diagonal and head 0 is dealt,
    so that every head has targets in every block it sees (a head lost from that block's dK / dV sum shows)."""
    diag = diagonals(n_q, n_k, causal).tolist()
    base = [[d if d >= 0 else -1 for d in diag] for _ in range(n_heads)]
    cells = backward_cells(n_q, n_k, causal)
    if not cells:
        return torch.tensor(base, dtype=torch.int64).reshape(n_heads, n_q), 1
    given = {d for d in diag if d >= 0} if causal else set()
    needed = _unique_inside([0, n_k - 2, n_k - 1] + [p for _, j, on in cells if on for p in range(CELL * j, CELL * (j + 1))], n_k)
    needed = [p for p in needed if p not in given]
    bands = {}
    for i, j, _ in cells:
        bands.setdefault(i, []).append(j)

    def head_blocks(t, h):
        return {x // BWD_BLOCK for x in t[h] if x >= 0}

    seen_blocks = {j * CELL // BWD_BLOCK for _, j, _ in cells}
    phases, p, n_more, extra = [], 0, 1, False
    while True:
        # the diagonal's head: head 0; in the one extra phase a causal sequence gets when head 0's diagonals reach no key of some
        # 128-key block (n_k - n_q >= 128), head 1, so that head 0 is dealt there
        own = (1 if extra else 0) if causal else None
        dealt = [h for h in range(n_heads) if h != own]
        t = [row[:] for row in base]
        for i, js in bands.items():
            rows = [r for r in range(CELL * i, min(CELL * (i + 1), n_q)) if diag[r] >= 0]
            n_slots = len(rows) * len(dealt)
            if not n_slots:
                continue
            n_more = max(n_more, (len(js) + n_slots - 1) // n_slots)
            band_needed = [] if causal else [n_k - 1]
            for s in range(n_slots):          # row after row, the heads' order turning with the row and the band
                r = rows[s // len(dealt)]
                h = dealt[(s + s // len(dealt) + i) % len(dealt)]
                j = js[(s + p * n_slots) % len(js)]
                lo, hi = CELL * j, min(CELL * j + CELL - 1, diag[r])
                if hi < lo:
                    continue
                pick = None
                for pool in (band_needed, needed):
                    pick = next((x for x in pool if lo <= x <= hi), None)
                    if pick is not None:
                        pool.remove(pick)
                        break
                t[h][r] = pick if pick is not None else lo + (r + 5 * h) % (hi - lo + 1)
        phases.append(t)
        p += 1
        if extra or p >= 64:
            break
        if p >= n_more and not needed:
            if causal and n_heads > 1 and not seen_blocks <= set().union(*(head_blocks(ph, 0) for ph in phases)):
                extra = True
                continue
            break
    return torch.tensor(phases[phase % len(phases)], dtype=torch.int64).reshape(n_heads, n_q), len(phases)


def build_cell_sequence(n_q, n_k, n_heads, n_kv_heads, dtype, causal, phase=0, seed=0, device="cpu", kv=None):
    """build_sequence with the cell-covering targets -> the same dict, with `cells` (backward_cells) in place of `listed`"""
    targets, n_phases = assign_cell_targets(n_q, n_heads, n_k, causal, phase)
    group = n_heads // n_kv_heads
    if kv is None:
        pairs = [beacon_kv(n_k, dtype, None, seed * 1000 + 2 * h, device) for h in range(n_kv_heads)]
        kv = torch.stack([p[0] for p in pairs], dim=1), torch.stack([p[1] for p in pairs], dim=1)
    k, v = kv
    diag = diagonals(n_q, n_k, causal, device)
    step = BETA_STEP * (1.0 - 2.0 * (torch.arange(n_q, device=device) % 2))
    q = torch.stack([beacon_q(k[:, h // group], n_k, targets[h].to(device), diag, dtype, seed * 1000 + 2 * h + 1 + 7919 * phase,
                              beta_shift=step) for h in range(n_heads)], dim=1) if n_q else torch.zeros((0, n_heads, D), dtype=dtype, device=device)
    return dict(q=q, k=k, v=v, targets=targets, diag=diag.cpu(), n_phases=n_phases, n_q=n_q, n_k=n_k, listed=[], causal=causal,
                cells=backward_cells(n_q, n_k, causal))


def cell_coverage(seqs):
    """The phases of ONE (n_q, n_k, causal) -> (live cells no (row, head) target lies in, needed keys no row targets,
    (head, 128-key block) pairs in which the head has no target although some row of the sequence sees the block)"""
    first = seqs[0]
    n_k, heads = first["n_k"], first["q"].shape[1]
    hit, keys, blocks = set(), set(), set()
    for s in seqs:
        for h in range(heads):
            for r, t in enumerate(s["targets"][h].tolist()):
                if t >= 0:
                    hit.add((r // CELL, t // CELL))
                    keys.add(t)
                    blocks.add((h, t // BWD_BLOCK))
    cells = first["cells"]
    needed = _unique_inside([0, n_k - 2, n_k - 1] + [p for _, j, on in cells if on for p in range(CELL * j, CELL * (j + 1))], n_k)
    seen_blocks = {j * CELL // BWD_BLOCK for _, j, _ in cells}
    return ([c[:2] for c in cells if c[:2] not in hit], [p for p in needed if p not in keys],
            [(h, b) for h in range(heads) for b in sorted(seen_blocks) if (h, b) not in blocks])


def _target_values(seq):
    """v[t_r] of every (row, head) -> (n_q, H, 128) fp32 (rows without a target: key 0's, unused)"""
    v, targets = seq["v"].float(), seq["targets"].to(seq["q"].device)
    group = seq["q"].shape[1] // v.shape[1]
    return torch.stack([v[targets[h].clamp_min(0), h // group] for h in range(targets.shape[0])], dim=1)


def beacon_dout(seq, o32, seed=0, along=None):
    """dout (n_q, H, 128) in the sequence's dtype: seeded N(0, 1) noise z plus the component `along` (default DOUT_ALONG) along
    e_r = (v[t_r] - o32_r) / |v[t_r] - o32_r|, with the sign of z . e_r, so that dP - delta = dout_r . (v[t_r] - o32_r) on the
    target has size |v[t_r] - o32_r| (|z . e_r| + along) and is never small by chance.  A row whose o32 IS its target's value
    (it sees one key) and a row without a target get the noise alone.  o32: the fp32 reference forward's (references)."""
    along = DOUT_ALONG if along is None else along
    device = seq["q"].device
    z = torch.randn(seq["q"].shape, generator=torch.Generator(device=device).manual_seed(seed), device=device)
    e = _target_values(seq) - o32
    w = e.norm(dim=-1, keepdim=True)
    e = torch.where(w > 1e-6, e / w.clamp_min(1e-6), torch.zeros_like(e))
    e = e * (seq["targets"].to(device).t() >= 0)[..., None]
    ze = (z * e).sum(-1, keepdim=True)
    return (z + torch.where(ze >= 0, 1.0, -1.0) * along * e).to(seq["q"].dtype)


def target_ds(seq, dout, o32, lse32):
    """fp32 dS of every row's target, P[r, t_r] (dout_r . (v[t_r] - o32_r)) -> (H, n_q), and target_probabilities' mask of the
    rows the DS_FLOOR condition holds for (live rows that see two keys or more)"""
    p, several = target_probabilities(seq, lse32)
    return p * ((_target_values(seq) - o32) * dout.float()).sum(-1).t(), several


def reference_backward(seq, dout, hook=None, want_parts=False):
    """The explicit fp32 backward of one sequence: P = exp(S - lse32) on the keys the row sees, delta = sum dO o O, dP = dO V^T,
    dS = P o (dP - delta), dV = P^T dO, dK = dS^T Q / sqrt(d), dQ = dS K / sqrt(d), dK and dV summed over the group
    -> dq (n_q, H, 128), dk, dv (n_k, Hkv, 128)[, parts].  The dK / dV pass and the dQ pass each form P and dS of their own, as
    the kernels do, from a state dict the hook may change first: hook(name, state), name "dkdv" or "dq", state = lse (H, n_q),
    delta (H, n_q), visible (H, n_q, n_k) bool, weight (H, n_q, n_k) -- multiplies P and dS: 0 drops a product, 2 counts it
    twice -- and, for "dkdv", head_weight (H, n_k): the weight of a query head's dK / dV rows in the group's sum.  A key made
    visible takes its probability from the state's lse, as a kernel would."""
    n_q, n_k = seq["n_q"], seq["n_k"]
    q, k, v, do = seq["q"].float(), seq["k"][:n_k].float(), seq["v"][:n_k].float(), dout.float()
    heads, kv_heads = q.shape[1], k.shape[1]
    group = heads // kv_heads
    kk, vv = k.repeat_interleave(group, dim=1), v.repeat_interleave(group, dim=1)
    s = torch.einsum("qhd,khd->hqk", q, kk) * (1.0 / math.sqrt(D))
    visible = torch.arange(n_k, device=q.device)[None, :] <= seq["diag"].to(q.device)[:, None]
    dead = ~visible.any(dim=1)
    lse = torch.logsumexp(s.masked_fill(~visible[None], NEG_INF).masked_fill(dead[None, :, None], 0.0), dim=-1)
    lse = lse.masked_fill(dead[None], NEG_INF)
    p_true = torch.where(visible[None] & ~dead[None, :, None], torch.exp(s - lse[..., None]), torch.zeros_like(s))
    o = torch.einsum("hqk,khd->qhd", p_true, vv)
    delta = (do * o).sum(-1).t().contiguous()
    dp = torch.einsum("qhd,khd->hqk", do, vv)
    parts = dict(s=s, lse=lse, delta=delta, dp=dp, o=o, q=q, kk=kk, vv=vv, do=do, visible=visible)
    for name in ("dkdv", "dq"):
        state = dict(lse=lse.clone(), delta=delta.clone(), visible=visible[None].expand(heads, -1, -1).clone(), weight=torch.ones_like(s))
        if name == "dkdv":
            state["head_weight"] = torch.ones((heads, n_k), device=q.device)
        if hook is not None:
            hook(name, state)
        alive = state["visible"] & torch.isfinite(state["lse"])[..., None]
        p = torch.where(alive, torch.exp(s - state["lse"].masked_fill(~torch.isfinite(state["lse"]), 0.0)[..., None]), torch.zeros_like(s))
        p = p * state["weight"]
        ds = p * (dp - state["delta"][..., None])
        if name == "dkdv":
            hw = state["head_weight"].t()[..., None]
            dv_h = torch.einsum("hqk,qhd->khd", p, do) * hw
            dk_h = torch.einsum("hqk,qhd->khd", ds, q) * (hw / math.sqrt(D))
            dv, dk = (x.reshape(n_k, kv_heads, group, D).sum(2) for x in (dv_h, dk_h))
            parts.update(p=p, ds=ds, dk_h=dk_h, dv_h=dv_h)
        else:
            dq = torch.einsum("hqk,khd->qhd", ds, kk) * (1.0 / math.sqrt(D))
    return (dq, dk, dv, parts) if want_parts else (dq, dk, dv)


def eager_backward(seq, dout, dtype):
    """autograd through eager() in `dtype` arithmetic -> [dq, dk, dv] as fp32: the gradient rule's two references"""
    n_k = seq["n_k"]
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (seq["q"], seq["k"][:n_k], seq["v"][:n_k])]
    eager(*leaves, seq["diag"], dtype)[0].backward(dout.to(dtype))
    return [t.grad.float() for t in leaves]


def grad_bounds(r32, r16):
    """The gradient rule's two bounds for one gradient of one sequence (tests/test_varlen_qk_gpu.py's _check_grad, flash-attn's
    rule): max|g - g32| <= 2 max|g16 - g32| + 1e-4 and ||g - g32|| / ||g32|| <= 2 ||g16 - g32|| / ||g32|| + 1e-3
    -> dict(bound, rel_bound, norm); a gradient that is zero throughout has no relative part (norm 0)"""
    norm = r32.norm().item()
    rel16 = ((r16 - r32).norm().item() / norm) if norm > 0 else 0.0
    return dict(bound=2 * (r16 - r32).abs().max().item() + 1e-4, rel_bound=2 * rel16 + 1e-3, norm=norm)


def grad_rule_stats(err, err_norm, bounds, finite=True):
    """The rule on the two figures of g - g32, its largest entry and its L2 norm (a difference that is zero outside a few rows
    has those rows' figures) -> dict(ok, err, bound, rel, rel_bound, ratio): ratio > 1 means rejected"""
    rel = err_norm / bounds["norm"] if bounds["norm"] > 0 else 0.0
    ok = finite and err <= bounds["bound"] and rel <= bounds["rel_bound"]
    return dict(ok=ok, err=err, bound=bounds["bound"], rel=rel, rel_bound=bounds["rel_bound"],
                ratio=max(err / bounds["bound"], rel / bounds["rel_bound"]) if finite else float("inf"))


def grad_rule(g, r32, r16, bounds=None):
    """The gradient rule for ONE gradient of one sequence or batch entry: g from the code under test, r32 / r16 fp32 and 16-bit
    eager autograd (eager_backward) -> grad_rule_stats' dict"""
    g = g.float()
    diff = g - r32
    finite = bool(torch.isfinite(g).all()) and g.shape == r32.shape
    return grad_rule_stats(diff.abs().max().item() if diff.numel() else 0.0, diff.norm().item(), bounds or grad_bounds(r32, r16), finite)
