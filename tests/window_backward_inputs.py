"""Inputs and references for the sliding-window varlen backward: tests/test_bwd_window_cpu.py and
tests/test_bwd_window_gpu.py share them.  Built on tests/beacon_inputs.py, which stays as it is.

The sequences are bi.build_window_sequence's with an empty position list: head 0 (every even head) of each live row targets
the row's own last key hi_r, head 1 (every odd head) its first key lo_r, and the query leaks onto hi_r + 1 and lo_r - 1, the
first keys the row must NOT see on either side -- a mask off by one at either edge lets a key in that dominates the row, or
drops the key that holds half of it.  As the rows slide, the two edges pass over every key of the window's band, so every
64-key tile and 128-key block boundary the band crosses is some row's edge.  dout is bi.beacon_dout's, so |dS| on the target
is at least bi.DS_FLOOR.  The references are autograd through bi.eager with the window mask (lo=, and delta= / delta_lo= for
the CPU proof's mutants) in fp32 and in the 16-bit type: the two references of the gradient rule bi.grad_rule.

Plain helper module: no tests, no fixtures; runs on the CPU or the GPU with a seed."""
import torch

import beacon_inputs as bi

# the launches of tests/test_bwd_window_gpu.py; the kernels work in 128-row blocks and 64-row tiles
PAIRS = [(300, 300), (130, 700), (700, 130), (257, 513), (64, 64), (1, 200), (65, 63), (0, 50), (50, 0)]   # (len_q, len_k)
LOOSE = (1024, 2048)                      # the second launch's (max_seqlen_q, max_seqlen_k)
HEADS = [(4, 4), (8, 2), (4, 1)]
WINDOWS = [(0, 0, False), (1, -1, True), (63, 0, False), (64, -1, True), (65, 0, False), (100, -1, True), (17, 9, False),
           (3, 2, False), (-1, 5, False), (5, -1, False), (200, 200, False), (0, 64, False)]   # (left, right, causal)
# the cases the construction was checked on when it was written (bf16): (len_q, len_k, (left, right))
PROOF_CASES = [(300, 300, (63, 0)), (130, 700, (100, 0)), (257, 513, (17, 9)), (300, 300, (200, -1))]


def sequence(n_q, n_k, heads, dtype, left, right, seed=0, device="cpu"):
    """One sequence under window (left, right) (causal: pass right = 0) -> bi.build_window_sequence's dict (q, k, v, targets,
    diag = hi, lo); n_q = 0 gives an empty q"""
    if n_q == 0:
        pairs = [bi.beacon_kv(n_k, dtype, None, seed * 1000 + 2 * h, device) for h in range(heads[1])]
        empty = torch.zeros((0,), dtype=torch.int64)
        return dict(q=torch.zeros((0, heads[0], bi.D), dtype=dtype, device=device), k=torch.stack([p[0] for p in pairs], dim=1),
                    v=torch.stack([p[1] for p in pairs], dim=1), targets=torch.zeros((heads[0], 0), dtype=torch.int64), diag=empty,
                    lo=empty, n_phases=1, n_q=0, n_k=n_k, listed=[])
    return bi.build_window_sequence(n_q, n_k, heads[0], heads[1], [], dtype, left, right, seed=seed, device=device)


def forward_and_dout(seq, seed=0):
    """-> (o32, lse32, dout): the fp32 windowed reference forward and bi.beacon_dout on it"""
    o32, lse32, _ = bi.references(seq)
    return o32, lse32, bi.beacon_dout(seq, o32, seed=seed)


def eager_backward(seq, dout, dtype, delta=0, delta_lo=0, extra=0):
    """autograd through bi.eager with the window mask in `dtype` arithmetic -> [dq, dk, dv] as fp32, dk and dv of n_k rows.
    delta / delta_lo: the upper / the lower edge moved (a deliberately wrong mask); extra: key rows behind n_k that take part
    (row n_k holds a beacon: an upper edge moved up reaches it)."""
    n_q, n_k = seq["n_q"], seq["n_k"]
    shapes = [t.shape for t in (seq["q"], seq["k"][:n_k], seq["v"][:n_k])]
    if n_q == 0 or n_k == 0:
        return [torch.zeros(s, dtype=torch.float32, device=seq["q"].device) for s in shapes]
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (seq["q"], seq["k"][:n_k + extra], seq["v"][:n_k + extra])]
    bi.eager(*leaves, seq["diag"], dtype, delta=delta, lo=seq["lo"], delta_lo=delta_lo)[0].backward(dout.to(dtype))
    return [leaves[0].grad.float(), leaves[1].grad.float()[:n_k], leaves[2].grad.float()[:n_k]]


def mutants(seq, left, right):
    """The masks off by one the window can express -> [(delta, delta_lo, extra)]: hi +- 1 unless right is unbounded (hi is the
    last key: nothing above it in a packed layout, and below it no window's edge), lo +- 1 unless left is unbounded; lo - 1
    only where some live row has a key below its window."""
    live = seq["diag"] >= seq["lo"]
    out = []
    if right >= 0:
        out += [(1, 0, 1), (-1, 0, 0)]
    if left >= 0:
        out += [(0, 1, 0)] + ([(0, -1, 0)] if bool((seq["lo"][live] >= 1).any()) else [])
    return out


def unseen_keys(seq):
    """bool (n_k,): keys no row of the sequence sees"""
    n_k = seq["n_k"]
    seen = torch.zeros(n_k + 1, dtype=torch.int64)
    for lo, hi in zip(seq["lo"].tolist(), seq["diag"].tolist()):
        if hi >= lo:
            seen[lo] += 1
            seen[hi + 1] -= 1
    return seen.cumsum(0)[:n_k] == 0


def visited_tiles_brute(n_q, n_k, left, right):
    """(dQ key tiles, dK / dV row tiles) a launch visits, counted cell by cell from bi.window_bounds: per 128-row block the
    64-key tiles from its live rows' lowest floor to their highest ceiling; per 128-key block the 64-row tiles from the first to
    the last row that sees one of its keys"""
    lo, hi = (t.tolist() for t in bi.window_bounds(n_q, n_k, left, right)) if n_q else ([], [])
    dq = 0
    for r0 in range(0, n_q, 128):
        live = [r for r in range(r0, min(r0 + 128, n_q)) if hi[r] >= lo[r]]
        if live:
            dq += max(hi[r] for r in live) // 64 - min(lo[r] for r in live) // 64 + 1
    dkdv = 0
    for k0 in range(0, n_k, 128):
        k1 = min(k0 + 128, n_k) - 1
        rows = [r for r in range(n_q) if hi[r] >= lo[r] and lo[r] <= k1 and hi[r] >= k0]
        if rows:
            dkdv += rows[-1] // 64 - rows[0] // 64 + 1
    return dq, dkdv
