"""The tests of the beacon tests, without a device: the inputs, positions and comparison of tests/beacon_inputs.py, as GPU
tests/test_beacon_gpu.py uses them, applied to deliberately wrong fp32 references (lengths capped for the CPU: varlen and dense
lengths above 1100 become 1024 + n % 64, the decode entry of 33 000 keys 1064, decode lengths of 4097 and below stay; the
inputs come from the same generator, not the same tensors -- the GPU test draws on its device, with the cache's capacity
behind every entry -- so it asserts the probability condition again at its own lengths).  Every mutant must FAIL the comparison, the
16-bit eager reference must pass it, every listed position must be the target of a live row, and every target must carry an fp32
probability in [0.25, 0.75] (1 where the target is the only key the row sees: decode entries of length 1, the first row of
an equal-length causal sequence).

The mutants: the mask's diagonal (without a mask: the length) shifted by +1 and by -1 -- computed in full, with the beacon
behind the last key as key n_k; each listed position dropped, and counted twice; the last key's contribution replaced by a
copy of key n - 2's (the fetch clamp's failure).  The last three are exact rank-one updates of the fp32 result in float64:
dropping key p turns o into (o - P_p v_p) / (1 - P_p) and lse into lse + ln(1 - P_p), and so on.

The windowed decode family (tests/test_window_beacon_gpu.py's launches: every length, seqlen_q, window and split count) has two
edges per row and the mutants of both: the lower edge shifted by -1 (the key below the window, a beacon the query leaks towards,
becomes visible) and by +1, the upper edge by +1 and -1, each listed position dropped and counted twice, key lo_min's
contribution replaced by a copy of key lo_min + 1's (the lower fetch clamp's failure) and the last key's by key n - 2's.

The backward (tests/test_backward_beacon_gpu.py's inputs; the section "the backward's cells" below) has the gradient rule in place
of the comparison and mutants of the explicit fp32 backward, one per live (32-row band, 32-key cell) pair, diagonal tile, 64-row
tile, query head and split part: each must fail bi.grad_rule, and the 16-bit eager gradients must pass it."""
import ctypes

import pytest
import torch

from flash_attention_from_scratch_amd import _capi
from tests import beacon_inputs as bi
from tests.test_decode_cpu import _args
from tests.test_window_cpu import _w

DTYPES = [torch.bfloat16, torch.float16]


def _rank_one(o32, lse32, p32, vv, take, give):
    """The fp32 result with the weight of keys `take` removed and that of `give` = [(weight column, value row)] added:
    o32 (n_q, H, 128), lse32 (H, n_q), p32 (H, n_q, n_k), vv (n_k, H, 128) -> (o, lse) in float64 precision, as fp32"""
    o = o32.double().permute(1, 0, 2)
    mass = torch.ones_like(lse32, dtype=torch.float64)
    for j in take:
        w = p32[:, :, j].double()
        o = o - w[..., None] * vv[j].double()[:, None, :]
        mass = mass - w
    for j_w, j_v in give:
        w = p32[:, :, j_w].double()
        o = o + w[..., None] * vv[j_v].double()[:, None, :]
        mass = mass + w
    empty = mass < 1e-9
    o = torch.where(empty[..., None], torch.zeros_like(o), o / mass.clamp_min(1e-9)[..., None])
    lse = torch.where(empty, torch.full_like(mass, bi.NEG_INF), lse32.double() + torch.log(mass.clamp_min(1e-9)))
    return o.permute(1, 0, 2).float(), lse.float()


def _check_sequence(tag, seq, covered):
    """One sequence (one phase): the conditions on the inputs, the 16-bit eager accepted, every mutant rejected.  `covered`
    collects the listed positions this phase targets."""
    n_q, n_k, dtype = seq["n_q"], seq["n_k"], seq["q"].dtype
    q, k, v, diag, targets = seq["q"], seq["k"], seq["v"], seq["diag"], seq["targets"]
    group = q.shape[1] // k.shape[1]
    o32, lse32, p32 = bi.eager(q, k[:n_k], v[:n_k], diag, torch.float32, want_p=True)
    o16, _ = bi.eager(q, k[:n_k], v[:n_k], diag, dtype)
    assert torch.isfinite(k.float()).all() and torch.isfinite(v.float()).all() and k.shape[0] > n_k   # a finite key behind the last
    base = bi.compare(o16, None, o32, lse32, o16, dtype)
    assert base["ok"], (tag, base)
    assert bi.compare(o32, lse32, o32, lse32, o16, dtype)["ok"], tag
    # the targets: inside the row's sight, with about half of the row's probability
    live = diag >= 0
    assert (targets[:, ~live] == -1).all() and (targets[:, live] >= 0).all() and (targets[:, live] <= diag[None, live]).all(), tag
    if live.any():
        p_t = p32[:, live].gather(2, targets[:, live, None]).squeeze(2)
        several = (diag[live] >= 1)[None, :].expand_as(p_t)
        assert ((p_t[several] >= bi.P_LO) & (p_t[several] <= bi.P_HI)).all(), (tag, p_t[several].min().item(), p_t[several].max().item())
        assert (p_t[~several] == 1).all(), tag
    hit = set(targets[:, live].flatten().tolist()) & set(seq["listed"])
    covered |= hit

    def rejected(name, o, lse):
        res = bi.compare(o, lse, o32, lse32, o16, dtype)
        assert not res["ok"], (tag, name, res)

    # +1: every row points at the first key it must not see (key n_k is the beacon behind the last key); -1: the rows that
    # target their own diagonal notice, and every sequence has some
    assert (targets[:, live] == diag[None, live]).any(), tag
    for delta in (1, -1):
        o, lse = bi.eager(q, k[:n_k + 1], v[:n_k + 1], diag, torch.float32, delta=delta)
        rejected(f"diagonal {delta:+d}", o, lse)
    vv = v[:n_k].float().repeat_interleave(group, dim=1)
    for p in sorted(hit):
        rejected(f"key {p} dropped", *_rank_one(o32, lse32, p32, vv, [p], []))
        rejected(f"key {p} twice", *_rank_one(o32, lse32, p32, vv, [], [(p, p)]))
    assert n_k - 1 in hit, tag
    if n_k >= 2:
        rejected("last key fetched from n - 2", *_rank_one(o32, lse32, p32, vv, [n_k - 1], [(n_k - 2, n_k - 2)]))


def _rule_splits(H, Hkv, Sq):
    lib = _capi.load()
    a = _args(batch=len(bi.DECODE_LENGTHS), Sq=Sq, H=H, Hkv=Hkv, cache=bi.DECODE_CACHE_LEN, num_splits=0)
    ns = lib.fa_decode_num_splits(ctypes.byref(a))
    assert ns >= 1, _capi.last_error()
    return ns


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("H,Hkv,Sq", bi.DECODE_SHAPES)
def test_decode_family_rejects_every_mutant(dtype, causal, H, Hkv, Sq):
    for b, n in enumerate(bi.DECODE_LENGTHS):
        n = bi.cpu_cap(n, 4097)   # (33000 -> 1064 keys, the CPU's cap; 4097 and below stay)
        kv = None
        for splits in bi.DECODE_SPLITS:
            ns = splits or _rule_splits(H, Hkv, Sq)
            listed = bi.decode_positions(n, Sq, ns)
            assert {0, n - 1} <= set(listed) and all(0 <= p < n for p in listed)
            covered, phase, n_phases = set(), 0, 1
            while phase < n_phases:
                seq = bi.build_sequence(Sq, n, H, Hkv, listed, dtype, causal, phase, seed=b, kv=kv)   # (keys up to n: the CPU's cap)
                kv = (seq["k"], seq["v"])
                _check_sequence(f"decode len {n} splits {ns} phase {phase}", seq, covered)
                n_phases, phase = seq["n_phases"], phase + 1
            assert covered == set(listed), (n, ns, set(listed) ^ covered)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("heads", bi.VARLEN_HEADS)
@pytest.mark.parametrize("name", list(bi.VARLEN_FAMILIES))
def test_varlen_family_rejects_every_mutant(dtype, causal, heads, name):
    seqs, _ = bi.varlen_family(name, heads[0], heads[1], dtype, causal, cap=bi.cpu_cap)
    covered = {}
    for seq in seqs:
        pair = (seq["n_q"], seq["n_k"])
        _check_sequence(f"varlen {name} {pair}", seq, covered.setdefault(pair, set()))
    assert {(s["n_q"], s["n_k"]) for s in seqs} == {(bi.cpu_cap(a), bi.cpu_cap(b)) for a, b in bi.VARLEN_FAMILIES[name][0]}   # no pair dropped
    for (n_q, n_k), hit in covered.items():
        want = set(bi.varlen_positions(n_q, n_k))
        assert hit == want, ((n_q, n_k), want ^ hit)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("n,causal", bi.DENSE_CASES)
def test_dense_family_rejects_every_mutant(dtype, n, causal):
    n = min(n, 1024)   # (the CPU's cap: the same tiles at the two ends, fewer in between)
    listed = bi.dense_positions(n)
    seq = bi.build_sequence(n, n, 4, 4, listed, dtype, causal, seed=5)
    assert seq["n_phases"] == 1
    covered = set()
    seq["listed"] = bi.dense_positions(n, diagonals=False)   # the mutants of the ends and the tile boundaries; the diagonals have the +- 1 mutants
    _check_sequence(f"dense {n} causal={causal}", seq, covered)
    assert set(seq["targets"].flatten().tolist()) == set(listed)
    assert covered == set(seq["listed"])


# ---- the windowed decode family ---------------------------------------------------------------------------------------------------

def _check_window_sequence(tag, seq, covered, lo_min):
    """_check_sequence for one windowed entry (one phase): lo beside diag (= hi), and the mutants of both edges.  No row sees a
    key below lo_min, and the lower edge's -1 mutant reaches lo_min - 1 at the lowest: everything is computed on the keys from
    `base` = lo_min - 1 on, positions counted from there (rows that see no key exist only where lo_min, and so base, is 0)."""
    base, dtype = max(lo_min - 1, 0), seq["q"].dtype
    assert base == 0 or (seq["diag"] >= seq["lo"]).all(), tag
    tag, n_k, lo_min, listed = f"{tag} (keys from {base})", seq["n_k"] - base, lo_min - base, {p - base for p in seq["listed"]}
    q, k, v, lo, hi, targets = seq["q"], seq["k"][base:], seq["v"][base:], seq["lo"] - base, seq["diag"] - base, seq["targets"] - base
    group = q.shape[1] // k.shape[1]
    o32, lse32, p32 = bi.eager(q, k[:n_k], v[:n_k], hi, torch.float32, want_p=True, lo=lo)
    o16, _ = bi.eager(q, k[:n_k], v[:n_k], hi, dtype, lo=lo)
    assert torch.isfinite(k.float()).all() and torch.isfinite(v.float()).all() and k.shape[0] > n_k   # a finite key behind the last
    accepted = bi.compare(o16, None, o32, lse32, o16, dtype)
    assert accepted["ok"], (tag, accepted)
    assert bi.compare(o32, lse32, o32, lse32, o16, dtype)["ok"], tag
    live = hi >= lo
    assert (lo >= 0).all() and (hi < n_k).all() and (hi[~live] < 0).all() and live.any(), tag
    assert int(lo[live].min()) == lo_min, tag
    assert (targets[:, ~live] == -1).all() and (targets[:, live] >= lo[None, live]).all() and (targets[:, live] <= hi[None, live]).all(), tag
    assert (torch.isinf(lse32[:, ~live])).all() and torch.isfinite(lse32[:, live]).all(), tag
    p_t = p32[:, live].gather(2, targets[:, live, None]).squeeze(2)
    several = (hi[live] - lo[live] >= 1)[None, :].expand_as(p_t)      # the ONLY exemption: rows that see fewer than two keys
    p_range = (p_t[several].min().item(), p_t[several].max().item()) if several.any() else None
    assert p_range is None or (bi.P_LO <= p_range[0] and p_range[1] <= bi.P_HI), (tag, p_range)
    assert (p_t[~several] == 1).all(), tag
    hit = set(targets[:, live].flatten().tolist()) & listed
    covered |= {p + base for p in hit}

    def rejected(name, o, lse):
        res = bi.compare(o, lse, o32, lse32, o16, dtype)
        assert not res["ok"], (tag, name, res)

    # the edges: in every phase some row targets its own first key and some row its own last key
    assert (targets[:, live] == lo[None, live]).any() and (targets[:, live] == hi[None, live]).any(), tag
    if (lo[live] >= 1).any():   # lo - 1: the key below the window, which the rows leak towards, is in the cache and now seen
        rejected("lower edge -1", *bi.eager(q, k[:n_k + 1], v[:n_k + 1], hi, torch.float32, lo=lo, delta_lo=-1))
    rejected("lower edge +1", *bi.eager(q, k[:n_k + 1], v[:n_k + 1], hi, torch.float32, lo=lo, delta_lo=1))
    for delta in (1, -1):       # hi + 1: the first hidden key (key n_k: the beacon behind the last key)
        rejected(f"upper edge {delta:+d}", *bi.eager(q, k[:n_k + 1], v[:n_k + 1], hi, torch.float32, delta=delta, lo=lo))
    vv = v[:n_k].float().repeat_interleave(group, dim=1)
    for p in sorted(hit):
        rejected(f"key {p} dropped", *_rank_one(o32, lse32, p32, vv, [p], []))
        rejected(f"key {p} twice", *_rank_one(o32, lse32, p32, vv, [], [(p, p)]))
    assert {lo_min, n_k - 1} <= hit, tag
    if lo_min + 1 < n_k:
        rejected("key lo_min fetched from lo_min + 1", *_rank_one(o32, lse32, p32, vv, [lo_min], [(lo_min + 1, lo_min + 1)]))
    if n_k >= 2:
        rejected("last key fetched from n - 2", *_rank_one(o32, lse32, p32, vv, [n_k - 1], [(n_k - 2, n_k - 2)]))
    return p_range


def _rule_window_splits(H, Hkv, Sq, left, right, causal):
    lib = _capi.load()
    a = _args(batch=len(bi.WINDOW_LENGTHS), Sq=Sq, H=H, Hkv=Hkv, cache=bi.WINDOW_CACHE_LEN, num_splits=0, causal=1 if causal else 0)
    ns = lib.fa_decode_window_num_splits(ctypes.byref(a), ctypes.byref(_w(left, right)))
    assert ns >= 1, _capi.last_error()
    return ns


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("H,Hkv,Sq", bi.DECODE_SHAPES)
def test_window_family_rejects_every_mutant(dtype, H, Hkv, Sq):
    """Every (length, window, split count) tests/test_window_beacon_gpu.py launches at this shape: nothing skipped."""
    assert bi.WINDOW_CACHE_LEN % 256 == 0 and bi.WINDOW_CACHE_LEN > max(bi.WINDOW_LENGTHS) and min(bi.WINDOW_LENGTHS) < Sq
    lo_mins, p_lo, p_hi, checked = set(), 1.0, 0.0, 0
    for b, n in enumerate(bi.WINDOW_LENGTHS):
        n = bi.cpu_cap(n, 4097)   # (as the decode family: 4097 and below stay)
        kv = None
        for left, right, causal in bi.WINDOWS:
            side = bi.window_sides(left, right, causal)
            lo_min = bi.window_lo_min(n, Sq, left)
            lo_mins.add(lo_min)
            for splits in bi.WINDOW_SPLITS:
                ns = splits or _rule_window_splits(H, Hkv, Sq, left, right, causal)
                listed = bi.window_positions(n, Sq, *side, ns)
                assert {lo_min, n - 1} <= set(listed) and all(lo_min <= p < n for p in listed)
                covered, phase, n_phases = set(), 0, 1
                while phase < n_phases:
                    seq = bi.build_window_sequence(Sq, n, H, Hkv, listed, dtype, *side, phase, seed=b, kv=kv)
                    kv = (seq["k"], seq["v"])
                    rng = _check_window_sequence(f"window {(left, right, causal)} len {n} splits {ns} phase {phase}", seq, covered, lo_min)
                    if rng:
                        p_lo, p_hi = min(p_lo, rng[0]), max(p_hi, rng[1])
                    n_phases, phase, checked = seq["n_phases"], phase + 1, checked + 1
                assert covered == set(listed), (n, (left, right, causal), ns, set(listed) ^ covered)
    assert checked >= len(bi.WINDOW_LENGTHS) * len(bi.WINDOWS) * len(bi.WINDOW_SPLITS)
    print(f"window family {dtype} H={H} Hkv={Hkv} Sq={Sq}: {checked} sequences, target probabilities {p_lo:.3f} .. {p_hi:.3f}")
    # where lo_min falls: on a tile boundary, in a tile's first unit, on its second unit's first key, inside its second unit;
    # and inside a 256-key page but not in that page's first tile -- at this shape, every one with keys below the window
    below = {m for m in lo_mins if m > 0}
    residues = {m % 64 for m in below}
    assert 0 in residues and 32 in residues and residues & set(range(1, 32)) and residues & set(range(33, 64)), sorted(residues)
    assert any(m % 256 >= 64 for m in below), sorted(below)


def test_window_family_keeps_the_required_windows():
    """a right > 0 with a bounded left and with an unbounded one, left = 0, a window wider than every length"""
    sides = [bi.window_sides(*w) for w in bi.WINDOWS]
    assert any(l >= 0 and r > 0 for l, r in sides) and any(l < 0 and r > 0 for l, r in sides)
    assert any(l == 0 for l, _ in sides) and any(l >= max(bi.WINDOW_LENGTHS) and r <= 0 for l, r in sides)
    assert any(n < Sq for n in bi.WINDOW_LENGTHS for _, _, Sq in bi.DECODE_SHAPES) and (8, 1, 8) in bi.DECODE_SHAPES


# ---- the backward's cells -----------------------------------------------------------------------------------------------------------
#
# The mutants are those of a backward that works in (row range x key range) pairs ("Backward cells").  Every one
# changes the fp32 gradients by a difference that is zero outside a few rows, and the rule needs that difference's largest entry
# and L2 norm only (bi.grad_rule_stats), so a cell's contribution is computed once and serves "dropped" and "counted twice";
# test_backward_hooks_give_the_same_mutants holds these differences to bi.reference_backward's hooks, which redo the whole pass.

def _group_sum(x, kv_heads, dim):
    """sum the query heads of each K / V head: dimension `dim` (H) -> Hkv"""
    if x.shape[dim] == kv_heads:
        return x
    shape = list(x.shape)
    shape[dim:dim + 1] = [kv_heads, shape[dim] // kv_heads]
    return x.reshape(shape).sum(dim + 1)


def _stats(diff):
    return diff.abs().max().item() if diff.numel() else 0.0, diff.norm().item()


def _blocks(n, size):
    return [slice(a, min(a + size, n)) for a in range(0, n, size)]


def _backward_mutants(seq, parts):
    """-> yields (name, {gradient name: (largest entry, L2 norm) of the mutant's difference from the fp32 backward})"""
    n_q, n_k, diag = seq["n_q"], seq["n_k"], seq["diag"]
    s, lse, delta, dp, p, ds = (parts[x] for x in ("s", "lse", "delta", "dp", "p", "ds"))
    q, kk, do, visible = (parts[x] for x in ("q", "kk", "do", "visible"))
    heads, kv_heads, rs = q.shape[1], seq["k"].shape[1], 1.0 / bi.D ** 0.5
    n_j = (n_k + bi.CELL - 1) // bi.CELL
    pad = n_j * bi.CELL - n_k
    padded = lambda x: torch.nn.functional.pad(x, (0, pad))                       # (the key axis last)
    kk_cells = torch.nn.functional.pad(kk, (0, 0, 0, 0, 0, pad)).reshape(n_j, bi.CELL, heads, bi.D)
    live = {}
    for i, j, on in seq["cells"]:
        live.setdefault(i, {})[j] = on

    # every live cell: dropped from / counted twice in dK and dV, and in dQ alone
    for i, js in live.items():
        rows = slice(bi.CELL * i, min(bi.CELL * (i + 1), n_q))
        p_c = padded(p[:, rows]).reshape(heads, -1, n_j, bi.CELL)
        ds_c = padded(ds[:, rows]).reshape(heads, -1, n_j, bi.CELL)
        dv_c = _group_sum(torch.einsum("hajb,ahd->jhbd", p_c, do[rows]), kv_heads, 1)
        dk_c = _group_sum(torch.einsum("hajb,ahd->jhbd", ds_c, q[rows]), kv_heads, 1) * rs
        dq_c = torch.einsum("hajb,jbhd->jahd", ds_c, kk_cells) * rs
        for j in js:
            for what in ("dropped from", "counted twice in"):
                yield f"cell ({i}, {j}) {what} dK / dV", dict(dk=_stats(dk_c[j]), dv=_stats(dv_c[j]))
                yield f"cell ({i}, {j}) {what} dQ", dict(dq=_stats(dq_c[j]))

    # every diagonal cell: the diagonal shifted by -1 (the row's last key lost) and by +1 (the key behind it seen, with the
    # probability the true lse gives it), inside the cell, in one pass
    r_all = torch.arange(n_q)
    for shift in (-1, 1):
        key = diag + (1 if shift == 1 else 0)                                    # the entry that leaves or enters
        ok = (diag >= 0) & (key < n_k)
        kc = key.clamp(0, max(n_k - 1, 0))
        ok_l, kc_l = ok.tolist(), kc.tolist()
        s_e, dp_e = s[:, r_all, kc], dp[:, r_all, kc]
        p_e = torch.exp(s_e - lse.masked_fill(~torch.isfinite(lse), 0.0)) * torch.isfinite(lse)
        ds_e = p_e * (dp_e - delta)                                              # (H, n_q)
        dv_e = _group_sum(p_e.t()[..., None] * do, kv_heads, 1)                  # (n_q, Hkv, 128): lands on key kc[r]
        dk_e = _group_sum(ds_e.t()[..., None] * q, kv_heads, 1) * rs
        dq_e = ds_e.t()[..., None] * kk[kc] * rs                                 # (n_q, H, 128): row r's own
        for i, js in live.items():
            for j, on in js.items():
                if not on:
                    continue
                rows = [r for r in range(bi.CELL * i, min(bi.CELL * (i + 1), n_q)) if ok_l[r] and kc_l[r] // bi.CELL == j]
                if not rows:      # (+1 where every row's next key lies in the next cell, or behind the last key)
                    continue
                onto = torch.zeros((bi.CELL, len(rows)))                          # several rows may share a key (no mask: all do)
                onto[kc[rows] - bi.CELL * j, torch.arange(len(rows))] = 1.0
                dv_d, dk_d = (onto @ x[rows].reshape(len(rows), -1) for x in (dv_e, dk_e))
                yield f"cell ({i}, {j}) diagonal {shift:+d} in dK / dV", dict(dk=_stats(dk_d), dv=_stats(dv_d))
                yield f"cell ({i}, {j}) diagonal {shift:+d} in dQ", dict(dq=_stats(dq_e[rows]))

    # the mask absent from one whole visit that holds the diagonal: (64-row tile x 128-key block) of the dK / dV sweep,
    # (128-row block x 64-key tile) of the dQ sweep
    lse_f = lse.masked_fill(~torch.isfinite(lse), 0.0)
    for name, row_size, key_size in (("dK / dV", bi.BWD_TILE, bi.BWD_BLOCK), ("dQ", bi.BWD_BLOCK, bi.BWD_TILE)):
        for rows in _blocks(n_q, row_size):
            for keys in _blocks(n_k, key_size):
                vis = visible[rows, keys] & torch.isfinite(lse[0, rows])[:, None]
                if not vis.any() or vis.all():
                    continue
                p_x = torch.exp(s[:, rows, keys] - lse_f[:, rows, None]) * (~vis)[None]
                ds_x = p_x * (dp[:, rows, keys] - delta[:, rows, None])
                tag = f"mask absent from rows {rows.start}.. x keys {keys.start}.. of {name}"
                if name == "dQ":
                    yield tag, dict(dq=_stats(torch.einsum("hqk,khd->qhd", ds_x, kk[keys]) * rs))
                else:
                    yield tag, dict(dv=_stats(_group_sum(torch.einsum("hqk,qhd->khd", p_x, do[rows]), kv_heads, 1)),
                                    dk=_stats(_group_sum(torch.einsum("hqk,qhd->khd", ds_x, q[rows]), kv_heads, 1) * rs))

    # one 64-row tile's delta, and separately its lse, read from the row above
    above = (r_all - 1).clamp_min(0)
    d_delta = delta[:, above] - delta                                             # dS' = P (dP - delta') = dS - P d_delta
    fine = torch.isfinite(lse) & torch.isfinite(lse[:, above])
    factor = torch.where(fine, torch.exp(lse_f - lse_f[:, above]) - 1.0, torch.zeros_like(lse))   # P' = P exp(lse - lse')
    for rows in _blocks(n_q, bi.BWD_TILE):
        ds_d = -p[:, rows] * d_delta[:, rows, None]
        p_l, ds_l = p[:, rows] * factor[:, rows, None], ds[:, rows] * factor[:, rows, None]
        yield f"delta of rows {rows.start}.. from the row above in dK / dV", \
            dict(dk=_stats(_group_sum(torch.einsum("hqk,qhd->khd", ds_d, q[rows]), kv_heads, 1) * rs))
        yield f"delta of rows {rows.start}.. from the row above in dQ", dict(dq=_stats(torch.einsum("hqk,khd->qhd", ds_d, kk) * rs))
        yield f"lse of rows {rows.start}.. from the row above in dK / dV", \
            dict(dk=_stats(_group_sum(torch.einsum("hqk,qhd->khd", ds_l, q[rows]), kv_heads, 1) * rs),
                 dv=_stats(_group_sum(torch.einsum("hqk,qhd->khd", p_l, do[rows]), kv_heads, 1)))
        yield f"lse of rows {rows.start}.. from the row above in dQ", dict(dq=_stats(torch.einsum("hqk,khd->qhd", ds_l, kk) * rs))

    # GQA: one query head, or one part of a split (consecutive or strided heads of the group), missing from / added twice to one
    # 128-key block's sum
    group = heads // kv_heads
    if group > 1:
        dk_h, dv_h = parts["dk_h"], parts["dv_h"]
        sets = [(f"head {h}", [h]) for h in range(heads)]
        for split in range(2, group):
            if group % split == 0:
                per = group // split
                for g in range(kv_heads):
                    for part in range(split):
                        sets.append((f"part {part} / {split} of group {g} (consecutive)", [g * group + part * per + x for x in range(per)]))
                        sets.append((f"part {part} / {split} of group {g} (strided)", [g * group + part + split * x for x in range(per)]))
        for keys in _blocks(n_k, bi.BWD_BLOCK):
            seen = visible[:, keys].any()
            for tag, hs in sets:
                if seen:
                    st = dict(dk=_stats(dk_h[keys][:, hs].sum(1)), dv=_stats(dv_h[keys][:, hs].sum(1)))
                    for what in ("missing from", "added twice to"):
                        yield f"{tag} {what} keys {keys.start}..", st


def _check_backward_sequence(tag, seq, seed, worst):
    """One sequence (one phase): the conditions on the inputs, the fp32 backward equal to autograd, the 16-bit eager gradients
    accepted -> {mutant: the rule's ratio, > 1 means rejected}.  worst: dict collecting the largest accepted ratio and the
    smallest |dS| of a target."""
    dtype = seq["q"].dtype
    o32, lse32, _ = bi.references(seq)
    p_t, several = bi.target_probabilities(seq, lse32)
    assert ((p_t[several] >= bi.P_LO) & (p_t[several] <= bi.P_HI)).all(), (tag, p_t[several].min().item(), p_t[several].max().item())
    dout = bi.beacon_dout(seq, o32, seed=seed)
    ds_t, _ = bi.target_ds(seq, dout, o32, lse32)
    if several.any():
        assert (ds_t[several].abs() >= bi.DS_FLOOR).all(), (tag, ds_t[several].abs().min().item())
        worst["ds"] = min(worst.get("ds", 1e9), ds_t[several].abs().min().item())
    dq, dk, dv, parts = bi.reference_backward(seq, dout, want_parts=True)
    g32, g16 = bi.eager_backward(seq, dout, torch.float32), bi.eager_backward(seq, dout, dtype)
    bounds = {}
    for name, g, r32, r16 in zip(("dq", "dk", "dv"), (dq, dk, dv), g32, g16):
        assert (g - r32).norm().item() <= 1e-5 * r32.norm().item() + 1e-9, (tag, name, ((g - r32).norm() / r32.norm()).item())
        bounds[name] = bi.grad_bounds(r32, r16)
        accepted = bi.grad_rule(r16, r32, r16, bounds[name])
        assert accepted["ok"] and bi.grad_rule(r32, r32, r16, bounds[name])["ok"], (tag, name, accepted)
        worst["accepted"] = max(worst.get("accepted", 0.0), accepted["ratio"])
    return {name: max(bi.grad_rule_stats(err, norm, bounds[g])["ratio"] for g, (err, norm) in diffs.items())
            for name, diffs in _backward_mutants(seq, parts)}


def _check_backward_phases(tag, n_q, n_k, heads, dtype, causal, seed, worst):
    """Every phase of one (n_q, n_k): full coverage over the phases, and every mutant rejected in some phase (a phase is a copy of
    the sequence in the same launch: a kernel wrong in one cell is wrong in every copy)."""
    seqs, phase, n_phases = [], 0, 1
    while phase < n_phases:
        seqs.append(bi.build_cell_sequence(n_q, n_k, heads[0], heads[1], dtype, causal, phase, seed=seed + phase))
        n_phases, phase = seqs[-1]["n_phases"], phase + 1
    assert bi.cell_coverage(seqs) == ([], [], []), (tag, bi.cell_coverage(seqs))
    ratios = {}
    for phase, seq in enumerate(seqs):
        for name, ratio in _check_backward_sequence(f"{tag} phase {phase}", seq, seed + 100 + phase, worst).items():
            ratios[name] = max(ratios.get(name, 0.0), ratio)
    assert ratios
    name = min(ratios, key=ratios.get)
    worst.update(ratio=ratios[name], mutant=f"{tag}: {name}", mutants=len(ratios), phases=len(seqs))
    passed = sorted((r, n) for n, r in ratios.items() if r <= 1.0)
    assert not passed, (tag, len(passed), passed[:4])
    return seqs


BACKWARD_CPU_CASES = [(n, n, causal) for n in (256, 512) for causal in (False, True)] + [(300, 300, False), (300, 300, True),
                                                                                         (129, 300, False), (129, 300, True)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("heads", bi.BACKWARD_HEADS)
@pytest.mark.parametrize("n_q,n_k,causal", BACKWARD_CPU_CASES)
def test_backward_cells_reject_every_mutant(dtype, heads, n_q, n_k, causal):
    worst = {}
    _check_backward_phases(f"backward ({n_q}, {n_k}) causal={causal} heads={heads}", n_q, n_k, heads, dtype, causal, 3, worst)
    print(f"backward cells {dtype} ({n_q}, {n_k}) causal={causal} heads={heads}: {worst['mutants']} mutants, smallest ratio "
          f"{worst['ratio']:.2f} ({worst['mutant']}), 16-bit eager at {worst['accepted']:.3f}, smallest |dS| {worst['ds']:.2f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_backward_cells_reject_every_mutant_at_1024(dtype):
    worst = {}
    _check_backward_phases("backward (1024, 1024) causal", 1024, 1024, (4, 4), dtype, True, 3, worst)
    print(f"backward cells {dtype} 1024 causal: {worst['mutants']} mutants, smallest ratio {worst['ratio']:.2f} ({worst['mutant']}), "
          f"16-bit eager at {worst['accepted']:.3f}, smallest |dS| {worst['ds']:.2f}")


def test_backward_hooks_give_the_same_mutants():
    """One mutant of every class, made a second time through bi.reference_backward's hooks -- the whole pass redone with the
    cell's weight, the visible set, delta, lse or a head's weight changed -- has the figures _backward_mutants derives."""
    seq = bi.build_cell_sequence(256, 256, 8, 2, torch.bfloat16, True, seed=3)
    o32, _, _ = bi.references(seq)
    dout = bi.beacon_dout(seq, o32, seed=103)
    dq, dk, dv, parts = bi.reference_backward(seq, dout, want_parts=True)
    derived = dict(_backward_mutants(seq, parts))
    diag = seq["diag"]
    band3 = torch.arange(96, 128)

    def set_(which, key, rows, cols, value):
        def hook(name, state):
            if name == which:
                r, c = torch.as_tensor(rows), torch.as_tensor(cols)
                if state[key].dim() == 3:
                    state[key][:, r[:, None], c[None, :]] = value
                else:
                    state[key][r[:, None], c[None, :]] = value
        return hook

    def diagonal(which, shift):
        def hook(name, state):
            if name == which:      # rows 96 .. 127, inside key cell 3 (keys 96 .. 127)
                for r in band3.tolist():
                    key = int(diag[r]) + (1 if shift == 1 else 0)
                    if 96 <= key < 128:
                        state["visible"][:, r, key] = shift == 1
        return hook

    def above(which, key):
        def hook(name, state):
            if name == which:
                state[key][:, 64:128] = state[key][:, 63:127].clone()
        return hook

    cases = {
        "cell (5, 2) dropped from dK / dV": set_("dkdv", "weight", range(160, 192), range(64, 96), 0.0),
        "cell (5, 2) counted twice in dQ": set_("dq", "weight", range(160, 192), range(64, 96), 2.0),
        "cell (3, 3) diagonal +1 in dK / dV": diagonal("dkdv", 1),
        "cell (3, 3) diagonal -1 in dQ": diagonal("dq", -1),
        "mask absent from rows 64.. x keys 0.. of dK / dV": set_("dkdv", "visible", range(64, 128), range(0, 128), True),
        "mask absent from rows 128.. x keys 192.. of dQ": set_("dq", "visible", range(128, 256), range(192, 256), True),
        "delta of rows 64.. from the row above in dQ": above("dq", "delta"),
        "lse of rows 64.. from the row above in dK / dV": above("dkdv", "lse"),
        "head 1 missing from keys 128..": set_("dkdv", "head_weight", [1], range(128, 256), 0.0),
        "part 0 / 2 of group 0 (consecutive) added twice to keys 0..": set_("dkdv", "head_weight", [0, 1], range(0, 128), 2.0),
        "part 1 / 2 of group 1 (strided) missing from keys 0..": set_("dkdv", "head_weight", [5, 7], range(0, 128), 0.0),
    }
    for name, hook in cases.items():
        got = dict(zip(("dq", "dk", "dv"), bi.reference_backward(seq, dout, hook=hook)))
        for g, ref in zip(("dq", "dk", "dv"), (dq, dk, dv)):
            err, norm = _stats(got[g] - ref)
            want = derived[name].get(g)
            if want is None:
                assert norm <= 1e-4 * ref.norm().item(), (name, g, norm)     # a gradient this mutant leaves alone
            else:
                assert abs(err - want[0]) <= 1e-3 * want[0] + 1e-5 and abs(norm - want[1]) <= 1e-3 * want[1] + 1e-5, (name, g, err, norm, want)
