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
contribution replaced by a copy of key lo_min + 1's (the lower fetch clamp's failure) and the last key's by key n - 2's."""
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
