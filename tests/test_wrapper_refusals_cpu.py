"""The Python wrapper's refusals on the KV-cache paths, recorded (tests/golden/wrapper_refusals.json, from the commit the file
names): forward_kvcache, kvcache_num_splits, append_kvcache and forward_varlen_kvcache, one argument (or one listed pair) changed
at a time, the exception's type and message compared for every case.  This file holds the cases (the GPU tier,
tests/test_wrapper_refusals_gpu.py, imports them) and runs what is refused before a tensor's device matters: window_size values,
non-tensors, the rules that run first, all on CPU tensors.

    python -m tests.test_wrapper_refusals_cpu     # this tier's records as JSON (tests.test_wrapper_refusals_gpu: the other's)
"""
import hashlib
import json
import os
import sys

import pytest
import torch

from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests.conftest import GOLDEN

RECORDED = os.path.join(GOLDEN, "wrapper_refusals.json")
FUNCTIONS = ("forward_kvcache", "kvcache_num_splits", "append_kvcache", "forward_varlen_kvcache")
B, H, HKV, D, PAGE = 2, 2, 1, 128, 64   # batch / n_seqs, heads, K / V heads, d_head, the page size


def _randn(shape, seed, dtype=torch.bfloat16):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def base(fn, device, paged=False, fp8=False, keys=128):
    """Valid keyword arguments of `fn`: tiny tensors on `device`, a contiguous cache of `keys` keys per entry or a paged one of
    64-key pages, 16-bit or e4m3fn with descales."""
    kc, vc = _randn((B, keys, HKV, D), 1), _randn((B, keys, HKV, D), 2)
    kw = dict(cache_seqlens=torch.tensor([50, keys - 3], dtype=torch.int32))
    if paged:
        kc, vc = (t.reshape(B * keys // PAGE, PAGE, HKV, D) for t in (kc, vc))
        kw["block_table"] = torch.arange(B * keys // PAGE, dtype=torch.int32).reshape(B, keys // PAGE)
    if fp8:
        kc, vc = kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)
        kw.update(k_descale=torch.tensor([[0.5], [2.0]]), v_descale=torch.tensor([[1.5], [0.25]]))
    kw.update(k_cache=kc, v_cache=vc)
    if fn in ("forward_kvcache", "kvcache_num_splits"):
        kw["q"] = _randn((B, 1, H, D), 3)
        if fn == "kvcache_num_splits":
            kw.pop("k_descale", None), kw.pop("v_descale", None)
    elif fn == "append_kvcache":
        kw.update(k=_randn((B, 2, HKV, D), 4), v=_randn((B, 2, HKV, D), 5), q=_randn((B, 1, H, D), 3),
                  rotary_cos=_randn((keys, 32), 6), rotary_sin=_randn((keys, 32), 7))
    else:
        kw.update(q=_randn((5, H, D), 3), cu_seqlens_q=torch.tensor([0, 2, 5], dtype=torch.int32), max_seqlen_q=3)
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}


def _wide(t, pad):
    """t's values in a view whose row stride is `pad` elements longer."""
    buf = torch.zeros(t.shape[:-1] + (t.shape[-1] + pad,), dtype=t.dtype, device=t.device)
    buf[..., :t.shape[-1]] = t
    return buf[..., :t.shape[-1]]


def _shifted(t, by):
    """t's values in a view that begins `by` elements into its storage."""
    buf = torch.zeros(t.numel() + by, dtype=t.dtype, device=t.device)
    out = buf[by:].view(t.shape)
    out.copy_(t)
    return out


def _set(key, f):
    def mutate(kw):
        kw[key] = f(kw[key])
    return (key,), (key,), mutate


def _put(**values):
    """Set keyword arguments; a callable value is called with the arguments so far (a tensor for the cache's device)."""
    def mutate(kw):
        kw.update({k: (v(kw) if callable(v) else v) for k, v in values.items()})
    return (), tuple(values), mutate


def _both(f, *keys):
    def mutate(kw):
        for k in keys:
            kw[k] = f(kw[k])
    return keys, keys, mutate


def _more(t):
    """t with its first entry once more at the end (through bytes: the fp8 types have no cat)."""
    return torch.cat([t.view(torch.uint8), t[:1].view(torch.uint8)]).view(t.dtype) if t.dtype in fak._FLOAT8_DTYPES else torch.cat([t, t[:1]])


def _ones(kw):
    return torch.ones(B, HKV, device=kw["k_cache"].device)


# name -> (the keyword arguments it needs to be there, those it sets, what it does to them)
MUTATIONS = {
    "q:fp32": _set("q", lambda t: t.float()),
    "q:fp16": _set("q", lambda t: t.half()),
    "q:dim": _set("q", lambda t: t[0]),
    "q:d_head": _set("q", lambda t: t[..., :64]),
    "q:cpu": _set("q", lambda t: t.cpu()),
    "q:strided": _set("q", lambda t: _wide(t, 8)),
    "k_cache:fp16": _set("k_cache", lambda t: t.half()),
    "k_cache:e5m2": _set("k_cache", lambda t: t.to(torch.float8_e5m2)),
    "v_cache:e5m2": _set("v_cache", lambda t: t.to(torch.float8_e5m2)),
    "v_cache:e4m3": _set("v_cache", lambda t: t.to(torch.float8_e4m3fn)),
    "k_cache:dim": _set("k_cache", lambda t: t[0]),
    "v_cache:shape": _set("v_cache", lambda t: t[:, :32]),
    "k_cache:cpu": _set("k_cache", lambda t: t.cpu()),
    "v_cache:cpu": _set("v_cache", lambda t: t.cpu()),
    "k_cache:transposed": _set("k_cache", lambda t: t.transpose(1, 3).contiguous().transpose(1, 3)),
    "v_cache:other strides": _set("v_cache", lambda t: _wide(t, 16)),
    "k_cache:misaligned": _set("k_cache", lambda t: _shifted(t, 4)),
    "caches:row stride +8": _both(lambda t: _wide(t, 8), "k_cache", "v_cache"),
    "caches:row stride +16": _both(lambda t: _wide(t, 16), "k_cache", "v_cache"),
    "k_cache:extra entry": _set("k_cache", _more),
    "cache_seqlens:int64": _set("cache_seqlens", lambda t: t.long()),
    "cache_seqlens:shape": _set("cache_seqlens", lambda t: torch.cat([t, t[:1]])),
    "cache_seqlens:2d": _set("cache_seqlens", lambda t: t[:, None]),
    "cache_seqlens:cpu": _set("cache_seqlens", lambda t: t.cpu()),
    "cache_seqlens:strided": _set("cache_seqlens", lambda t: torch.stack([t, t], 1)[:, 0]),
    "block_table:int64": _set("block_table", lambda t: t.long()),
    "block_table:1d": _set("block_table", lambda t: t[0]),
    "block_table:rows": _set("block_table", lambda t: torch.cat([t, t[:1]])),
    "block_table:transposed": _set("block_table", lambda t: t.t().contiguous().t()),
    "block_table:cpu": _set("block_table", lambda t: t.cpu()),
    "block_table:none": _put(block_table=None),
    "max_seqlen_k:str": _put(max_seqlen_k="64"),
    "max_seqlen_k:float": _put(max_seqlen_k=64.0),
    "max_seqlen_k:bool": _put(max_seqlen_k=True),
    "max_seqlen_k:beyond": _put(max_seqlen_k=4096),
    "max_seqlen_k:negative": _put(max_seqlen_k=-1),
    "max_seqlen_k:128": _put(max_seqlen_k=128),
    "num_splits:-1": _put(num_splits=-1),
    "num_splits:2": _put(num_splits=2),
    "causal": _put(causal=True),
    "descales:16-bit cache": _put(k_descale=_ones, v_descale=_ones),
    "k_descale:none": _put(k_descale=None),
    "descales:none": _put(k_descale=None, v_descale=None),
    "k_descale:fp16": _set("k_descale", lambda t: t.half()),
    "v_descale:shape": _set("v_descale", lambda t: torch.cat([t, t], 1)),
    "k_descale:cpu": _set("k_descale", lambda t: t.cpu()),
    "v_descale:expanded": _set("v_descale", lambda t: t[:1].expand(B, HKV)),
    "k_descale:list": _put(k_descale=[[1.0], [1.0]]),
    "k:dim": _set("k", lambda t: t[0]),
    "k:fp32": _set("k", lambda t: t.float()),
    "v:shape": _set("v", lambda t: t[:, :1]),
    "k:cpu": _set("k", lambda t: t.cpu()),
    "rotary_cos:none": _put(rotary_cos=None),
    "rotary:none": _put(rotary_cos=None, rotary_sin=None),
    "rotary_sin:shape": _set("rotary_sin", lambda t: t[:, :16]),
    "rotary:dim 24": _both(lambda t: t[:, :12], "rotary_cos", "rotary_sin"),
    "seqlens_out:int64": _put(seqlens_out=lambda kw: kw["cache_seqlens"].long()),
    "cu_seqlens_q:int64": _set("cu_seqlens_q", lambda t: t.long()),
    "cu_seqlens_q:one": _set("cu_seqlens_q", lambda t: t[:1]),
    "max_seqlen_q:float": _put(max_seqlen_q=3.0),
    "window:(1,)": _put(window_size=(1,)),
    "window:str": _put(window_size="ab"),
    "window:float": _put(window_size=(1.0, 0)),
    "window:bool": _put(window_size=(True, 0)),
    "window:left -2": _put(window_size=(-2, 0)),
    "window:right -2": _put(window_size=(0, -2)),
    "window:2^31": _put(window_size=(2 ** 31, 0)),
    "window:causal right 5": _put(window_size=(4, 5), causal=True),
    "window:(16,0)": _put(window_size=(16, 0)),
    "window:list (8,8)": _put(window_size=[8, 8]),
    "q:none": _put(q=None),
    "q:list": _put(q=[1.0]),
    "k_cache:none": _put(k_cache=None),
    "v_cache:str": _put(v_cache="v"),
    "cache_seqlens:list": _put(cache_seqlens=[50, 60]),
    "block_table:list": _put(block_table=[[0, 1], [2, 3]]),
    "k:none": _put(k=None),
    "cu_seqlens_q:list": _put(cu_seqlens_q=[0, 2, 5]),
}
PAIRS = (("q:fp32", "k_cache:fp16"), ("q:dim", "k_cache:dim"), ("k_cache:cpu", "cache_seqlens:int64"), ("cache_seqlens:shape", "block_table:int64"),
         ("k_cache:e5m2", "descales:none"), ("v_cache:shape", "cache_seqlens:cpu"), ("k_cache:misaligned", "max_seqlen_k:str"),
         ("block_table:1d", "max_seqlen_k:float"), ("v_cache:other strides", "k_descale:fp16"), ("cache_seqlens:strided", "v_descale:shape"),
         ("q:cpu", "k_cache:transposed"), ("k_cache:extra entry", "cache_seqlens:shape"), ("window:left -2", "q:none"),
         ("k:dim", "k_cache:dim"), ("rotary_cos:none", "k_cache:e5m2"), ("k:fp32", "cache_seqlens:int64"), ("q:fp16", "descales:16-bit cache"),
         ("cu_seqlens_q:int64", "cache_seqlens:int64"), ("max_seqlen_q:float", "block_table:rows"), ("k_descale:none", "k_cache:cpu"))

# what the CPU tier takes: window_size, non-tensors, and the rules that run before any device is asked
CPU_TIER = ("window:(1,)", "window:str", "window:float", "window:bool", "window:left -2", "window:right -2", "window:2^31",
            "window:causal right 5", "window:(16,0)", "window:list (8,8)", "q:none", "q:list", "k_cache:none", "v_cache:str", "cache_seqlens:list",
            "block_table:list", "k:none", "cu_seqlens_q:list", "k_descale:list", "rotary_cos:none", "rotary:none", "k_cache:e5m2", "v_cache:e5m2",
            "v_cache:e4m3", "k_descale:none", "descales:none", "descales:16-bit cache", "k_descale:fp16", "v_descale:shape", "v_descale:expanded")
CPU_PAIRS = (("window:left -2", "q:none"), ("rotary_cos:none", "k_cache:e5m2"), ("k_cache:e5m2", "descales:none"))


def _accepts(fn, names):
    """Does `fn` take what the mutations named act on?  (window_size: the two decode functions; descales: not kvcache_num_splits)"""
    code = getattr(fak, fn).__code__
    params = code.co_varnames[:code.co_argcount]
    return all(k in params for name in names for k in MUTATIONS[name][0] + MUTATIONS[name][1])


def case_ids(tier):
    """-> [(id, function, paged, fp8, mutation names)] of a tier, in a fixed order."""
    singles, pairs = (CPU_TIER, CPU_PAIRS) if tier == "cpu" else (tuple(MUTATIONS), PAIRS)
    out = []
    for fn in FUNCTIONS:
        for paged, fp8 in ((False, False), (True, False), (False, True), (True, True)):
            for names in [(n,) for n in singles] + list(pairs):
                if _accepts(fn, names):
                    out.append((f"{fn}[{'paged' if paged else 'contig'},{'fp8' if fp8 else '16bit'}] {' + '.join(names)}", fn, paged, fp8, names))
            if tier == "gpu":
                out.append((f"{fn}[{'paged' if paged else 'contig'},{'fp8' if fp8 else '16bit'}] valid", fn, paged, fp8, ()))
    return out


def _digest(result, kw):
    """What a call that went through gave, as bits: its tensors (and the caches, which the append writes)."""
    parts = list(result) if isinstance(result, (tuple, list)) else [result]
    parts += [kw["k_cache"], kw["v_cache"]]
    h = hashlib.sha256()
    for p in parts:
        if isinstance(p, torch.Tensor):
            t = p.detach().cpu().contiguous()
            h.update(str((t.dtype, tuple(t.shape))).encode())
            h.update(t.view(torch.uint8).numpy().tobytes())
        else:
            h.update(repr(p).encode())
    return h.hexdigest()


def run_case(device, fn, paged, fp8, names):
    """-> [exception type, message], or ["ok", digest of what came back], or ["n/a", ...] where a mutation has nothing to act on."""
    kw = base(fn, device, paged, fp8)
    for name in names:
        needs, _, mutate = MUTATIONS[name]
        if any(kw.get(k) is None for k in needs):
            return ["n/a", name]
        mutate(kw)
    try:
        result = getattr(fak, fn)(**kw)
    except Exception as e:   # noqa: BLE001 (the type is the record)
        return [type(e).__name__, str(e)]
    return ["ok", _digest(result, kw)]


def collect(tier, device):
    return {cid: run_case(device, fn, paged, fp8, names) for cid, fn, paged, fp8, names in case_ids(tier)}


@pytest.fixture(scope="module")
def recorded():
    with open(RECORDED) as f:
        g = json.load(f)
    return dict(g, cpu={k: g["records"][i] for k, i in g["cpu"].items()}, gpu={k: g["records"][i] for k, i in g["gpu"].items()})


def test_cpu_tier_every_case_as_recorded(recorded):
    got = collect("cpu", "cpu")
    assert len(got) == recorded["n_cpu"] == len(recorded["cpu"])
    wrong = [f"{cid}: recorded {recorded['cpu'].get(cid)}, now {rec}" for cid, rec in got.items() if recorded["cpu"].get(cid) != rec]
    assert not wrong, "\n".join(wrong[:20])
    # nothing on a CPU tensor goes through, and the tier is not one refusal repeated
    assert not any(rec[0] == "ok" for rec in got.values())
    assert len({tuple(rec) for rec in got.values() if rec[0] != "n/a"}) >= 20


if __name__ == "__main__":
    json.dump(collect("cpu", "cpu"), sys.stdout, indent=0)
