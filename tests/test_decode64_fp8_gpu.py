"""KV-cache decode at d_head = 64 against an fp8 (e4m3fn) cache: forward_kvcache_d64 with descales against
tests/test_decode64_gpu.py's eager attention on the DEQUANTIZED cache (values about N(0, 1), descales near 1 / 100), fp32 and 16-bit:
quantization error enters no bar.  The pass rule is beacon_inputs.compare unchanged; rows that see no key are exact."""
import ctypes
import functools

import pytest
import torch

import beacon_inputs as bi
import flash_attention as fa
from flash_attention_from_scratch_amd import _capi
from flash_attention_from_scratch_amd import flash_attention_kernels as fak
from tests.test_decode64_gpu import LENS, WINDOWS, Z, eager

pytestmark = pytest.mark.gpu
DEV, D, H, HKV, CACHE, F8 = "cuda:0", 64, 8, 2, bi.WINDOW_CACHE_LEN, torch.float8_e4m3fn
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
ARMS = [("32", "1"), ("32", "2"), ("64", "1")]   # (FA_DECODE64_UNIT, FA_DECODE64_AHEAD): every instantiated form
NAN_CODE = 0x7F
_i32 = functools.partial(torch.tensor, dtype=torch.int32, device=DEV)


def _same(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _inputs(dtype, scaled=True):
    """-> q * 3, dequantized fp32 k, v (CPU); caches name -> (k8, v8, kwargs) as in the 16-bit test, " nan": the NaN byte; q, descales (device)"""
    gen, B = torch.Generator().manual_seed(6408), len(LENS)
    q = (torch.randn((B, 16, H, D), generator=gen) * 3).to(dtype)
    ds = [(c * (0.75 + 0.5 * torch.rand((B, HKV), generator=gen))).float() if scaled else torch.ones((B, HKV)) for c in (0.011, 0.013)]
    assert not scaled or all(bool((torch.frexp(d)[0] != 0.5).all()) and d.unique().numel() == d.numel() for d in ds)   # no power of two, distinct
    x8 = [(torch.randn((B, CACHE, HKV, D), generator=gen) / d[:, None, :, None]).clamp(-448.0, 448.0).to(F8) for d in ds]
    assert not any(bool(((x.view(torch.uint8) & 0x7F) == NAN_CODE).any()) for x in x8)
    deq = [x.float() * d[:, None, :, None] for x, d in zip(x8, ds)]
    caches = {}
    for tag, fill in (("", 0), (" nan", NAN_CODE)):
        kv = [x.view(torch.uint8).clone() for x in x8]
        for b, n in enumerate(LENS if tag else []):
            kv[0][b, n:], kv[1][b, n:] = fill, fill
        caches["contiguous" + tag] = (kv[0].view(F8).to(DEV), kv[1].view(F8).to(DEV), {})
        for page in (64, 256):
            n = CACHE // page
            table = torch.randperm(B * n + 3, generator=gen)[:B * n]
            pages = [torch.full((B * n + 3, page, HKV, D), fill, dtype=torch.uint8).index_copy_(0, table, t.view(B * n, page, HKV, D)) for t in kv]
            caches[f"pages of {page}{tag}"] = (pages[0].view(F8).to(DEV), pages[1].view(F8).to(DEV), dict(block_table=table.view(B, n).to(torch.int32).to(DEV)))
    return q, deq[0], deq[1], caches, q.to(DEV), ds[0].to(DEV), ds[1].to(DEV)


@functools.lru_cache(maxsize=None)
def _refs(dtype, Sq, window, sunk, scaled=True):
    q, k, v = _inputs(dtype, scaled)[:3]
    entries = [(q[b, :Sq], k[b, :n], v[b, :n], Z if sunk else None, window) for b, n in enumerate(LENS)]
    return [eager(*e, torch.float32) + eager(*e, dtype)[:1] for e in entries]


def _run(dtype, Sq, cache, window, z, scaled=True, **kw):
    (kc, vc, more), lens = _inputs(dtype, scaled)[3][cache], kw.pop("lens", None)
    kd, vd = kw.pop("descales", _inputs(dtype, scaled)[5:7])
    return fa.forward_kvcache_d64(_inputs(dtype, scaled)[4][:, :Sq], kc, vc, _i32(LENS) if lens is None else lens, z, return_lse=True,
                                  window_size=window[:2], causal=window[2], k_descale=kd, v_descale=vd, **more, **kw)


def _check(got, dtype, Sq, window, sunk, scaled, tag):
    o, lse = got
    for b, (o32, lse32, o16) in enumerate(_refs(dtype, Sq, window, sunk, scaled)):
        res = bi.compare(o[b].cpu(), lse[b].cpu(), o32, lse32, o16, dtype)
        assert res["ok"], (tag, b, res)
        lo, hi = bi.window_bounds(Sq, LENS[b], *bi.window_sides(*window))
        want = Z[:, None] if sunk else torch.full((H, 1), bi.NEG_INF)
        assert bool((o[b].cpu()[hi < lo] == 0).all()) and torch.equal(lse[b].cpu()[:, hi < lo], want.expand(-1, int((hi < lo).sum()))), (tag, b)


@DTYPES
@pytest.mark.parametrize("Sq", [1, 5, 16])
@pytest.mark.parametrize("sunk", [False, True], ids=["plain", "sinks"])
@pytest.mark.parametrize("arm", ARMS, ids=["u32a1", "u32a2", "u64a1"])
def test_parity_every_split_count_and_the_bit_identities(dtype, Sq, sunk, arm, monkeypatch):
    """Every form, NT 1 / 2 / 4; per window and split count: the rule, dead rows exact, lse across splits, the same bits from every cache"""
    monkeypatch.setenv("FA_DECODE64_UNIT", arm[0]), monkeypatch.setenv("FA_DECODE64_AHEAD", arm[1])
    z = Z.to(DEV) if sunk else None
    for window in WINDOWS:
        one = None
        for ns in (1, 3, 16, 0):
            o, lse = _run(dtype, Sq, "contiguous", window, z, num_splits=ns)
            _check((o, lse), dtype, Sq, window, sunk, True, (window, ns))
            one = lse if one is None else one
            assert float(((lse - one).abs() / one.abs().clamp_min(1.0)).nan_to_num(0.0).max()) <= 1e-5, (window, ns)
            for cache in _inputs(dtype)[3]:
                assert _same((o, lse), _run(dtype, Sq, cache, window, z, num_splits=ns)), (window, ns, cache)


@DTYPES
def test_unit_descales_and_null_pointers_give_the_bits_of_ones(dtype):
    window, Sq, z, lib = (100, -1, True), 5, Z.to(DEV), _capi.load()
    (kc, vc, _), lens = _inputs(dtype, False)[3]["contiguous"], _i32(LENS)
    for ns in (1, 3):
        got = _run(dtype, Sq, "contiguous", window, z, scaled=False, num_splits=ns)
        _check(got, dtype, Sq, window, True, False, ns)
        q, args, w, sk, _ = fak._decode_d64_args(_inputs(dtype, False)[4][:, :Sq], kc, vc, lens, z, None, True, None, ns, window[:2],
                                                 *_inputs(dtype, False)[5:7])
        o, lse = torch.empty_like(got[0]), torch.empty_like(got[1])
        more = (ctypes.byref(w), ctypes.byref(sk))
        ws = torch.empty(max(lib.fa_decode_fp8_d64_workspace_bytes(ctypes.byref(args), *more), 16), dtype=torch.uint8, device=DEV)
        args.o, args.lse, args.workspace, args.k_descale, args.v_descale = o.data_ptr(), lse.data_ptr(), ws.data_ptr(), None, None
        _capi.check(lib.fa_decode_fp8_d64_launch(ctypes.byref(args), *more, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), None))
        torch.cuda.synchronize()
        assert _same(got, (o, lse)), ns


def test_a_captured_graph_sees_lengths_sinks_and_descales_rewritten_in_place():
    dtype, window = torch.bfloat16, (-1, -1, True)
    lens, z, kd, vd = _i32(LENS), Z.to(DEV), _inputs(dtype)[5].clone(), _inputs(dtype)[6].clone()
    kc, vc, more = _inputs(dtype)[3]["pages of 256"]
    assert fa.kvcache_d64_num_splits(_inputs(dtype)[4][:, :5], kc, vc, lens, z, causal=True, k_descale=kd, v_descale=vd, **more) == 16
    step = lambda: _run(dtype, 5, "pages of 256", window, z, lens=lens, descales=(kd, vd))   # noqa: E731
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()   # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    kd0, vd0 = kd.clone(), vd.clone()
    for new_lens, new_z, f in ((LENS, Z, 1.0), (LENS[::-1], Z + 1.0, 1.5), ([n // 2 for n in LENS], Z.flip(0), 0.7), (LENS, Z, 1.0)):
        lens.copy_(_i32(new_lens)), z.copy_(new_z), kd.copy_(kd0 * f), vd.copy_(vd0.flip(0) * f)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(got, step()), new_lens
