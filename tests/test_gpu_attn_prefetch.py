"""Decode attention with prefetch blocks (`attn_dec_pf`).

The prefetching kernel variant shares the attention body with the plain
kernel and adds blocks that only load.  So: every output bit equals the
plain kernel's and the prefetch blocks write nowhere.  The graph-replay
and engine tests are in test_gpu_engine_attn_prefetch.py: they capture
graphs, which takes hardware queues, and test_gpu_comm.py needs one free
queue per simulated rank when it runs, so nothing that sorts ahead of it
may open streams.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NH, KVH, S = 8, 2, 128
POSITIONS = [0, 1, 7, 33, 100]
SPLITS = [1, 2, 4]
PF_BLOCKS = [0, 8, 24]


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def dev():
    return torch.device("cuda:0")


def randn(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


_INPUTS = {}


def inputs(hd, kv8):
    key = (hd, kv8)
    if key in _INPUTS:
        return _INPUTS[key]
    qkv = randn((NH + 2 * KVH) * hd, seed=700 + hd).to(torch.bfloat16)
    kh = randn(KVH, S, hd, seed=701 + hd)
    vh = randn(KVH, S, hd, seed=702 + hd)
    if kv8:
        ks = kh.abs().amax(dim=-1).clamp_min(1e-8) / 448.0
        vs = vh.abs().amax(dim=-1).clamp_min(1e-8) / 448.0
        kc = (kh / ks[..., None]).to(torch.float8_e4m3fn).view(torch.uint8)
        vc = (vh / vs[..., None]).to(torch.float8_e4m3fn).view(torch.uint8)
        pool = (kc.to(dev()), vc.to(dev()), ks.to(dev()), vs.to(dev()))
    else:
        pool = (kh.to(torch.bfloat16).to(dev()),
                vh.to(torch.bfloat16).to(dev()), None, None)
    inv = 1.0 / (10000.0 ** (np.arange(0, hd, 2) / hd))
    fr = np.outer(np.arange(S, dtype=np.float64), inv)
    cos_t = torch.from_numpy(np.cos(fr).astype(np.float32)).to(dev())
    sin_t = torch.from_numpy(np.sin(fr).astype(np.float32)).to(dev())
    _INPUTS[key] = (qkv.to(dev()), pool, cos_t, sin_t)
    return _INPUTS[key]


def weights():
    """A 200 KB + 16 B 'matrix' for the prefetch blocks to walk."""
    if "w" not in _INPUTS:
        _INPUTS["w"] = (torch.arange(200 * 1024 + 16, dtype=torch.int32)
                        % 251).to(torch.uint8).to(dev())
        _INPUTS["sink"] = torch.zeros(256, dtype=torch.float32, device=dev())
    return _INPUTS["w"], _INPUTS["sink"]


def bits(t):
    """Bit pattern of a tensor as a numpy byte array."""
    return t.contiguous().view(torch.uint8).cpu().numpy()


def run(hd, kv8, split, pos0, window, softcap, pf_blocks, scratch, cnt):
    """One launch on a fresh copy of the state; pf_blocks None = the
    plain `attn_dec`.  Returns the bits of (out, K pool, V pool, scales)."""
    from llm_np_cp_amd.ops import hip_ops as ho

    qkv, (kc, vc, ks, vs), cos_t, sin_t = inputs(hd, kv8)
    w, sink = weights()
    pos = torch.tensor([pos0], dtype=torch.int32, device=dev())
    kcx, vcx = kc.clone(), vc.clone()
    ksx = ks.clone() if kv8 else None
    vsx = vs.clone() if kv8 else None
    o = torch.full((NH * hd,), float("nan"), dtype=torch.bfloat16,
                   device=dev())
    kw = dict(softcap=softcap, window=window, split=split, kS=ksx, vS=vsx)
    if pf_blocks is None:
        ho.attn_dec(qkv, kcx, vcx, o, pos, cos_t, sin_t, scratch, cnt,
                    NH, KVH, hd, hd ** -0.5, **kw)
    else:
        # two regions; the first walked by consumer-block class for the
        # larger block count, flat for the smaller
        n0 = 128 * 1024
        regs = [(w.data_ptr(), n0), (w.data_ptr() + n0, w.numel() - n0)]
        ho.attn_dec_pf(qkv, kcx, vcx, o, pos, cos_t, sin_t, scratch, cnt,
                       NH, KVH, hd, hd ** -0.5, regions=regs,
                       pf_blocks=pf_blocks,
                       stride0=4096 if pf_blocks == 24 else 0, sink=sink,
                       **kw)
    torch.cuda.synchronize()
    assert cnt.sum().item() == 0, "ticket counters not re-armed"
    sc = (np.concatenate([bits(ksx), bits(vsx)]) if kv8
          else np.zeros(0, np.uint8))
    return bits(o), bits(kcx), bits(vcx), sc


def check_equal(hd, kv8, split, pos0, window=0, softcap=0.0):
    scratch = torch.zeros(NH * split * (hd + 2), dtype=torch.float32,
                          device=dev())
    cnt = torch.zeros(NH, dtype=torch.int32, device=dev())
    ref = run(hd, kv8, split, pos0, window, softcap, None, scratch, cnt)
    for pfb in PF_BLOCKS:
        # twice in a row on the same scratch / counters, not re-zeroed
        for rep in range(2):
            got = run(hd, kv8, split, pos0, window, softcap, pfb, scratch,
                      cnt)
            for name, a, b in zip(("out", "k pool", "v pool", "scales"),
                                  ref, got):
                assert np.array_equal(a, b), (
                    f"{name} differs: split={split} pos={pos0} "
                    f"pf_blocks={pfb} launch {rep}")


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16kv", "fp8kv"])
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_dec_pf_bits_equal_plain(hd, kv8):
    """out, the whole KV pool and the fp8 scales: bit for bit the plain
    kernel's, for every split x position x prefetch block count."""
    for split in SPLITS:
        for pos0 in POSITIONS:
            check_equal(hd, kv8, split, pos0)


@pytest.mark.parametrize("name,case", [
    ("window", (64, False, 2, 100, 24, 0.0)),
    ("softcap", (128, True, 4, 33, 0, 30.0))])
def test_attn_dec_pf_bits_window_softcap(name, case):
    hd, kv8, split, pos0, window, softcap = case
    check_equal(hd, kv8, split, pos0, window, softcap)


# region lists as (offset into the allocation or None for a null pointer,
# bytes); ALLOC is the allocation's size
ALLOC = (1 << 20) + 8192
REGION_CASES = {
    "zero": [(4096, 0)],
    "one_segment": [(4096, 16)],
    "trip_plus_16": [(4096, 4096 + 16)],
    "not_mult_16": [(4096, 1000)],
    "one_mb": [(4096, 1 << 20)],
    "null_second": [(4096, 4096 + 16), (None, 4096), (8192 + 64, 1000)],
    "four": [(0, 4096 + 16), (16384, 1000), (32768, 1 << 19), (4096, 16)],
    "ends_at_alloc_end": [(ALLOC - 4096 - 16, 4096 + 16)],
    "near_alloc_end_odd": [(4096, 16), (ALLOC - 1008, 1000)],
}


@pytest.mark.parametrize("case", sorted(REGION_CASES))
def test_attn_dec_pf_writes_nothing(case):
    """The regions sit inside a patterned allocation: after the launch
    the allocation and the sink hold the same bits as before.  (An
    out-of-range *read* is not detectable here; the kernel clamps every
    segment index to the region, see `attn_pf_trip`.)"""
    from llm_np_cp_amd.ops import hip_ops as ho

    hd, split = 64, 2
    qkv, (kc, vc, _, _), cos_t, sin_t = inputs(hd, False)
    pattern = (torch.arange(ALLOC, dtype=torch.int32) % 253).to(torch.uint8)
    buf = pattern.to(dev())
    assert buf.data_ptr() % 16 == 0
    sink = torch.full((256,), 3.25, dtype=torch.float32, device=dev())
    scratch = torch.zeros(NH * split * (hd + 2), dtype=torch.float32,
                          device=dev())
    cnt = torch.zeros(NH, dtype=torch.int32, device=dev())
    pos = torch.tensor([33], dtype=torch.int32, device=dev())
    regs = [(0, n) if off is None else (buf.data_ptr() + off, n)
            for off, n in REGION_CASES[case]]
    for stride0, pfb in ((0, 24), (4096, 24), (2048, 8)):
        o = torch.empty(NH * hd, dtype=torch.bfloat16, device=dev())
        ho.attn_dec_pf(qkv, kc.clone(), vc.clone(), o, pos, cos_t, sin_t,
                       scratch, cnt, NH, KVH, hd, hd ** -0.5, split=split,
                       regions=regs, pf_blocks=pfb, stride0=stride0,
                       sink=sink)
        torch.cuda.synchronize()
        assert torch.equal(buf.cpu(), pattern), (stride0, pfb)
        assert (sink == 3.25).all().item()
        assert cnt.sum().item() == 0
