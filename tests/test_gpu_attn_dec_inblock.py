"""Decode attention, in-block split merge against the ticket merge.

`attn_dec(merge="block")` runs one block of 256 * split threads per head
and merges the chunk partials through LDS; `merge="ticket"` runs one
256-thread block per chunk and merges through global scratch behind a
ticket.  Both run the same chunk and merge source, so everything they
write must agree bit for bit: `out`, the pool row at `pos`, and (fp8
pool) that row's scales.  The ticket form's bits are pinned to a recorded
run by test_gpu_attn_dec_bits.py.

nh 4 / kvh 2: heads 0 and 2 are the first q-heads of their kv-heads and
write the pool.  Positions cover every chunk empty (0), only chunk 0
non-empty (1, and 2 for split >= 3), chunks of unequal length, and
several scan iterations per wave.  The block form never touches
`scratch` or `cnt`: they go in NaN / sentinel filled and must come back
byte-identical.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NH, KVH, S = 4, 2, 128
HDS = [64, 128, 256]
SPLITS = [2, 3, 4]
POSITIONS = [0, 1, 2, 7, 8, 9, 31, 32, 33, 100]
SENTINEL = 0x5A5A5A5


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def dev():
    return torch.device("cuda:0")


def randn(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def bits(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


_INPUTS = {}
BMAX = 3


def inputs(hd, kv8):
    """BMAX rows of qkv, full S-position pools (+ scales) and the RoPE
    tables: made once per (hd, kv8), cloned before every call."""
    key = (hd, kv8)
    if key in _INPUTS:
        return _INPUTS[key]
    qkv = randn(BMAX, (NH + 2 * KVH) * hd, seed=700 + hd).to(torch.bfloat16)
    kh = randn(BMAX, KVH, S, hd, seed=701 + hd)
    vh = randn(BMAX, KVH, S, hd, seed=702 + hd)
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


def run(hd, kv8, split, positions, merge, window=0, softcap=0.0, pf=False,
        calls=1):
    """`calls` launches in a row on fresh copies of the state, one batch
    row per entry of `positions`.  Returns the bits of (out, the pool
    rows at each row's position, their scales) of the last launch, after
    checking that every launch gave the same."""
    from llm_np_cp_amd.ops import hip_ops as ho

    B = len(positions)
    qkv, (kc, vc, ks, vs), cos_t, sin_t = inputs(hd, kv8)
    pos = torch.tensor(positions, dtype=torch.int32, device=dev())
    n = B * NH * split * (hd + 2)
    if merge == "block":
        scratch = torch.full((n,), float("nan"), dtype=torch.float32,
                             device=dev())
        cnt = torch.full((B * NH,), SENTINEL, dtype=torch.int32, device=dev())
    else:
        scratch = torch.zeros(n, dtype=torch.float32, device=dev())
        cnt = torch.zeros(B * NH, dtype=torch.int32, device=dev())
    scratch0, cnt0 = bits(scratch), bits(cnt)
    got = []
    for _ in range(calls):
        kcx, vcx = kc[:B].clone(), vc[:B].clone()
        ksx = ks[:B].clone() if kv8 else None
        vsx = vs[:B].clone() if kv8 else None
        o = torch.full((B, NH * hd), float("nan"), dtype=torch.bfloat16,
                       device=dev())
        kw = dict(softcap=softcap, window=window, split=split, kS=ksx,
                  vS=vsx, batch=B, merge=merge)
        if pf:
            w = torch.arange(96 * 1024 + 16, dtype=torch.int32) % 251
            w = w.to(torch.uint8).to(dev())
            sink = torch.zeros(256, dtype=torch.float32, device=dev())
            ho.attn_dec_pf(qkv[:B], kcx, vcx, o, pos, cos_t, sin_t, scratch,
                           cnt, NH, KVH, hd, hd ** -0.5,
                           regions=[(w.data_ptr(), w.numel())], pf_blocks=4,
                           stride0=0, sink=sink, **kw)
        else:
            ho.attn_dec(qkv[:B], kcx, vcx, o, pos, cos_t, sin_t, scratch,
                        cnt, NH, KVH, hd, hd ** -0.5, **kw)
        torch.cuda.synchronize()
        if merge == "block":
            assert np.array_equal(bits(scratch), scratch0), "scratch touched"
            assert np.array_equal(bits(cnt), cnt0), "cnt touched"
        else:
            assert cnt.sum().item() == 0, "ticket counters not re-armed"
        rows = [torch.stack([kcx[b, :, p], vcx[b, :, p]])
                for b, p in enumerate(positions)]
        sc = ([torch.stack([ksx[b, :, p], vsx[b, :, p]])
               for b, p in enumerate(positions)] if kv8 else [])
        got.append((bits(o), bits(torch.stack(rows)),
                    bits(torch.stack(sc)) if kv8 else np.zeros(0, np.uint8)))
    for g in got[1:]:
        for a, b in zip(got[0], g):
            assert np.array_equal(a, b), "a repeated call differs"
    assert not np.isnan(
        torch.from_numpy(got[-1][0].copy()).view(torch.bfloat16).float()
        .numpy()).any(), "out not fully written"
    return got[-1]


def check_equal(hd, kv8, split, positions, **kw):
    blk = run(hd, kv8, split, positions, "block", calls=2, **kw)
    tic = run(hd, kv8, split, positions, "ticket", **kw)
    for name, a, b in zip(("out", "pool row", "scales"), blk, tic):
        assert np.array_equal(a, b), (
            f"{name}: hd {hd} fp8 {kv8} split {split} pos {positions} {kw}")


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("hd", HDS)
def test_block_equals_ticket_grid(hd, kv8):
    for split in SPLITS:
        for pos0 in POSITIONS:
            check_equal(hd, kv8, split, [pos0])


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("hd", HDS)
def test_block_equals_ticket_window_softcap(hd, kv8):
    for split in SPLITS:
        check_equal(hd, kv8, split, [100], window=24)
        check_equal(hd, kv8, split, [33], softcap=30.0)


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("hd", HDS)
def test_block_equals_ticket_ragged_batch(hd, kv8):
    for split in SPLITS:
        check_equal(hd, kv8, split, [0, 9, 100])


def test_block_rejects_split_8():
    with pytest.raises(RuntimeError):
        run(64, False, 8, [100], "block")
    with pytest.raises(ValueError):
        run(64, False, 2, [100], "lds")


def test_auto_split_8_is_ticket():
    """split 8 does not fit a block: "auto" launches the ticket kernels
    (it re-arms the zeroed counters, which `run` checks)."""
    auto = run(64, False, 8, [100], "auto")
    tic = run(64, False, 8, [100], "ticket")
    for a, b in zip(auto, tic):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
def test_prefetch_block_equals_plain_ticket(kv8):
    """`attn_dec_pf` (split 2, one small region, 4 prefetch blocks) in
    the block form and by default against plain ticket `attn_dec`."""
    for pos0 in (0, 9, 100):
        tic = run(64, kv8, 2, [pos0], "ticket")
        for merge in ("block", "auto"):
            got = run(64, kv8, 2, [pos0], merge, pf=True)
            for a, b in zip(got, tic):
                assert np.array_equal(a, b), (merge, pos0)
