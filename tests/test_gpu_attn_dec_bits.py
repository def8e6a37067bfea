"""Fused decode attention (`attn_dec`): bits pinned to a recorded run.

`k_attn_dec_t` issues its first K/V history loads ahead of the RoPE
arithmetic and the pool write.  That moves loads, not arithmetic, so the
outputs must stay what they were bit for bit: `out`, the pool row
written at `pos`, and (fp8 pool) the row's scales are compared with
`tests/golden/attn_dec_bits.npz`, recorded from the build of the commit
before that change on the same seeded inputs:

    python tests/test_gpu_attn_dec_bits.py --record

Every case is also checked against the unfused rope_cache + attn chain
(fp8 pool: the chain over the dequantized history, see `unfused`) with
the tolerance of test_attn_dec_fused_matches_unfused, and runs
twice on the same scratch and ticket counters (they must re-arm).

History lengths: empty, one partial iteration, exact and +-1 around the
8-position (hd 64: one wave iteration) and 32-position (all four waves)
strides, and several iterations per wave.
"""

import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "attn_dec_bits.npz")
NH, KVH, S = 2, 1, 128
HDS = [64, 128]
SPLITS = [1, 2, 4]
POSITIONS = [0, 1, 7, 8, 9, 31, 32, 33, 100]
# name -> (hd, kv8, split, pos, window, softcap)
EXTRA = {"window": (64, False, 2, 100, 24, 0.0),
         "window_fp8": (128, True, 4, 33, 8, 0.0),
         "softcap": (128, False, 4, 100, 0, 50.0),
         "softcap_fp8": (64, True, 1, 33, 0, 30.0)}


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
    """qkv, a full S-position history pool (+ scales) and the RoPE
    tables: made once per (hd, kv8), cloned before every call."""
    key = (hd, kv8)
    if key in _INPUTS:
        return _INPUTS[key]
    qkv = randn((NH + 2 * KVH) * hd, seed=900 + hd).to(torch.bfloat16)
    kh = randn(KVH, S, hd, seed=901 + hd)
    vh = randn(KVH, S, hd, seed=902 + hd)
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


def fused(hd, kv8, split, pos0, window=0, softcap=0.0):
    """Two calls in a row on the same scratch / counters.  Returns, as
    numpy bit patterns, (out, pool rows [2, KVH*hd], scales [2, KVH])
    of the second call, after checking the first gave the same."""
    from llm_np_cp_amd.ops import hip_ops as ho

    qkv, (kc, vc, ks, vs), cos_t, sin_t = inputs(hd, kv8)
    pos = torch.tensor([pos0], dtype=torch.int32, device=dev())
    scratch = torch.zeros(NH * split * (hd + 2), dtype=torch.float32,
                          device=dev())
    cnt = torch.zeros(NH, dtype=torch.int32, device=dev())
    got = []
    for _ in range(2):
        kcx, vcx = kc.clone(), vc.clone()
        ksx = ks.clone() if kv8 else None
        vsx = vs.clone() if kv8 else None
        o = torch.full((NH * hd,), float("nan"), dtype=torch.bfloat16,
                       device=dev())
        ho.attn_dec(qkv, kcx, vcx, o, pos, cos_t, sin_t, scratch, cnt,
                    NH, KVH, hd, hd ** -0.5, softcap=softcap, window=window,
                    split=split, kS=ksx, vS=vsx)
        torch.cuda.synchronize()
        assert cnt.sum().item() == 0, "ticket counters not re-armed"
        rows = torch.stack([kcx[:, pos0].reshape(-1), vcx[:, pos0].reshape(-1)])
        rows = rows.view(torch.uint8 if kv8 else torch.int16).cpu().numpy()
        sc = (torch.stack([ksx[:, pos0], vsx[:, pos0]]).cpu().numpy()
              if kv8 else np.zeros((2, KVH), np.float32))
        got.append((o.view(torch.int16).cpu().numpy(), rows, sc, o))
    assert np.array_equal(got[0][0], got[1][0]), "second call differs"
    assert np.array_equal(got[0][1], got[1][1])
    assert np.array_equal(got[0][2].view(np.int32), got[1][2].view(np.int32))
    return got[1]


def unfused(hd, kv8, pos0, window=0, softcap=0.0):
    """The unfused rope_cache + attn chain on the same history.

    fp8 pool: the chain runs on the pool's DEQUANTIZED history, held in
    bf16 (an e4m3 value times its scale has 4 significant bits; rounding
    it to bf16 costs at most 2^-9 relative).  That is the function
    `attn_dec` computes — fp8 history, the new token from registers,
    unquantized.  The chain's own fp8 mode is a different function: it
    quantizes the new token's k/v to e4m3 before attending it, an error
    of up to 2^-4 = 6 % per element, three times the tolerance used
    here, and at pos 0 (out = v) all of it shows: measured against that
    mode, max |diff| was .102 / .078 / .023 (hd 64) and .094 / .094 /
    .032 (hd 128) at pos 0 / 1 / 7, the fused kernel returning v itself
    and the chain v's e4m3 rounding.  A reference that far from the
    exact result cannot check anything at 2e-2."""
    from llm_np_cp_amd.ops import hip_ops as ho

    qkv, (kc, vc, ks, vs), cos_t, sin_t = inputs(hd, kv8)
    pos = torch.tensor([pos0], dtype=torch.int32, device=dev())
    if kv8:
        def deq(c, s):  # on the CPU: plain e4m3fn -> fp32 conversion
            return (c.cpu().view(torch.float8_e4m3fn).float()
                    * s.cpu()[..., None]).to(torch.bfloat16).to(dev())
        kcx, vcx = deq(kc, ks), deq(vc, vs)
    else:
        kcx, vcx = kc.clone(), vc.clone()
    q = qkv[:NH * hd].clone()
    k = qkv[NH * hd:(NH + KVH) * hd].clone()
    v = qkv[(NH + KVH) * hd:].clone()
    ho.rope_cache(q, k, v, kcx, vcx, cos_t, sin_t, pos, 1, NH, KVH, hd)
    out = torch.empty(NH * hd, dtype=torch.bfloat16, device=dev())
    ho.attn(q, kcx, vcx, out, pos, 1, NH, KVH, hd, hd ** -0.5,
            softcap=softcap, window=window)
    torch.cuda.synchronize()
    return out, kcx[:, pos0], vcx[:, pos0]


def check_fp8_row(hd, pos0, rows_b, sc):
    """The e4m3 row and scales written at `pos` against a computed
    reference: the new token's k (RoPE'd in fp32 on the CPU) and v.

    scale = max(absmax, 1e-8) / 448 per kv head: fp32 arithmetic on both
    sides, a few roundings apart -> rtol 1e-5.  Each byte, dequantized
    with the kernel's scale, must be the correctly rounded e4m3 of the
    exact value: within half a spacing, i.e. 2^-4 of the value for
    normals and 2^-10 (in scaled units) for subnormals; 1 % slack for
    the fp32 differences in the RoPE and the reciprocal multiply."""
    qkv, _, cos_t, sin_t = inputs(hd, True)
    f = qkv.float().cpu()
    k = f[NH * hd:(NH + KVH) * hd].view(KVH, hd)
    v = f[(NH + KVH) * hd:].view(KVH, hd)
    c, s = cos_t[pos0].cpu(), sin_t[pos0].cpu()
    lo, hi = k[:, :hd // 2], k[:, hd // 2:]
    kr = torch.cat([lo * c - hi * s, hi * c + lo * s], dim=1)
    for i, exact in enumerate((kr, v)):
        scale = torch.from_numpy(sc[i].copy())
        ref_scale = exact.abs().amax(dim=1).clamp_min(1e-8) / 448.0
        torch.testing.assert_close(scale, ref_scale, rtol=1e-5, atol=0.0)
        deq = (torch.from_numpy(rows_b[i].copy()).view(torch.float8_e4m3fn)
               .float().view(KVH, hd) * scale[:, None])
        bound = 1.01 * torch.maximum(exact.abs() * 2.0 ** -4,
                                     scale[:, None] * 2.0 ** -10)
        err = (deq - exact).abs()
        assert (err <= bound).all(), (
            f"fp8 row {'kv'[i]} hd {hd} pos {pos0}: "
            f"{(err > bound).sum().item()} elements off, worst "
            f"{(err / bound).max().item():.2f} x the half spacing")


def assert_close(got, ref, rtol=2e-2, atol=2e-2):
    torch.testing.assert_close(got.float().cpu(), ref.float().cpu(),
                               rtol=rtol, atol=atol)


def check_case(gold, name, hd, kv8, split, pos0, window=0, softcap=0.0,
               with_ref=True):
    out_b, rows_b, sc, o = fused(hd, kv8, split, pos0, window, softcap)
    if with_ref:
        ref, kref, vref = unfused(hd, kv8, pos0, window, softcap)
        d = (o.float() - ref.float()).abs()
        print(f"{name}: vs unfused max abs {d.max().item():.4f} max rel "
              f"{(d / ref.float().abs().clamp_min(1e-3)).max().item():.4f}")
        assert_close(o, ref)
        if not kv8:
            rows = torch.from_numpy(rows_b).view(torch.bfloat16)
            assert_close(rows[0], kref.reshape(-1))
            assert_close(rows[1], vref.reshape(-1))
    assert np.array_equal(out_b, gold["out_" + name]), f"out bits: {name}"
    assert np.array_equal(rows_b, gold["rows_" + name]), f"pool row: {name}"
    if kv8:
        assert np.array_equal(sc.view(np.int32),
                              gold["scales_" + name].view(np.int32)), name
        check_fp8_row(hd, pos0, rows_b, sc)


def grid_name(hd, kv8, split, pos0):
    return f"{hd}_{'fp8' if kv8 else 'bf16'}_s{split}_p{pos0}"


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLDEN)
    packed = {k: g[k] for k in g.files}
    out = {}
    # the grid is stored packed: one array per (hd, dtype) and kind
    for hd in HDS:
        for kv8 in (False, True):
            tag = f"{hd}_{'fp8' if kv8 else 'bf16'}"
            for si, split in enumerate(SPLITS):
                for pi, pos0 in enumerate(POSITIONS):
                    n = grid_name(hd, kv8, split, pos0)
                    out["out_" + n] = packed["out_" + tag][si, pi]
                    out["rows_" + n] = packed["rows_" + tag][si, pi]
                    out["scales_" + n] = packed["scales_" + tag][si, pi]
    for n in EXTRA:
        for kind in ("out_", "rows_", "scales_"):
            out[kind + n] = packed[kind + n]
    return out


@pytest.mark.parametrize("kv8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("hd", HDS)
def test_attn_dec_bits_grid(gold, hd, kv8):
    """Recorded bits for the whole grid; bf16 also against the unfused
    chain (fp8 against it: test_attn_dec_fp8_vs_unfused)."""
    for split in SPLITS:
        for pos0 in POSITIONS:
            check_case(gold, grid_name(hd, kv8, split, pos0), hd, kv8,
                       split, pos0, with_ref=not kv8)


@pytest.mark.parametrize("pos0", POSITIONS)
@pytest.mark.parametrize("hd", HDS)
def test_attn_dec_fp8_vs_unfused(hd, pos0):
    """fp8 pool against the unfused chain over the dequantized history
    (see `unfused`), at the bf16 test's tolerance (rtol = atol = 2e-2),
    every split."""
    for split in SPLITS:
        _, _, _, o = fused(hd, True, split, pos0)
        ref, _, _ = unfused(hd, True, pos0)
        d = (o.float() - ref.float()).abs()
        print(f"hd {hd} pos {pos0} split {split}: max abs "
              f"{d.max().item():.4f}")
        assert_close(o, ref)


@pytest.mark.parametrize("name", sorted(EXTRA))
def test_attn_dec_bits_window_softcap(gold, name):
    hd, kv8, split, pos0, window, softcap = EXTRA[name]
    check_case(gold, name, hd, kv8, split, pos0, window, softcap)


def record(path=GOLDEN, lib=None):
    """Writes the golden file from the build in the tree (or `lib`)."""
    if lib:
        from llm_np_cp_amd.ops import hip_ops as ho
        ho._LIB_PATH = os.path.abspath(lib)
    packed = {}
    for hd in HDS:
        for kv8 in (False, True):
            tag = f"{hd}_{'fp8' if kv8 else 'bf16'}"
            outs, rows, scs = [], [], []
            for split in SPLITS:
                for pos0 in POSITIONS:
                    o, r, s, _ = fused(hd, kv8, split, pos0)
                    outs.append(o), rows.append(r), scs.append(s)
            shp = (len(SPLITS), len(POSITIONS))
            packed["out_" + tag] = np.stack(outs).reshape(shp + (-1,))
            packed["rows_" + tag] = np.stack(rows).reshape(shp + (2, -1))
            packed["scales_" + tag] = np.stack(scs).reshape(shp + (2, -1))
    for n, (hd, kv8, split, pos0, window, softcap) in EXTRA.items():
        o, r, s, _ = fused(hd, kv8, split, pos0, window, softcap)
        packed["out_" + n], packed["rows_" + n] = o, r
        packed["scales_" + n] = s
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **packed)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    # --record [--out FILE] [--lib BUILT_LIBRARY]
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    args = sys.argv[1:]
    opt = {a: args[i + 1] for i, a in enumerate(args)
           if a in ("--out", "--lib")}
    if "--record" in args:
        record(opt.get("--out", GOLDEN), opt.get("--lib"))
