"""`ho.attn_verify` (k_attn_verify + merge) against a float64 reference,
`rope_cache`'s pool bits, and its own bits property (1 GPU)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S = 128  # pool capacity: 4 chunks of 32


@pytest.fixture(scope="module", autouse=True)
def _build():
    from csrc.build import ensure_built
    ensure_built()


def dev():
    return torch.device("cuda:0")


# hd, fp8 KV, nh, kvh, window, softcap, n, R, chunk (0 = the S rule)
CASES = [
    (64, False, 4, 1, 0, 0.0, 0, 7, 32),      # causal triangle only
    (128, False, 7, 1, 0, 0.0, 5, 16, 32),    # new rows straddle a 16-tile
    (256, False, 2, 2, 8, 0.0, 29, 5, 32),    # ... and a chunk
    (128, False, 4, 1, 8, 0.0, 70, 9, 32),    # chunk 0 dead, still writes
    (64, False, 4, 1, 0, 50.0, 70, 9, 0),     # several chunks, last partial
    (128, True, 4, 1, 0, 50.0, 70, 9, 32),
    (64, True, 7, 1, 8, 0.0, 29, 5, 32),
    (256, True, 2, 2, 0, 0.0, 5, 16, 0),
    (128, True, 2, 2, 0, 0.0, 70, 1, 32),     # R = 1
    (256, False, 7, 1, 0, 0.0, 0, 1, 32),
]


class Rig:
    """Inputs of one case: tables, qkv rows, and a pool whose history
    [0, n) was written by `rope_cache` and whose other slots hold NaN."""

    def __init__(self, hd, kv8, nh, kvh, n, R, seed=0):
        from llm_np_cp_amd.ops import hip_ops as ho
        self.ho, self.hd, self.kv8, self.nh, self.kvh = ho, hd, kv8, nh, kvh
        g = torch.Generator().manual_seed(1000 + seed)
        ang = torch.arange(S, dtype=torch.float64)[:, None] * \
            (10000.0 ** (-torch.arange(hd // 2, dtype=torch.float64)
                         / (hd // 2)))[None]
        self.cos, self.sin = (f(ang).float().to(dev())
                              for f in (torch.cos, torch.sin))
        w = (nh + 2 * kvh) * hd
        rows = torch.randn(n + R, w, generator=g).to(dev(), torch.bfloat16)
        self.qkv = rows[n:].contiguous()
        if kv8:
            self.pool = [torch.full((kvh, S, hd), 0x7f, dtype=torch.uint8,
                                    device=dev()) for _ in range(2)] + \
                [torch.full((kvh, S), float("nan"), device=dev())
                 for _ in range(2)]
        else:
            self.pool = [torch.full((kvh, S, hd), float("nan"),
                                    dtype=torch.bfloat16, device=dev())
                         for _ in range(2)]
        if n:
            self.rope_cache(self.pool, rows[:n], 0)

    def split(self, rows):
        a, b = self.nh * self.hd, (self.nh + self.kvh) * self.hd
        return (rows[:, :a].contiguous(), rows[:, a:b].contiguous(),
                rows[:, b:].contiguous())

    def rope_cache(self, pool, rows, n):
        """The existing pair's first half; returns the roped q."""
        q, k, v = self.split(rows)
        pos = torch.tensor([n], dtype=torch.int32, device=dev())
        self.ho.rope_cache(q, k, v, pool[0], pool[1], self.cos, self.sin, pos,
                           rows.shape[0], self.nh, self.kvh, self.hd,
                           **self.scales(pool))
        return q

    @staticmethod
    def scales(pool):
        return dict(kS=pool[2], vS=pool[3]) if len(pool) == 4 else {}

    def verify(self, pool, rows, n, window=0, cap=0.0, chunk=32):
        ho, R = self.ho, rows.shape[0]
        ck = chunk or ho.attn_verify_chunk(S)
        scratch = torch.full(
            (ho.attn_verify_scratch_words(R, self.nh, self.hd, S, ck),),
            float("nan"), device=dev())
        out = torch.zeros(R, self.nh * self.hd, dtype=torch.bfloat16,
                          device=dev())
        ln = torch.tensor([n], dtype=torch.int32, device=dev())
        ho.attn_verify(rows, pool[0], pool[1], out, ln, self.cos, self.sin,
                       scratch, R, self.nh, self.kvh, self.hd,
                       self.hd ** -0.5, softcap=cap, window=window,
                       chunk=chunk, **self.scales(pool))
        torch.cuda.synchronize()
        assert int(ln.item()) == n
        return out


def bits(t):
    return t.contiguous().view(torch.uint8).cpu()


def reference(rig, pool, n, R, window, cap):
    """float64: RoPE of the bf16 q, the pool's values below n + R."""
    hd, nh, kvh = rig.hd, rig.nh, rig.kvh
    T = n + R
    if rig.kv8:
        K, V = (p[:, :T].view(torch.float8_e4m3fn).double().cpu()
                * s[:, :T, None].double().cpu()
                for p, s in ((pool[0], pool[2]), (pool[1], pool[3])))
    else:
        K, V = pool[0][:, :T].double().cpu(), pool[1][:, :T].double().cpu()
    c = rig.cos[n:T].double().cpu()[:, None]
    s = rig.sin[n:T].double().cpu()[:, None]

    def rope(x):
        x1, x2 = x[..., :hd // 2], x[..., hd // 2:]
        return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    q, k, v = (t.double().cpu().view(R, -1, hd) for t in rig.split(rig.qkv))
    q = rope(q)
    if not rig.kv8:  # bf16 pool: the new rows from the inputs themselves
        K[:, n:], V[:, n:] = rope(k).transpose(0, 1), v.transpose(0, 1)
    ref = torch.empty(R, nh, hd, dtype=torch.float64)
    for r in range(R):
        lo = max(0, n + r + 1 - window) if window else 0
        for h in range(nh):
            kv = h // (nh // kvh)
            sc = (K[kv, lo:n + r + 1] @ q[r, h]) * hd ** -0.5
            if cap:
                sc = cap * torch.tanh(sc / cap)
            ref[r, h] = torch.softmax(sc, -1) @ V[kv, lo:n + r + 1]
    return ref.view(R, nh * hd)


@pytest.mark.parametrize("hd,kv8,nh,kvh,window,cap,n,R,chunk", CASES)
def test_output_pool_and_len(hd, kv8, nh, kvh, window, cap, n, R, chunk):
    rig = Rig(hd, kv8, nh, kvh, n, R)
    before = [p.clone() for p in rig.pool]
    other = [p.clone() for p in rig.pool]
    rig.rope_cache(other, rig.qkv, n)
    out = rig.verify(rig.pool, rig.qkv, n, window, cap, chunk)
    # the new rows carry rope_cache's bits; nothing else moved
    for got, want, old in zip(rig.pool, other, before):
        assert torch.equal(bits(got[:, n:n + R]), bits(want[:, n:n + R]))
        rest = got.clone()
        rest[:, n:n + R] = old[:, n:n + R]
        assert torch.equal(bits(rest), bits(old))
    ref = reference(rig, other, n, R, window, cap)
    torch.testing.assert_close(out.double().cpu(), ref, rtol=4e-2, atol=4e-2)


@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("window", [0, 8])
def test_row_bits_do_not_depend_on_the_pass(kv8, window):
    """One R-row launch == R single-row launches on the pool as it then
    stands, and a repeated launch repeats its bits."""
    n, R = 29, 5
    rig = Rig(128, kv8, 4, 1, n, R, seed=1)
    single = [p.clone() for p in rig.pool]
    out = rig.verify(rig.pool, rig.qkv, n, window)
    rows = [rig.verify(single, rig.qkv[r:r + 1], n + r, window)
            for r in range(R)]
    assert torch.equal(out, torch.cat(rows))
    for a, b in zip(rig.pool, single):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(out, rig.verify(rig.pool, rig.qkv, n, window))


def test_binding_errors():
    from llm_np_cp_amd.ops import hip_ops as ho
    rig = Rig(128, False, 4, 1, 0, 1)
    pos = torch.zeros(1, dtype=torch.int32, device=dev())
    big = torch.zeros(ho.attn_verify_scratch_words(17, 4, 128, S, 32),
                      device=dev())
    qkv = torch.zeros(17, 6 * 128, dtype=torch.bfloat16, device=dev())
    out = torch.zeros(17, 4 * 128, dtype=torch.bfloat16, device=dev())

    def call(R=4, hd=128, scratch=big):
        ho.attn_verify(qkv, rig.pool[0], rig.pool[1], out, pos, rig.cos,
                       rig.sin, scratch, R, 4, 1, hd, 1.0, chunk=32)
    call()
    for bad in (dict(R=17), dict(hd=16),
                dict(scratch=big[:ho.attn_verify_scratch_words(
                    4, 4, 128, S, 32) - 1])):
        with pytest.raises(ValueError):
            call(**bad)
    torch.cuda.synchronize()
