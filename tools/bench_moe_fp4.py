#!/usr/bin/env python3
"""Mixtral-8x7B layer shape (H 4096, I 14336, E 8, top-2): the grouped
expert GEMMs and the decode GEMVs of a layer, MXFP4 against fp8
(profiles/moe_fp4.md).
usage: python tools/bench_moe_fp4.py [--lib PATH] [--only-fp4-gemm]
--lib: another build of the kernel library (e.g. -DMOE_FP4_ONE_MFMA)."""
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from llm_np_cp_amd.ops import hip_ops as ho

if "--lib" in sys.argv:
    ho._LIB_PATH = sys.argv[sys.argv.index("--lib") + 1]
ONLY = "--only-fp4-gemm" in sys.argv
H, I, E, K2 = 4096, 14336, 8, 2
dev = "cuda"
u8 = dict(dtype=torch.uint8, device=dev)
torch.manual_seed(0)


def q8w(rows, k):
    q, s = torch.empty(rows, k, **u8), torch.empty(rows, device=dev)
    for r0 in range(0, rows, 16384):
        t = torch.randn(min(16384, rows - r0), k, dtype=torch.bfloat16, device=dev)
        ho.quant_fp8(t, q[r0:], s[r0:])
    torch.cuda.synchronize()
    return q, s


def q4w(rows, k):
    q, e = torch.empty(rows, k // 2, **u8), torch.empty(rows, k // 32, **u8)
    for r0 in range(0, rows, 16384):
        t = torch.randn(min(16384, rows - r0), k, dtype=torch.bfloat16, device=dev)
        ho.quant_fp4(t, q[r0:], e[r0:])
    torch.cuda.synchronize()
    return q, e


def timeit(fn, iters):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def compare(label, fns, iters, rounds=5):
    """Alternate the variants, `rounds` windows each; median and spread (ms)."""
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(timeit(fn, iters))
    print(label, " ".join(f"{k}: med {statistics.median(v):.4f} ms "
                          f"[{min(v):.4f}..{max(v):.4f}]" for k, v in ts.items()),
          flush=True)


wgu8, sgu8 = (None, None) if ONLY else q8w(E * 2 * I, H)
wd8, sd8 = (None, None) if ONLY else q8w(E * H, I)
wgu4, egu4 = q4w(E * 2 * I, H)
wd4, ed4 = q4w(E * H, I)
i32 = dict(dtype=torch.int32, device=dev)

for M in (2048, 16):
    n = M * K2
    idx = torch.rand(M, E, device=dev).argsort(1)[:, :K2].to(torch.int32).contiguous()
    w = torch.full((n,), 0.5, device=dev)
    tm = ho.moe_tile_rows(M, K2, E)
    b = dict(slot_row=torch.zeros(n, **i32), slot_w=torch.zeros(n, device=dev),
             pair_slot=torch.zeros(n, **i32), grp_off=torch.zeros(E + 1, **i32),
             tiles=torch.zeros(1 + 3 * ho.moe_max_tiles(M, K2, E, 32), **i32))
    ho.moe_group(idx.view(-1), w, M, K2, E, **b)
    xq, sx = torch.empty(M, H, **u8), torch.empty(M, device=dev)
    ho.quant_fp8(torch.randn(M, H, dtype=torch.bfloat16, device=dev), xq, sx)
    aq, sa = torch.empty(n, I, **u8), torch.empty(n, device=dev)
    ho.quant_fp8(torch.randn(n, I, dtype=torch.bfloat16, device=dev), aq, sa)
    act = torch.empty(n, I, dtype=torch.bfloat16, device=dev)
    y = torch.empty(n, H, device=dev)
    iters = 20 if M == 2048 else 50
    g4 = lambda: ho.moe_gemm_fp4_glu(xq, sx, b["slot_row"], wgu4, egu4, b["tiles"], act, M, K2, tm)
    d4 = lambda: ho.moe_gemm_fp4_down(aq, sa, wd4, ed4, b["tiles"], y, M, K2, tm)
    fg, fd = {"fp4": g4}, {"fp4": d4}
    if not ONLY:
        fg["fp8"] = lambda: ho.moe_gemm_fp8_glu(xq, sx, b["slot_row"], wgu8, sgu8, b["tiles"], act, M, K2, tm)
        fd["fp8"] = lambda: ho.moe_gemm_fp8_down(aq, sa, wd8, sd8, b["tiles"], y, M, K2, tm)
    compare(f"glu  M={M} tm={tm}", fg, iters)
    compare(f"down M={M} tm={tm}", fd, iters)

if not ONLY:
    # single-sequence decode: the topk loop of expert-indexed GEMV pairs
    bf = dict(dtype=torch.bfloat16, device=dev)
    xn, gu, h = torch.randn(H, **bf), torch.empty(2 * I, **bf), torch.randn(H, **bf)
    eidx = torch.tensor([5, 2], **i32)
    osc = torch.full((2,), 0.5, device=dev)

    def dec4():
        for j in range(K2):
            ho.gemv_fp4(wgu4[:2 * I], egu4[:2 * I], xn, gu, eidx=eidx[j:j + 1], wstride=2 * I * H)
            ho.gemv_fp4(wd4[:H], ed4[:H], gu[:I], h, res=h, stage=ho.STAGE_GLU, x2=gu[I:], act=0,
                        eidx=eidx[j:j + 1], wstride=H * I, oscale=osc[j:j + 1])

    def dec8():
        for j in range(K2):
            ho.gemv_fp8(wgu8[:2 * I], sgu8[:2 * I], xn, gu, eidx=eidx[j:j + 1], wstride=2 * I * H,
                        sstride=2 * I)
            ho.gemv_fp8(wd8[:H], sd8[:H], gu[:I], h, res=h, stage=ho.STAGE_GLU, x2=gu[I:], act=0,
                        eidx=eidx[j:j + 1], wstride=H * I, sstride=H, oscale=osc[j:j + 1])
    compare("decode MoE GEMVs per layer (4 launches)", {"fp4": dec4, "fp8": dec8}, 100)
