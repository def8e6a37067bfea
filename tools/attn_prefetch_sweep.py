#!/usr/bin/env python3
"""Ceiling for the attention-carried weight prefetch (runs on an MI355X).

Times `attn_dec -> o_proj -> gate+up` at the Llama-3.2-1B shapes over 16
distinct weight sets (1.2 GB, past the 256 MB Infinity Cache, so the
consumers are cold as in the decode step), captured in one graph, events
around replays, best of 5.  Per-kernel figures come from graphs that
stop after the first / second kernel of the triple.  Sweeps the byte
budget and the prefetch block count; `--stride` turns the o_proj L2
placement walk on.  Results: profiles/attn_prefetch.md.
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def time_graph(fn, replays=40, best_of=5):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(best_of):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / replays)
    return best  # us per replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stride", type=int, default=0,
                    help="1: walk wo by consumer-block XCD class")
    ap.add_argument("--T", type=int, default=120, help="context length")
    ap.add_argument("--blocks", type=str, default="64,128,192,384,768")
    ap.add_argument("--wgu-mb", type=str, default="-1,0,16,32,48,64",
                    help="-1 = prefetch off, 0 = wo only")
    args = ap.parse_args()

    from llm_np_cp_amd.ops import hip_ops as ho
    from llm_np_cp_amd.models.attn_prefetch import (consumer_stride,
                                                    plan_attn_prefetch)

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    H, I, L = 2048, 8192, 16
    nh, kvh, hd, S, split = 32, 8, 64, 2048, 2
    bf = dict(dtype=torch.bfloat16, device=dev)
    layers = [dict(wo=torch.randn(H, H, **bf) * 0.02,
                   wgu=torch.randn(2 * I, H, **bf) * 0.02,
                   kc=torch.randn(kvh, S, hd, **bf),
                   vc=torch.randn(kvh, S, hd, **bf)) for _ in range(L)]
    qkv = torch.randn((nh + 2 * kvh) * hd, **bf)
    att = torch.empty(nh * hd, **bf)
    h = torch.zeros(H, **bf)
    gu = torch.empty(2 * I, **bf)
    g1 = torch.ones(H, device=dev)
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd))
    fr = torch.outer(torch.arange(S).float(), inv)
    cos_t, sin_t = torch.cos(fr).to(dev), torch.sin(fr).to(dev)
    scratch = torch.zeros(nh * split * (hd + 2), dtype=torch.float32,
                          device=dev)
    cnt = torch.zeros(nh, dtype=torch.int32, device=dev)
    sink = torch.zeros(256, dtype=torch.float32, device=dev)
    pos = torch.tensor([args.T - 1], dtype=torch.int32, device=dev)
    wo_b, wgu_b = H * H * 2, 2 * I * H * 2
    stride0 = consumer_stride(wo_b, H, 4) if args.stride else 0

    def chain(upto, budget, blocks):
        def fn():
            for lw in layers:
                if budget <= 0:
                    ho.attn_dec(qkv, lw["kc"], lw["vc"], att, pos, cos_t,
                                sin_t, scratch, cnt, nh, kvh, hd, hd ** -0.5,
                                split=split)
                else:
                    base = {"wo": lw["wo"].data_ptr(),
                            "wgu": lw["wgu"].data_ptr()}
                    regs = [(base[n] + o, b) for n, o, b in
                            plan_attn_prefetch(wo_b, wgu_b, I, H, budget)]
                    ho.attn_dec_pf(qkv, lw["kc"], lw["vc"], att, pos, cos_t,
                                   sin_t, scratch, cnt, nh, kvh, hd,
                                   hd ** -0.5, split=split, regions=regs,
                                   pf_blocks=blocks, stride0=stride0,
                                   sink=sink)
                if upto >= 2:
                    ho.gemv(lw["wo"], att, h, res=h)
                if upto >= 3:
                    ho.gemv(lw["wgu"], h, gu, stage=ho.STAGE_NORM, g=g1,
                            glu_pair=True, act=0)
        return fn

    def row(label, budget, blocks):
        t = [time_graph(chain(u, budget, blocks)) / L for u in (1, 2, 3)]
        print(f"{label:>22} | attn {t[0]:6.2f} | o_proj {t[1] - t[0]:6.2f} | "
              f"gate+up {t[2] - t[1]:6.2f} | triple {t[2]:6.2f}", flush=True)

    print(f"T={args.T} split={split} stride0={stride0}  (us per layer)")
    for mb in [int(x) for x in args.wgu_mb.split(",")]:
        if mb < 0:
            row("off", 0, 0)
            row("off (again)", 0, 0)
            continue
        budget = wo_b + mb * (1 << 20)
        for blocks in [int(x) for x in args.blocks.split(",")]:
            row(f"wo+{mb}MB x{blocks}", budget, blocks)


if __name__ == "__main__":
    main()
