#!/usr/bin/env python
"""The speculative verify pass on the skinny kernels against the prefill-path
pass, and `attn_verify` against the pair it replaces
(profiles/spec_skinny.md).  Both sides run in one process, alternated round
by round, timed with device events over a warmed-up window.

    python tools/bench_spec_skinny.py --target llama-3.2-1b --dtype bf16
    python tools/bench_spec_skinny.py --target llama-3.1-8b \
        --draft llama-3.2-1b --dtype fp8
    python tools/bench_spec_skinny.py --kernel-only
    python tools/bench_spec_skinny.py --target llama-3.2-1b --trace-pass 50
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, iters):
    """ms per call: device events around ``iters`` back-to-back calls."""
    import torch
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def spread(v):
    return {"median": round(statistics.median(v), 4),
            "min": round(min(v), 4), "max": round(max(v), 4)}


def kernel_bench(iters, rounds):
    """`attn_verify` (+ merge) against rope_cache + attn_prefill_mfma at the
    Llama-3.1-8B attention shape."""
    import torch
    from llm_np_cp_amd.ops import hip_ops as ho
    nh, kvh, hd, S = 32, 8, 128, 8192 + 64
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    cos = torch.rand(S, hd // 2, generator=g).to(dev)
    sin = torch.rand(S, hd // 2, generator=g).to(dev)
    chunk = ho.attn_verify_chunk(S)
    for kv8 in (False, True):
        if kv8:
            pool = [torch.randint(0, 120, (kvh, S, hd), generator=g,
                                  dtype=torch.uint8).to(dev) for _ in "kv"]
            sc = dict(kS=torch.rand(kvh, S, generator=g).to(dev),
                      vS=torch.rand(kvh, S, generator=g).to(dev))
        else:
            pool = [torch.randn(kvh, S, hd, generator=g).to(
                dev, torch.bfloat16) for _ in "kv"]
            sc = {}
        for R in (5, 9):
            qkv = torch.randn(R, (nh + 2 * kvh) * hd, generator=g).to(
                dev, torch.bfloat16)
            q, k, v = (t.contiguous() for t in qkv.split(
                [nh * hd, kvh * hd, kvh * hd], dim=1))
            out = torch.zeros(R, nh * hd, dtype=torch.bfloat16, device=dev)
            scratch = torch.zeros(ho.attn_verify_scratch_words(
                R, nh, hd, S, chunk), device=dev)
            for n in (128, 2048, 8192):
                ln = torch.tensor([n], dtype=torch.int32, device=dev)

                def new():
                    ho.attn_verify(qkv, pool[0], pool[1], out, ln, cos, sin,
                                   scratch, R, nh, kvh, hd, hd ** -0.5, **sc)

                def old():
                    ho.rope_cache(q, k, v, pool[0], pool[1], cos, sin, ln, R,
                                  nh, kvh, hd, **sc)
                    ho.attn_prefill_mfma(q, pool[0], pool[1], out, ln, R, nh,
                                         kvh, hd, hd ** -0.5, **sc)
                timed(new, 20), timed(old, 20)
                t_new, t_old = [], []
                for _ in range(rounds):
                    t_old.append(timed(old, iters) * 1e3)
                    t_new.append(timed(new, iters) * 1e3)
                print(json.dumps({
                    "kernel": "attn_verify", "kv": "fp8" if kv8 else "bf16",
                    "R": R, "history": n, "chunk": chunk,
                    "pair_us": spread(t_old), "verify_us": spread(t_new)}),
                    flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", default="llama-3.2-1b")
    ap.add_argument("--draft", default=None, help="default: the target")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8", "fp4"])
    ap.add_argument("--ks", default="2,4,8")
    ap.add_argument("--history", type=int, default=128)
    ap.add_argument("--max-seq", type=int, default=1024)
    ap.add_argument("--max-tokens", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--trace-pass", type=int, default=0,
                    help="run only N prefill-path passes at k = 4 (to be "
                         "started under a kernel trace)")
    args = ap.parse_args()

    import numpy as np
    import torch
    import llm_np_cp_amd as L
    from csrc.build import ensure_built
    ensure_built()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spec_skinny measures on the GPU; none found")
    if args.kernel_only:
        kernel_bench(args.iters * 4, args.rounds)
        return

    os.environ["LLM_SPEC_SKINNY"] = "1"
    _, T, cfg = L.load_model(args.target, backend="gpu", dtype=args.dtype,
                             max_seq=args.max_seq, seed=0)
    os.environ["LLM_SPEC_SKINNY"] = "0"
    _, D, _ = L.load_model(args.draft or args.target, backend="gpu",
                           dtype=args.dtype, max_seq=args.max_seq, seed=1)
    assert T.spec_skinny
    n = args.history
    pid = np.random.default_rng(0).integers(
        0, cfg.vocab_size, n).astype(np.int32)
    T.prefill(pid)
    D.out_ring[:16].copy_(torch.arange(100, 116, dtype=torch.int32))
    T._spec_alloc()

    def one_pass(k, skinny):
        def fn():
            T.spec_skinny = skinny
            T.rewind(n)
            T.spec_verify_pass(D, k)
        return fn

    if args.trace_pass:
        for _ in range(args.trace_pass):
            one_pass(4, False)()
        torch.cuda.synchronize()
        return

    t_step = []
    for _ in range(args.rounds):
        T.rewind(n)
        T.decode_steps_async(4)
        T.rewind(n)
        t_step.append(timed(lambda: T.decode_steps_async(1), 32))
    for k in (int(x) for x in args.ks.split(",")):
        timed(one_pass(k, False), 5), timed(one_pass(k, True), 5)
        res = {False: [], True: []}
        cyc = {False: [], True: []}
        for _ in range(args.rounds):
            for sk in (False, True):
                res[sk].append(timed(one_pass(k, sk), args.iters))
        # whole cycles: decode time / verify passes, host clock around a
        # synchronised run, as tools/bench_speculative.py takes it
        import time
        for r in range(args.rounds + 1):
            for sk in (False, True):
                T.spec_skinny = sk
                t0 = time.perf_counter()
                _, recs = T.speculative_tokens(D, pid, args.max_tokens, k=k)
                dt = time.perf_counter() - t0 - T.last_prefill_time_s
                if r:                       # round 0 warms both paths
                    cyc[sk].append(dt * 1e3 / max(len(recs), 1))
        step = statistics.median(t_step)
        print(json.dumps({
            "target": args.target, "draft": args.draft or args.target,
            "dtype": args.dtype, "k": k, "history": n,
            "pass_ms_prefill_path": spread(res[False]),
            "pass_ms_skinny": spread(res[True]),
            "t_cycle_ms_prefill_path": spread(cyc[False]),
            "t_cycle_ms_skinny": spread(cyc[True]),
            "t_step_ms": spread(t_step),
            "break_even_prefill_path": round(
                statistics.median(cyc[False]) / step, 2),
            "break_even_skinny": round(
                statistics.median(cyc[True]) / step, 2)}), flush=True)
        T.prefill(pid)                      # the pool as the passes expect


if __name__ == "__main__":
    main()
