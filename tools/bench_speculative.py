#!/usr/bin/env python3
"""Device-side greedy speculative decoding against the host loop of the same
build and the target's plain greedy decode, in ONE process with alternating
rounds (profiles/spec_device.md).

Synthetic weights give no natural acceptance, so two set-ups bracket it:
``same`` — the draft carries the target's weights (acceptance near 100 %,
the ceiling; needs --draft == --target) and ``other`` — a draft with another
seed (acceptance near 0 %, the pure overhead of a cycle).

    python tools/bench_speculative.py --target llama-3.2-1b
    python tools/bench_speculative.py --target llama-3.1-8b \
        --draft llama-3.2-1b --dtype fp8 --setups other
    python tools/bench_speculative.py --kernel-only    # k_spec_verify sweep

Every figure is a median over --rounds with its min-max; times are decode
times (prefill excluded), each ending in a device synchronise.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def mmm(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def kernel_sweep(V, k, iters):
    """k_spec_verify launch time (device events over ``iters`` back-to-back
    launches) per blocks-per-row setting, bf16 rows."""
    import torch
    from llm_np_cp_amd.ops import hip_ops as ho
    dev = torch.device("cuda")
    logits = torch.randn(k + 1, V, device=dev).to(torch.bfloat16)
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=dev)
    scratch = torch.zeros(ho.SPEC_SCRATCH_WORDS, dtype=torch.int64,
                          device=dev)
    st = dict(t_len=i32(1), t_next=i32(1), t_ring=i32(1 << 16),
              t_nout=i32(1), d_len=i32(1), d_next=i32(1), d_nout=i32(1),
              rec=torch.zeros(64, ho.SPEC_REC_WORDS, dtype=torch.int32,
                              device=dev), nrec=i32(1))
    drafts = i32(k)
    out = {}
    for blocks in (1, 2, 4, 8, 16, 32, 63):
        times = []
        for rep in range(6):
            st["t_nout"].zero_()
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                ho.spec_verify(logits, k, drafts, scratch, blocks=blocks,
                               **st)
            e1.record()
            torch.cuda.synchronize()
            if rep:                       # rep 0 warms up
                times.append(e0.elapsed_time(e1) * 1e3 / iters)
        out[blocks] = mmm(times)
        print(json.dumps({"kernel": "k_spec_verify", "V": V, "k": k,
                          "blocks": blocks, "us": out[blocks]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", default="llama-3.2-1b")
    ap.add_argument("--draft", default=None, help="default: the target")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8", "fp4"])
    ap.add_argument("--max-tokens", type=int, default=256)
    ap.add_argument("--ks", default="2,4,8")
    ap.add_argument("--setups", default="same,other")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-seq", type=int, default=1024)
    ap.add_argument("--chunks", default="",
                    help="also sweep SPEC_CHUNK over these values (k = 4, "
                         "first set-up)")
    ap.add_argument("--prompt", default="Once upon a time")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--kernel-iters", type=int, default=200)
    args = ap.parse_args()

    import torch
    import llm_np_cp_amd as L
    from csrc.build import ensure_built
    from llm_np_cp_amd.runtime.speculative import generate_speculative
    ensure_built()
    if not torch.cuda.is_available():
        raise SystemExit("bench_speculative measures on the GPU; none found")
    if args.kernel_only:
        kernel_sweep(128256, 4, args.kernel_iters)
        return

    dname = args.draft or args.target
    tok, target, _ = L.load_model(args.target, backend="gpu",
                                  dtype=args.dtype, max_seq=args.max_seq,
                                  seed=0)
    pid = [int(t) for t in tok.encode(args.prompt)]
    N = args.max_tokens

    def plain():
        target.generate_tokens(pid, N, greedy=True, chunk=N)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids = target.generate_tokens(pid, N, greedy=True, chunk=N)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0 - target.last_prefill_time_s
        return len(ids), dt

    def spec(draft, k, device):
        res = generate_speculative(args.prompt, tok, draft, target,
                                   max_tokens=N, k=k, stop_on_eos=False,
                                   device=device)
        return res

    for setup in args.setups.split(","):
        if setup == "same" and dname != args.target:
            continue
        _, draft, _ = L.load_model(dname, backend="gpu", dtype=args.dtype,
                                   max_seq=args.max_seq,
                                   seed=0 if setup == "same" else 1)
        for k in (int(x) for x in args.ks.split(",")):
            spec(draft, k, True)                      # warm both paths,
            spec(draft, k, False)                     # every shape
            rows = {"device": [], "host": [], "plain": [], "cycle_ms": []}
            stats = None
            for _ in range(args.rounds):
                r = spec(draft, k, True)
                rows["device"].append(len(r.token_ids) / r.decode_time_s)
                rows["cycle_ms"].append(
                    r.decode_time_s * 1e3 / r.spec_stats["verify_passes"])
                stats = r.spec_stats
                r = spec(draft, k, False)
                rows["host"].append(len(r.token_ids) / r.decode_time_s)
                n, dt = plain()
                rows["plain"].append(n / dt)
            step_ms = 1e3 / statistics.median(rows["plain"])
            cyc = statistics.median(rows["cycle_ms"])
            print(json.dumps({
                "target": args.target, "draft": dname, "dtype": args.dtype,
                "setup": setup, "k": k, "tokens": N,
                "acceptance": stats["accepted"] / max(stats["proposed"], 1),
                "device_tok_s": mmm(rows["device"]),
                "host_tok_s": mmm(rows["host"]),
                "plain_tok_s": mmm(rows["plain"]),
                "T_cycle_ms": mmm(rows["cycle_ms"]),
                "T_step_ms": step_ms,
                "break_even_tokens_per_cycle": cyc / step_ms,
                "chunk": target.SPEC_CHUNK}), flush=True)
        if args.chunks:
            keep = target.SPEC_CHUNK
            for c in (int(x) for x in args.chunks.split(",")):
                target.SPEC_CHUNK = c
                spec(draft, 4, True)
                v = []
                for _ in range(args.rounds):
                    r = spec(draft, 4, True)
                    v.append(len(r.token_ids) / r.decode_time_s)
                print(json.dumps({"setup": setup, "k": 4, "chunk": c,
                                  "device_tok_s": mmm(v)}), flush=True)
            target.SPEC_CHUNK = keep
            args.chunks = ""
        del draft
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
