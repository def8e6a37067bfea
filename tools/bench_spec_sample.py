#!/usr/bin/env python3
"""Device-side stochastic speculative sampling (profiles/spec_sample.md).

    python tools/bench_spec_sample.py --kernel-only
        one ``ho.spec_sample`` call (its three launches together, device
        events) at V = 128256 per k and blocks-per-row, and ``ho.spec_keep``;
        under ``rocprofv3 --kernel-trace --stats`` the same run gives the
        three kernels' own durations
    python tools/bench_spec_sample.py --target llama-3.2-1b
        min-p speculative decoding on the device against the host loop (the
        host loop is the parent commit's, untouched by the device path), one
        process, alternating rounds; ``same`` / ``other`` drafts as in
        tools/bench_speculative.py

Every figure is a median over the rounds with its min-max; decode times
exclude the prefill and end in a device synchronise.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def mmm(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def timed(fn, iters, reps=6):
    import torch
    out = []
    for rep in range(reps):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if rep:                           # rep 0 warms up
            out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return mmm(out)


def kernel_sweep(V, iters):
    import torch
    from llm_np_cp_amd.ops import hip_ops as ho
    dev = torch.device("cuda")
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=dev)
    scratch = torch.zeros(ho.SPEC_SAMPLE_SCRATCH_WORDS, dtype=torch.int64,
                          device=dev)
    part = torch.zeros(ho.spec_sample_part_words(V), dtype=torch.float32,
                       device=dev)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    for k in (4, 8):
        x = torch.randn(2 * k + 1, V, device=dev).to(torch.bfloat16)
        trows, drows = x[:k + 1].contiguous(), x[k + 1:].float().contiguous()
        drafts = torch.argmax(drows, 1).to(torch.int32)
        st = dict(t_len=i32(1), t_next=i32(1), t_ring=i32(1 << 16),
                  t_nout=i32(1), d_len=i32(1), d_next=i32(1), d_nout=i32(1),
                  rec=torch.zeros(64, ho.SPEC_REC_WORDS, dtype=torch.int32,
                                  device=dev), nrec=i32(1))
        for blocks in (1, 2, 4, 8, 16, 32, 63):
            def call():
                st["t_nout"].zero_()
                ho.spec_sample(trows, drows, k, drafts, 1.25, 0.1, 7, ctr,
                               scratch, part, blocks=blocks, **st)
            print(json.dumps({"call": "spec_sample", "V": V, "k": k,
                              "blocks": blocks, "us": timed(call, iters)}),
                  flush=True)
    kept = torch.zeros(ho.SPEC_MAX_K + 1, V, device=dev)
    row, nout = torch.randn(V, device=dev), i32(1, 3)
    print(json.dumps({"call": "spec_keep", "V": V, "us": timed(
        lambda: ho.spec_keep(row, kept, nout), iters)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", default="llama-3.2-1b")
    ap.add_argument("--draft", default=None, help="default: the target")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8", "fp4"])
    ap.add_argument("--max-tokens", type=int, default=128)
    ap.add_argument("--ks", default="4,8")
    ap.add_argument("--setups", default="same,other")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-seq", type=int, default=1024)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--min-p", type=float, default=0.1)
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
        raise SystemExit("bench_spec_sample measures on the GPU; none found")
    if args.kernel_only:
        kernel_sweep(128256, args.kernel_iters)
        return
    os.environ["LLM_SPEC_SAMPLE"] = "1"
    dname = args.draft or args.target
    tok, target, _ = L.load_model(args.target, backend="gpu",
                                  dtype=args.dtype, max_seq=args.max_seq,
                                  seed=0)
    params = L.SamplingParams(strategy="min_p", min_p=args.min_p,
                              temperature=args.temperature, seed=1)

    def spec(draft, k, device):
        return generate_speculative(args.prompt, tok, draft, target,
                                    max_tokens=args.max_tokens, k=k,
                                    stop_on_eos=False, params=params,
                                    device=device)

    for setup in args.setups.split(","):
        if setup == "same" and dname != args.target:
            continue
        _, draft, _ = L.load_model(dname, backend="gpu", dtype=args.dtype,
                                   max_seq=args.max_seq,
                                   seed=0 if setup == "same" else 1)
        for k in (int(x) for x in args.ks.split(",")):
            spec(draft, k, True)                      # warm both paths
            spec(draft, k, False)
            rows = {"device": [], "host": [], "acc_d": [], "acc_h": [],
                    "cycle_d": [], "cycle_h": []}
            for _ in range(args.rounds):
                for name, dev in (("d", True), ("h", False)):
                    r = spec(draft, k, dev)
                    s = r.spec_stats
                    rows["device" if dev else "host"].append(
                        len(r.token_ids) / r.decode_time_s)
                    rows["acc_" + name].append(
                        s["accepted"] / max(s["proposed"], 1))
                    rows["cycle_" + name].append(
                        r.decode_time_s * 1e3 / s["verify_passes"])
            print(json.dumps({
                "target": args.target, "draft": dname, "dtype": args.dtype,
                "setup": setup, "k": k, "tokens": args.max_tokens,
                "temperature": args.temperature, "min_p": args.min_p,
                "device_tok_s": mmm(rows["device"]),
                "host_tok_s": mmm(rows["host"]),
                "device_acceptance": mmm(rows["acc_d"]),
                "host_acceptance": mmm(rows["acc_h"]),
                "device_cycle_ms": mmm(rows["cycle_d"]),
                "host_cycle_ms": mmm(rows["cycle_h"])}), flush=True)
        del draft
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
