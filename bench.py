#!/usr/bin/env python3
"""Flagship decode benchmark (driver contract).

Measures the BASELINE.json metric: decode tokens/sec, batch 1, synthetic
prompt, random-init weights, bf16.  Default model is Llama-3.2-1B at
EVERY N (TP=N) so the driver's 1/2/4/8-GPU curve compares like with
like; the metric's second config (Gemma-2-9B TP=8, fp8) runs via
``--model gemma-2-9b --dtype fp8``.  A "step" is one decoded token; the
timed region is K hipGraph-replayed decode steps (full forward incl.
lm_head + sampling).

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--model M]
                       [--dump-outputs DIR] [--full]
A plain run sets up, warms up, times the K steps and prints one JSON
result line; ``--dump-outputs DIR`` additionally saves the last step's
logits and the emitted token ids as .npy (its untimed prefill skips the
atomic split-K GEMM path so that the dump is bitwise reproducible at
batch 1), and ``--full`` is where any secondary measurement belongs.
Launched by the driver for N>1 via torch.distributed.run (one rank/GPU).
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


DUMP_MAX_BYTES = 24 << 20  # per array; two arrays stay far below 64 MB


def emitted_counts(model, batch):
    """Ids emitted so far, read from the device counters: (B,) int array
    batched, (1,) at batch 1."""
    c = model.bt_nout[:batch] if batch > 1 else model.nout
    return c.cpu().numpy().astype(int)


def dump_outputs(out_dir, model, batch, start):
    """Write the last timed step's results as ``out_dir/<name>.npy``.

    ``start`` is emitted_counts() taken right before the timed region;
    everything the device appended to the output ring since then is what
    the timed steps emitted (so a timed loop that ran another number of
    steps than --steps shows in the array's length).

    ``logits``    float32 — the logits the last step sampled from
                  ((vocab,) at batch 1, (B, vocab) batched);
    ``token_ids`` float64 — the ids the timed steps emitted, oldest
                  first ((steps,) at batch 1, (B, steps) batched).
    An array above DUMP_MAX_BYTES is reduced to a fixed, seeded sample
    of its flattened elements (same indices every run).
    """
    import numpy as np

    end = emitted_counts(model, batch)
    if batch > 1:
        logits = model.bt_logits[:batch].float().cpu().numpy()
        ring = model.bt_ring[:batch].cpu().numpy()
        ids = np.stack([ring[b, start[b]:end[b]] for b in range(batch)])
    else:
        logits = model.b_logits.float().cpu().numpy()
        ids = model.out_ring[start[0]:end[0]].cpu().numpy()
    arrays = {"logits": logits.astype(np.float32),
              "token_ids": ids.astype(np.float64)}
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        if a.nbytes > DUMP_MAX_BYTES:
            keep = DUMP_MAX_BYTES // a.itemsize
            idx = np.sort(np.random.default_rng(0).choice(
                a.size, size=keep, replace=False))
            a = a.ravel()[idx]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--model", type=str, default="llama-3.2-1b",
                    help="model preset (default llama-3.2-1b at every N "
                         "so the driver's 1/2/4/8-GPU scaling curve "
                         "compares like with like; gemma-2-9b etc. via "
                         "this flag; synthetic random-init weights)")
    ap.add_argument("--prompt-len", type=int, default=64)
    ap.add_argument("--max-seq", type=int, default=None)
    ap.add_argument("--dtype", type=str, default="bf16",
                    choices=["bf16", "fp8", "fp4"],
                    help="weight dtype (constant across N for honest "
                         "scaling; fp8 = BASELINE config 4)")
    ap.add_argument("--kv-dtype", type=str, default="bf16",
                    choices=["bf16", "fp8"],
                    help="KV-pool dtype (fp8 = e4m3 with per-head-pos "
                         "scales; halves the attention read stream)")
    ap.add_argument("--batch", type=int, default=1,
                    help="lockstep batched decode (throughput mode; "
                         "value = aggregate tokens/s over the batch)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed "
                         "step computed (logits, sampled token ids) as "
                         "DIR/<name>.npy; inputs are seeded, so two builds "
                         "can be compared output for output")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement or check; "
                         "a plain run only sets up, warms up, times the "
                         "steps and prints the result line (there are no "
                         "secondary measurements yet: the per-kernel, "
                         "prefill and server figures live in tools/)")
    args = ap.parse_args()

    import numpy as np
    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    n_gpus = max(world, args.gpus)
    model_name = args.model

    from csrc.build import ensure_built
    ensure_built()

    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import LazyRandomWeights
    from llm_np_cp_amd.models.engine import GPUModel
    from llm_np_cp_amd.parallel.tp import init_distributed

    rank, world = init_distributed()
    dtype = args.dtype
    cfg = L.preset_config(model_name)
    max_seq = args.max_seq or min(
        cfg.max_position_embeddings,
        args.prompt_len + args.steps + args.warmup + 64)
    w = LazyRandomWeights(cfg, seed=0)
    model = GPUModel(cfg, w, max_seq=max_seq, seed=0, dtype=dtype,
                     kv_dtype=args.kv_dtype, max_batch=args.batch)

    if rank == 0 and world > 1:
        from llm_np_cp_amd.parallel import tp as _tp
        mode = ("one-shot xGMI" if _tp.xgmi_comm() is not None
                else "RCCL fallback")
        print(f"# decode collectives: {mode} (world={world})",
              file=sys.stderr)

    rng = np.random.default_rng(0)
    prompt = rng.integers(0, cfg.vocab_size, size=args.prompt_len)

    def barrier():
        if world > 1:
            torch.distributed.barrier()

    # prefill + warmup
    use_graph = not args.no_graph
    # The small-M prefill GEMMs split K and accumulate with fp32 atomics,
    # so the KV they leave differs in the last bits from run to run, and a
    # greedy rollout over random weights amplifies that into different
    # tokens.  For a dump that two builds can compare, the (untimed)
    # prefill runs without the split-K scratch; the decode steps — the
    # timed path — are exactly those of a plain run.
    gemm_acc = model.b_gemm_acc
    if args.dump_outputs:
        model.b_gemm_acc = None
    if args.batch > 1:
        prompts = rng.integers(0, cfg.vocab_size,
                               size=(args.batch, args.prompt_len))
        model.prefill_batch(prompts)
        model.b_gemm_acc = gemm_acc
        model.decode_batch(max(args.warmup, 2), greedy=True,
                           use_graph=use_graph)
        if model._graph_mode is None:
            use_graph = False
    else:
        model.prefill(prompt)
        model.b_gemm_acc = gemm_acc
        if args.warmup > 0:
            model.decode(args.warmup, greedy=True, use_graph=use_graph,
                         first_from_logits=True)

    if use_graph and args.batch == 1:
        # no-op if the warmup already captured; on failure the step it
        # executed is harmless here (untimed region)
        _, ok = model.capture_decode_graph(True, 0.1)
        if not ok:
            if rank == 0:
                err = getattr(model, "_graph_error", None)
                print(f"# graph capture unavailable "
                      f"({type(err).__name__ if err else '?'}: {err}); "
                      f"timing eager launches", file=sys.stderr)
            use_graph = False

    # device-side emitted-id counters before the timed region, so the
    # dump holds what the timed steps really appended (reads sync; untimed)
    dump_start = (emitted_counts(model, args.batch)
                  if args.dump_outputs and rank == 0 else None)

    # timed region: exactly K decode steps
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if use_graph:
        for _ in range(args.steps):
            model._graph.replay()
    elif args.batch > 1:
        for _ in range(args.steps):
            model._decode_batch_step(args.batch, True, 0.1)
    else:
        for _ in range(args.steps):
            model._decode_step(True, 0.1)
    torch.cuda.synchronize()
    barrier()
    t1 = time.perf_counter()

    elapsed = t1 - t0
    if world > 1:
        t = torch.tensor([elapsed], device=model.device)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    toks_per_s = args.steps * args.batch / elapsed
    ms_per_step = elapsed / args.steps * 1e3

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, args.batch, dump_start)

    if rank == 0:
        out = {
            "metric": "decode tokens/sec",
            "value": toks_per_s,
            "unit": "tokens/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": dtype,
            "data": "synthetic",
            "config": {
                "model": model_name,
                "kv_dtype": args.kv_dtype,
                "global_batch": args.batch,
                "seq_len": args.prompt_len + args.warmup + args.steps,
                "parallelism": f"tp{world}",
            },
        }
        print(json.dumps(out))


if __name__ == "__main__":
    main()
