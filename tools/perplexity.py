#!/usr/bin/env python3
"""Teacher-forced NLL / perplexity of ONE token stream under several engine
settings (runs on an MI355X box), all through ``GPUModel.prompt_logprobs``:

    weights bf16 / fp8 / fp4   x   kv_dtype bf16 / fp8

The model is a preset with random weights (default) or a local checkpoint
directory; the stream is ``--text FILE`` tokenised with the checkpoint's
tokenizer, or a seeded random stream.  One table: NLL per setting and the
delta against bf16 weights + bf16 KV.  With random weights the absolute
values mean nothing (a random model is near-uniform: NLL ~ ln V) — only the
deltas carry information.  Every setting is scored twice; the last column
is how far the two NLLs are apart.  By default the engine's split-K scratch
is taken away first (as ``bench.py --dump-outputs`` does): the small-N
prefill GEMMs otherwise accumulate with fp32 atomics, and on the quantised
engines that alone moves the NLL of one and the same stream by ~3e-3 from
run to run — as much as the deltas this table is for (``--split-k`` keeps
it).  ``tools/fp8_accuracy.py`` stays the tool for logit-level error and
greedy agreement.
"""

import argparse
import gc
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SETTINGS = [("bf16", "bf16"), ("fp8", "bf16"), ("fp4", "bf16"),
            ("bf16", "fp8"), ("fp8", "fp8")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-3.2-1b",
                    help="preset name (random weights) or checkpoint dir")
    ap.add_argument("--text", default=None,
                    help="text file to score (default: seeded random ids)")
    ap.add_argument("--tokens", type=int, default=2048,
                    help="stream length (the text is cut to it)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--settings", nargs="*", default=None,
                    help="weights:kv pairs, e.g. bf16:bf16 fp8:fp8")
    ap.add_argument("--split-k", action="store_true",
                    help="keep the engine's atomic split-K prefill GEMMs "
                         "(default: off, as bench.py --dump-outputs does — "
                         "their fp32 atomics make a pass differ from run to "
                         "run by more than the deltas measured here)")
    ap.add_argument("--json", action="store_true",
                    help="also print one JSON line")
    a = ap.parse_args()

    from csrc.build import ensure_built
    ensure_built()
    import llm_np_cp_amd as L
    from llm_np_cp_amd.io.loader import random_weights
    from llm_np_cp_amd.models.engine import GPUModel

    settings = ([tuple(s.split(":")) for s in a.settings]
                if a.settings else SETTINGS)
    is_dir = os.path.isdir(a.model)
    if is_dir:
        weights, cfg = None, None
    else:
        cfg = L.preset_config(a.model)
        weights = random_weights(cfg, seed=a.seed)

    ids = None
    rows = []
    for wdt, kvdt in settings:
        if is_dir:
            tok, m, cfg = L.load_model(a.model, backend="gpu", dtype=wdt,
                                       kv_dtype=kvdt, max_seq=a.tokens)
        else:
            tok = L.ByteTokenizer()
            m = GPUModel(cfg, weights, dtype=wdt, kv_dtype=kvdt,
                         max_seq=a.tokens)
        if ids is None:
            if a.text is not None:
                with open(a.text, encoding="utf-8") as f:
                    ids = np.asarray(tok.encode(f.read())[:a.tokens],
                                     dtype=np.int32)
            else:
                rng = np.random.default_rng(a.seed)
                ids = rng.integers(0, cfg.vocab_size, size=a.tokens,
                                   dtype=np.int32)
        if not a.split_k:
            m.b_gemm_acc = None
        lp, _, _ = m.prompt_logprobs(ids, 0)
        nll = float(-lp.astype(np.float64).mean())
        lp2, _, _ = m.prompt_logprobs(ids, 0)
        rows.append({"weights": wdt, "kv": kvdt, "nll": nll,
                     "ppl": float(np.exp(nll)),
                     "repeat": abs(float(-lp2.astype(np.float64).mean())
                                   - nll)})
        del m
        gc.collect()
        torch.cuda.empty_cache()

    base = next((r["nll"] for r in rows
                 if (r["weights"], r["kv"]) == ("bf16", "bf16")),
                rows[0]["nll"])
    print(f"model {a.model}  tokens {len(ids)}  "
          f"source {'text ' + a.text if a.text else f'random ids, seed {a.seed}'}")
    print(f"{'weights':<8}{'kv':<6}{'NLL':>12}{'dNLL vs bf16':>16}"
          f"{'perplexity':>16}{'|NLL - rerun|':>16}")
    for r in rows:
        r["dnll"] = r["nll"] - base
        print(f"{r['weights']:<8}{r['kv']:<6}{r['nll']:>12.5f}"
              f"{r['dnll']:>+16.5f}{r['ppl']:>16.2f}{r['repeat']:>16.2e}")
    if a.json:
        print(json.dumps({"model": a.model, "tokens": int(len(ids)),
                          "rows": rows}))


if __name__ == "__main__":
    main()
