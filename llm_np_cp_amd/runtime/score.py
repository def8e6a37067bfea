"""Teacher-forced scoring: log p(token_t | tokens_<t) of a given text.

``score`` returns per-token logprobs (optionally with the top-N
alternatives), the mean NLL and the perplexity; ``loglikelihood`` is the
(context, continuation) form evaluation harnesses ask for.

Two paths, chosen by what the model advertises:

* device — ``model.device_prompt_logprobs >= top_n`` (the single-GPU
  ``GPUModel``): ``model.prompt_logprobs(ids, top_n)`` runs the prefill
  pass, reduces every logits row on the device (``k_logprob_rows``) and
  hands back one record per position.
* host — everything else (``NumpyModel``, tensor-parallel engines,
  ``top_n`` beyond the device record width): all-position logits, then a
  float64 log-softmax per row.  Ties are ordered by ascending id, as on
  the device.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from .generate import logprob_entries


@dataclass
class ScoreResult:
    token_ids: List[int]
    # one entry per token; entry 0 is None (nothing conditions it)
    logprobs: List[Optional[float]]
    # per token the ``logprob_entries`` dict {"id", "token", "logprob",
    # "top": [...]}; entry 0 is None
    top: List[Optional[dict]]
    nll: float          # mean over the scored tokens (all but the first)
    perplexity: float   # exp(nll)


def _all_position_logits(model, ids: np.ndarray) -> np.ndarray:
    """(n, V) logits of every position: the engine's ``forward_full`` or
    the oracle's ``forward`` over a fresh cache."""
    if hasattr(model, "forward_full"):
        return np.asarray(model.forward_full(ids))
    if hasattr(model, "make_cache"):
        cache = model.make_cache(len(ids) + 1)
    else:
        from ..models.numpy_ref import NumpyKVCache
        cache = NumpyKVCache(model.config, len(ids) + 1)
    return np.asarray(model.forward(np.asarray(ids, dtype=np.int64), cache, 0))


def host_prompt_logprobs(logits: np.ndarray, ids, top_n: int):
    """Records ``(lp [n-1] f32, top_ids [n-1, N] i32, top_lp [n-1, N]
    f32)`` from all-position logits ``[n, V]`` — the shape
    ``GPUModel.prompt_logprobs`` returns.  float64 log-softmax per row;
    top-N descending, ties by ascending id (stable sort of the negated
    row); a vocabulary shorter than N fills id -1 / logprob -inf."""
    ids = np.asarray(ids).ravel()
    n, N = len(ids), max(int(top_n), 0)
    lp = np.empty(n - 1, dtype=np.float32)
    top_ids = np.full((n - 1, N), -1, dtype=np.int32)
    top_lp = np.full((n - 1, N), -np.inf, dtype=np.float32)
    for t in range(n - 1):
        z = np.asarray(logits[t], dtype=np.float64)
        z = z - z.max()
        row = z - np.log(np.exp(z).sum())
        lp[t] = row[int(ids[t + 1])]
        if N:
            order = np.argsort(-row, kind="stable")[:N]
            top_ids[t, :len(order)] = order
            top_lp[t, :len(order)] = row[order]
    return lp, top_ids, top_lp


def score(prompt_or_ids, tokenizer, model, top_n: int = 0) -> ScoreResult:
    """Score a text (str, tokenised with ``tokenizer``) or a token-id
    sequence under ``model``.  ``top_n`` > 0 adds the top-N alternatives at
    every scored position."""
    if isinstance(prompt_or_ids, str):
        ids = [int(i) for i in tokenizer.encode(prompt_or_ids)]
    else:
        ids = [int(i) for i in np.asarray(prompt_or_ids).ravel()]
    top_n = int(top_n)
    if top_n < 0:
        raise ValueError(f"top_n must be >= 0, got {top_n}")
    if len(ids) < 2:
        raise ValueError(f"scoring needs at least 2 tokens, got {len(ids)}")
    arr = np.asarray(ids, dtype=np.int32)
    dev = int(getattr(model, "device_prompt_logprobs", 0) or 0)
    if dev > 0 and top_n <= dev and hasattr(model, "prompt_logprobs"):
        records = model.prompt_logprobs(arr, top_n)
    else:
        records = host_prompt_logprobs(_all_position_logits(model, arr),
                                       arr, top_n)
    lp = np.asarray(records[0], dtype=np.float64)
    entries = logprob_entries(ids[1:], records, top_n, tokenizer)
    nll = float(-lp.mean())
    return ScoreResult(token_ids=ids,
                       logprobs=[None] + [float(v) for v in lp],
                       top=[None] + entries, nll=nll,
                       perplexity=float(np.exp(nll)))


def loglikelihood(context: str, continuation: str, tokenizer,
                  model) -> Tuple[float, bool]:
    """``(sum log p(continuation | context), is_greedy)``: the two strings
    are tokenised separately and concatenated; ``is_greedy`` says every
    continuation token is the model's top-1 at its position."""
    ctx = [int(i) for i in tokenizer.encode(context)]
    cont = [int(i) for i in tokenizer.encode(continuation)]
    if not ctx or not cont:
        raise ValueError("context and continuation must both tokenise to "
                         "at least one token")
    res = score(ctx + cont, tokenizer, model, top_n=1)
    total, greedy = 0.0, True
    for t in range(len(ctx), len(ctx) + len(cont)):
        total += res.logprobs[t]
        top = res.top[t]["top"]
        greedy = greedy and bool(top) and top[0]["id"] == res.token_ids[t]
    return total, greedy
