"""Token samplers.

Reference parity: the live sampler in the reference is min-p with
p_base=0.1 over an (unstabilized) softmax followed by ``torch.multinomial``
(``/root/reference/llama3.2_model.py:1000-1013``).  Here: stabilized
softmax, explicit generator for reproducibility, plus greedy /
temperature / top-k / top-p which the reference only had commented out
(``llama3.2_model.py:895-896``).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np


@dataclass
class SamplingParams:
    # "min_p" | "greedy" | "top_k" | "top_p" | "temperature" | "chain".
    # "chain" applies top_k, then top_p, then min_p together (each has an
    # "off" value: top_k <= 0, top_p >= 1, min_p <= 0); with the defaults
    # below all three are on.  Every other strategy reads its own field only.
    strategy: str = "min_p"
    min_p: float = 0.1
    temperature: float = 1.0
    top_k: int = 50
    top_p: float = 0.9
    seed: Optional[int] = None
    # OpenAI-style per-token logit offsets {token_id: bias}; applied to
    # the raw logits before temperature/filtering (+-100 ~ ban/force)
    logit_bias: Optional[dict] = None
    # history-aware processors, applied to the raw logits in this order
    # and BEFORE logit_bias (see apply_logit_processors):
    # HF-style repetition penalty over prompt + generated ids (> 0;
    # 1.0 = off), then OpenAI-style frequency / presence penalties over
    # the generated ids only (0.0 = off)
    repetition_penalty: float = 1.0
    frequency_penalty: float = 0.0
    presence_penalty: float = 0.0


def active_processors(params: "SamplingParams") -> frozenset:
    """Names of the logit processors ``params`` actually switches on."""
    act = set()
    if params.repetition_penalty != 1.0:
        act.add("repetition_penalty")
    if params.frequency_penalty != 0.0:
        act.add("frequency_penalty")
    if params.presence_penalty != 0.0:
        act.add("presence_penalty")
    if params.logit_bias:
        act.add("logit_bias")
    return frozenset(act)


def has_processors(params: "SamplingParams") -> bool:
    """True when any penalty is off its identity value or a logit_bias
    is present — i.e. the logits row is edited before the sampler."""
    return bool(active_processors(params))


def apply_logit_processors(logits: np.ndarray, params: "SamplingParams",
                           prompt_ids=(), output_ids=()) -> np.ndarray:
    """Raw logits row -> the row the sampler reads.  Fixed order:

    1. repetition_penalty r over every id in prompt_ids or output_ids:
       ``l/r`` if ``l > 0`` else ``l*r`` (HF rule);
    2. with c[i] the count of i in output_ids only:
       ``l[i] -= frequency_penalty*c[i] + presence_penalty*(c[i] > 0)``;
    3. ``l[i] += logit_bias[i]``.

    fp32 arithmetic on a copy; without processors the input comes back
    as is."""
    if not has_processors(params):
        return logits
    logits = np.array(logits, dtype=np.float32, copy=True)
    V = len(logits)
    r = float(params.repetition_penalty)
    f = float(params.frequency_penalty)
    p = float(params.presence_penalty)
    if r <= 0.0:
        raise ValueError(f"repetition_penalty must be > 0, got {r}")
    out = np.asarray(list(output_ids), dtype=np.int64).reshape(-1)
    out = out[(out >= 0) & (out < V)]
    if r != 1.0:
        pr = np.asarray(list(prompt_ids), dtype=np.int64).reshape(-1)
        pr = pr[(pr >= 0) & (pr < V)]
        seen = np.unique(np.concatenate([pr, out]))
        l = logits[seen]
        logits[seen] = np.where(l > 0, l / np.float32(r), l * np.float32(r))
    if (f != 0.0 or p != 0.0) and len(out):
        c = np.bincount(out, minlength=V).astype(np.float32)
        logits -= np.float32(f) * c + np.float32(p) * (c > 0)
    return _apply_bias(logits, params)


def _apply_bias(logits: np.ndarray, params: "SamplingParams") -> np.ndarray:
    if not params.logit_bias:
        return logits
    logits = np.array(logits, dtype=np.float32, copy=True)
    for tid, b in params.logit_bias.items():
        t = int(tid)
        if 0 <= t < len(logits):
            logits[t] += float(b)
    return logits


def _softmax(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.float64)
    m = x.max()
    e = np.exp(x - m)
    return e / e.sum()


def filter_probs(logits: np.ndarray, params: SamplingParams,
                 prompt_ids=(), output_ids=()) -> np.ndarray:
    """The sampling DISTRIBUTION the strategy defines: temperature-scaled
    softmax with the strategy's support filter applied, renormalized.
    (fp64, sums to 1.)  ``sample_token`` draws from this; speculative
    sampling (runtime/speculative.py) needs the vector itself to compute
    accept ratios p(x)/q(x) and the residual distribution.  The logit
    processors (penalties over ``prompt_ids`` / ``output_ids``, then
    logit_bias) apply first, so every consumer (host sampler,
    speculative accept/reject) sees the same adjusted distribution."""
    logits = apply_logit_processors(logits, params, prompt_ids, output_ids)
    if params.strategy == "greedy":
        p = np.zeros(len(logits), dtype=np.float64)
        p[int(np.argmax(logits))] = 1.0
        return p
    if params.temperature != 1.0:
        logits = logits / max(params.temperature, 1e-6)
    probs = _softmax(logits)
    if params.strategy == "min_p":
        # keep tokens with p >= min_p * p_max (reference: 0.1 * p_max,
        # llama3.2_model.py:1004-1008)
        keep = probs >= params.min_p * probs.max()
        probs = np.where(keep, probs, 0.0)
    elif params.strategy == "top_k":
        k = min(params.top_k, len(probs))
        thresh = np.partition(probs, -k)[-k]
        probs = np.where(probs >= thresh, probs, 0.0)
    elif params.strategy == "top_p":
        order = np.argsort(-probs)
        csum = np.cumsum(probs[order])
        cutoff = np.searchsorted(csum, params.top_p) + 1
        mask = np.zeros_like(probs, dtype=bool)
        mask[order[:cutoff]] = True
        probs = np.where(mask, probs, 0.0)
    elif params.strategy == "chain":
        probs = _chain_filter(probs, params)
    elif params.strategy != "temperature":
        raise ValueError(f"unknown sampling strategy {params.strategy!r}")
    return probs / probs.sum()


def _chain_filter(probs: np.ndarray, params: SamplingParams) -> np.ndarray:
    """top-k -> top-p (over the renormalised top-k survivors) -> min-p on
    a softmax vector; each step is the single-filter branch of
    ``filter_probs`` on what the step before kept, so a chain with one
    filter on is that strategy's vector.  Not renormalised."""
    if not 0.0 < params.top_p:
        raise ValueError(f"top_p must be > 0, got {params.top_p}")
    if not params.min_p <= 1.0:
        raise ValueError(f"min_p must be <= 1, got {params.min_p}")
    p_max = probs.max()
    k_on = 0 < params.top_k < len(probs)  # k >= V keeps the whole row
    if k_on:
        thresh = np.partition(probs, -params.top_k)[-params.top_k]
        probs = np.where(probs >= thresh, probs, 0.0)
    if params.top_p < 1.0:
        renorm = probs / probs.sum() if k_on else probs
        order = np.argsort(-renorm)
        csum = np.cumsum(renorm[order])
        cutoff = np.searchsorted(csum, params.top_p) + 1
        mask = np.zeros_like(probs, dtype=bool)
        mask[order[:cutoff]] = True
        probs = np.where(mask, probs, 0.0)
    if params.min_p > 0.0:
        # p_max survives both steps above, so the cut is that of "min_p"
        probs = np.where(probs >= params.min_p * p_max, probs, 0.0)
    return probs


def device_sampler_kwargs(params: SamplingParams) -> dict:
    """Engine keyword arguments (``generate_tokens`` / ``prefill_row`` /
    ``decode_rows``) that make the in-graph device sampler draw from the
    distribution ``filter_probs`` defines for ``params``.  greedy and
    min_p yield exactly ``greedy`` / ``min_p`` / ``temperature``, so
    engines that predate the device-side filters keep working; the filter
    keys appear only for the strategies that need them.  ``processors``
    (the penalties and logit_bias of the device logit-adjust stage)
    appears only when ``has_processors(params)``; callers send such a
    request to the device only when the engine lists every active one
    in ``device_processors``.  (``seed`` is not part of this keyword
    set: it travels in ``device_row_sampler_kwargs``, to engines that
    advertise ``device_row_sampler``.)"""
    kw = dict(greedy=params.strategy == "greedy", min_p=params.min_p,
              temperature=params.temperature)
    if has_processors(params):
        kw["processors"] = dict(
            repetition_penalty=float(params.repetition_penalty),
            frequency_penalty=float(params.frequency_penalty),
            presence_penalty=float(params.presence_penalty),
            logit_bias=dict(params.logit_bias) if params.logit_bias
            else None)
    if params.strategy in ("greedy", "min_p"):
        return kw
    kw["min_p"] = 0.0  # empty min-p cut: the whole vocabulary stays
    if params.strategy == "top_k":
        kw["top_k"] = max(1, int(params.top_k))
    elif params.strategy == "top_p":
        if not 0.0 < params.top_p:
            raise ValueError(f"top_p must be > 0, got {params.top_p}")
        kw["top_p"] = min(1.0, float(params.top_p))
    elif params.strategy == "chain":
        # composed cuts exist on the per-row sampler only: the legacy
        # values are not used when a ``row_sampler`` goes with them
        pass
    elif params.strategy != "temperature":
        raise ValueError(f"unknown sampling strategy {params.strategy!r}")
    return kw


def device_row_sampler_kwargs(params: SamplingParams) -> dict:
    """The ``row_sampler`` dict of engines that advertise
    ``device_row_sampler`` (``generate_tokens`` / ``prefill_row``): the
    request's own sampler settings as per-row device data, drawing from
    the distribution ``filter_probs`` defines for ``params``.  Same rules
    as ``device_sampler_kwargs``: ``temperature`` and ``top_p`` >= 1 are a
    min-p cut with ``min_p = 0`` (the whole vocabulary stays), ``top_k``
    is at least 1 (the engine clamps it to the vocabulary).  ``seed`` is
    the request's seed (None: the engine derives one per request).
    ``"chain"`` carries all three filter values with the off-rules
    applied: ``top_k`` 0 = off (the engine also treats >= vocabulary as
    off), ``top_p`` 1.0 = off, ``min_p`` 0.0 = off."""
    kw = dict(strategy=params.strategy,
              temperature=float(params.temperature), seed=params.seed)
    if params.strategy == "min_p":
        kw["min_p"] = float(params.min_p)
    elif params.strategy == "top_k":
        kw["top_k"] = max(1, int(params.top_k))
    elif params.strategy == "top_p":
        if not 0.0 < params.top_p:
            raise ValueError(f"top_p must be > 0, got {params.top_p}")
        if params.top_p >= 1.0:
            kw.update(strategy="min_p", min_p=0.0)
        else:
            kw["top_p"] = float(params.top_p)
    elif params.strategy == "temperature":
        kw.update(strategy="min_p", min_p=0.0)
    elif params.strategy == "chain":
        if not 0.0 < params.top_p:
            raise ValueError(f"top_p must be > 0, got {params.top_p}")
        if not params.min_p <= 1.0:
            raise ValueError(f"min_p must be <= 1, got {params.min_p}")
        kw.update(top_k=max(0, int(params.top_k)),
                  top_p=min(1.0, float(params.top_p)),
                  min_p=max(0.0, float(params.min_p)))
    elif params.strategy != "greedy":
        raise ValueError(f"unknown sampling strategy {params.strategy!r}")
    return kw


def sample_token(logits: np.ndarray, params: SamplingParams,
                 rng: Optional[np.random.Generator] = None,
                 prompt_ids=(), output_ids=()) -> int:
    """logits: (vocab,) fp32. Returns a token id (int).  ``prompt_ids``
    / ``output_ids`` feed the penalties (apply_logit_processors)."""
    if params.strategy == "greedy":
        return int(np.argmax(apply_logit_processors(
            logits, params, prompt_ids, output_ids)))
    if rng is None:
        rng = np.random.default_rng(params.seed)
    probs = filter_probs(logits, params, prompt_ids, output_ids)
    return int(rng.choice(len(probs), p=probs))
