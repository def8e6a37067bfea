"""GPU inference engine: Llama-3.2 / Gemma-2 forward on hand-written
CDNA4 HIP kernels, PyTorch tensors as memory containers only.

MI355X-first design (SURVEY §7 stages 2-4):
  - every compute op is a kernel from ``csrc/llm_ops.hip`` — no ATen math
    in the forward pass, no eager fallback (ops fail loudly if the
    extension is missing);
  - preallocated KV pool per layer (in-place writes, no concat);
  - decode state (seq length, sampled token, RNG counter, output ring)
    lives in device memory so a decode step is hipGraph-replayable with
    zero host round-trips (torch.cuda.CUDAGraph == hipGraph on ROCm);
  - tensor parallelism: head/row/col-sharded weights per rank, RCCL
    all-reduce after o_proj and down_proj, all-gather for logits
    (world_size==1 skips collectives — same code path).

Reference parity: this replaces the CuPy model classes
(``/root/reference/llama3.2_model.py:334-822``) — same capability
(forward with KV cache, returns logits), built from the architectural
spec in SURVEY §2.4 rather than translated.
"""

from __future__ import annotations

import gc
from functools import partial
from typing import Dict, Optional

import numpy as np
import torch

from ..core.config import ModelConfig
from ..ops import hip_ops as ho
from ..parallel import tp as tpu
from ..utils.tracing import trace_range
from .decode_spec import RowState, SampleSpec


class DeviceCacheHandle:
    """Host-side mirror of the device seq-length (generate()-compatible)."""

    def __init__(self, engine):
        self.engine = engine
        self.seq_len = 0


class GPUModel:
    # sampling strategies the in-graph device sampler implements; the
    # runtime (generate(), the server's batch scheduler) routes on this
    # ("chain" is served through ``row_sampler`` only)
    device_strategies = frozenset(
        {"greedy", "min_p", "top_k", "top_p", "temperature", "chain"})
    # logit processors the in-graph logit-adjust stage applies (set per
    # instance: everything at world == 1, nothing under tensor parallel)
    device_processors = frozenset()
    # largest top-N the in-graph logprob stage reports per token (set per
    # instance: LOGPROBS_MAX_TOP at world == 1, 0 under tensor parallel)
    device_logprobs = 0
    # the sampler reads strategy / temperature / filter / seed per row
    # from device memory (``row_sampler=``): requests with different
    # sampler settings share one lockstep group and one captured graph,
    # and ``seed`` is honored (set per instance: True at world == 1)
    device_row_sampler = False
    # greedy speculative decoding runs device-side with this engine as
    # target or draft (``speculative_tokens``; set per instance: True at
    # world == 1 without MoE)
    device_speculative = False
    # verify cycles a speculative chunk runs between two host reads
    # (profiles/spec_device.md)
    SPEC_CHUNK = 4

    def __init__(self, config: ModelConfig, weights: Dict[str, np.ndarray],
                 dtype: str = "bf16", max_seq: Optional[int] = 4096,
                 prefill_chunk: int = 2048, device: Optional[str] = None,
                 seed: int = 0, force_tp_path: bool = False,
                 kv_dtype: str = "bf16", max_batch: int = 1):
        """``max_seq=None`` sizes the KV pool from FREE HBM after the
        weights land (288 GB per MI355X — SURVEY §5 long-context), capped
        at config.max_position_embeddings.  ``max_batch>1`` allocates
        per-sequence KV pools for lockstep batched decode
        (prefill_batch/decode_batch; beyond-parity serving capability)."""
        if not torch.cuda.is_available():
            raise RuntimeError("GPUModel requires a GPU (MI355X)")
        self.config = config
        self.seed = seed
        assert 1 <= max_batch <= 256
        self.max_batch = max_batch
        self._pb = 0  # current sequence row during per-sequence prefill
        self.dtype = dtype
        if dtype not in ("bf16", "fp8", "fp4"):
            raise ValueError(f"unsupported dtype {dtype!r}")
        # fp4 = MXFP4 weights on the single-sequence DECODE GEMVs (half
        # the fp8 stream); prefill and batched decode run on the fp8
        # copy (the fp8 machinery flag covers both quantized modes)
        self.fp8 = dtype in ("fp8", "fp4")
        self.wq4 = dtype == "fp4"
        # fp4 + batch pools: the skinny MFMA GEMM consumes fp8, so keep
        # the fp8 copy only then; max_batch=1 fp4 engines are SINGLE-COPY
        self.keep_fp8 = (dtype == "fp8") or (self.wq4 and max_batch > 1)
        if kv_dtype not in ("bf16", "fp8"):
            raise ValueError(f"unsupported kv_dtype {kv_dtype!r}")
        self.kv_dtype = kv_dtype
        self.kv8 = kv_dtype == "fp8"  # e4m3 KV pool, per-(head,pos) scales
        # Mixtral sparse MoE: per-token top-k routed experts (decode:
        # expert-indexed GEMVs off device idx; prefill: dense per-expert
        # GEMM loop weighted by router probs)
        self.moe = config.is_moe
        self.topk = config.num_experts_per_tok
        if self.moe:
            if self.wq4:
                raise ValueError("MoE + fp4 weights not supported yet")
            if config.model_type == "gemma2":
                raise ValueError("MoE is a llama-family (Mixtral) feature")
        self.rank, self.world = tpu.init_distributed()
        # exercise the TP code path on 1 GPU (collectives no-op at
        # world=1, partial sums are then exact) — used by tests
        self.tp_branch = self.world > 1 or force_tp_path
        if self.world == 1:
            self.device_processors = frozenset(
                {"logit_bias", "repetition_penalty", "frequency_penalty",
                 "presence_penalty"})
        # logit-adjust state (stat / proc / bias rows): allocated by the
        # first request that brings processors, never otherwise
        self.p_stat = self.p_proc = self.p_bias = None
        # host mirror of the device rows: slot -> bias_on, for every
        # slot whose proc row is not identity (compact_row moves only
        # what a row actually has; a stale entry is cleared by the next
        # prefill_row into that slot)
        self._proc_rows = {}
        if self.world == 1:
            self.device_logprobs = ho.LOGPROBS_MAX_TOP
        # logprob state (cfg / stage / scan scratch / record rings, raw
        # snapshot): allocated by the first request that asks for
        # logprobs.  _lp_rows: slot -> top-N of every row that is on
        self.lp_cfg = self.lp_stage = self.lp_part = None
        self.lp_val = self.lp_idx = self.lp_raw = None
        self._lp_rows = {}
        self._lp_batch = False  # records follow bt_nout (else nout)
        self.last_logprobs = None
        # prompt scoring (prompt_logprobs): 0 under TP — the vocabulary is
        # sharded, callers take the host path; scratch on first use
        self.device_prompt_logprobs = \
            ho.LOGPROBS_MAX_TOP if self.world == 1 else 0
        self.pl_logits = self.pl_tgt = self.pl_val = self.pl_idx = None
        # speculative verify state (logits / scratch / record ring):
        # allocated by the first verify pass
        self.device_speculative = self.world == 1 and not self.moe
        self.sp_logits = self.sp_scratch = self.sp_rec = self.sp_nrec = None
        if self.world == 1:
            self.device_row_sampler = True
        # host mirror of the per-row sampler table: slot -> mode of every
        # lockstep slot set up with ``row_sampler`` (the launcher is told
        # which stages the rows present need); _req_serial numbers the
        # requests that came without a seed of their own
        self._samp_modes = {}
        self._req_serial = 0
        # slot -> ``ho.samp_row_chain`` bits of every composed row (a
        # second filter beside its mode's): what the sampler launches on
        # top of the modes while such a row is present
        self._samp_chain = {}
        # mode set of the single-sequence table row (all zero = greedy)
        # and that row's chain bits
        self._s_rows = frozenset({0})
        self._s_chain = 0
        # host mirrors of len_buf / bt_lens (overflow guards) and the
        # number of lockstep rows in use
        self._host_len = 0
        self._host_lens = [0] * max_batch
        self._batch_n = 0
        if device is None:
            device = f"cuda:{self.rank % max(torch.cuda.device_count(), 1)}"
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)

        cfg = config
        tp = self.world
        assert cfg.num_attention_heads % tp == 0, "nh must divide tp"
        assert cfg.num_key_value_heads % tp == 0, \
            f"kv heads {cfg.num_key_value_heads} not divisible by tp {tp}"
        assert cfg.intermediate_size % tp == 0
        assert cfg.vocab_size % tp == 0
        if self.moe and tp > 1:
            raise ValueError("MoE tensor parallelism (expert parallel) "
                             "is not implemented yet — run TP=1")
        self.nh_l = cfg.num_attention_heads // tp
        self.kvh_l = cfg.num_key_value_heads // tp
        self.inter_l = cfg.intermediate_size // tp
        self.vocab_l = cfg.vocab_size // tp
        self.hd = cfg.head_dim
        self.H = cfg.hidden_size

        # one-shot xGMI collectives for decode-sized payloads (validated
        # on hardware at init; silent RCCL fallback when unavailable)
        if self.world > 1:
            slot_bytes = max(self.H * 2, self.vocab_l * 4, 1 << 16)
            tpu.init_xgmi(self.device, slot_bytes)
        # prefill-sized all-reduces: RCCL async on its own stream,
        # overlapped with the next row-chunk's GEMM (north star: comm
        # overlap on a second HIP stream).  Needs the nccl(=RCCL)
        # backend; gloo (CPU CI) takes the inline path.
        import torch.distributed as dist
        self._async_ar = bool(
            self.world > 1 and dist.is_initialized()
            and "nccl" in str(dist.get_backend()).lower())

        self._upload_weights(weights)
        if max_seq is None:
            max_seq = self._auto_max_seq()
        self.max_seq = max_seq
        self._alloc_state(prefill_chunk)
        # single-slot graph of decode / decode_batch, per-key graphs of
        # decode_rows; a failed capture switches capturing off for good
        self._graph = None
        self._graph_mode = None
        self._bgraphs = {}
        self._graph_failed = False
        self._graph_error = None
        self._plan_attn_pf()

    def _plan_attn_pf(self):
        """Weight prefetch carried by the decode attention launch
        (`ho.attn_dec_pf`): per-layer regions, computed once here.
        LLM_ATTN_PF = byte budget per layer, 0 = off, default `auto`
        (o_proj's matrix when it fits the attention window, see
        `attn_prefetch.default_budget`); LLM_ATTN_PF_BLOCKS = prefetch
        blocks per launch (default 4 grid rows of nh).  Measured in
        profiles/attn_prefetch.md."""
        import os as _os
        from .attn_prefetch import (consumer_stride, default_budget,
                                    plan_attn_prefetch)
        self._attn_pf = None
        _b = _os.environ.get("LLM_ATTN_PF", "auto").strip().lower()
        if _b in ("", "0") or self.moe:
            return
        sfx = "_q4" if self.wq4 else "_q" if self.fp8 else ""
        plans = []
        for lw in self.layers:
            wo, wgu = lw["wo" + sfx], lw["wgu" + sfx]
            nb = {"wo": wo.numel() * wo.element_size(),
                  "wgu": wgu.numel() * wgu.element_size()}
            budget = (default_budget(nb["wo"], nb["wgu"]) if _b == "auto"
                      else int(_b))
            base = {"wo": wo.data_ptr(), "wgu": wgu.data_ptr()}
            plans.append([(base[n] + off, size) for n, off, size in
                          plan_attn_prefetch(nb["wo"], nb["wgu"],
                                             self.inter_l, self.H, budget)])
            # o_proj block b owns 4 consecutive rows of wo
            self.attn_pf_stride = consumer_stride(nb["wo"], self.H, 4)
        _n = _os.environ.get("LLM_ATTN_PF_BLOCKS")
        self.attn_pf_blocks = int(_n) if _n else 4 * self.nh_l
        if self.attn_pf_blocks > 0 and any(plans):
            self._attn_pf = plans
            self._pf_sink = torch.zeros(256, dtype=torch.float32,
                                        device=self.device)

    # ------------------------------------------------------------------
    def _auto_max_seq(self) -> int:
        """KV pool length from free HBM (post-weights): fill the 288 GB
        MI355X budget instead of a fixed 4k default,
        capped at the model's max_position_embeddings."""
        cfg = self.config
        free, _total = torch.cuda.mem_get_info(self.device)
        esz = 1 if self.kv8 else 2
        per_pos = (cfg.num_hidden_layers * self.kvh_l * self.hd * 2 * esz
                   * self.max_batch)
        if self.kv8:
            per_pos += (cfg.num_hidden_layers * self.kvh_l * 2 * 4
                        * self.max_batch)  # scales
        per_pos += self.hd * 4 + 8  # rope tables + ring slot
        budget = int(free * 0.9) - (2 << 30)  # headroom for scratch/graph
        n = max(1024, budget // max(per_pos, 1))
        return int(min(cfg.max_position_embeddings, n))

    def _upload_weights(self, w: Dict[str, np.ndarray]):
        from ..io.loader import validate_weights

        validate_weights(self.config, w)  # actionable error vs KeyError
        cfg, dev = self.config, self.device
        tp, r = self.world, self.rank
        gemma = cfg.model_type == "gemma2"

        def bf16(a: np.ndarray) -> torch.Tensor:
            return torch.from_numpy(np.ascontiguousarray(a)).to(
                dev, torch.bfloat16, non_blocking=False)

        def gamma(a: np.ndarray) -> torch.Tensor:
            g = a.astype(np.float32) + (1.0 if gemma else 0.0)
            return torch.from_numpy(g).to(dev)

        def quant4(a: np.ndarray):
            """MXFP4: e2m1 packed 2/byte + e8m0 scale per 32 elems."""
            t = bf16(a)
            N, K = t.shape
            q = torch.empty(N, K // 2, dtype=torch.uint8, device=dev)
            e = torch.empty(N, K // 32, dtype=torch.uint8, device=dev)
            ho.quant_fp4(t, q, e)
            torch.cuda.synchronize()
            return q, e

        def quant8(a: np.ndarray):
            """Per-output-row e4m3fn quantization ON DEVICE (k_quant_
            fp8_rows): one bf16 upload, quantize, drop the bf16 copy —
            fp8 models hold a single weight copy in HBM and load in
            seconds (round-1 host quant took ~90 s for 9B)."""
            t = bf16(a)
            N, K = t.shape
            q = torch.empty(N, K, dtype=torch.uint8, device=dev)
            s = torch.empty(N, dtype=torch.float32, device=dev)
            ho.quant_fp8(t, q, s)
            torch.cuda.synchronize()  # t freed right after
            return q, s

        self.embed = bf16(w["model.embed_tokens.weight"])
        lm_w = w.get("lm_head.weight", w["model.embed_tokens.weight"])
        if self.fp8:
            lmw = lm_w if tp == 1 else tpu.shard_rows(lm_w, r, tp)
            if self.keep_fp8:
                self.lm_head_q, self.lm_head_s = quant8(lmw)
            self.lm_head = None  # single-copy: no bf16 duplicate
            if self.wq4:
                self.lm_head_q4, self.lm_head_e4 = quant4(lmw)
        elif tp > 1:
            self.lm_head = bf16(tpu.shard_rows(lm_w, r, tp))
        elif lm_w is w.get("model.embed_tokens.weight", None) or \
                cfg.tie_word_embeddings and "lm_head.weight" not in w:
            self.lm_head = self.embed  # tied, share device memory
        else:
            self.lm_head = bf16(lm_w)
        self.g_final = gamma(w["model.norm.weight"])

        hd = cfg.head_dim
        self.layers = []
        for i in range(cfg.num_hidden_layers):
            p = f"model.layers.{i}"
            a = f"{p}.self_attn"
            hrows = lambda x: tpu.shard_rows(x, r, tp) if tp > 1 else x
            hcols = lambda x: tpu.shard_cols(x, r, tp) if tp > 1 else x
            import numpy as _np
            qkv_np = _np.concatenate([
                hrows(w[f"{a}.q_proj.weight"]),
                hrows(w[f"{a}.k_proj.weight"]),
                hrows(w[f"{a}.v_proj.weight"])], axis=0)
            if self.moe:
                # stacked per-expert [gate; up] rows (E*2I, H) and down
                # rows (E*H, I) — ONE device tensor per projection so the
                # decode GEMV can index expert e as a row offset
                # (eidx * 2I resp. eidx * H) off a device int32
                m = f"{p}.block_sparse_moe"
                E = cfg.num_local_experts
                gu_np = _np.concatenate(
                    [x for e in range(E)
                     for x in (w[f"{m}.experts.{e}.w1.weight"],
                               w[f"{m}.experts.{e}.w3.weight"])], axis=0)
                down_np = _np.concatenate(
                    [w[f"{m}.experts.{e}.w2.weight"] for e in range(E)],
                    axis=0)
            else:
                gu_np = _np.concatenate([
                    hrows(w[f"{p}.mlp.gate_proj.weight"]),
                    hrows(w[f"{p}.mlp.up_proj.weight"])], axis=0)
                down_np = hcols(w[f"{p}.mlp.down_proj.weight"])
            o_np = hcols(w[f"{a}.o_proj.weight"])
            nq = self.nh_l * hd
            nkv = self.kvh_l * hd
            I = self.inter_l
            lw = {
                "g_in": gamma(w[f"{p}.input_layernorm.weight"]),
                "g_post": gamma(w[f"{p}.post_attention_layernorm.weight"]),
            }
            if self.fp8:
                # SINGLE fp8 copy: decode GEMV and prefill fp8-MFMA GEMM
                # both read these (no bf16 duplicate in HBM)
                for name, arr in [("wqkv", qkv_np), ("wgu", gu_np),
                                  ("wo", o_np), ("wdown", down_np)]:
                    if self.keep_fp8:
                        lw[name + "_q"], lw[name + "_s"] = quant8(arr)
                    if self.wq4:
                        lw[name + "_q4"], lw[name + "_e4"] = quant4(arr)
                if self.keep_fp8:
                    lw.update({
                        "wq_q": lw["wqkv_q"][:nq],
                        "wq_s": lw["wqkv_s"][:nq],
                        "wk_q": lw["wqkv_q"][nq:nq + nkv],
                        "wk_s": lw["wqkv_s"][nq:nq + nkv],
                        "wv_q": lw["wqkv_q"][nq + nkv:],
                        "wv_s": lw["wqkv_s"][nq + nkv:],
                        "wgate_q": lw["wgu_q"][:I],
                        "wgate_s": lw["wgu_s"][:I],
                        "wup_q": lw["wgu_q"][I:], "wup_s": lw["wgu_s"][I:],
                    })
                if self.wq4:
                    lw.update({
                        "wq_q4": lw["wqkv_q4"][:nq],
                        "wq_e4": lw["wqkv_e4"][:nq],
                        "wk_q4": lw["wqkv_q4"][nq:nq + nkv],
                        "wk_e4": lw["wqkv_e4"][nq:nq + nkv],
                        "wv_q4": lw["wqkv_q4"][nq + nkv:],
                        "wv_e4": lw["wqkv_e4"][nq + nkv:],
                        "wgate_q4": lw["wgu_q4"][:I],
                        "wgate_e4": lw["wgu_e4"][:I],
                        "wup_q4": lw["wgu_q4"][I:],
                        "wup_e4": lw["wgu_e4"][I:],
                    })
            else:
                wqkv = bf16(qkv_np)
                wgu = bf16(gu_np)
                lw.update({
                    # fused tensors (decode path) + contiguous row views
                    "wqkv": wqkv,
                    "wq": wqkv[:nq], "wk": wqkv[nq:nq + nkv],
                    "wv": wqkv[nq + nkv:],
                    "wgu": wgu, "wgate": wgu[:I], "wup": wgu[I:],
                    "wo": bf16(o_np),
                    "wdown": bf16(down_np),
                })
            if self.moe:
                # router weights + decode-shaped views: the GEMV sees the
                # FIRST expert's rows (N=2I / N=H) and offsets the base
                # pointer by eidx * wstride device-side
                lw["wg"] = bf16(w[f"{p}.block_sparse_moe.gate.weight"])
                I2, H2 = 2 * self.inter_l, self.H
                if self.fp8:
                    lw["wgu_q_all"] = lw.pop("wgu_q")
                    lw["wgu_s_all"] = lw.pop("wgu_s")
                    lw["wdown_q_all"] = lw.pop("wdown_q")
                    lw["wdown_s_all"] = lw.pop("wdown_s")
                    lw["wgu_q"] = lw["wgu_q_all"][:I2]
                    lw["wgu_s"] = lw["wgu_s_all"][:I2]
                    lw["wdown_q"] = lw["wdown_q_all"][:H2]
                    lw["wdown_s"] = lw["wdown_s_all"][:H2]
                else:
                    lw["wgu_all"] = lw.pop("wgu")
                    lw["wdown_all"] = lw.pop("wdown")
                    lw["wgu"] = lw["wgu_all"][:I2]
                    lw["wdown"] = lw["wdown_all"][:H2]
            if gemma:
                lw["g_preffn"] = gamma(w[f"{p}.pre_feedforward_layernorm.weight"])
                lw["g_postffn"] = gamma(w[f"{p}.post_feedforward_layernorm.weight"])
            if cfg.attention_bias:
                # Qwen-2 family: fused qkv bias (decode GEMV adds it via
                # the res slot; prefill adds it after the GEMM)
                bias_np = _np.concatenate([
                    hrows(w[f"{a}.q_proj.bias"]),
                    hrows(w[f"{a}.k_proj.bias"]),
                    hrows(w[f"{a}.v_proj.bias"])], axis=0)
                bqkv = bf16(bias_np.reshape(1, -1))[0]
                lw["bqkv"] = bqkv
                lw["bias_q"] = bqkv[:nq]
                lw["bias_k"] = bqkv[nq:nq + nkv]
                lw["bias_v"] = bqkv[nq + nkv:]
            self.layers.append(lw)

    def _alloc_state(self, prefill_chunk: int):
        cfg, dev = self.config, self.device
        S, hd = self.max_seq, self.hd
        L = cfg.num_hidden_layers
        bf = dict(dtype=torch.bfloat16, device=dev)
        kvt = torch.uint8 if self.kv8 else torch.bfloat16
        B = self.max_batch
        kv_shape = (self.kvh_l, S, hd) if B == 1 else (B, self.kvh_l, S, hd)
        self.k_cache = [torch.zeros(*kv_shape, dtype=kvt, device=dev)
                        for _ in range(L)]
        self.v_cache = [torch.zeros(*kv_shape, dtype=kvt, device=dev)
                        for _ in range(L)]
        if self.kv8:
            ks = (self.kvh_l, S) if B == 1 else (B, self.kvh_l, S)
            self.k_scale = [torch.zeros(*ks, dtype=torch.float32,
                                        device=dev) for _ in range(L)]
            self.v_scale = [torch.zeros(*ks, dtype=torch.float32,
                                        device=dev) for _ in range(L)]
        else:
            self.k_scale = [None] * L
            self.v_scale = [None] * L

        # RoPE tables fp32 (host-precomputed: guide App.B — no device trig)
        inv = cfg.rope_inv_freq()                      # (hd/2,) fp64
        t = np.arange(S, dtype=np.float64)
        freqs = np.outer(t, inv)
        self.cos_t = torch.from_numpy(np.cos(freqs).astype(np.float32)).to(dev)
        self.sin_t = torch.from_numpy(np.sin(freqs).astype(np.float32)).to(dev)

        PC = self.PC = min(prefill_chunk, max(256, self.max_seq))
        H, I = self.H, self.inter_l
        self.b_h = torch.zeros(PC, H, **bf)
        self.b_xn = torch.zeros(PC, H, **bf)
        self.b_t1 = torch.zeros(PC, H, **bf)
        self.b_q = torch.zeros(PC, self.nh_l * hd, **bf)
        self.b_k = torch.zeros(PC, self.kvh_l * hd, **bf)
        self.b_v = torch.zeros(PC, self.kvh_l * hd, **bf)
        self.b_att = torch.zeros(PC, self.nh_l * hd, **bf)
        self.b_gate = torch.zeros(PC, I, **bf)
        self.b_up = torch.zeros(PC, I, **bf)
        self.b_gemm_acc = torch.zeros(PC * max(I, H), dtype=torch.float32,
                                      device=dev)
        if self.fp8:
            # activation-quant scratch for the fp8 MFMA prefill GEMMs
            kmax = max(H, I, self.nh_l * hd)
            self.b_xq = torch.zeros(PC * kmax, dtype=torch.uint8, device=dev)
            self.b_sx = torch.zeros(PC, dtype=torch.float32, device=dev)
        self.b_logits_l = torch.zeros(self.vocab_l, dtype=torch.float32,
                                      device=dev)
        self.b_logits = (self.b_logits_l if not self.tp_branch else
                         torch.zeros(cfg.vocab_size, dtype=torch.float32,
                                     device=dev))
        self.b_qkv = torch.zeros((self.nh_l + 2 * self.kvh_l) * hd, **bf)
        if self.moe:
            E = cfg.num_local_experts
            self.moe_idx = torch.zeros(PC * self.topk, dtype=torch.int32,
                                       device=dev)
            self.moe_w = torch.zeros(PC * self.topk, dtype=torch.float32,
                                     device=dev)
            self.moe_dense = torch.zeros(PC * E, dtype=torch.float32,
                                         device=dev)
        self.b_hb = torch.zeros(H, **bf)   # gemma residual ping-pong
        self.b_t2 = torch.zeros(H, **bf)   # gemma ffn-out delta
        self.b_gu = torch.zeros(2 * I, **bf)
        # split-T decode attention scratch (partials + per-head tickets)
        import os as _os
        _sp = _os.environ.get("LLM_ATTN_SPLIT")
        # measured (fp8 llama-1b): T~100 split2 1493 > split4 1483;
        # T~4k split8 1108 > split16 1050; T~8k split16 963 > split32
        self.attn_split = (int(_sp) if _sp else
                           min(16, max(2, self.max_seq // 512)))
        # how a head's chunks combine (ho.attn_dec `merge`): same bits
        # either way; "auto" is one block per head while split <= 4
        self.attn_merge = _os.environ.get("LLM_ATTN_MERGE") or "auto"
        if self.attn_merge not in ho.ATTN_MERGE:
            raise ValueError(f"LLM_ATTN_MERGE must be one of "
                             f"{sorted(ho.ATTN_MERGE)}, got "
                             f"{self.attn_merge!r}")
        self.attn_scratch = torch.zeros(
            self.nh_l * self.attn_split * (hd + 2), dtype=torch.float32,
            device=dev)
        self.attn_cnt = torch.zeros(self.nh_l, dtype=torch.int32, device=dev)
        self.s_gmax = torch.zeros(1, dtype=torch.int64, device=dev)
        self.s_pick = torch.zeros(1, dtype=torch.int64, device=dev)
        self.s_cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        # top-k / top-p selection scratch (radix-select state + histogram)
        self.s_sel = torch.zeros(1, ho.SAMPLE_SEL_WORDS, dtype=torch.int64,
                                 device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.ids_buf = torch.zeros(PC, **i32)
        self.next_token = torch.zeros(1, **i32)
        self.out_ring = torch.zeros(max(65536, S + 16), **i32)
        self.nout = torch.zeros(1, **i32)
        self.len_buf = torch.zeros(1, **i32)
        self.rng_ctr = torch.zeros(1, dtype=torch.int64, device=dev)
        # per-row sampler table (mode, 1/T, min_p, top_k, top_p, seed,
        # draw counter) of the single-sequence path
        self.s_samp = torch.zeros(1, ho.SAMP_WORDS, **i32)
        # what the sampling tail works on: the single sequence's state ...
        self._sv = RowState(self.s_samp, self.s_gmax, self.s_pick,
                            self.s_cnt, self.s_sel, self.next_token,
                            self.out_ring, self.nout, self.len_buf)

        if self.max_batch > 1:
            B, nhh = self.max_batch, self.nh_l * hd
            i64 = dict(dtype=torch.int64, device=dev)
            self.bt_qkv = torch.zeros(B, (self.nh_l + 2 * self.kvh_l) * hd,
                                      **bf)
            self.bt_logits = torch.zeros(B, self.vocab_l, **bf)
            self.bt_logits32 = torch.zeros(B, cfg.vocab_size,
                                           dtype=torch.float32, device=dev)
            self.bt_next = torch.zeros(B, **i32)
            self.bt_lens = torch.zeros(B, **i32)  # ragged positions
            self.bt_ring = torch.zeros(B, S + 16, **i32)
            self.bt_nout = torch.zeros(B, **i32)
            self.bt_gmax = torch.zeros(B, **i64)
            self.bt_pick = torch.zeros(B, **i64)
            self.bt_cnt = torch.zeros(B, **i32)
            self.bt_sel = torch.zeros(B, ho.SAMPLE_SEL_WORDS, **i64)
            self.bt_samp = torch.zeros(B, ho.SAMP_WORDS, **i32)
            # ... and the lockstep rows'
            self._bv = RowState(self.bt_samp, self.bt_gmax, self.bt_pick,
                                self.bt_cnt, self.bt_sel, self.bt_next,
                                self.bt_ring, self.bt_nout, self.bt_lens)
            self.bt_scratch = torch.zeros(
                B * self.nh_l * self.attn_split * (hd + 2),
                dtype=torch.float32, device=dev)
            self.bt_attn_cnt = torch.zeros(B * self.nh_l, **i32)
            # fused multi-x path scratch (fp8, B<=8)
            self.bt_gu = torch.zeros(B, 2 * I, **bf)
            self.bt_t1 = torch.zeros(B, H, **bf)
            self.bt_t2 = torch.zeros(B, H, **bf)
            self.bt_hb = torch.zeros(B, H, **bf)

        self.act = 0 if cfg.hidden_act == "silu" else 1
        self.gemma = cfg.model_type == "gemma2"
        self.attn_softcap = float(cfg.attn_logit_softcapping or 0.0)
        self.final_softcap = float(cfg.final_logit_softcapping or 0.0)
        self.scale = float(cfg.attn_scale)

    # ------------------------------------------------------------------
    # cache interface (generate()-compatible)
    # ------------------------------------------------------------------
    def make_cache(self, n: int) -> DeviceCacheHandle:
        if n > self.max_seq:
            raise ValueError(f"requested cache {n} > max_seq {self.max_seq}")
        self.reset()
        return DeviceCacheHandle(self)

    def reset(self):
        self.len_buf.zero_()
        self.nout.zero_()
        self.rng_ctr.zero_()
        self.s_gmax.zero_()
        self.s_pick.zero_()
        self.s_cnt.zero_()
        self.s_sel.zero_()
        self._host_len = 0  # host mirror of len_buf (overflow guard)

    # ------------------------------------------------------------------
    # layer stack over rows [0, M) of the scratch buffers
    # ------------------------------------------------------------------
    def _linear(self, lw, name, x, y, res=None, M: int = 1,
                softcap: float = 0.0):
        """Projection by weight NAME so dtype routing stays in one
        place: bf16 GEMV/MFMA-GEMM, or (fp8) GEMV / fp8-MFMA GEMM with
        on-the-fly activation row quantization."""
        if M == 1:
            if self.wq4:
                ho.gemv_fp4(lw[name + "_q4"], lw[name + "_e4"], x, y,
                            res=res, softcap=softcap)
            elif self.fp8:
                ho.gemv_fp8(lw[name + "_q"], lw[name + "_s"], x, y,
                            res=res, softcap=softcap)
            else:
                ho.gemv(lw[name], x, y, res=res, softcap=softcap)
        elif self.wq4:
            ho.gemm_fp4w(x[:M], lw[name + "_q4"], lw[name + "_e4"], y[:M],
                         res=res[:M] if res is not None else None,
                         accbuf=self.b_gemm_acc)
        elif self.fp8:
            K = x.shape[-1]
            ho.quant_fp8(x[:M], self.b_xq, self.b_sx)
            ho.gemm_fp8(self.b_xq, self.b_sx, lw[name + "_q"],
                        lw[name + "_s"], y[:M], M, K,
                        res=res[:M] if res is not None else None,
                        accbuf=self.b_gemm_acc)
        else:
            ho.gemm(x[:M], lw[name], y, res=res[:M] if res is not None else None,
                    accbuf=self.b_gemm_acc)

    def _rowpar_ar(self, lw, name, x, y, M: int):
        """Row-parallel projection followed by all-reduce over TP ranks.
        For prefill-sized M the rows are split in two: the all-reduce of
        chunk A runs on RCCL's comm stream while chunk B's GEMM occupies
        the compute stream (SURVEY §2.3 'overlap comm on 2nd stream' —
        the reference has no distributed code at all)."""
        if not (self._async_ar and M >= 512):
            self._linear(lw, name, x, y, M=M)
            tpu.all_reduce(y[:M])
            return
        import torch.distributed as dist
        K = x.shape[-1]
        if self.fp8 and not self.wq4:
            ho.quant_fp8(x[:M], self.b_xq, self.b_sx)
        works = []
        M2 = M // 2
        for a, b in ((0, M2), (M2, M)):
            if self.wq4:
                ho.gemm_fp4w(x[a:b], lw[name + "_q4"], lw[name + "_e4"],
                             y[a:b], accbuf=self.b_gemm_acc)
            elif self.fp8:
                ho.gemm_fp8(self.b_xq[a * K:], self.b_sx[a:],
                            lw[name + "_q"], lw[name + "_s"], y[a:b],
                            b - a, K, accbuf=self.b_gemm_acc)
            else:
                ho.gemm(x[a:b], lw[name], y[a:b], accbuf=self.b_gemm_acc)
            # async -> lands on the RCCL stream after the chunk's GEMM;
            # the compute stream proceeds to the next chunk immediately
            works.append(dist.all_reduce(y[a:b], async_op=True))
        for wk in works:
            wk.wait()  # compute stream waits on the comm stream

    def _kc(self, i):
        return self.k_cache[i] if self.max_batch == 1 else \
            self.k_cache[i][self._pb]

    def _vc(self, i):
        return self.v_cache[i] if self.max_batch == 1 else \
            self.v_cache[i][self._pb]

    def _ks(self, i):
        s = self.k_scale[i]
        return s if (s is None or self.max_batch == 1) else s[self._pb]

    def _vs(self, i):
        s = self.v_scale[i]
        return s if (s is None or self.max_batch == 1) else s[self._pb]

    def _layers_forward(self, M: int, layer_hook=None,
                        batch_attn: bool = False):
        """Layer stack over rows [0, M).  ``batch_attn``: rows are M
        INDEPENDENT sequences at the same position (lockstep batched
        decode) — the fused decode-attention kernel runs per row over
        per-sequence KV pools instead of the prefill attention."""
        cfg = self.config
        eps = cfg.rms_norm_eps
        h, xn, t1 = self.b_h, self.b_xn, self.b_t1
        if layer_hook is not None:
            layer_hook(-1, h[:M])  # embedding output
        for i, lw in enumerate(self.layers):
            window = cfg.sliding_window if cfg.is_sliding(i) else 0
            ho.rmsnorm(h[:M], lw["g_in"], xn[:M], eps=eps)
            if batch_attn:
                self._linear(lw, "wqkv", xn, self.bt_qkv, M=M)
                if "bqkv" in lw:
                    ho.bias_add(self.bt_qkv, lw["bqkv"], M)
                ho.attn_dec(self.bt_qkv, self.k_cache[i], self.v_cache[i],
                            self.b_att[0], self.bt_lens, self.cos_t,
                            self.sin_t, self.bt_scratch, self.bt_attn_cnt,
                            self.nh_l, self.kvh_l, self.hd, self.scale,
                            softcap=self.attn_softcap, window=window or 0,
                            split=self.attn_split, kS=self.k_scale[i],
                            vS=self.v_scale[i], batch=M,
                            merge=self.attn_merge)
            else:
                self._linear(lw, "wq", xn, self.b_q, M=M)
                self._linear(lw, "wk", xn, self.b_k, M=M)
                self._linear(lw, "wv", xn, self.b_v, M=M)
                if "bqkv" in lw:
                    ho.bias_add(self.b_q, lw["bias_q"], M)
                    ho.bias_add(self.b_k, lw["bias_k"], M)
                    ho.bias_add(self.b_v, lw["bias_v"], M)
                ho.rope_cache(self.b_q, self.b_k, self.b_v, self._kc(i),
                              self._vc(i), self.cos_t, self.sin_t,
                              self.len_buf, M, self.nh_l, self.kvh_l,
                              self.hd, kS=self._ks(i), vS=self._vs(i))
                if self.hd in (64, 128, 256):
                    ho.attn_prefill_mfma(
                        self.b_q, self._kc(i), self._vc(i), self.b_att,
                        self.len_buf, M, self.nh_l, self.kvh_l, self.hd,
                        self.scale, softcap=self.attn_softcap,
                        window=window or 0,
                        kS=self._ks(i), vS=self._vs(i))
                else:
                    # per-query VALU kernel: every production head_dim is
                    # 64/128/256 (MFMA above); kept as the documented
                    # debugging/odd-shape fallback
                    ho.attn(self.b_q, self._kc(i), self._vc(i),
                            self.b_att, self.len_buf, M, self.nh_l,
                            self.kvh_l, self.hd, self.scale,
                            softcap=self.attn_softcap,
                            window=window or 0,
                            kS=self._ks(i), vS=self._vs(i))
            if self.gemma:
                self._rowpar_ar(lw, "wo", self.b_att, t1, M)
                ho.rmsnorm(t1[:M], lw["g_post"], h[:M], res=h[:M], eps=eps)
                ho.rmsnorm(h[:M], lw["g_preffn"], xn[:M], eps=eps)
            else:
                if self.tp_branch:
                    self._rowpar_ar(lw, "wo", self.b_att, t1, M)
                    ho.addinto(h[:M], t1[:M])
                else:
                    self._linear(lw, "wo", self.b_att, h, res=h, M=M)
                ho.rmsnorm(h[:M], lw["g_post"], xn[:M], eps=eps)
            if self.moe:
                self._moe_mlp_rows(lw, M)
                if layer_hook is not None:
                    layer_hook(i, h[:M])
                continue
            self._linear(lw, "wgate", xn, self.b_gate, M=M)
            self._linear(lw, "wup", xn, self.b_up, M=M)
            ho.glu(self.b_gate[:M], self.b_up[:M], self.b_gate[:M], self.act)
            if self.gemma:
                self._rowpar_ar(lw, "wdown", self.b_gate, t1, M)
                ho.rmsnorm(t1[:M], lw["g_postffn"], h[:M], res=h[:M], eps=eps)
            else:
                if self.tp_branch:
                    self._rowpar_ar(lw, "wdown", self.b_gate, t1, M)
                    ho.addinto(h[:M], t1[:M])
                else:
                    self._linear(lw, "wdown", self.b_gate, h, res=h, M=M)
            if layer_hook is not None:
                layer_hook(i, h[:M])

    def _moe_mlp_rows(self, lw, M: int):
        """Prefill/batch MoE MLP over rows [0, M): router weights per
        row (dense M x E grid), then ONE GEMM pass per expert with the
        output folded into h weighted by that row's prob (0 if
        unrouted).  Work is E/topk x the routed minimum — prefill is
        compute-rich and this keeps the MFMA GEMM path; decode uses the
        expert-indexed GEMVs instead (`_decode_step`)."""
        cfg = self.config
        E, I, H = cfg.num_local_experts, self.inter_l, self.H
        eps = cfg.rms_norm_eps
        xn, gate, up, t1 = self.b_xn, self.b_gate, self.b_up, self.b_t1
        ho.moe_route(self.b_h, lw["g_post"], lw["wg"], M, self.topk,
                     self.moe_idx, self.moe_w, dense=self.moe_dense,
                     eps=eps)
        for e in range(E):
            g_lo, g_hi = e * 2 * I, e * 2 * I + I
            u_hi = (e + 1) * 2 * I
            d_lo, d_hi = e * H, (e + 1) * H
            if self.fp8:
                ho.quant_fp8(xn[:M], self.b_xq, self.b_sx)
                ho.gemm_fp8(self.b_xq, self.b_sx,
                            lw["wgu_q_all"][g_lo:g_hi],
                            lw["wgu_s_all"][g_lo:g_hi], gate[:M], M, H,
                            accbuf=self.b_gemm_acc)
                ho.gemm_fp8(self.b_xq, self.b_sx,
                            lw["wgu_q_all"][g_hi:u_hi],
                            lw["wgu_s_all"][g_hi:u_hi], up[:M], M, H,
                            accbuf=self.b_gemm_acc)
                ho.glu(gate[:M], up[:M], gate[:M], self.act)
                ho.quant_fp8(gate[:M], self.b_xq, self.b_sx)
                ho.gemm_fp8(self.b_xq, self.b_sx,
                            lw["wdown_q_all"][d_lo:d_hi],
                            lw["wdown_s_all"][d_lo:d_hi], t1[:M], M, I,
                            accbuf=self.b_gemm_acc)
            else:
                ho.gemm(xn[:M], lw["wgu_all"][g_lo:g_hi], gate[:M],
                        accbuf=self.b_gemm_acc)
                ho.gemm(xn[:M], lw["wgu_all"][g_hi:u_hi], up[:M],
                        accbuf=self.b_gemm_acc)
                ho.glu(gate[:M], up[:M], gate[:M], self.act)
                ho.gemm(gate[:M], lw["wdown_all"][d_lo:d_hi], t1[:M],
                        accbuf=self.b_gemm_acc)
            ho.moe_scale_add(self.b_h, t1, self.moe_dense[e:], E, M, H)

    def _lm_head_last(self, M: int):
        """Final norm + lm_head on the last row -> self.b_logits (f32, V);
        the norm rides in the GEMV staging pass (no separate launch)."""
        hrow = self.b_h[M - 1] if M > 1 else self.b_h[0]
        self._lm_head_gemv(hrow, stage=ho.STAGE_NORM, g=self.g_final,
                           eps=self.config.rms_norm_eps,
                           softcap=self.final_softcap)

    def forward_full(self, ids: np.ndarray,
                     return_hidden_states: bool = False):
        """All-positions logits (M, V) — reference-parity API (the HF
        tuple shape).  Prefill-style pass; vocab GEMM per
        chunk.  Resets the cache.  With ``return_hidden_states`` also
        returns the L+1 per-layer hidden states (embedding output +
        each decoder layer, reference ``all_hidden_states``
        llama3.2_model.py:682-716) as fp32 numpy arrays."""
        ids = np.asarray(ids, dtype=np.int32).ravel()
        self.reset()
        if not return_hidden_states:
            return self.forward_positions(ids, 0)
        n = len(ids)
        out = np.empty((n, self.config.vocab_size), dtype=np.float32)
        L = self.config.num_hidden_layers
        hidden = [np.empty((n, self.H), dtype=np.float32)
                  for _ in range(L + 1)]
        logits_buf = torch.empty(self.PC, self.vocab_l,
                                 dtype=torch.bfloat16, device=self.device)
        done = 0
        while done < n:
            M = min(n - done, self.PC)
            self.ids_buf[:M].copy_(
                torch.from_numpy(ids[done:done + M].astype(np.int32)))
            ho.i32_set(self.len_buf, done)
            ho.embed(self.embed, self.ids_buf, self.b_h, M,
                     self.config.embed_scale)
            d0 = done

            def hook(i, h):
                torch.cuda.synchronize()
                hidden[i + 1][d0:d0 + h.shape[0]] = \
                    h.float().cpu().numpy()
            self._layers_forward(M, layer_hook=hook)
            ho.rmsnorm(self.b_h[:M], self.g_final, self.b_xn[:M],
                       eps=self.config.rms_norm_eps)
            if self.wq4:
                ho.gemm_fp4w(self.b_xn[:M], self.lm_head_q4,
                             self.lm_head_e4, logits_buf[:M],
                             accbuf=self.b_gemm_acc)
            elif self.fp8:
                ho.quant_fp8(self.b_xn[:M], self.b_xq, self.b_sx)
                ho.gemm_fp8(self.b_xq, self.b_sx, self.lm_head_q,
                            self.lm_head_s, logits_buf[:M], M, self.H,
                            accbuf=self.b_gemm_acc)
            else:
                ho.gemm(self.b_xn[:M], self.lm_head, logits_buf[:M],
                        accbuf=self.b_gemm_acc)
            if self.final_softcap:
                ho.softcap(logits_buf[:M], self.final_softcap)
            if self.world > 1:
                # gather vocab shards on-device (each rank holds the
                # columns [r*vocab_l, (r+1)*vocab_l) of rows [0, M))
                import torch.distributed as dist
                t = logits_buf[:M].float().contiguous()
                chunks = [torch.empty_like(t) for _ in range(self.world)]
                dist.all_gather(chunks, t)
                loc = torch.cat(chunks, dim=1).cpu().numpy()
            else:
                torch.cuda.synchronize()
                loc = logits_buf[:M].float().cpu().numpy()
            out[done:done + M] = loc
            done += M
        ho.i32_set(self.len_buf, n)
        # mirror the device len so a following decode()'s overflow guard
        # counts from the right base (KV-pool OOB otherwise)
        self._host_len = n
        if return_hidden_states:
            return out, hidden
        return out

    def forward_positions(self, ids: np.ndarray, pos0: int) -> np.ndarray:
        """All-position logits (M, V) fp32, CONTINUING from pos0 (no
        cache reset: KV for ids lands at [pos0, pos0+M) and the pool can
        be rolled back afterwards with ``rewind``).  This is the
        speculative-decoding VERIFY pass: the target model scores k
        draft tokens in one prefill-shaped pass instead of k decode
        steps (ROADMAP §5; the reference has nothing comparable)."""
        ids = np.asarray(ids, dtype=np.int32).ravel()
        n = len(ids)
        if n == 0:
            raise ValueError("empty ids")
        if pos0 + n > self.max_seq:
            raise ValueError(f"sequence {pos0}+{n} exceeds max_seq "
                             f"{self.max_seq}")
        out = np.empty((n, self.config.vocab_size), dtype=np.float32)
        logits_buf = torch.empty(self.PC, self.vocab_l,
                                 dtype=torch.bfloat16, device=self.device)
        done = 0
        while done < n:
            M = min(n - done, self.PC)
            self.ids_buf[:M].copy_(
                torch.from_numpy(ids[done:done + M].astype(np.int32)))
            ho.i32_set(self.len_buf, pos0 + done)
            ho.embed(self.embed, self.ids_buf, self.b_h, M,
                     self.config.embed_scale)
            self._layers_forward(M)
            ho.rmsnorm(self.b_h[:M], self.g_final, self.b_xn[:M],
                       eps=self.config.rms_norm_eps)
            if self.wq4:
                ho.gemm_fp4w(self.b_xn[:M], self.lm_head_q4,
                             self.lm_head_e4, logits_buf[:M],
                             accbuf=self.b_gemm_acc)
            elif self.fp8:
                ho.quant_fp8(self.b_xn[:M], self.b_xq, self.b_sx)
                ho.gemm_fp8(self.b_xq, self.b_sx, self.lm_head_q,
                            self.lm_head_s, logits_buf[:M], M, self.H,
                            accbuf=self.b_gemm_acc)
            else:
                ho.gemm(self.b_xn[:M], self.lm_head, logits_buf[:M],
                        accbuf=self.b_gemm_acc)
            if self.final_softcap:
                ho.softcap(logits_buf[:M], self.final_softcap)
            if self.world > 1:
                # gather vocab shards on-device (each rank holds the
                # columns [r*vocab_l, (r+1)*vocab_l) of rows [0, M))
                import torch.distributed as dist
                t = logits_buf[:M].float().contiguous()
                chunks = [torch.empty_like(t) for _ in range(self.world)]
                dist.all_gather(chunks, t)
                loc = torch.cat(chunks, dim=1).cpu().numpy()
            else:
                torch.cuda.synchronize()
                loc = logits_buf[:M].float().cpu().numpy()
            out[done:done + M] = loc
            done += M
        ho.i32_set(self.len_buf, pos0 + n)
        self._host_len = pos0 + n
        return out

    # rows per lm_head GEMM + k_logprob_rows launch of prompt_logprobs
    # (docs/KERNELS.md: bounds the logits scratch to PL_ROWS x V bf16)
    PL_ROWS = 512

    def _pl_alloc(self):
        """Scratch of ``prompt_logprobs``, allocated by the first call and
        kept: logits [min(PC, PL_ROWS), V] bf16, targets [max_seq] i32,
        records val [max_seq, 21] f32 / idx [max_seq, 20] i32."""
        assert self.world == 1, "device prompt logprobs are single-GPU"
        if self.pl_logits is None:
            dev, W = self.device, ho.LOGPROBS_MAX_TOP
            self.pl_logits = torch.empty(
                min(self.PC, self.PL_ROWS), self.config.vocab_size,
                dtype=torch.bfloat16, device=dev)
            self.pl_tgt = torch.full((self.max_seq,), -1, dtype=torch.int32,
                                     device=dev)
            self.pl_val = torch.zeros(self.max_seq, 1 + W,
                                      dtype=torch.float32, device=dev)
            self.pl_idx = torch.zeros(self.max_seq, W, dtype=torch.int32,
                                      device=dev)

    def prompt_logprobs(self, ids: np.ndarray, top_n: int = 0):
        """Teacher-forced logprobs of a prompt, device-side: returns
        ``(lp [n-1] f32, top_ids [n-1, N] i32, top_lp [n-1, N] f32)``
        numpy arrays; entry t describes ``ids[t+1]`` given ``ids[:t+1]``
        (``top_lp`` descending, ties by ascending id).  The pass is
        ``forward_full``'s — reset, chunks of PC, final norm, lm_head GEMM
        in the engine's weight dtype, final softcap — but the logits stay on
        the device: ``k_logprob_rows`` reduces every row to one record and
        only the records cross to the host, once, at the end.  Afterwards
        the KV pool holds the prompt, the length is n and the last row's
        logits are staged, so ``decode`` continues as after ``prefill``."""
        ids = np.asarray(ids, dtype=np.int32).ravel()
        n, N = len(ids), int(top_n)
        if not self.device_prompt_logprobs:
            raise ValueError("device prompt logprobs are single-GPU; use "
                             "the host path (runtime.score) under TP")
        if n < 2:
            raise ValueError(f"scoring needs at least 2 tokens, got {n}")
        if not 0 <= N <= self.device_prompt_logprobs:
            raise ValueError(f"top_n must be within 0.."
                             f"{self.device_prompt_logprobs}, got {N}")
        if n > self.max_seq:
            raise ValueError(f"sequence {n} exceeds max_seq {self.max_seq}")
        V = self.config.vocab_size
        if ids.min() < 0 or ids.max() >= V:
            raise ValueError(f"token ids must be within [0, {V})")
        self._pl_alloc()
        self.reset()
        # row t's target is ids[t+1] (across chunk boundaries too); the
        # last row has none
        tgt = np.empty(n, dtype=np.int32)
        tgt[:-1] = ids[1:]
        tgt[-1] = -1
        self.pl_tgt[:n].copy_(torch.from_numpy(tgt))
        sub = self.pl_logits.shape[0]
        done = 0
        while done < n:
            M = min(n - done, self.PC)
            self.ids_buf[:M].copy_(torch.from_numpy(ids[done:done + M]))
            ho.i32_set(self.len_buf, done)
            ho.embed(self.embed, self.ids_buf, self.b_h, M,
                     self.config.embed_scale)
            self._layers_forward(M)
            ho.rmsnorm(self.b_h[:M], self.g_final, self.b_xn[:M],
                       eps=self.config.rms_norm_eps)
            for r0 in range(0, M, sub):
                m = min(M - r0, sub)
                x, y = self.b_xn[r0:r0 + m], self.pl_logits[:m]
                if self.wq4:
                    ho.gemm_fp4w(x, self.lm_head_q4, self.lm_head_e4, y,
                                 accbuf=self.b_gemm_acc)
                elif self.fp8:
                    ho.quant_fp8(x, self.b_xq, self.b_sx)
                    ho.gemm_fp8(self.b_xq, self.b_sx, self.lm_head_q,
                                self.lm_head_s, y, m, self.H,
                                accbuf=self.b_gemm_acc)
                else:
                    ho.gemm(x, self.lm_head, y, accbuf=self.b_gemm_acc)
                if self.final_softcap:
                    ho.softcap(y, self.final_softcap)
                a = done + r0
                ho.logprob_rows(y, self.pl_tgt[a:a + m], N,
                                self.pl_val[a:a + m], self.pl_idx[a:a + m])
            done += M
        ho.i32_set(self.len_buf, n)
        self._host_len = n
        self._lm_head_last(M)
        torch.cuda.synchronize()
        val = self.pl_val[:n - 1].cpu().numpy()
        idx = self.pl_idx[:n - 1].cpu().numpy()
        return (val[:, 0].copy(), idx[:, :N].copy(), val[:, 1:1 + N].copy())

    def rewind(self, n: int):
        """Roll the sequence back to length n — O(1): the KV pool is
        preallocated and the attention kernels read the device length
        from len_buf, so positions >= n are dead until overwritten.
        Speculative decoding uses this to discard rejected draft KV."""
        if not 0 <= n <= self.max_seq:
            raise ValueError(f"rewind {n} outside [0, {self.max_seq}]")
        ho.i32_set(self.len_buf, n)
        self._host_len = n

    # ------------------------------------------------------------------
    # device-side greedy speculative decoding (this engine = the target)
    # ------------------------------------------------------------------
    # records a chunk can hold (its cycle count is capped to this)
    SPEC_REC = 64

    def _spec_alloc(self):
        """State of the speculative verify pass, allocated by the first
        call and kept: logits [SPEC_MAX_K+1, V] bf16, the verify kernel's
        scratch (zeroed here once, re-armed on the device), the record
        ring [SPEC_REC, 1+SPEC_MAX_K] i32 and its counter."""
        assert self.device_speculative
        if self.sp_logits is None:
            dev = self.device
            self.sp_logits = torch.zeros(
                ho.SPEC_MAX_K + 1, self.config.vocab_size,
                dtype=torch.bfloat16, device=dev)
            self.sp_scratch = torch.zeros(ho.SPEC_SCRATCH_WORDS,
                                          dtype=torch.int64, device=dev)
            self.sp_rec = torch.zeros(self.SPEC_REC, ho.SPEC_REC_WORDS,
                                      dtype=torch.int32, device=dev)
            self.sp_nrec = torch.zeros(1, dtype=torch.int32, device=dev)

    def decode_steps_async(self, n: int):
        """``n`` greedy decode steps with no synchronise and no ring
        read-back: replays of the greedy decode graph (captured here when
        it is not there yet; its warm-up is one REAL step and counts as
        one of the n), or eager steps when capture failed.  The
        speculative draft loop; ``decode`` keeps its behaviour."""
        if n < 1:
            return
        if self._host_len + n > self.max_seq:
            raise ValueError(
                f"decode would overflow the KV pool: len {self._host_len} "
                f"+ {n} > max_seq {self.max_seq}")
        self._host_len += n
        taken, ok = self.capture_decode_graph()
        n -= taken
        if ok:
            for _ in range(n):
                self._graph.replay()
        else:
            spec = SampleSpec()
            for _ in range(n):
                self._step(spec)

    def spec_verify_pass(self, draft: Optional["GPUModel"], k: int,
                         blocks: int = 0):
        """One verify pass of greedy speculative decoding on this engine,
        nothing crossing to the host: stage [next_token, draft.out_ring[:k]]
        into ids_buf, embed, the layer stack over k+1 rows from len_buf,
        final norm, lm_head GEMM in the weight dtype into the kept
        ``sp_logits`` rows, final softcap, then ``spec_verify`` commits the
        accepted prefix and the target's own token into both engines'
        state (docs/KERNELS.md).  ``k`` = 0 is a plain greedy step through
        the same kernels (``draft`` unused, may be None): the sampling
        tail commits row 0.  The caller guarantees len + k + 1 <= max_seq
        on both engines."""
        self._spec_alloc()
        M = k + 1
        ho.spec_stage(self.ids_buf, self.next_token,
                      draft.out_ring if k else self.out_ring, k)
        ho.embed(self.embed, self.ids_buf, self.b_h, M,
                 self.config.embed_scale)
        self._layers_forward(M)
        ho.rmsnorm(self.b_h[:M], self.g_final, self.b_xn[:M],
                   eps=self.config.rms_norm_eps)
        y = self.sp_logits[:M]
        if self.wq4:
            ho.gemm_fp4w(self.b_xn[:M], self.lm_head_q4, self.lm_head_e4, y,
                         accbuf=self.b_gemm_acc)
        elif self.fp8:
            ho.quant_fp8(self.b_xn[:M], self.b_xq, self.b_sx)
            ho.gemm_fp8(self.b_xq, self.b_sx, self.lm_head_q,
                        self.lm_head_s, y, M, self.H,
                        accbuf=self.b_gemm_acc)
        else:
            ho.gemm(self.b_xn[:M], self.lm_head, y, accbuf=self.b_gemm_acc)
        if self.final_softcap:
            ho.softcap(y, self.final_softcap)
        if k == 0:
            self._sample_tail(y, self._sv, 1, SampleSpec())
            return
        ho.spec_verify(y, k, self.ids_buf[1:1 + k], self.sp_scratch,
                       self.len_buf, self.next_token, self.out_ring,
                       self.nout, draft.len_buf, draft.next_token,
                       draft.nout, self.sp_rec, self.sp_nrec, blocks=blocks)

    def spec_chunk(self, draft: "GPUModel", k: int, cycles: int,
                   nout0: int):
        """``cycles`` speculative cycles back to back, ONE synchronise at
        the end.  A cycle: k+1 draft steps (the last one writes the KV of
        the k-th proposal, so a fully accepted cycle leaves the draft
        nothing to catch up on; its own proposal is dropped), one verify
        pass, the commit.  ``k`` = 0: ``cycles`` plain target steps.
        ``nout0``: the target's ring count before the chunk.  Returns
        ``(ids, recs)``: the tokens emitted (int32 array) and, for k > 0,
        one ``(m, drafts)`` per cycle; both engines' ``_host_len`` mirror
        the device lengths afterwards.  The caller has checked that
        len + cycles * (k+1) fits both pools."""
        n = self._host_len
        need = n + cycles * (k + 1)
        if need > self.max_seq or (k and need > draft.max_seq):
            raise ValueError(f"speculative chunk {n} + {cycles} x {k + 1} "
                             f"exceeds a KV pool")
        if not 1 <= cycles <= self.SPEC_REC:
            raise ValueError(f"cycles must be within 1..{self.SPEC_REC}")
        self._spec_alloc()
        if k:
            ho.i32_set(self.sp_nrec, 0)
            draft._host_len = n
        for _ in range(cycles):
            if k:
                draft.decode_steps_async(k + 1)
            self.spec_verify_pass(draft, k)
        scal = torch.cat([self.nout, self.len_buf,
                          draft.len_buf if k else self.len_buf])
        torch.cuda.synchronize()
        nout, t_len, d_len = (int(v) for v in scal.cpu().numpy())
        ids = self.out_ring[nout0:nout].cpu().numpy()
        self._host_len = t_len
        recs = []
        if k:
            draft._host_len = d_len
            for row in self.sp_rec[:cycles].cpu().numpy():
                recs.append((int(row[0]), [int(t) for t in row[1:1 + k]]))
        return ids, recs

    def speculative_tokens(self, draft: "GPUModel", prompt_ids,
                           max_tokens: int, k: int = 4, eos_id=None,
                           on_ids=None):
        """Greedy decode of this engine (the target) accelerated by
        ``draft``, device-side: the token stream is this engine's own
        greedy chain under the verify pass's numerics.  Both engines are
        prefilled with the prompt, the first token comes from the target's
        prefill logits, then chunks of ``SPEC_CHUNK`` cycles run between two
        host reads.  Before each chunk the cycle count, then k, shrink
        until len + cycles * (k+1) fits both pools — the positions a chunk
        writes at most, [len, len + cycles * (k+1)), so no slot of a pool
        stays unused and the run ends where the host loop's ends; without
        room for a draft the target takes plain steps until its pool is
        full.  ``on_ids`` sees each chunk's new ids (cut at EOS and
        at ``max_tokens``).  Returns ``(ids, recs)``: at most ``max_tokens``
        ids, ending with the first EOS, and one ``(k, m, drafts)`` per
        verify pass that ran (the passes of a chunk that follow an EOS
        included)."""
        import time as _time
        if not (self.device_speculative
                and getattr(draft, "device_speculative", False)):
            raise ValueError("device-side speculative decoding needs "
                             "single-GPU, non-MoE GPUModel engines")
        if draft is self:
            raise ValueError("draft and target must be two engines")
        if draft.device != self.device:
            raise ValueError(f"draft on {draft.device}, target on "
                             f"{self.device}: the engines must share a device")
        if draft.config.vocab_size != self.config.vocab_size:
            raise ValueError(
                f"draft vocabulary {draft.config.vocab_size} != target "
                f"vocabulary {self.config.vocab_size}")
        if not 1 <= k <= ho.SPEC_MAX_K:
            raise ValueError(f"k must be within 1..{ho.SPEC_MAX_K}, got {k}")
        prompt_ids = np.asarray(prompt_ids, dtype=np.int32).ravel()
        P0 = len(prompt_ids)
        pool = min(self.max_seq, draft.max_seq)
        if P0 + 1 > pool:
            raise ValueError(f"prompt {P0} fills the KV pool ({pool})")
        eos_set = (set() if eos_id is None else
                   {int(eos_id)} if np.isscalar(eos_id) else
                   {int(e) for e in eos_id})
        C = max(1, min(int(self.SPEC_CHUNK), self.SPEC_REC))
        t0 = _time.perf_counter()
        with trace_range("prefill"):
            self._pb = draft._pb = 0
            self.prefill(prompt_ids)
            draft.prefill(prompt_ids)
            # first token: greedy tail on the prefill logits (no length
            # bump), handed to the draft as its pending token
            self._sample_tail(self.b_logits, self._sv, 1, SampleSpec(),
                              first=True)
            draft.next_token.copy_(self.next_token)
            draft.nout.zero_()
            torch.cuda.synchronize()
            out = [int(self.out_ring[0].item())]
        self.last_prefill_time_s = _time.perf_counter() - t0
        if on_ids:
            on_ids(out[:max_tokens])
        recs = []
        with trace_range("decode"):
            while len(out) < max_tokens and out[-1] not in eos_set:
                n = self._host_len
                kk = min(k, self.max_seq - n - 1, draft.max_seq - n - 1)
                left = max_tokens - len(out)
                if kk < 1:
                    if n + 1 >= self.max_seq:
                        break                 # target pool exhausted
                    kk = 0
                    c = min(C, left, self.max_seq - 1 - n)
                else:
                    # no more cycles than full acceptance would need: no
                    # pass ever starts past the budget, as in the host loop
                    c = min(C, -(-left // (kk + 1)), (pool - n) // (kk + 1))
                ids, rr = self.spec_chunk(draft, kk, c, len(out))
                recs.extend((kk, m, d) for m, d in rr)
                take = [int(t) for t in ids][:left]
                hit = [j for j, t in enumerate(take) if t in eos_set]
                if hit:
                    take = take[:hit[0] + 1]
                out.extend(take)
                if on_ids and take:
                    on_ids(take)
                if hit:
                    break
        return out[:max_tokens], recs

    def forward_hf(self, ids: np.ndarray):
        """Reference-parity output tuple ``(loss, logits, kv_cache,
        hidden_states, attentions)`` (llama3.2_model.py:726-822).
        ``loss`` is None (inference-only, as in the reference) and
        ``attentions`` is None by design: the fused attention kernels
        use online softmax and never materialize the probability
        matrix."""
        logits, hidden = self.forward_full(ids, return_hidden_states=True)
        cache = DeviceCacheHandle(self)
        cache.seq_len = len(np.ravel(ids))
        return None, logits, cache, hidden, None

    # ------------------------------------------------------------------
    # logit processors (penalties / logit_bias): per-row device state
    # ------------------------------------------------------------------
    _PROC_IDENTITY = (1.0, 0.0, 0.0, 0.0)

    def _proc_alloc(self):
        """stat [R, V] i32, proc [R, 4] f32, bias [R, V] f32 with one row
        per sequence slot (the single-sequence path uses row 0)."""
        if self.p_stat is not None:
            return
        assert self.world == 1, "device logit processors are single-GPU"
        R, V = self.max_batch, self.config.vocab_size
        dev = self.device
        self.p_stat = torch.zeros(R, V, dtype=torch.int32, device=dev)
        self.p_bias = torch.zeros(R, V, dtype=torch.float32, device=dev)
        self.p_proc = torch.tensor([self._PROC_IDENTITY] * R,
                                   dtype=torch.float32, device=dev)

    def setup_processors(self, b: int, prompt_ids, processors):
        """Start row b's history: zero stat, flag the prompt ids, write
        the row's penalties and its dense bias.  ``processors`` is the
        dict of ``sampling.device_sampler_kwargs``; None / missing keys
        mean identity.  Values are device DATA — captured graphs that
        carry the adjust stage serve every setting."""
        self._proc_alloc()
        pr = processors or {}
        r = float(pr.get("repetition_penalty", 1.0))
        f = float(pr.get("frequency_penalty", 0.0))
        pp = float(pr.get("presence_penalty", 0.0))
        if not r > 0.0:
            raise ValueError(f"repetition_penalty must be > 0, got {r}")
        V = self.config.vocab_size
        bias = {int(k): float(v)
                for k, v in (pr.get("logit_bias") or {}).items()
                if 0 <= int(k) < V}
        self.p_stat[b].zero_()
        ids = np.ascontiguousarray(np.asarray(prompt_ids).ravel(),
                                   dtype=np.int32)
        if len(ids):
            ho.tokstat_mark(self.p_stat[b],
                            torch.from_numpy(ids).to(self.device))
        if bias:
            self.p_bias[b].zero_()
            idx = torch.tensor(list(bias.keys()), dtype=torch.int64,
                               device=self.device)
            val = torch.tensor(list(bias.values()), dtype=torch.float32,
                               device=self.device)
            self.p_bias[b].index_copy_(0, idx, val)
        self.p_proc[b].copy_(torch.tensor(
            [r, f, pp, 1.0 if bias else 0.0], dtype=torch.float32))
        self._proc_rows[b] = bool(bias)

    def _proc_clear(self, b: int):
        """Row b carries no processors: identity proc (nothing else of
        its state is read then)."""
        if self._proc_rows.pop(b, None) is not None:
            self.p_proc[b].copy_(torch.tensor(self._PROC_IDENTITY))

    # ------------------------------------------------------------------
    # logprobs: per-row device state of the in-graph logprob stage
    # ------------------------------------------------------------------
    def _lp_alloc(self, raw: bool = False):
        """lp_cfg [R] i32 (-1 = off), stage [R, 48] f32, scan scratch
        [R, words(V)] i64, record rings lp_val [R, LP_RING, 21] f32 /
        lp_idx [R, LP_RING, 20] i32 with one row per sequence slot (the
        single-sequence path uses row 0).  ``raw``: also the fp32 logits
        snapshot [R, V], needed only by steps that adjust the logits."""
        assert self.world == 1, "device logprobs are single-GPU"
        R, V = self.max_batch, self.config.vocab_size
        dev = self.device
        if self.lp_cfg is None:
            W = ho.LOGPROBS_MAX_TOP
            self.lp_cfg = torch.full((R,), -1, dtype=torch.int32, device=dev)
            self.lp_stage = torch.zeros(R, ho.LP_STAGE_WORDS,
                                        dtype=torch.float32, device=dev)
            self.lp_part = torch.zeros(R, ho.logprob_part_words(V),
                                       dtype=torch.int64, device=dev)
            self.lp_val = torch.zeros(R, ho.LP_RING, 1 + W,
                                      dtype=torch.float32, device=dev)
            self.lp_idx = torch.zeros(R, ho.LP_RING, W, dtype=torch.int32,
                                      device=dev)
        if raw and self.lp_raw is None:
            self.lp_raw = torch.zeros(R, V, dtype=torch.float32, device=dev)

    def setup_logprobs(self, b: int, n):
        """Row b reports the chosen token's logprob and its top-``n``
        (0..device_logprobs) per token from now on; ``n`` None switches
        the row off.  N is device DATA — captured graphs that carry the
        logprob stage serve every N."""
        if n is None:
            self._lp_clear(b)
            return
        n = int(n)
        if not 0 <= n <= self.device_logprobs:
            raise ValueError(f"logprobs must be within 0.."
                             f"{self.device_logprobs}, got {n}")
        self._lp_alloc()
        ho.logprob_set_cfg(self.lp_cfg, b, n)
        self._lp_rows[b] = n

    def _lp_clear(self, b: int):
        """Row b carries no logprobs: cfg -1 (the kernels then touch
        nothing of the row)."""
        if self._lp_rows.pop(b, None) is not None:
            ho.logprob_set_cfg(self.lp_cfg, b, -1)

    def logprob_records(self, n: int, row: int = 0):
        """Records of the last ``n`` tokens committed on ``row``:
        ``(chosen_lp [n] f32, top_ids [n, N] i32, top_lp [n, N] f32)``
        numpy arrays, N the row's own top-N; ``top_lp`` is sorted
        descending (ties by ascending id).  The ring keeps LP_RING
        tokens, so drain at least that often."""
        if row not in self._lp_rows:
            raise ValueError(f"row {row} has no logprobs set up")
        if not 0 <= n <= ho.LP_RING:
            raise ValueError(f"the logprob ring keeps {ho.LP_RING} records, "
                             f"asked for {n}")
        N = self._lp_rows[row]
        torch.cuda.synchronize()
        cnt = self.bt_nout if self._lp_batch else self.nout
        end = int(cnt[row].item())
        if n > end:
            raise ValueError(f"row {row} committed {end} tokens, asked for "
                             f"{n} records")
        slots = (np.arange(end - n, end) % ho.LP_RING).astype(np.int64)
        val = self.lp_val[row].cpu().numpy()[slots]
        idx = self.lp_idx[row].cpu().numpy()[slots]
        return (val[:, 0].copy(), idx[:, :N].copy(), val[:, 1:1 + N].copy())

    # ------------------------------------------------------------------
    # per-row sampler: strategy / temperature / filter / seed as device data
    # ------------------------------------------------------------------
    def _samp_pack(self, row_sampler):
        """``row_sampler`` dict (``sampling.device_row_sampler_kwargs``:
        strategy fields + optional ``seed``) -> (table row as int32[8] host
        tensor, mode).  Raises ValueError on bad values, ahead of any
        launch.  A request without a seed gets one from the engine seed
        and a per-engine request serial, so two identical unseeded
        requests draw different streams (and a re-run of the same engine
        repeats them)."""
        assert self.world == 1, "the per-row sampler is single-GPU"
        seed = row_sampler.get("seed")
        words = ho.samp_row(row_sampler, 0 if seed is None else seed,
                            self.config.vocab_size)
        if seed is None:
            # splitmix64 of (engine seed, serial)
            z = (int(self.seed) * 0x9E3779B97F4A7C15
                 + (self._req_serial + 1) * 0xD1B54A32D192ED03) & (2**64 - 1)
            self._req_serial += 1
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
            z ^= z >> 31
            words[5], words[6] = z & 0xFFFFFFFF, z >> 32
        return torch.from_numpy(words.view(np.int32)), int(words[0])

    def _row_modes(self, B: int) -> frozenset:
        """Modes present in lockstep rows [0, B) (host mirror)."""
        missing = [b for b in range(B) if b not in self._samp_modes]
        if missing:
            raise ValueError(f"rows {missing} were not set up with "
                             f"prefill_row(row_sampler=...)")
        return frozenset(self._samp_modes[b] for b in range(B))

    def _row_chain(self, B: int) -> int:
        """Chain bits of lockstep rows [0, B), ORed (host mirror)."""
        bits = 0
        for b in range(B):
            bits |= self._samp_chain.get(b, 0)
        return bits

    def _stage_setup(self, n: int, proc: bool, logprobs: bool,
                     lp_batch: bool):
        """State of the stages an ``n``-token decode call switches on:
        processor rows, logprob rows (with the raw snapshot when the
        logits are adjusted too); ``lp_batch``: the records follow
        bt_nout (else nout)."""
        if proc:
            self._proc_alloc()
        if logprobs:
            if n > ho.LP_RING:
                raise ValueError(f"logprobs: at most {ho.LP_RING} tokens "
                                 f"per call, got {n}")
            self._lp_alloc(raw=proc)
            self._lp_batch = lp_batch

    def _sample_tail(self, logits, v: RowState, B: int, spec: SampleSpec,
                     first: bool = False, before_adjust=None):
        """The end of every decode step, over ``B`` rows of ``logits``
        and their state ``v``: logprob scan of the RAW rows (with a
        snapshot when they are adjusted next), logit adjust, sampler,
        logprob commit.  ``first``: the token after a prefill — nothing
        generated yet, so the adjust stage counts no input and the
        sampler leaves the length alone.  ``before_adjust`` runs between
        scan and adjust (``prefill_row`` writes the row's processor
        state there)."""
        sl = v.sl or slice(0, B)
        if spec.logprobs:
            raw = self.lp_raw[sl] if spec.proc else None
            ho.logprob_scan(logits, self.lp_cfg[sl], self.lp_part[sl],
                            self.lp_stage[sl], raw=raw, batch=B)
        if before_adjust is not None:
            before_adjust()
        if spec.proc:
            # counts next_token (committed by the previous sample) into
            # the history, then penalties + bias in place (the whole
            # state goes with the tables from row 0, a narrowed one with
            # its own rows)
            pst = (self.p_stat, self.p_proc, self.p_bias)
            if v.sl is not None:
                pst = [t[v.sl] for t in pst]
            ho.logit_adjust(logits, *pst, v.next_token, not first, batch=B)
        if spec.rows is None:
            ho.sample(logits, spec.min_p, spec.greedy, self.seed,
                      self.rng_ctr, v.gmax, v.pick, v.next_token, v.ring,
                      v.nout, v.lens, bump_len=not first,
                      temperature=spec.temperature, cnt=v.cnt, batch=B,
                      top_k=spec.top_k, top_p=spec.top_p, sel=v.sel)
        else:
            ho.sample_rows(logits, v.samp, v.gmax, v.pick, v.cnt,
                           v.next_token, v.ring, v.nout, v.lens, v.sel, B,
                           not first, spec.rows, chain=spec.chain)
        if spec.logprobs:
            ho.logprob_commit(logits, self.lp_cfg[sl], self.lp_stage[sl],
                              v.next_token, v.nout, self.lp_val[sl],
                              self.lp_idx[sl], raw=raw, batch=B)

    def generate_tokens(self, prompt_ids, max_tokens: int,
                        greedy: bool = True, min_p: float = 0.1,
                        eos_id=None, chunk: int = 16, on_ids=None,
                        temperature: float = 1.0, stop_fn=None,
                        top_k: int = 0, top_p: float = 1.0,
                        processors=None, logprobs=None, row_sampler=None):
        """Fast generate: device-side hipGraph decode in chunks, host
        sees ids every `chunk` tokens (streaming + EOS stop).  Used by
        runtime.generate() for every strategy in ``device_strategies``
        (``top_k`` > 0 / ``top_p`` < 1 select the device-side filter; 0 /
        1.0 = off).  ``processors`` (dict, see ``setup_processors``) switches
        on the in-graph logit-adjust stage: penalties over the prompt and
        the generated ids, then logit_bias.  ``logprobs`` (int N within
        0..``device_logprobs``, or None) switches on the in-graph logprob
        stage: afterwards ``self.last_logprobs`` holds ``(chosen_lp [n],
        top_ids [n, N], top_lp [n, N])`` numpy arrays of the RAW model
        distribution (before processors / temperature), one row per
        returned id (a caller that truncates the ids on a stop string
        truncates them alike); None when logprobs were not asked for.
        ``row_sampler`` (dict of ``sampling.device_row_sampler_kwargs``:
        ``strategy`` and its fields, optional ``seed``) replaces greedy /
        min_p / temperature / top_k / top_p: the sampler reads them from
        the device table, and the stream is a function of the seed alone
        (same seed, same tokens).
        ``eos_id`` may be an int or a collection of ints (HF configs
        often store a list, e.g. Llama-3.2-Instruct).  ``stop_fn``
        (optional) sees the accumulated ids after each chunk and returns
        True to end generation early (stop-string support; the caller
        truncates — chunking may have produced up to chunk-1 extra
        ids)."""
        import time as _time
        prompt_ids = np.asarray(prompt_ids)
        room = self.max_seq - len(prompt_ids.ravel()) - 1
        if room <= 0:
            raise ValueError(f"prompt fills the {self.max_seq}-token pool")
        max_tokens = min(max_tokens, room)
        eos_set = (set() if eos_id is None else
                   {int(eos_id)} if np.isscalar(eos_id) else
                   {int(e) for e in eos_id})
        rskw = {}
        if row_sampler is not None:
            words, mode = self._samp_pack(row_sampler)
            self._s_rows = frozenset({mode})
            self._s_chain = ho.samp_row_chain(words.numpy())
            rskw = {"row_sampler": True}
        t0 = _time.perf_counter()
        with trace_range("prefill"):
            self.prefill(prompt_ids)
            if row_sampler is not None:
                self.s_samp[0].copy_(words)  # draw counter back to 0
            if processors is not None:
                self.setup_processors(0, prompt_ids, processors)
            if logprobs is not None:
                self.setup_logprobs(0, logprobs)
                chunk = min(chunk, ho.LP_RING)  # drained per chunk
        self.last_prefill_time_s = _time.perf_counter() - t0
        self.last_logprobs = None
        lpkw = {"logprobs": True} if logprobs is not None else {}
        recs = []
        out = []
        produced = 0
        first = True
        with trace_range("decode"):
            while produced < max_tokens:
                n = min(chunk, max_tokens - produced)
                ids = self.decode(n, greedy=greedy, min_p=min_p,
                                  use_graph=True, first_from_logits=first,
                                  temperature=temperature, top_k=top_k,
                                  top_p=top_p,
                                  processors=processors is not None, **lpkw,
                                  **rskw)
                first = False
                produced += n
                stop = False
                take = list(ids)
                hit = [j for j, t in enumerate(take) if int(t) in eos_set]
                if hit:
                    take = take[:hit[0] + 1]
                    stop = True
                out.extend(take)
                if logprobs is not None:
                    rec = self.logprob_records(len(ids))
                    recs.append(tuple(a[:len(take)] for a in rec))
                if on_ids:
                    on_ids(take)
                if stop:
                    break
                if stop_fn is not None and stop_fn(out):
                    break
        if logprobs is not None:
            N = int(logprobs)
            self.last_logprobs = (
                np.concatenate([r[0] for r in recs]) if recs
                else np.zeros(0, np.float32),
                np.concatenate([r[1] for r in recs]) if recs
                else np.zeros((0, N), np.int32),
                np.concatenate([r[2] for r in recs]) if recs
                else np.zeros((0, N), np.float32))
        return out

    # ------------------------------------------------------------------
    # generic forward (oracle-parity / generate()-compatible)
    # ------------------------------------------------------------------
    def forward(self, ids: np.ndarray, cache: DeviceCacheHandle,
                pos0: int) -> np.ndarray:
        """Returns last-position logits (1, V) fp32 numpy."""
        ids = np.asarray(ids, dtype=np.int32).ravel()
        if pos0 != cache.seq_len:
            raise ValueError("GPU engine requires sequential positions")
        n = len(ids)
        if n == 0:
            raise ValueError("empty ids")
        if pos0 + n > self.max_seq:
            raise ValueError(f"sequence {pos0}+{n} exceeds max_seq "
                             f"{self.max_seq}")
        done = 0
        while done < n:
            M = min(n - done, self.PC)
            self.ids_buf[:M].copy_(
                torch.from_numpy(ids[done:done + M].astype(np.int32)))
            ho.i32_set(self.len_buf, pos0 + done)
            ho.embed(self.embed, self.ids_buf, self.b_h, M,
                     self.config.embed_scale)
            self._layers_forward(M)
            done += M
        ho.i32_set(self.len_buf, pos0 + n)
        self._host_len = pos0 + n
        self._lm_head_last(M)
        cache.seq_len = pos0 + n
        torch.cuda.synchronize()
        return self.b_logits.float().cpu().numpy()[None, :]

    # ------------------------------------------------------------------
    # fast device-side decode loop (graph-replayable)
    # ------------------------------------------------------------------
    def _dgemv(self, lw, name, x, y, **kw):
        """Decode GEMV: MXFP4 / fp8 / bf16 weights by engine dtype."""
        if self.wq4:
            ho.gemv_fp4(lw[name + "_q4"], lw[name + "_e4"], x, y, **kw)
        elif self.fp8:
            ho.gemv_fp8(lw[name + "_q"], lw[name + "_s"], x, y, **kw)
        else:
            ho.gemv(lw[name], x, y, **kw)

    def _lm_head_gemv(self, x, **kw):
        """lm_head over the staged row ``x`` -> b_logits (f32, V): the
        engine's own ``lm_head*`` tensors through ``_dgemv``, then the
        vocab all-gather under TP."""
        self._dgemv(vars(self), "lm_head", x, self.b_logits_l, **kw)
        if self.tp_branch:
            tpu.all_gather_into(self.b_logits, self.b_logits_l)

    def _decode_step(self, greedy: bool, min_p: float,
                     temperature: float = 1.0, top_k: int = 0,
                     top_p: float = 1.0, proc: bool = False,
                     logprobs: bool = False, rows=None):
        """One single-sequence decode step with the sampler request given
        as plain arguments (see ``_step``)."""
        self._step(SampleSpec(greedy, min_p, temperature, top_k, top_p,
                              proc, logprobs, rows))

    def _step(self, spec: SampleSpec):
        """One single-sequence decode step: layer stack, then the
        sampling tail on b_logits.  Graph-replayable."""
        self._decode_layers()
        self._sample_tail(self.b_logits, self._sv, 1, spec)

    def _decode_layers(self):
        """Fused decode path: 4 kernels/layer (llama) or 5 (gemma) —
        RMSNorm lives inside the GEMV staging pass, RoPE + KV write
        inside the attention kernel.  bf16 weights: the gate+up GEMV
        computes the GLU itself (paired rows) and the down projection
        reads the I-long activation directly; fp8 / MXFP4 weights: the
        GLU is the down projection's staging pre-op.  With LLM_ATTN_PF
        set, the attention launch also prefetches the layer's o_proj and
        gate+up weights (`_plan_attn_pf`)."""
        cfg = self.config
        eps = cfg.rms_norm_eps
        if self.fp8 or self.wq4:
            gukw = {}
            downkw = dict(stage=ho.STAGE_GLU, x2=self.b_gu[self.inter_l:],
                          act=self.act)
        else:
            gukw = dict(glu_pair=True, act=self.act)
            downkw = {}  # RAW: x straight from L2 per wave, as o_proj
        h = self.b_h[0]
        hnext = self.b_hb
        t1 = self.b_t1[0]
        t2 = self.b_t2
        prev = None  # previous gemma layer (its postffn norm fused here)
        for i, lw in enumerate(self.layers):
            window = cfg.sliding_window if cfg.is_sliding(i) else 0
            if self.gemma and prev is not None:
                # h' = h + norm(t2_prev)*g_postffn_prev; stage norm(h')*g_in
                self._dgemv(lw, "wqkv", t2, self.b_qkv,
                            stage=ho.STAGE_NORM2, x2=h,
                            g=prev["g_postffn"], g2=lw["g_in"], res=hnext,
                            eps=eps)
                h, hnext = hnext, h
            elif i == 0 and "bqkv" not in lw:
                # layer 0: embed gather fused into the QKV staging pass
                # (x = table, x2 = sampled token id, res = persisted h)
                self._dgemv(lw, "wqkv", self.embed, self.b_qkv,
                            stage=ho.STAGE_NORM_EMBED, x2=self.next_token,
                            g=lw["g_in"], res=h, eps=eps,
                            escale=cfg.embed_scale)
            else:
                if i == 0:  # bias models keep the separate embed gather
                    ho.embed(self.embed, self.next_token, self.b_h, 1,
                             cfg.embed_scale)
                self._dgemv(lw, "wqkv", h, self.b_qkv, stage=ho.STAGE_NORM,
                            g=lw["g_in"], res=lw.get("bqkv"), eps=eps)
            prev = lw
            pfkw = {}
            attn_dec = ho.attn_dec
            if self._attn_pf is not None and self._attn_pf[i]:
                attn_dec = ho.attn_dec_pf
                pfkw = dict(regions=self._attn_pf[i],
                            pf_blocks=self.attn_pf_blocks,
                            stride0=self.attn_pf_stride,
                            sink=self._pf_sink)
            attn_dec(self.b_qkv, self.k_cache[i], self.v_cache[i],
                     self.b_att[0], self.len_buf, self.cos_t, self.sin_t,
                     self.attn_scratch, self.attn_cnt,
                     self.nh_l, self.kvh_l, self.hd, self.scale,
                     softcap=self.attn_softcap, window=window or 0,
                     split=self.attn_split, merge=self.attn_merge,
                     kS=self.k_scale[i], vS=self.v_scale[i], **pfkw)
            if self.gemma:
                self._dgemv(lw, "wo", self.b_att[0], t1)
                tpu.all_reduce(t1)
                # NORM2: h' = h + norm(t1)*g_post (persisted to hnext),
                # stage = norm(h')*g_preffn — both sandwich norms fused
                self._dgemv(lw, "wgu", t1, self.b_gu, stage=ho.STAGE_NORM2,
                            x2=h, g=lw["g_post"], g2=lw["g_preffn"],
                            res=hnext, eps=eps, **gukw)
                h, hnext = hnext, h
                self._dgemv(lw, "wdown", self.b_gu[:self.inter_l], t2,
                            **downkw)
                tpu.all_reduce(t2)
            else:
                if self.tp_branch:
                    self._dgemv(lw, "wo", self.b_att[0], t1)
                    tpu.all_reduce(t1)
                    ho.addinto(h, t1)
                else:
                    self._dgemv(lw, "wo", self.b_att[0], h, res=h)
                if self.moe:
                    # router -> topk expert-indexed GEMV pairs: W base
                    # offset by the device idx, output scaled by the
                    # device router prob, accumulated into h via res.
                    # xn is staged ONCE: expert 0's down-proj already
                    # updates h, so expert 1 must not re-norm it
                    ho.moe_route(h, lw["g_post"], lw["wg"], 1, self.topk,
                                 self.moe_idx, self.moe_w, eps=eps)
                    xn0 = self.b_xn[0]
                    ho.rmsnorm(h, lw["g_post"], xn0, eps=eps)
                    I, H = self.inter_l, self.H
                    for j in range(self.topk):
                        ei = self.moe_idx[j:j + 1]
                        osc = self.moe_w[j:j + 1]
                        if self.fp8:
                            ho.gemv_fp8(lw["wgu_q"], lw["wgu_s"], xn0,
                                        self.b_gu, eidx=ei,
                                        wstride=2 * I * H, sstride=2 * I)
                            ho.gemv_fp8(lw["wdown_q"], lw["wdown_s"],
                                        self.b_gu[:I], h, res=h,
                                        stage=ho.STAGE_GLU,
                                        x2=self.b_gu[I:], act=self.act,
                                        eidx=ei, wstride=H * I,
                                        sstride=H, oscale=osc)
                        else:
                            ho.gemv(lw["wgu"], xn0, self.b_gu, eidx=ei,
                                    wstride=2 * I * H)
                            ho.gemv(lw["wdown"], self.b_gu[:I], h, res=h,
                                    stage=ho.STAGE_GLU, x2=self.b_gu[I:],
                                    act=self.act, eidx=ei,
                                    wstride=H * I, oscale=osc)
                    continue
                self._dgemv(lw, "wgu", h, self.b_gu, stage=ho.STAGE_NORM,
                            g=lw["g_post"], eps=eps, **gukw)
                if self.tp_branch:
                    self._dgemv(lw, "wdown", self.b_gu[:self.inter_l], t1,
                                **downkw)
                    tpu.all_reduce(t1)
                    ho.addinto(h, t1)
                else:
                    self._dgemv(lw, "wdown", self.b_gu[:self.inter_l], h,
                                res=h, **downkw)
        if self.gemma:
            # last layer's post-ffn sandwich norm + final norm, both
            # fused into the lm_head staging (NORM2: h' = h + norm(t2)*
            # g_postffn, then stage norm(h')*g_final)
            self._lm_head_gemv(t2, stage=ho.STAGE_NORM2, x2=h,
                               g=self.layers[-1]["g_postffn"],
                               g2=self.g_final, res=hnext, eps=eps,
                               softcap=self.final_softcap)
        else:
            # final norm fused into the lm_head staging pass
            self._lm_head_gemv(h, stage=ho.STAGE_NORM, g=self.g_final,
                               eps=eps, softcap=self.final_softcap)

    # ------------------------------------------------------------------
    # lockstep batched decode (throughput mode; beyond-parity capability)
    # ------------------------------------------------------------------
    def _decode_batch_step(self, B: int, greedy: bool, min_p: float,
                           temperature: float = 1.0, top_k: int = 0,
                           top_p: float = 1.0, proc: bool = False,
                           logprobs: bool = False, rows=None):
        """One lockstep decode step with the sampler request given as
        plain arguments (see ``_batch_step``)."""
        self._batch_step(B, SampleSpec(greedy, min_p, temperature, top_k,
                                       top_p, proc, logprobs, rows))

    def _batch_step(self, B: int, spec: SampleSpec):
        """One decode step for B lockstep sequences: layer stack into
        bt_logits[:B], then the sampling tail.  fp8 weights take a fused
        stack (`_batch_layers_fused`) — the skinny fp8 MFMA GEMM up to
        B=16, or with LLM_BATCH_MX_MAX the multi-x GEMV (one weight
        stream feeds B accumulators); otherwise the layer stack runs as
        M=B-row MFMA GEMMs.  Graph-replayable (all state device-side)."""
        # measured (profiles/decode_kernels_r02.md): the SKINNY fp8 MFMA
        # GEMM wins at every B (even B=2: 1.34 vs the multi-x GEMV's
        # 1.44 ms — the GEMV is VALU-ISSUE-bound, 64 irreducible
        # v_pk_fma per 16 weight bytes at B=8).  The multi-x path stays
        # available via LLM_BATCH_MX_MAX for comparison.
        import os as _os  # noqa: delayed so env changes apply per call
        cfg = self.config
        mx_max = int(_os.environ.get("LLM_BATCH_MX_MAX", "0"))
        if (self.fp8 and B <= mx_max and not cfg.attention_bias
                and not self.moe):
            self._batch_layers_fused(B, partial(self._proj_mx, B))
        elif self.fp8 and B <= 16 and not self.moe:
            self._batch_layers_fused(B, partial(self._proj_skinny, B))
        else:
            self._batch_layers_gemm(B)
        self._sample_tail(self.bt_logits[:B], self._bv, B, spec)

    def _batch_layers_gemm(self, B: int):
        """Lockstep layer stack as M=B-row MFMA GEMMs (any dtype, MoE)."""
        cfg = self.config
        ho.embed(self.embed, self.bt_next, self.b_h, B, cfg.embed_scale)
        self._layers_forward(B, batch_attn=True)
        ho.rmsnorm(self.b_h[:B], self.g_final, self.b_xn[:B],
                   eps=cfg.rms_norm_eps)
        if self.fp8:
            ho.quant_fp8(self.b_xn[:B], self.b_xq, self.b_sx)
            ho.gemm_fp8(self.b_xq, self.b_sx, self.lm_head_q,
                        self.lm_head_s, self.bt_logits[:B], B, self.H,
                        accbuf=self.b_gemm_acc)
        else:
            ho.gemm(self.b_xn[:B], self.lm_head, self.bt_logits[:B],
                    accbuf=self.b_gemm_acc)
        if self.final_softcap:
            ho.softcap(self.bt_logits[:B], self.final_softcap)

    def _proj_mx(self, B, wq, ws, x, xstride, y, K, N, *, res=None,
                 bias=None, softcap=0.0, **stage_kw):
        """y[B, N] = W @ stage(x): ONE multi-x fp8 GEMV, the staging op
        (norm / embed / GLU) inside it.  Strides in elements."""
        assert bias is None, "bias models take the skinny path"
        ho.gemv_fp8_mx(wq, ws, x, y, B, xstride, N, res=res,
                       rstride=N if res is not None else 0,
                       softcap=softcap, **stage_kw)

    def _proj_skinny(self, B, wq, ws, x, xstride, y, K, N, *, res=None,
                     bias=None, softcap=0.0, **stage_kw):
        """The same projection as a (stage + e4m3 quant of the K-long
        rows, skinny fp8 MFMA GEMM) pair: B up to 16, W streamed once."""
        ho.stage_quant_mx(x, xstride, self.b_xq, self.b_sx, B, K, **stage_kw)
        ho.gemm_fp8_skinny(self.b_xq, self.b_sx, wq, ws, y, B, N, res=res,
                           rstride=N if res is not None else 0, bias=bias,
                           softcap=softcap, accbuf=self.b_gemm_acc)

    def _batch_layers_fused(self, B: int, proj):
        """Fused lockstep layer stack (fp8): mirrors `_decode_layers`'
        4-5 projections per layer over B rows, each one ``proj(wq, ws, x,
        xstride, y, K, N, res=, bias=, softcap=, **stage_kw)`` with the
        norm / embed gather / GLU as its staging op (`_proj_mx` or
        `_proj_skinny`)."""
        cfg = self.config
        eps = cfg.rms_norm_eps
        H, I = self.H, self.inter_l
        h = self.b_h            # (PC, H): rows 0..B = per-seq h
        hb = self.bt_hb         # gemma ping-pong
        t1, t2, gu = self.bt_t1, self.bt_t2, self.bt_gu
        qkvw = (self.nh_l + 2 * self.kvh_l) * self.hd
        nhh = self.nh_l * self.hd
        glu = dict(stage=ho.STAGE_GLU, x2=gu[:, I:], x2stride=2 * I,
                   act=self.act)

        def norm2(g, g2):
            # h' = h + norm(x)*g persisted to the other h buffer, stage
            # norm(h')*g2: both gemma sandwich norms in one staging pass
            return dict(stage=ho.STAGE_NORM2, x2=h, x2stride=H, g=g, g2=g2,
                        hout=hb, hstride=H, eps=eps)
        prev = None
        for i, lw in enumerate(self.layers):
            window = cfg.sliding_window if cfg.is_sliding(i) else 0
            x, xstride = h, H
            if self.gemma and prev is not None:
                x, st = t2, norm2(prev["g_postffn"], lw["g_in"])
                h, hb = hb, h
            elif i == 0:
                # embed gather fused into the QKV staging pass
                x, xstride = self.embed, 0
                st = dict(stage=ho.STAGE_NORM_EMBED, x2=self.bt_next,
                          g=lw["g_in"], hout=h, hstride=H, eps=eps,
                          escale=cfg.embed_scale)
            else:
                st = dict(stage=ho.STAGE_NORM, g=lw["g_in"], eps=eps)
            proj(lw["wqkv_q"], lw["wqkv_s"], x, xstride, self.bt_qkv, H,
                 qkvw, bias=lw.get("bqkv"), **st)
            prev = lw
            ho.attn_dec(self.bt_qkv, self.k_cache[i], self.v_cache[i],
                        self.b_att[0], self.bt_lens, self.cos_t, self.sin_t,
                        self.bt_scratch, self.bt_attn_cnt,
                        self.nh_l, self.kvh_l, self.hd, self.scale,
                        softcap=self.attn_softcap, window=window or 0,
                        split=self.attn_split, kS=self.k_scale[i],
                        vS=self.v_scale[i], batch=B, merge=self.attn_merge)
            if self.gemma:
                proj(lw["wo_q"], lw["wo_s"], self.b_att, nhh, t1, nhh, H)
                proj(lw["wgu_q"], lw["wgu_s"], t1, H, gu, H, 2 * I,
                     **norm2(lw["g_post"], lw["g_preffn"]))
                h, hb = hb, h
                proj(lw["wdown_q"], lw["wdown_s"], gu, 2 * I, t2, I, H,
                     **glu)
            else:
                proj(lw["wo_q"], lw["wo_s"], self.b_att, nhh, h, nhh, H,
                     res=h)
                proj(lw["wgu_q"], lw["wgu_s"], h, H, gu, H, 2 * I,
                     stage=ho.STAGE_NORM, g=lw["g_post"], eps=eps)
                proj(lw["wdown_q"], lw["wdown_s"], gu, 2 * I, h, I, H,
                     res=h, **glu)
        if self.gemma:
            x, st = t2, norm2(self.layers[-1]["g_postffn"], self.g_final)
        else:
            x, st = h, dict(stage=ho.STAGE_NORM, g=self.g_final, eps=eps)
        proj(self.lm_head_q, self.lm_head_s, x, H, self.bt_logits, H,
             self.vocab_l, softcap=self.final_softcap, **st)

    def prefill_batch(self, prompts) -> None:
        """Prefill B prompts (RAGGED lengths allowed) into per-sequence
        KV pools; each row then decodes from its own position
        (bt_lens[b] device-side)."""
        seqs = [np.asarray(p, dtype=np.int32).ravel() for p in prompts]
        B = len(seqs)
        assert 1 <= B <= self.max_batch and self.max_batch > 1
        assert self.world == 1, "batched decode is single-GPU for now"
        lens = [len(sq) for sq in seqs]
        if min(lens) == 0:
            raise ValueError("empty prompt in batch")
        if max(lens) + 1 >= self.max_seq:
            raise ValueError(f"prompt {max(lens)} fills the "
                             f"{self.max_seq} pool")
        self.reset()
        self.bt_nout.zero_()
        for b in range(B):
            self._pb = b
            P = lens[b]
            done = 0
            while done < P:
                M = min(P - done, self.PC)
                self.ids_buf[:M].copy_(
                    torch.from_numpy(seqs[b][done:done + M]))
                ho.i32_set(self.len_buf, done)
                ho.embed(self.embed, self.ids_buf, self.b_h, M,
                         self.config.embed_scale)
                self._layers_forward(M)
                done += M
            self._lm_head_last(M)
            self.bt_logits32[b].copy_(self.b_logits)
        self._pb = 0
        self.bt_lens[:B].copy_(torch.tensor(lens, dtype=torch.int32))
        self._host_lens = lens
        self._batch_n = B

    def decode_batch(self, n_tokens: int, greedy: bool = True,
                     min_p: float = 0.1, temperature: float = 1.0,
                     use_graph: bool = True,
                     first_from_logits: bool = True,
                     top_k: int = 0, top_p: float = 1.0,
                     logprobs: bool = False) -> np.ndarray:
        """Decode n_tokens for every prefilled sequence; returns int32
        ids of shape (B, n_tokens).  ``first_from_logits=False``
        continues a previous decode_batch (chunked serving).
        ``logprobs``: run the logprob stage for the rows switched on with
        ``setup_logprobs`` (read back with ``logprob_records``)."""
        B = self._batch_n
        spec = SampleSpec(greedy, min_p, temperature, top_k, top_p,
                          logprobs=bool(logprobs))
        self._stage_setup(n_tokens, False, spec.logprobs, lp_batch=True)
        if max(self._host_lens) + n_tokens > self.max_seq:
            raise ValueError("decode_batch would overflow the KV pool")
        self._host_lens = [p + n_tokens for p in self._host_lens]
        if first_from_logits:
            # first tokens from the prefill logits (fp32, batch rows)
            self._sample_tail(self.bt_logits32[:B], self._bv, B, spec,
                              first=True)
        n_steps = n_tokens - (1 if first_from_logits else 0)
        key = spec.graph_key("decode_batch", B)
        step = partial(self._batch_step, B, spec)
        if use_graph and n_steps > 0 and self._graph_mode != key \
                and not self._graph_failed:
            g = self._warm_and_capture(step)
            n_steps -= 1  # the warm-up was a real step
            if g is not None:
                self._graph, self._graph_mode = g, key
        if use_graph and self._graph_mode == key:
            for _ in range(n_steps):
                self._graph.replay()
        else:
            for _ in range(n_steps):
                step()
        torch.cuda.synchronize()
        n = int(self.bt_nout[0].item())
        out = self.bt_ring[:B, :n].cpu().numpy()
        return out[:, max(0, n - n_tokens):]

    # ---- continuous batching primitives (rows join/leave the group) ----
    def prefill_row(self, b: int, ids, greedy: bool = True,
                    min_p: float = 0.1, temperature: float = 1.0,
                    top_k: int = 0, top_p: float = 1.0, processors=None,
                    logprobs=None, row_sampler=None):
        """Prefill ONE sequence into slot b (other rows untouched) and
        sample its first token — a request JOINING the lockstep group
        between decode chunks (server continuous batching).
        ``row_sampler`` (dict of ``sampling.device_row_sampler_kwargs``:
        ``strategy`` and its fields, optional ``seed``) replaces greedy /
        min_p / temperature / top_k / top_p: the row's own sampler
        settings are written to the device table (draw counter 0) for
        ``decode_rows(row_sampler=True)``, where rows of any settings
        share one graph; the row's stream depends on its seed only.
        ``logprobs`` (int N within 0..``device_logprobs``, or None): the
        row's own top-N for ``decode_rows(logprobs=True)``; its first
        token's record is written here.  A row without it is switched
        off, so it may still ride in a logprobs group.
        ``processors`` (dict, see ``setup_processors``): the row's own
        penalties / logit_bias for ``decode_rows(processors=True)``; a
        row without them gets identity settings, so it may still ride in
        a processors group."""
        ids = np.asarray(ids, dtype=np.int32).ravel()
        P = len(ids)
        if P == 0:
            raise ValueError("empty prompt")
        assert 0 <= b < self.max_batch and self.max_batch > 1
        assert self.world == 1
        if P + 1 >= self.max_seq:
            raise ValueError(f"prompt {P} fills the {self.max_seq} pool")
        if row_sampler is not None:
            samp_words, samp_mode = self._samp_pack(row_sampler)
        self._pb = b
        done = 0
        while done < P:
            M = min(P - done, self.PC)
            self.ids_buf[:M].copy_(torch.from_numpy(ids[done:done + M]))
            ho.i32_set(self.len_buf, done)
            ho.embed(self.embed, self.ids_buf, self.b_h, M,
                     self.config.embed_scale)
            self._layers_forward(M)
            done += M
        self._lm_head_last(M)
        self._pb = 0
        self.bt_lens[b:b + 1].fill_(P)
        self.bt_nout[b:b + 1].zero_()
        rb = slice(b, b + 1)
        self._samp_chain.pop(b, None)
        if row_sampler is not None:
            self.bt_samp[b].copy_(samp_words)
            self._samp_modes[b] = samp_mode
            bits = ho.samp_row_chain(samp_words.numpy())
            if bits:
                self._samp_chain[b] = bits
        else:
            self._samp_modes.pop(b, None)
        spec = SampleSpec(greedy, min_p, temperature, top_k, top_p,
                          proc=processors is not None,
                          logprobs=logprobs is not None,
                          rows=(frozenset({samp_mode})
                                if row_sampler is not None else None),
                          chain=self._samp_chain.get(b, 0))
        self._stage_setup(1, spec.proc, spec.logprobs, lp_batch=True)
        if spec.logprobs:
            self.setup_logprobs(b, logprobs)
        else:
            self._lp_clear(b)
        if not spec.proc:
            self._proc_clear(b)
        # first token for this row only (row-sliced state); the row's
        # processor state is written once the raw logits are scanned
        self._sample_tail(
            self.b_logits, self._bv.rows(rb), 1, spec, first=True,
            before_adjust=(lambda: self.setup_processors(b, ids, processors))
            if spec.proc else None)
        while len(self._host_lens) < self.max_batch:
            self._host_lens.append(0)
        self._host_lens[b] = P
        self._batch_n = max(self._batch_n, b + 1)

    def compact_row(self, dst: int, src: int):
        """Move sequence slot src -> dst (KV pools, scales, device row
        state) so retired rows leave the group dense."""
        if dst == src:
            return
        for i in range(self.config.num_hidden_layers):
            self.k_cache[i][dst].copy_(self.k_cache[i][src])
            self.v_cache[i][dst].copy_(self.v_cache[i][src])
            if self.kv8:
                self.k_scale[i][dst].copy_(self.k_scale[i][src])
                self.v_scale[i][dst].copy_(self.v_scale[i][src])
        for t in (self.bt_lens, self.bt_next, self.bt_nout, self.bt_gmax,
                  self.bt_pick, self.bt_cnt):
            t[dst:dst + 1].copy_(t[src:src + 1])
        self.bt_ring[dst].copy_(self.bt_ring[src])
        if src in self._samp_modes:
            # sampler settings, seed and draw counter travel with the
            # row: its stream continues where it was
            self.bt_samp[dst].copy_(self.bt_samp[src])
            self._samp_modes[dst] = self._samp_modes[src]
        else:
            self._samp_modes.pop(dst, None)
        self._samp_chain.pop(dst, None)
        if src in self._samp_chain:
            self._samp_chain[dst] = self._samp_chain[src]
        if src in self._proc_rows:
            # the row's history and settings travel with it (the 4·V-byte
            # bias row only when it has one); rows without processors
            # cost nothing here
            has_bias = self._proc_rows[src]
            self.p_stat[dst].copy_(self.p_stat[src])
            self.p_proc[dst].copy_(self.p_proc[src])
            if has_bias:
                self.p_bias[dst].copy_(self.p_bias[src])
            self._proc_rows[dst] = has_bias
        else:
            self._proc_clear(dst)
        if src in self._lp_rows:
            # cfg, stage and the record ring travel with the row; the
            # scan scratch is all zero between steps and the raw
            # snapshot lives within one step, so neither moves
            for t in (self.lp_cfg, self.lp_stage, self.lp_val, self.lp_idx):
                t[dst:dst + 1].copy_(t[src:src + 1])
            self._lp_rows[dst] = self._lp_rows[src]
        else:
            self._lp_clear(dst)
        self._host_lens[dst] = self._host_lens[src]

    def decode_rows(self, B: int, n: int, greedy: bool = True,
                    min_p: float = 0.1, temperature: float = 1.0,
                    use_graph: bool = True, top_k: int = 0,
                    top_p: float = 1.0, processors: bool = False,
                    logprobs: bool = False, row_sampler: bool = False):
        """n lockstep steps for rows [0, B) (each already holding a
        sampled next token from prefill_row / a previous chunk).
        ``row_sampler``: every row samples with its own settings from the
        device table (rows set up by ``prefill_row(row_sampler=...)``);
        greedy / min_p / temperature / top_k / top_p are then unused and
        the graph is keyed on which sampler stages the rows need, not on
        any value.
        ``processors``: run the graph variant with the logit-adjust
        stage (rows set up by ``prefill_row(processors=...)``).
        ``logprobs``: run the graph variant with the logprob stage (rows
        set up by ``prefill_row(logprobs=N)``; at most LP_RING steps per
        call — drain with ``logprob_records`` in between).
        Returns a list of B arrays: each row's n new token ids."""
        assert 1 <= B <= self.max_batch
        processors, logprobs = bool(processors), bool(logprobs)
        self._stage_setup(n, processors, logprobs, lp_batch=True)
        if max(self._host_lens[:B]) + n > self.max_seq:
            raise ValueError("decode_rows would overflow the KV pool")
        for b in range(B):
            self._host_lens[b] += n
        spec = SampleSpec(greedy, min_p, temperature, top_k, top_p,
                          processors, logprobs,
                          self._row_modes(B) if row_sampler else None,
                          self._row_chain(B) if row_sampler else 0)
        key = spec.graph_key("decode_rows", B)
        step = partial(self._batch_step, B, spec)
        g = self._bgraphs.get(key)
        remaining = n
        if use_graph and g is None and n > 1 and not self._graph_failed:
            g = self._warm_and_capture(step)
            remaining -= 1  # the warm-up was a real step
            if g is not None:
                self._bgraphs[key] = g
        if g is not None and use_graph:
            for _ in range(remaining):
                g.replay()
        else:
            for _ in range(remaining):
                step()
        torch.cuda.synchronize()
        comm = tpu.xgmi_comm()
        if comm is not None:
            comm.check()
        nouts = self.bt_nout[:B].cpu().numpy()
        ring = self.bt_ring[:B].cpu().numpy()
        # each step appends exactly one id per row
        return [ring[b, max(0, int(nouts[b]) - n):int(nouts[b])]
                for b in range(B)]

    def generate_tokens_batch(self, prompts, max_tokens: int,
                              greedy: bool = True, min_p: float = 0.1,
                              temperature: float = 1.0, top_k: int = 0,
                              top_p: float = 1.0) -> np.ndarray:
        """Convenience: prefill_batch + decode_batch -> (B, max_tokens)."""
        self.prefill_batch(prompts)
        return self.decode_batch(max_tokens, greedy=greedy, min_p=min_p,
                                 temperature=temperature, top_k=top_k,
                                 top_p=top_p)

    def capture_decode_graph(self, greedy: bool = True, min_p: float = 0.1,
                             temperature: float = 1.0, top_k: int = 0,
                             top_p: float = 1.0, processors: bool = False,
                             logprobs: bool = False, rows=None,
                             chain: int = 0):
        """Capture one decode step into a hipGraph (fixed shapes: KV pool
        is preallocated and the position is a device scalar — SURVEY §7
        'graph must be shape-stable').  ``logprobs``: the step carries the
        logprob stage (scan ahead of the adjust stage, commit after the
        sampler).  ``rows``: the mode set of a ``row_sampler`` run,
        ``chain``: its row's chain bits (``ho.samp_row_chain``).  The
        arguments make a ``SampleSpec``; its ``graph_key`` is the mode the
        single graph slot is cached under.

        NOTE: the warm-up executes ONE REAL decode step (advances the
        sequence by one token).  Returns ``(steps_taken, ok)``:
        ``steps_taken`` is the number of real decode steps executed here
        (1 whenever the warm-up ran, 0 when the cached graph is reused)
        — callers MUST account for it even when ``ok`` is False.  On
        capture failure ``ok`` is False, ``self._graph_failed`` is set
        (no further capture attempts) and the exception is kept in
        ``self._graph_error``."""
        spec = SampleSpec(greedy, min_p, temperature, top_k, top_p,
                          bool(processors), bool(logprobs), rows,
                          int(chain))
        # the stages are part of the key; the logprob top-N and, with
        # rows, the sampler values are not (device data)
        mode = spec.graph_key("decode")
        if spec.logprobs:
            self._lp_alloc(raw=spec.proc)
        if self._graph_mode == mode:
            return 0, True
        if self._graph_failed:
            return 0, False
        g = self._warm_and_capture(partial(self._step, spec))
        if g is None:
            # the warm-up step DID run (token committed to out_ring,
            # len_buf advanced) — report it so decode() does not
            # double-count
            torch.cuda.synchronize()
            return 1, False
        self._graph = g
        self._graph_mode = mode
        return 1, True

    def _warm_and_capture(self, step):
        """``step()`` once on a side stream — a REAL decode step, the
        caller accounts for it — then captured into a hipGraph.  Returns
        the graph, or None when capture failed: ``_graph_failed`` is then
        set (no further capture attempts) and the exception kept in
        ``_graph_error``."""
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        # No cyclic-garbage collection may land inside the capture: a dead
        # cycle can hold another engine's tensors and captured graphs, and
        # releasing those calls HIP APIs a capturing process must not make
        # (the process aborts).  torch.cuda.graph() no longer collects on
        # entry by default, so collect here and hold the collector off
        # until the capture has ended.
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
        except Exception as e:
            self._graph_failed = True
            self._graph_error = e
            return None
        finally:
            if gc_was_on:
                gc.enable()
        return g

    def prefill(self, ids: np.ndarray, cache: Optional[DeviceCacheHandle] = None):
        cache = cache or self.make_cache(self.max_seq)
        with trace_range(f"prefill[{len(np.asarray(ids).ravel())}]"):
            logits = self.forward(ids, cache, 0)
        return cache, logits

    def decode(self, n_tokens: int, greedy: bool = True, min_p: float = 0.1,
               use_graph: bool = True, first_from_logits: bool = True,
               temperature: float = 1.0, top_k: int = 0,
               top_p: float = 1.0, processors: bool = False,
               logprobs: bool = False, row_sampler: bool = False):
        """Generate n_tokens ids device-side; returns int32 numpy ids.
        Assumes prefill() ran (len_buf == prompt length, logits ready).
        ``processors``: run the logit-adjust stage ahead of every sample
        with row 0's state (``generate_tokens`` sets it up).
        ``logprobs``: run the logprob stage around every sample with row
        0's top-N (``setup_logprobs(0, N)``; ``generate_tokens`` does it);
        read the records with ``logprob_records`` — at most LP_RING
        tokens per call.
        ``row_sampler``: sample with the settings ``generate_tokens`` wrote
        to the single-sequence sampler table (greedy / min_p / temperature
        / top_k / top_p are then unused)."""
        spec = SampleSpec(greedy, min_p, temperature, top_k, top_p,
                          bool(processors), bool(logprobs),
                          self._s_rows if row_sampler else None,
                          self._s_chain if row_sampler else 0)
        self._stage_setup(n_tokens, spec.proc, spec.logprobs, lp_batch=False)
        if self._host_len + n_tokens > self.max_seq:
            raise ValueError(
                f"decode would overflow the KV pool: len {self._host_len} "
                f"+ {n_tokens} > max_seq {self.max_seq}")
        self._host_len += n_tokens
        if first_from_logits:
            # sample token 0 from the prefill logits
            self._sample_tail(self.b_logits, self._sv, 1, spec, first=True)
        n_steps = n_tokens - (1 if first_from_logits else 0)
        if use_graph and n_steps > 0:
            # capture_decode_graph reports the warm-up step it executed
            # even when capture fails, so n_steps stays exact either way
            taken, ok = self.capture_decode_graph(
                greedy, min_p, temperature, top_k, top_p, spec.proc,
                spec.logprobs, spec.rows, spec.chain)
            n_steps -= taken
            if not ok:
                use_graph = False
        if use_graph and n_steps > 0:
            for _ in range(n_steps):
                self._graph.replay()
        else:
            for _ in range(n_steps):
                self._step(spec)
        torch.cuda.synchronize()
        comm = tpu.xgmi_comm()
        if comm is not None:
            comm.check()  # raise if a one-shot collective timed out
        n = int(self.nout.item())
        return self.out_ring[:n].cpu().numpy()[max(0, n - n_tokens):]
