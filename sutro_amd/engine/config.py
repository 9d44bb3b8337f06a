"""Engine configuration, sized for MI355X (288 GB HBM3E per GPU)."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from ..models.registry import ModelSpec

KV_BLOCK_SIZE = 32  # tokens per KV page (multiple of 16 for dwordx4-aligned rows)


@dataclass
class EngineConfig:
    spec: ModelSpec
    device: str = "cuda"            # "cuda" (=HIP on ROCm) or "cpu"
    dtype: torch.dtype = torch.bfloat16
    kv_block_size: int = KV_BLOCK_SIZE
    # "bf16" (default) or "fp8_e4m3": OCP e4m3 KV cache — halves KV bytes and
    # doubles resident batch capacity at ~2^-6 relative quantization error
    kv_dtype: str = "bf16"
    max_model_len: int = 8192        # scheduler cap on prompt+output length
    max_num_seqs: int = 1024         # max concurrently running sequences
    max_tokens_per_step: int = 32768  # token budget per scheduler step (prefill chunking)
    # throughput policy: while decodes are running, hold back new p1 prefills
    # until this many prompt tokens have accumulated (amortizes the eager
    # prefill pass; hipGraph decode steps stay pure and the decode batch stays
    # near its peak size). None = one full step budget (max_tokens_per_step) —
    # measured +18%% steady-state tokens/s at batch 2048 vs a 4096 threshold.
    # 0 = admit eagerly. p0 (interactive) rows always bypass the hold-back.
    min_prefill_batch_tokens: Optional[int] = None
    # EXPERIMENTAL: capture the prefill pass in a hipGraph at a fixed
    # max_tokens_per_step shape and replay it for accumulated waves (saves the
    # ~80-180 ms/wave eager launch overhead). Off until GPU-validated
    # (ROADMAP.md; engine/prefill_graph.py).
    graph_prefill: bool = False
    graph_prefill_min_tokens: int = 16384
    # EXPERIMENTAL: one-step-lagged decode. The sampled-token tensor of step
    # N feeds step N+1's input ids directly (device-side), so the host never
    # waits on the GPU inside a pure-decode streak: stop/FSM bookkeeping
    # consumes step N's tokens while step N+1 runs. Rows that finish decode
    # one extra discarded token. FSM-guided rows force the synchronous path
    # (their mask needs the sampled token). Off until GPU-validated
    # (ROADMAP.md item 4 — async decode).
    async_decode: bool = False
    gpu_memory_utilization: float = 0.90
    num_kv_blocks: Optional[int] = None  # None = derive from free memory
    default_max_new_tokens: int = 256
    seed: int = 0
    # optional safetensors checkpoint dir; None = deterministic random init
    weights_path: Optional[str] = None
    enforce_eager: bool = False      # disable hipGraph capture of the decode step
    # tensor parallelism (process group set up by the caller)
    tp_size: int = 1
    tp_rank: int = 0
    # MoE layers: shard EXPERTS across the tp group (expert parallelism)
    # instead of sharding every expert's intermediate dim
    moe_ep: bool = False
    # "bf16" (default) or "fp8_e4m3": store MoE expert weights as OCP e4m3
    # with f32 per-output-channel scales (quantised after load, per shard)
    # and run them on the block-scaled fp8 MFMA — halves expert bytes, which
    # frees memory for KV. Ignored for specs without experts (a service
    # hands one engine_kwargs to every model).
    # "mxfp4": OCP MX e2m1 codes with one e8m0 scale per 32 K-elements (4.25
    # bits per weight), dequantised inside the block-scaled MFMA (W4A8).
    moe_weight_dtype: str = "bf16"
    # "bf16" (default) or "fp8_e4m3": store the dense projections (qkv / o of
    # every attention block, gate_up / down of every dense MLP) as OCP e4m3
    # with f32 per-output-channel scales (quantised after load, per TP shard)
    # and run them W8A8 on the pipelined block-scaled fp8 MFMA GEMM
    # (csrc/gemm_tn_fp8_pipe.hip) — halves those bytes, which frees memory
    # for KV. Embeddings / lm_head, norms, the MoE router and the experts
    # keep their storage; independent of moe_weight_dtype.
    # "fp8_block128": the same projections as OCP e4m3 with one f32 scale per
    # 128x128 weight block (`weight` + `weight_scale_inv`, the layout of the
    # published block-FP8 checkpoints, which load without a bf16 stage) and
    # activations quantised per token and 128-wide K group, on
    # csrc/gemm_tn_fp8_block_pipe.hip. Projections that arrive unquantised
    # are quantised after load; ones that are not whole blocks stay bf16.
    dense_weight_dtype: str = "bf16"
    # block-hash prefix cache: full blocks of computed prompt tokens are
    # indexed by (parent block, token ids) and shared between rows by
    # reference count, so a job's common system prompt is prefilled and held
    # once (docs/ENGINE.md, "Prefix cache"). Forced off for embedding specs
    # (mean pooling needs every token's hidden state).
    enable_prefix_caching: bool = False
    # decode attention over shared prefix pages: "per_row" streams them once
    # per row (the ordinary kernel); "shared" streams them once per tile of
    # rows with a common prefix and hands the f32 softmax state to the
    # per-row kernel for the rest — bit-identical output. Meaningful only
    # with enable_prefix_caching on the GPU MFMA decode route.
    prefix_decode: str = "per_row"
    # local attention: run the spec's sliding-window layers with their window
    # and its attention sinks (ModelSpec.sliding_window /
    # sliding_window_pattern / attention_sinks; docs/ENGINE.md, "Local
    # attention"). Off: those fields are ignored and every layer is full
    # causal attention without a sinks parameter, as before. Ignored for
    # specs with neither (a service hands one engine_kwargs to every model).
    local_attention: bool = False

    def __post_init__(self) -> None:
        if self.prefix_decode not in ("per_row", "shared"):
            raise ValueError(
                f"prefix_decode must be 'per_row' or 'shared', "
                f"got {self.prefix_decode!r}")
        if not isinstance(self.local_attention, bool):
            raise ValueError(
                f"local_attention must be True or False, "
                f"got {self.local_attention!r}")
        if self.local_attention and (
                self.spec.sliding_window < 0
                or self.spec.sliding_window_pattern < 0
                or (self.spec.sliding_window_pattern > 0
                    and self.spec.sliding_window == 0)):
            raise ValueError(
                f"local_attention needs sliding_window > 0 where "
                f"sliding_window_pattern > 0, and neither negative (got "
                f"window {self.spec.sliding_window}, pattern "
                f"{self.spec.sliding_window_pattern})")
        if self.spec.embedding:
            self.enable_prefix_caching = False
        if self.moe_weight_dtype not in ("bf16", "fp8_e4m3", "mxfp4"):
            raise ValueError(
                f"moe_weight_dtype must be 'bf16', 'fp8_e4m3' or 'mxfp4', "
                f"got {self.moe_weight_dtype!r}")
        if self.dense_weight_dtype not in ("bf16", "fp8_e4m3",
                                           "fp8_block128"):
            raise ValueError(
                f"dense_weight_dtype must be 'bf16', 'fp8_e4m3' or "
                f"'fp8_block128', got {self.dense_weight_dtype!r}")
        if self.device == "cpu":
            self.dtype = torch.float32
        if self.max_model_len > self.spec.max_context:
            self.max_model_len = self.spec.max_context

    def derive_num_kv_blocks(self, free_bytes: int) -> int:
        """KV blocks that fit in `free_bytes` (both K and V, all layers)."""
        spec = self.spec
        kvh = spec.num_kv_heads // self.tp_size if spec.num_kv_heads >= self.tp_size else 1
        if self.kv_dtype == "fp8_e4m3":
            elem = 1
        elif self.dtype in (torch.bfloat16, torch.float16):
            elem = 2
        else:
            elem = 4
        bytes_per_block = (
            2  # K and V
            * spec.num_layers
            * kvh
            * self.kv_block_size
            * spec.head_dim
            * elem
        )
        return max(16, int(free_bytes // bytes_per_block))

    def kv_torch_dtype(self) -> torch.dtype:
        if self.kv_dtype == "fp8_e4m3":
            return torch.float8_e4m3fn
        return self.dtype
