"""Op dispatch: hand-written CDNA4 HIP kernels on GPU, torch reference on CPU.

The HIP extension (`sutro_amd._C`, built by `setup.py build_ext --inplace` or
`__graft_entry__.build()`) is REQUIRED on GPU: any op called with CUDA(HIP)
tensors raises if the extension is missing — no silent eager fallback on the
hot path.
"""

from __future__ import annotations

import os
from typing import Optional

import torch

from . import torch_ref

_C = None
_C_ERR: Optional[str] = None
try:
    from sutro_amd import _C as _C  # type: ignore
except Exception as e:  # pragma: no cover - exercised only without built ext
    _C_ERR = f"{type(e).__name__}: {e}"


def hip_available() -> bool:
    return _C is not None


def _require_hip():
    if _C is None:
        raise RuntimeError(
            "sutro_amd HIP extension (_C) is not built but a GPU tensor was passed. "
            "Build it with `python setup.py build_ext --inplace` "
            f"(import error: {_C_ERR})"
        )
    return _C


# Env escape hatch for A/B profiling only (never the default).
_FORCE_REF = os.environ.get("SUTRO_AMD_FORCE_TORCH_REF", "0") == "1"


def _use_hip(t: torch.Tensor) -> bool:
    return t.is_cuda and not _FORCE_REF


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    if _use_hip(x):
        out = torch.empty_like(x)
        _require_hip().rmsnorm(out, x, weight, eps)
        return out
    return torch_ref.rmsnorm(x, weight, eps)


# Row widths C at which fused_add_rmsnorm runs rmsnorm_wide_reg_kernel (row
# held in registers, csrc/rmsnorm.hip) instead of rmsnorm_wide_kernel. Same
# bits from both; listed are the widths measured to clear the project's
# margin at every measured row count (profiles/PROFILES.md capture A1).
RMSNORM_REG_RULE: frozenset = frozenset({5120})   # Qwen3-32B

# SUTRO_RMSNORM=v1 forces the reference kernel, =reg the register one (A/B
# only); unset follows RMSNORM_REG_RULE.
_RMSNORM_FORCE: Optional[bool] = {"reg": True, "v1": False}.get(
    os.environ.get("SUTRO_RMSNORM", ""))


def fused_add_rmsnorm(x, residual, weight, eps: float,
                      variant: Optional[str] = None):
    """`variant`: "v1" / "reg" pick the kernel explicitly (tests, A/B)."""
    if _use_hip(x):
        if variant is not None:
            reg = {"reg": True, "v1": False}[variant]
        elif _RMSNORM_FORCE is not None:
            reg = _RMSNORM_FORCE
        else:
            reg = x.shape[-1] in RMSNORM_REG_RULE
        # in-place: residual += x; x_out = rmsnorm(residual)
        _require_hip().fused_add_rmsnorm(x, residual, weight, eps,
                                         1 if reg else 0)
        return x, residual
    return torch_ref.fused_add_rmsnorm(x, residual, weight, eps)


def silu_mul(x: torch.Tensor) -> torch.Tensor:
    if _use_hip(x):
        T, two_i = x.shape
        out = torch.empty((T, two_i // 2), dtype=x.dtype, device=x.device)
        _require_hip().silu_mul(out, x)
        return out
    return torch_ref.silu_mul(x)


# Dense-MLP gate_up routing: (K, 2I) -> (min_M, held_back). The fused kernel
# (csrc/gemm_tn_pipe.hip, SwiGLU epilogue) runs for every token count
# M >= min_M, the smallest M from which every measured point beat the library
# GEMM + silu_mul pair by the margin of profiles/PROFILES.md capture G1;
# shapes not listed were not measured to win and stay on the library pair.
# held_back: hipGraph decode buckets kept on the library pair although they
# clear the margin. The fused kernel sums K in gemm_tn's order, which is also
# the order of the library kernels picked at the other buckets (identical
# results there, G1); at these three the library's kernel sums a few tiles
# differently, and a decode batch that shrinks through them would no longer
# return what the library path returns.
GATE_UP_FUSED_RULE: dict = {
    (5120, 51200): (1152, frozenset({1536, 1664, 1792})),   # Qwen3-32B
}

# SUTRO_GATE_UP_FUSED=1 forces the fused kernel wherever the shape qualifies,
# =0 forces the library pair (A/B only); unset follows GATE_UP_FUSED_RULE.
_GATE_UP_FORCE: Optional[bool] = {"1": True, "0": False}.get(
    os.environ.get("SUTRO_GATE_UP_FUSED", ""))


def set_gate_up_fused(mode: Optional[bool]) -> None:
    """In-process form of SUTRO_GATE_UP_FUSED: True / False force the path,
    None restores the measured rule."""
    global _GATE_UP_FORCE
    _GATE_UP_FORCE = mode


# Which fused kernel a routed (K, 2I, M) runs: (K, 2I) -> list of
# (min_M, max_M, variant, group_m, wide), first match wins, max_M None = no
# upper end; no match = "v1", the one-tile-per-block kernel in its plain tile
# order. variant 1 is the persistent kernel (seam prefetch), wide its dwordx4
# epilogue stores; group_m is the tile order of either kernel: > 0 groups of
# that many M-tiles, < 0 one band of M-tiles per XCD walked in groups of
# -group_m (csrc/gemm_tn_pipe.hip). Every
# variant returns the same bits, so this table is a speed choice only; it is
# consulted only for shapes GATE_UP_FUSED_RULE routes to the fused kernel and
# is filled from profiles/PROFILES.md capture G2 by G1's margin (median
# better than v1's by more than twice the larger min-max spread at every
# measured M of the range).
GATE_UP_VARIANT_RULE: dict = {
    # Qwen3-32B prefill waves: the one-tile kernel in the XCD-banded order,
    # groups of 8 M-tiles (the persistent kernel and the wide stores cleared
    # the margin against it nowhere, G2)
    (5120, 51200): [(8192, 32768, 0, -8, False)],
}
_V1 = (0, 0, False)


def _parse_variant(text: str):
    """"v1" | "persistent[,group_m[,wide]]" -> (variant, group_m, wide)."""
    parts = [p.strip() for p in text.split(",")]
    if parts[0] == "v1" and len(parts) == 1:
        return _V1
    if parts[0] == "persistent" and len(parts) <= 3:
        group_m = int(parts[1]) if len(parts) > 1 and parts[1] else 0
        wide = len(parts) > 2 and parts[2] == "wide"
        if len(parts) > 2 and parts[2] not in ("", "wide"):
            raise ValueError(f"bad gate_up variant {text!r}")
        return (1, group_m, wide)
    raise ValueError(f"bad gate_up variant {text!r}: expected 'v1' or "
                     "'persistent[,group_m[,wide]]'")


# SUTRO_GATE_UP_VARIANT=v1 forces the one-tile kernel wherever the fused
# kernel runs, =persistent[,group_m[,wide]] the persistent one (A/B only);
# unset follows GATE_UP_VARIANT_RULE.
_GATE_UP_VARIANT_FORCE = (
    _parse_variant(os.environ["SUTRO_GATE_UP_VARIANT"])
    if os.environ.get("SUTRO_GATE_UP_VARIANT") else None)


def set_gate_up_variant(mode) -> None:
    """In-process form of SUTRO_GATE_UP_VARIANT: the same string, or None to
    restore the measured table."""
    global _GATE_UP_VARIANT_FORCE
    _GATE_UP_VARIANT_FORCE = None if mode is None else _parse_variant(mode)


def gate_up_variant(k: int, two_i: int, m: int):
    """(variant, group_m, wide) of the fused kernel for a routed shape. The
    persistent kernel needs K % 128 == 0; other K stay on v1."""
    if k % 128 != 0:
        return _V1
    if _GATE_UP_VARIANT_FORCE is not None:
        return _GATE_UP_VARIANT_FORCE
    for lo, hi, variant, group_m, wide in GATE_UP_VARIANT_RULE.get(
            (k, two_i), ()):
        if m >= lo and (hi is None or m <= hi):
            return (variant, group_m, wide)
    return _V1


def gate_up_silu_qualifies(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """Shapes the fused kernel takes: bf16, contiguous, K % 64 == 0 and
    I % 128 == 0 (weight is the merged [2I, K], gate rows first)."""
    return (x.dim() == 2 and weight.dim() == 2 and x.shape[0] >= 1
            and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
            and x.is_contiguous() and weight.is_contiguous()
            and x.shape[1] == weight.shape[1] and x.shape[1] % 64 == 0
            and weight.shape[0] >= 256 and weight.shape[0] % 256 == 0)


def gate_up_silu(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """SwiGLU of the merged gate_up projection: silu(x Wg^T) * (x Wu^T) for
    weight = [Wg; Wu] of shape [2I, K]; returns [T, I]. On GPU, qualifying
    shapes selected by the routing rule run as ONE kernel (no [T, 2I]
    intermediate, no silu_mul pass); everything else is the library GEMM
    followed by silu_mul. No host sync, output from the caching allocator:
    safe under hipGraph capture."""
    if _use_hip(x) and gate_up_silu_qualifies(x, weight):
        if _GATE_UP_FORCE is None:
            min_m, held_back = GATE_UP_FUSED_RULE.get(
                (x.shape[1], weight.shape[0]), (None, ()))
            fused = (min_m is not None and x.shape[0] >= min_m
                     and x.shape[0] not in held_back)
        else:
            fused = _GATE_UP_FORCE
        if fused:
            v = gate_up_variant(x.shape[1], weight.shape[0], x.shape[0])
            if v == _V1:
                return _require_hip().gemm_gate_up_silu(x, weight)
            return _require_hip().gemm_gate_up_silu(
                x, weight, 2, 1, v[0], v[1], 0, v[2])
    return silu_mul(torch.nn.functional.linear(x, weight))


def fused_qkv_prep(
    qkv: torch.Tensor,            # [T, Hq*D + 2*Hk*D] (qkv GEMM output)
    num_heads: int, num_kv_heads: int, head_dim: int,
    positions: torch.Tensor, slot_mapping: torch.Tensor,
    k_cache: torch.Tensor, v_cache: torch.Tensor,
    cos_sin: torch.Tensor,
    q_norm_w: Optional[torch.Tensor] = None,
    k_norm_w: Optional[torch.Tensor] = None,
    eps: float = 1e-6,
) -> torch.Tensor:
    """Per-head qk-RMSNorm + RoPE + paged KV write; returns contiguous q
    [T, Hq, D]. One fused kernel on GPU (reads the GEMM output in place)."""
    T = qkv.shape[0]
    if _use_hip(qkv):
        q_out = torch.empty((T, num_heads, head_dim), dtype=qkv.dtype,
                            device=qkv.device)
        _require_hip().qkv_prep(qkv, q_out, k_cache, v_cache, positions,
                                slot_mapping, cos_sin, q_norm_w, k_norm_w, eps)
        return q_out
    q_size = num_heads * head_dim
    kv_size = num_kv_heads * head_dim
    q, k, v = qkv.split([q_size, kv_size, kv_size], dim=-1)
    q = q.reshape(T, num_heads, head_dim).contiguous()
    k = k.reshape(T, num_kv_heads, head_dim).contiguous()
    v = v.reshape(T, num_kv_heads, head_dim).contiguous()
    if q_norm_w is not None:
        q = torch_ref.rmsnorm(q, q_norm_w, eps)
    if k_norm_w is not None:
        k = torch_ref.rmsnorm(k, k_norm_w, eps)
    q, k = torch_ref.apply_rope(q, k, positions, cos_sin)
    torch_ref.write_kv_cache(k, v, k_cache, v_cache, slot_mapping)
    return q


def rope_and_cache(
    q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
    positions: torch.Tensor, slot_mapping: torch.Tensor,
    k_cache: torch.Tensor, v_cache: torch.Tensor,
    cos_sin: torch.Tensor,
) -> torch.Tensor:
    """Apply RoPE to q,k (in place on GPU) and scatter k,v into the paged cache.
    Returns q (rotated)."""
    if _use_hip(q):
        _require_hip().rope_and_cache(q, k, v, positions, slot_mapping,
                                      k_cache, v_cache, cos_sin)
        return q
    q, k = torch_ref.apply_rope(q, k, positions, cos_sin)
    torch_ref.write_kv_cache(k, v, k_cache, v_cache, slot_mapping)
    return q


_EMPTY_I32: Optional[torch.Tensor] = None


# Prefill attention routing: (G, head_dim) -> rows per q tile of the
# pipelined kernel (csrc/attn_prefill.hip, attn_prefill_pipe_kernel); a head
# layout that is not listed runs the one-tile-per-block reference kernel on
# 32-row tiles. Both kernels return the same bits, so this table is a speed
# choice only. It is filled from profiles/PROFILES.md capture A1 by the
# project's margin: a granularity is listed only where its median beat the
# reference kernel's by more than twice the larger min-max spread of the two
# at every measured shape, and of those the fastest at the wave shape.
PREFILL_TILE_ROWS: tuple = (32, 64, 128)
ATTN_PREFILL_RULE: dict = {
    (8, 128): 64,   # Qwen3-32B: 8 waves, each walking two 32-row sub-tiles
}

# SUTRO_ATTN_PREFILL=v1 forces the reference kernel, =pipe[,rows] the
# pipelined one at `rows` rows per tile (default 32) wherever it takes the
# head layout (A/B only); unset follows ATTN_PREFILL_RULE.


def _parse_attn_prefill(text: str):
    """"v1" | "pipe[,rows]" -> None (reference kernel) or rows per tile."""
    parts = [p.strip() for p in text.split(",")]
    if parts == ["v1"]:
        return None
    if parts[0] == "pipe" and len(parts) <= 2:
        rows = int(parts[1]) if len(parts) > 1 else 32
        if rows in PREFILL_TILE_ROWS:
            return rows
    raise ValueError(f"bad prefill attention variant {text!r}: expected "
                     "'v1' or 'pipe[,32|64|128]'")


_ATTN_PREFILL_FORCE = (
    (_parse_attn_prefill(os.environ["SUTRO_ATTN_PREFILL"]),)
    if os.environ.get("SUTRO_ATTN_PREFILL") else None)


def set_attn_prefill(mode) -> None:
    """In-process form of SUTRO_ATTN_PREFILL: the same string, or None to
    restore the measured table."""
    global _ATTN_PREFILL_FORCE
    _ATTN_PREFILL_FORCE = None if mode is None else (_parse_attn_prefill(mode),)


def attn_prefill_pipe_supported(num_heads: int, num_kv_heads: int,
                                head_dim: int, tile_rows: int) -> bool:
    """Mirror of the kernel's own check: G <= 8 heads per kv head (one wave
    each) and G * tile_rows / 32 (head, sub-tile) pairs per block of 1, 2, 4,
    8 or 16."""
    if num_kv_heads <= 0 or num_heads % num_kv_heads:
        return False
    if head_dim not in (64, 128) or tile_rows not in PREFILL_TILE_ROWS:
        return False
    g = num_heads // num_kv_heads
    return g <= 8 and g * (tile_rows // 32) in (1, 2, 4, 8, 16)


def prefill_tile_rows(num_heads: int, num_kv_heads: int,
                      head_dim: int) -> Optional[int]:
    """Rows per prefill q tile of the pipelined kernel for this head layout,
    or None where the reference kernel runs (its tiles have 32 rows). Callers
    build tile_seq / tile_q0 with a step of `prefill_tile_step(...)`."""
    if _ATTN_PREFILL_FORCE is not None:
        rows = _ATTN_PREFILL_FORCE[0]
    else:
        rows = ATTN_PREFILL_RULE.get(
            (num_heads // max(num_kv_heads, 1), head_dim))
    if rows is not None and attn_prefill_pipe_supported(
            num_heads, num_kv_heads, head_dim, rows):
        return rows
    return None


def prefill_tile_step(num_heads: int, num_kv_heads: int, head_dim: int,
                      max_new_tokens: Optional[int] = None,
                      local_attention: bool = False) -> int:
    """Step at which the engine builds its prefill tile lists. A batch whose
    longest chunk has at most 32 new tokens (`max_new_tokens`) is built at 32
    rows even where the layout's rule names more: the further sub-tiles of
    every block would be empty (measured in capture A1, seeded step).
    `local_attention`: the model has a layer with a window or sinks; those
    run the reference kernel, whose tiles have 32 rows, and one tile list
    serves every layer."""
    if local_attention:
        return 32
    rows = prefill_tile_rows(num_heads, num_kv_heads, head_dim) or 32
    if max_new_tokens is not None and max_new_tokens <= 32:
        return 32
    return rows


def paged_attention(
    q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
    block_tables: torch.Tensor, seq_lens: torch.Tensor,
    query_start_locs: torch.Tensor, scale: float,
    num_decodes_tail: int = 0,
    tile_seq: Optional[torch.Tensor] = None,
    tile_q0: Optional[torch.Tensor] = None,
    prefill_token_count: int = 0,
    tile_rows: int = 32,
    prefill_variant: Optional[str] = None,
    window: int = 0,
    sinks: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Attention of new tokens vs full cached KV (causal within the new chunk).

    `window` W > 0: a query at position i sees keys i - W < j <= i (0: all
    keys <= i). `sinks`: f32 [Hq], one extra softmax logit per head that adds
    to the denominator only (torch_ref.paged_attention states both). On the
    GPU either one routes prefill tiles to the reference kernel, so the tile
    lists must have 32 rows, and decode rows to the MFMA kernel.

    `num_decodes_tail`: trailing sequences that are single-token decodes (the
    GPU path routes them to the decode kernel). `tile_seq`/`tile_q0`: int32
    device arrays mapping prefill q-tiles of `tile_rows` rows (32, 64 or 128)
    to (seq, local row). `prefill_variant`: "v1" (reference kernel, 32-row
    tiles only) or "pipe"; None picks by the routing above: tiles of more
    than 32 rows need the pipelined kernel, 32-row tiles run it where the
    rule (or the env switch) routes this head layout to it."""
    if _use_hip(q):
        out = torch.empty_like(q)
        if tile_seq is None:
            tile_seq = torch.empty(0, dtype=torch.int32, device=q.device)
            tile_q0 = tile_seq
        if window < 0:
            raise ValueError(f"window must be >= 0, got {window}")
        if window > 0 or sinks is not None:
            _require_hip().paged_attention(
                out, q, k_cache, v_cache, block_tables, seq_lens,
                query_start_locs, scale, num_decodes_tail, tile_seq, tile_q0,
                prefill_token_count, tile_rows, 0, window, sinks)
            return out
        if prefill_variant is None:
            pipe = (tile_rows != 32 or prefill_tile_rows(
                q.shape[1], k_cache.shape[1], q.shape[2]) is not None)
        elif prefill_variant in ("v1", "pipe"):
            pipe = prefill_variant == "pipe"
        else:
            raise ValueError(f"bad prefill_variant {prefill_variant!r}")
        _require_hip().paged_attention(out, q, k_cache, v_cache, block_tables,
                                       seq_lens, query_start_locs, scale,
                                       num_decodes_tail, tile_seq, tile_q0,
                                       prefill_token_count, tile_rows,
                                       1 if pipe else 0)
        return out
    return torch_ref.paged_attention(q, k_cache, v_cache, block_tables,
                                     seq_lens, query_start_locs, scale,
                                     window=window, sinks=sinks)


PREFIX_CB = 4  # column blocks per wave of attn_prefix_partial_kernel


def prefix_tile_rows(num_heads: int, num_kv_heads: int) -> int:
    """Rows per shared-prefix tile: the GQA group is padded to Gp in
    {1,2,4,8} and a wave owns PREFIX_CB blocks of 16/Gp rows."""
    g = num_heads // num_kv_heads
    gp = 1
    while gp < g:
        gp *= 2
    return PREFIX_CB * 16 // gp


def shared_decode_supported(head_dim: int, num_heads: int, num_kv_heads: int,
                            block_size: int = 32) -> bool:
    """Where the MFMA decode route (and so the shared-prefix kernel) runs."""
    return (head_dim in (64, 128) and block_size == 32
            and num_heads % num_kv_heads == 0
            and num_heads // num_kv_heads <= 8)


def alloc_prefix_partials(n: int, num_heads: int, head_dim: int, device):
    """f32 scratch the partial kernel hands to the per-row kernel:
    (part_o [n, Hq, D] unnormalised, part_m [n, Hq], part_l [n, Hq])."""
    return (torch.empty((n, num_heads, head_dim), dtype=torch.float32, device=device),
            torch.empty((n, num_heads), dtype=torch.float32, device=device),
            torch.empty((n, num_heads), dtype=torch.float32, device=device))


def _check_shared_args(block_tables, seq_lens, row_prefix_pages, tile_rows,
                       n: int, block_size: int) -> None:
    """Host-side check of the caller's guarantees (eager mode only: it reads
    the index tensors back)."""
    bt = block_tables.cpu()
    sl = seq_lens.cpu()
    rp = row_prefix_pages.cpu()
    tr = tile_rows.cpu()
    assert int(rp[:n].min()) >= 0 and int(rp[:n].max()) <= bt.shape[1]
    assert bool((sl[:n] > rp[:n] * block_size).all()), \
        "every row needs a position beyond its shared prefix"
    seen = set()
    for t in range(tr.shape[0]):
        rows = [int(r) for r in tr[t] if int(r) >= 0]
        if not rows:
            continue
        assert all(r < n for r in rows), "tile row out of range"
        p = int(rp[rows[0]])
        assert p > 0, "tile rows need row_prefix_pages > 0"
        for r in rows:
            assert r not in seen, "row listed in two tiles"
            seen.add(r)
            assert int(rp[r]) == p and torch.equal(bt[r, :p], bt[rows[0], :p]), \
                "rows of a tile must share their leading pages"
    for r in range(n):
        assert r in seen or int(rp[r]) == 0, \
            "a row in no tile must have row_prefix_pages = 0"


def paged_attention_decode_shared(
    q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
    block_tables: torch.Tensor, seq_lens: torch.Tensor, scale: float,
    row_prefix_pages: torch.Tensor, tile_rows: torch.Tensor,
    partials=None, validate: Optional[bool] = None,
) -> torch.Tensor:
    """Decode-only paged attention (one query token per row) that walks the
    KV pages a tile of rows has in common once per tile.

    `row_prefix_pages` int32 [n]: leading pages of row i covered by its tile
    (0 = none). `tile_rows` int32 [NT, prefix_tile_rows(Hq, Hk)]: row indices,
    -1 = empty slot. The caller guarantees that the rows of a tile have the
    same row_prefix_pages = P > 0 and identical first P table entries, that
    rows in no tile have P = 0, and that every row has a position beyond its
    prefix. The result is plain paged attention over the full tables —
    bit-identical to `paged_attention` on the GPU."""
    n = q.shape[0]
    if _use_hip(q):
        C = _require_hip()
        if validate is None:
            validate = not torch.cuda.is_current_stream_capturing()
        if validate:
            _check_shared_args(block_tables, seq_lens, row_prefix_pages,
                               tile_rows, n, k_cache.shape[2])
        if partials is None:
            partials = alloc_prefix_partials(n, q.shape[1], q.shape[2], q.device)
        out = torch.empty_like(q)
        C.paged_attention_decode_shared(out, q, k_cache, v_cache, block_tables,
                                        seq_lens, scale, row_prefix_pages,
                                        tile_rows, *partials)
        return out
    if validate is None or validate:
        _check_shared_args(block_tables, seq_lens, row_prefix_pages, tile_rows,
                           n, k_cache.shape[2])
    qlocs = torch.arange(n + 1, dtype=torch.int32, device=q.device)
    return torch_ref.paged_attention(q, k_cache, v_cache, block_tables[:n],
                                     seq_lens[:n], qlocs, scale)


def mean_pool_normalize(hidden: torch.Tensor, query_start_locs: torch.Tensor) -> torch.Tensor:
    if _use_hip(hidden):
        S = query_start_locs.numel() - 1
        out = torch.empty((S, hidden.shape[-1]), dtype=torch.float32, device=hidden.device)
        _require_hip().mean_pool_normalize(out, hidden, query_start_locs)
        return out
    return torch_ref.mean_pool_normalize(hidden, query_start_locs)


def sampler_fused(logits, temps, top_ps, top_ks, u, packed_mask, vocab_limit,
                  out_tok, out_lp):
    """Fused mask+temperature+top-k/top-p+sample+logprob (csrc/sampler.hip).
    GPU-only: logits must be CUDA; raises if the extension is missing."""
    _require_hip().sampler_fused(logits, temps, top_ps, top_ks, u,
                                 packed_mask, vocab_limit, out_tok, out_lp)


def grouped_gemm(out, a, w, row_tok, tile_off, counts, max_tiles, gate_silu,
                 bm=64):
    """Dropless-MoE grouped GEMM: csrc/grouped_gemm.hip on GPU, torch
    reference on CPU (same padded-segment layout). bm = segment tile height
    (64 for small batches, 128 for large — host pads with the same value)."""
    if _use_hip(a):
        _require_hip().grouped_gemm(out, a, w, row_tok, tile_off, counts,
                                    max_tiles, gate_silu, bm)
        return out
    return torch_ref.grouped_gemm(out, a, w, row_tok, tile_off, counts,
                                  max_tiles, gate_silu, bm)


def quantize_rows_fp8(x, out_q, out_scale, row_limit=None, limit_mul=1):
    """x [R, K] -> e4m3 codes out_q [R, Kp] + f32 per-row scale out_scale [R]
    (scale = amax/448, Kp = K rounded up to 128 with a zero tail):
    csrc/grouped_gemm_fp8.hip on GPU (bf16 input), torch reference on CPU —
    bit-identical. row_limit (int32 device scalar) * limit_mul optionally
    bounds the rows written, without a host sync on GPU."""
    if _use_hip(x):
        _require_hip().quant_rows_fp8(x, out_q, out_scale, row_limit,
                                      limit_mul)
        return out_q, out_scale
    return torch_ref.quantize_rows_fp8(x, out_q, out_scale, row_limit,
                                       limit_mul)


def grouped_gemm_fp8(out, a_q, a_scale, w_q, w_scale, row_tok, tile_off,
                     counts, max_tiles, gate_silu, bm=64):
    """`grouped_gemm` with e4m3 operands: a_q [., Kp] + f32 row scales
    (stage 1: indexed through row_tok), w_q [E, N, Kp] + f32 per-output-
    channel scales [E, N], bf16 out. Block-scaled MFMA kernel
    (csrc/grouped_gemm_fp8.hip) on GPU, emulated arithmetic on CPU."""
    if _use_hip(a_q):
        _require_hip().grouped_gemm_fp8(out, a_q, a_scale, w_q, w_scale,
                                        row_tok, tile_off, counts, max_tiles,
                                        gate_silu, bm)
        return out
    return torch_ref.grouped_gemm_fp8(out, a_q, a_scale, w_q, w_scale,
                                      row_tok, tile_off, counts, max_tiles,
                                      gate_silu, bm)


def linear_fp8_qualifies(n: int, k: int) -> bool:
    """Weight shapes [n, k] the FP8 dense kernel takes (plain / residual
    epilogue): N % 64 == 0; K % 8 == 0 is the row quantiser's 16-byte load."""
    return n >= 64 and n % 64 == 0 and k >= 8 and k % 8 == 0


def gate_up_silu_fp8_qualifies(two_i: int, k: int) -> bool:
    """Merged gate_up shapes [2I, k] the FP8 SwiGLU epilogue takes:
    I % 128 == 0."""
    return two_i >= 256 and two_i % 256 == 0 and k >= 8 and k % 8 == 0


def linear_fp8(x, w_q, w_scale, residual=None):
    """Dense W8A8 projection: x [T, K] (bf16 on GPU) through w_q [N, Kp] e4m3
    with f32 per-output-channel scales w_scale [N]; returns [T, N] in x's
    dtype, optionally + residual (added in f32 before the one rounding).
    Arithmetic: torch_ref.linear_fp8. On GPU the row quantiser runs as its
    own pass, then csrc/gemm_tn_fp8_pipe.hip; no host sync, every tensor from
    the caching allocator."""
    if _use_hip(x):
        C = _require_hip()
        # fresh caching-allocator tensors: safe under hipGraph capture
        x_q, x_s = torch_ref.quantize_act_fp8(x, quantize_rows_fp8)
        return C.gemm_fp8_pipelined(x_q, x_s, w_q, w_scale, residual)
    return torch_ref.linear_fp8(x, w_q, w_scale, residual)


def gate_up_silu_fp8(x, w_q, w_scale):
    """SwiGLU of the merged W8A8 gate_up projection (w_q [2I, Kp], gate rows
    first): one kernel, f32 SwiGLU on the scaled products, one rounding.
    Arithmetic: torch_ref.gate_up_silu_fp8."""
    if _use_hip(x):
        C = _require_hip()
        # fresh caching-allocator tensors: safe under hipGraph capture
        x_q, x_s = torch_ref.quantize_act_fp8(x, quantize_rows_fp8)
        return C.gemm_fp8_gate_up_silu(x_q, x_s, w_q, w_scale)
    return torch_ref.gate_up_silu_fp8(x, w_q, w_scale)


def linear_fp8_block128_qualifies(n: int, k: int) -> bool:
    """Weight shapes [n, k] the block-scaled FP8 dense kernel takes (plain /
    residual epilogue): whole 128x128 scale blocks."""
    return n >= 128 and n % 128 == 0 and k >= 128 and k % 128 == 0


def gate_up_silu_fp8_block128_qualifies(two_i: int, k: int) -> bool:
    """Merged gate_up shapes [2I, k] the block-scaled SwiGLU epilogue takes:
    I % 128 == 0 (gate and up rows never share a scale block)."""
    return two_i >= 256 and two_i % 256 == 0 and k >= 128 and k % 128 == 0


def quantize_rows_fp8_block128(x):
    """x [R, K], K % 128 == 0 -> (e4m3 codes [R, K], f32 scales [K/128, R]):
    one scale = amax/448 per row and group of 128 K elements, K-block-major.
    csrc/gemm_tn_fp8_block_pipe.hip on GPU (bf16 input), torch reference on
    CPU — bit-identical. Fresh tensors, no host sync."""
    if _use_hip(x):
        q, s = _require_hip().quant_rows_fp8_block128(x.contiguous())
        return q, s
    return torch_ref.quantize_rows_fp8_block128(x)


def linear_fp8_block128(x, w_q, w_s, residual=None):
    """Block-scaled dense projection: x [T, K] (bf16 on GPU) through w_q
    [N, K] e4m3 with one f32 scale per 128x128 block, w_s [N/128, K/128]
    (`weight`, `weight_scale_inv` of the published block-FP8 checkpoints);
    returns [T, N] in x's dtype, optionally + residual (added in f32 before
    the one rounding). Arithmetic: torch_ref.linear_fp8_block128. On GPU the
    group quantiser runs as its own pass, then
    csrc/gemm_tn_fp8_block_pipe.hip; no host sync, every tensor from the
    caching allocator."""
    if _use_hip(x):
        C = _require_hip()
        # fresh caching-allocator tensors: safe under hipGraph capture
        x_q, x_s = C.quant_rows_fp8_block128(x.contiguous())
        return C.gemm_fp8_block_pipelined(x_q, x_s, w_q, w_s, residual)
    return torch_ref.linear_fp8_block128(x, w_q, w_s, residual)


def gate_up_silu_fp8_block128(x, w_q, w_s):
    """SwiGLU of the merged block-scaled gate_up projection (w_q [2I, K], gate
    rows first, w_s [2I/128, K/128]): one kernel, f32 SwiGLU on the unrounded
    products, one rounding. Arithmetic: torch_ref.gate_up_silu_fp8_block128."""
    if _use_hip(x):
        C = _require_hip()
        # fresh caching-allocator tensors: safe under hipGraph capture
        x_q, x_s = C.quant_rows_fp8_block128(x.contiguous())
        return C.gemm_fp8_block_gate_up_silu(x_q, x_s, w_q, w_s)
    return torch_ref.gate_up_silu_fp8_block128(x, w_q, w_s)


def quantize_weight_mxfp4(w):
    """w [..., K] -> MXFP4 (e2m1 code pairs uint8 [..., Kp/2], e8m0 block
    scales uint8 [..., Kp/32]); the format and rule are stated in
    torch_ref.quantize_weight_mxfp4. csrc/grouped_gemm_mxfp4.hip on GPU (bf16
    input), torch reference on CPU — bit-identical."""
    if _use_hip(w):
        *lead, K = w.shape
        Kp = torch_ref.fp8_padded_k(K)
        w2 = w.contiguous().view(-1, K)
        codes = torch.empty(w2.shape[0], Kp // 2, dtype=torch.uint8,
                            device=w.device)
        scales = torch.empty(w2.shape[0], Kp // 32, dtype=torch.uint8,
                             device=w.device)
        _require_hip().quant_weight_mxfp4(w2, codes, scales)
        return codes.view(*lead, Kp // 2), scales.view(*lead, Kp // 32)
    return torch_ref.quantize_weight_mxfp4(w)


def grouped_gemm_mxfp4(out, a_q, a_scale, codes, scales, row_tok, tile_off,
                       counts, max_tiles, gate_silu, bm=64):
    """`grouped_gemm_fp8` with MXFP4 weights (W4A8): a_q [., Kp] e4m3 + f32
    row scales, codes [E, N, Kp/2] + e8m0 block scales [E, N, Kp/32], bf16
    out. Block-scaled MFMA kernel (csrc/grouped_gemm_mxfp4.hip) on GPU,
    emulated arithmetic on CPU."""
    if _use_hip(a_q):
        _require_hip().grouped_gemm_mxfp4(out, a_q, a_scale, codes, scales,
                                          row_tok, tile_off, counts,
                                          max_tiles, gate_silu, bm)
        return out
    return torch_ref.grouped_gemm_mxfp4(out, a_q, a_scale, codes, scales,
                                        row_tok, tile_off, counts, max_tiles,
                                        gate_silu, bm)


def moe_combine(out, rows, padpos, w):
    """out[t] = sum_j w[t,j] * rows[padpos[t,j]]: fused bf16 gather-combine
    (csrc/grouped_gemm.hip) on GPU, deterministic torch gather on CPU."""
    if _use_hip(rows):
        _require_hip().moe_combine(out, rows, padpos, w)
        return out
    contrib = rows[padpos].float()          # [T, k, h]
    out.copy_((contrib * w.unsqueeze(-1)).sum(dim=1).to(out.dtype))
    return out


# largest hist_len + bias width one LDS table (16384 entries, half full) holds
PENALTY_MAX_ENTRIES = 8192


def apply_logit_penalties(logits, row_idx, hist, slot, hist_len, prompt_len,
                          rep, pres, freq, bias_tok=None, bias_val=None,
                          vocab_limit: Optional[int] = None,
                          max_hist_len: Optional[int] = None):
    """In-place repetition/presence/frequency penalties + logit_bias on the
    rows of `logits` [n, V] listed in `row_idx` (unique; m of them). All
    tensors live on the logits' device: hist int32 [S, Lcap], slot/hist_len/
    prompt_len int32 [m], rep/pres/freq f32 [m], bias_tok int32 [m, B] (-1
    padded) + bias_val f32 [m, B] or None. Semantics: torch_ref.
    apply_logit_penalties; csrc/logit_penalties.hip matches it bit for bit.

    `max_hist_len` is the caller's host-side bound on hist_len (the engine
    knows it; it sizes the LDS table). Left None it is read back from the
    device, which synchronizes. Calls whose hist_len + B exceed one table
    (> 8192, beyond the default max_model_len) run the torch reference on
    the device instead."""
    m = int(row_idx.numel())
    if m == 0:
        return logits
    vl = logits.shape[1] if vocab_limit is None else min(int(vocab_limit),
                                                         logits.shape[1])
    if _use_hip(logits):
        if max_hist_len is None:
            max_hist_len = int(hist_len.max())
        n_bias = 0 if bias_tok is None else int(bias_tok.shape[1])
        if max_hist_len + n_bias <= PENALTY_MAX_ENTRIES:
            _require_hip().logit_penalties(
                logits, row_idx, hist, slot, hist_len, prompt_len, rep, pres,
                freq, bias_tok, bias_val, vl, int(max_hist_len))
            return logits
    return torch_ref.apply_logit_penalties(
        logits, row_idx, hist, slot, hist_len, prompt_len, rep, pres, freq,
        bias_tok, bias_val, vl)
