"""Pure-PyTorch reference implementations of every engine op.

These are the CPU execution path AND the numerics oracle for the CDNA4 HIP
kernels (GPU tests compare the HIP kernels against these in fp32).
All reductions accumulate in fp32.
"""

from __future__ import annotations

import torch


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    var = xf.pow(2).mean(dim=-1, keepdim=True)
    y = xf * torch.rsqrt(var + eps)
    return (y * weight.float()).to(x.dtype)


def fused_add_rmsnorm(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float
):
    """residual += x; return (rmsnorm(residual), residual)."""
    res = (residual.float() + x.float())
    y = rmsnorm(res, weight, eps)
    return y, res.to(x.dtype)


def silu_mul(x: torch.Tensor) -> torch.Tensor:
    gate, up = x.chunk(2, dim=-1)
    return (torch.nn.functional.silu(gate.float()) * up.float()).to(x.dtype)


def rope_cos_sin(max_len: int, head_dim: int, theta: float) -> torch.Tensor:
    """[max_len, head_dim] fp32 table: first half cos, second half sin (NeoX)."""
    half = head_dim // 2
    inv_freq = 1.0 / (theta ** (torch.arange(half, dtype=torch.float64) / half))
    t = torch.arange(max_len, dtype=torch.float64)
    freqs = torch.outer(t, inv_freq)
    return torch.cat([freqs.cos(), freqs.sin()], dim=-1).float()


def apply_rope(q: torch.Tensor, k: torch.Tensor, positions: torch.Tensor,
               cos_sin: torch.Tensor):
    """NeoX rotate-half RoPE. q: [T, Hq, D], k: [T, Hk, D], positions: [T]."""
    d = q.shape[-1]
    half = d // 2
    cs = cos_sin[positions]              # [T, D]
    cos = cs[:, :half].unsqueeze(1)      # [T, 1, half]
    sin = cs[:, half:].unsqueeze(1)

    def rot(x: torch.Tensor) -> torch.Tensor:
        xf = x.float()
        x1, x2 = xf[..., :half], xf[..., half:]
        return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1).to(x.dtype)

    return rot(q), rot(k)


def write_kv_cache(
    k: torch.Tensor, v: torch.Tensor,
    k_cache: torch.Tensor, v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,
) -> None:
    """k/v: [T, Hk, D]; caches: [num_blocks, Hk, block_size, D]; slots: [T]."""
    nb, hk, bs, d = k_cache.shape
    blk = slot_mapping // bs
    off = slot_mapping % bs
    k_cache[blk, :, off] = k.to(k_cache.dtype)
    v_cache[blk, :, off] = v.to(v_cache.dtype)


def paged_attention(
    q: torch.Tensor,                 # [T, Hq, D] (new tokens, flat over seqs)
    k_cache: torch.Tensor,           # [num_blocks, Hk, bs, D]
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,      # [S, max_blocks] int32
    seq_lens: torch.Tensor,          # [S] total length incl. this step's tokens
    query_start_locs: torch.Tensor,  # [S+1] cu-seqlens of new tokens
    scale: float,
    window: int = 0,
    sinks: torch.Tensor | None = None,
) -> torch.Tensor:
    """Causal attention of each seq's new tokens against its full cached KV.

    New tokens MUST already be written to the cache (write_kv_cache first).

    `window` W > 0 (local attention): the query at absolute position i sees
    key j iff i - W < j <= i, i.e. W keys including its own; 0 is no window.
    `sinks` (f32 [Hq]): head h's softmax runs over the visible scores plus
    one extra logit sinks[h] (score units, not multiplied by `scale`) that
    adds to the denominator and nothing to the output.
    """
    if window < 0:
        raise ValueError(f"window must be >= 0, got {window}")
    if sinks is not None and sinks.numel() != q.shape[1]:
        raise ValueError(f"sinks must have one entry per q head "
                         f"({q.shape[1]}), got {sinks.numel()}")
    T, hq, d = q.shape
    nb, hk, bs, _ = k_cache.shape
    group = hq // hk
    out = torch.empty_like(q)
    S = seq_lens.numel()
    for s in range(S):
        q0, q1 = int(query_start_locs[s]), int(query_start_locs[s + 1])
        nq = q1 - q0
        if nq == 0:
            continue
        L = int(seq_lens[s])
        nblk = (L + bs - 1) // bs
        blocks = block_tables[s, :nblk].long()
        keys = k_cache[blocks].transpose(0, 1).reshape(hk, nblk * bs, d)[:, :L].float()
        vals = v_cache[blocks].transpose(0, 1).reshape(hk, nblk * bs, d)[:, :L].float()
        qs = q[q0:q1].float()  # [nq, hq, d]
        # head-major: [hq, nq, d]
        qs = qs.transpose(0, 1)
        kh = keys.repeat_interleave(group, dim=0)   # [hq, L, d]
        vh = vals.repeat_interleave(group, dim=0)
        scores = torch.einsum("hqd,hkd->hqk", qs, kh) * scale
        # causal mask: new token i (absolute pos L-nq+i) sees keys <= its pos
        kpos = torch.arange(L, device=q.device)
        qpos = torch.arange(L - nq, L, device=q.device)
        mask = kpos.unsqueeze(0) > qpos.unsqueeze(1)  # [nq, L]
        if window > 0:
            mask = mask | (kpos.unsqueeze(0) <= qpos.unsqueeze(1) - window)
        scores.masked_fill_(mask.unsqueeze(0), float("-inf"))
        if sinks is not None:
            # the sink is one more logit column; its probability is dropped
            col = sinks.float().to(q.device).view(hq, 1, 1).expand(hq, nq, 1)
            probs = torch.softmax(torch.cat([scores, col], dim=-1),
                                  dim=-1)[..., :L]
        else:
            probs = torch.softmax(scores, dim=-1)
        o = torch.einsum("hqk,hkd->hqd", probs, vh)   # [hq, nq, d]
        out[q0:q1] = o.transpose(0, 1).to(out.dtype)
    return out


def mean_pool_normalize(
    hidden: torch.Tensor,            # [T, H] flat hidden states
    query_start_locs: torch.Tensor,  # [S+1]
) -> torch.Tensor:
    """Per-sequence mean pool over tokens + L2 normalize -> [S, H]."""
    S = query_start_locs.numel() - 1
    out = torch.empty((S, hidden.shape[-1]), dtype=torch.float32, device=hidden.device)
    for s in range(S):
        a, b = int(query_start_locs[s]), int(query_start_locs[s + 1])
        m = hidden[a:b].float().mean(dim=0)
        out[s] = m / (m.norm() + 1e-12)
    return out


def topk_softmax_router(
    logits: torch.Tensor, top_k: int
):
    """MoE router: softmax over experts then top-k, renormalized.
    Returns (weights [T,k] fp32, indices [T,k] int64)."""
    probs = torch.softmax(logits.float(), dim=-1)
    w, idx = probs.topk(top_k, dim=-1)
    w = w / w.sum(dim=-1, keepdim=True)
    return w, idx


def grouped_gemm(out, a, w, row_tok, tile_off, counts, max_tiles, gate_silu,
                 bm: int = 64):
    """Reference for csrc/grouped_gemm.hip: per-expert segments padded to the
    bm tile; gate_silu fuses silu(gate)*up over the two N-halves of w.
    Padding rows of `out` are left untouched (the kernel writes deterministic
    garbage there; consumers must ignore them either way)."""
    E, N, K = w.shape
    n_cols = N // 2 if gate_silu else N
    for e in range(E):
        c = int(counts[e])
        if c == 0:
            continue
        s0 = int(tile_off[e]) * bm
        if row_tok is not None:
            toks = row_tok[s0:s0 + c].long().clamp(min=0)
            rows = a[toks].float()
        else:
            rows = a[s0:s0 + c].float()
        if gate_silu:
            g = rows @ w[e, :n_cols].T.float()
            u = rows @ w[e, n_cols:].T.float()
            out[s0:s0 + c] = (torch.nn.functional.silu(g) * u).to(out.dtype)
        else:
            out[s0:s0 + c] = (rows @ w[e].T.float()).to(out.dtype)
    return out


FP8_E4M3_MAX = 448.0


def fp8_padded_k(K: int) -> int:
    """K rounded up to the 128-element K-tile of csrc/grouped_gemm_fp8.hip."""
    return (K + 127) // 128 * 128


def quantize_rows_fp8(x, out_q, out_scale, row_limit=None, limit_mul: int = 1):
    """Reference for quant_rows_fp8 (csrc/grouped_gemm_fp8.hip) and the CPU
    path: x [R, K] -> OCP e4m3 codes out_q [R, Kp] + f32 scale out_scale [R].

        amax  = max_k |f32(x[r, k])|
        scale = amax / 448            (true f32 division; 1 when amax == 0)
        code  = e4m3_rne(clamp(f32(x) / scale, -448, 448))   (true division)

    The tail [K, Kp) is zero bytes. Both divisions are tensor / tensor so
    torch never substitutes a reciprocal multiply; the kernel follows the
    same sequence and agrees bit for bit. Rows >= row_limit[0] * limit_mul
    are left untouched when row_limit (an int tensor) is given."""
    R, K = x.shape
    if row_limit is not None:
        R = min(R, int(row_limit.reshape(-1)[0]) * limit_mul)
    xf = x[:R].float()
    amax = xf.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / torch.full_like(amax, FP8_E4M3_MAX),
                        torch.ones_like(amax))
    q = (xf / scale.unsqueeze(1)).clamp(-FP8_E4M3_MAX, FP8_E4M3_MAX)
    qb = out_q.view(torch.uint8)
    qb[:R, :K] = q.to(torch.float8_e4m3fn).view(torch.uint8)
    qb[:R, K:] = 0
    out_scale[:R] = scale
    return out_q, out_scale


def quantize_weight_fp8(w):
    """w [E, N, K] -> (w_q [E, N, Kp] e4m3, scale [E, N] f32): one scale per
    output channel, K zero-padded to the kernel's 128-element K-tile."""
    E, N, K = w.shape
    Kp = fp8_padded_k(K)
    w_q = torch.empty(E, N, Kp, dtype=torch.float8_e4m3fn, device=w.device)
    scale = torch.empty(E, N, dtype=torch.float32, device=w.device)
    quantize_rows_fp8(w.reshape(E * N, K), w_q.view(E * N, Kp), scale.view(-1))
    return w_q, scale


def fp8_linear(a_q, a_scale, w_q, w_scale):
    """Emulated e4m3 GEMM: (a_q @ w_q^T in fp32) * a_scale[:, None]
    * w_scale[None, :] -> fp32 [rows, N]. Scales are applied after the sum,
    in the kernel epilogue's order."""
    acc = a_q.float() @ w_q.float().T
    return acc * a_scale.unsqueeze(1) * w_scale.unsqueeze(0)


def quantize_act_fp8(x, quantize_rows=None):
    """x [T, K] -> (e4m3 codes [T, Kp], f32 row scales [T]) in fresh tensors,
    through `quantize_rows` (default: `quantize_rows_fp8` above; the op layer
    passes its dispatching one, so the GPU path shares this helper)."""
    T, K = x.shape
    x_q = torch.empty(T, fp8_padded_k(K), dtype=torch.float8_e4m3fn,
                      device=x.device)
    x_s = torch.empty(T, dtype=torch.float32, device=x.device)
    return (quantize_rows or quantize_rows_fp8)(x.contiguous(), x_q, x_s)


def linear_fp8(x, w_q, w_scale, residual=None):
    """THE statement of the dense W8A8 projection (csrc/gemm_tn_fp8_pipe.hip):
    x [T, K] -> out [T, N] in x's dtype, for w_q [N, Kp] e4m3 + w_scale [N]
    f32 (one scale per output channel, `quantize_weight_fp8` of the local
    shard):

        x_q, x_s = quantize_rows_fp8(x)              (per-row, amax / 448)
        y        = fp8_linear(x_q, x_s, w_q, w_scale)   (f32)
        y        = y + f32(residual)                  (when given)
        out      = y rounded once to x's dtype"""
    x_q, x_s = quantize_act_fp8(x)
    y = fp8_linear(x_q, x_s, w_q, w_scale)
    if residual is not None:
        y = y + residual.float()
    return y.to(x.dtype)


def gate_up_silu_fp8(x, w_q, w_scale):
    """SwiGLU of the merged W8A8 gate_up projection: w_q [2I, Kp] (gate rows
    first) + w_scale [2I]; returns [T, I] in x's dtype.

        y   = fp8_linear(quantize_rows_fp8(x), w_q, w_scale)    (f32 [T, 2I])
        out = silu(y[:, :I]) * y[:, I:] in f32, rounded once

    Unlike the bf16 gate_up path, the two products are NOT rounded before the
    activation (the grouped FP8 kernel's epilogue)."""
    x_q, x_s = quantize_act_fp8(x)
    y = fp8_linear(x_q, x_s, w_q, w_scale)
    inter = w_q.shape[0] // 2
    return (torch.nn.functional.silu(y[:, :inter]) * y[:, inter:]).to(x.dtype)


FP8_BLOCK = 128


def _quantize_groups_fp8(xf, amax):
    """The rule shared by both block quantisers: xf f32 and amax f32 (the
    group maximum, broadcastable to xf) -> (e4m3 codes, scale), with
    scale = amax / 448 by true division (1 when amax == 0) and
    code = e4m3_rne(clamp(xf / scale, -448, 448)) by true division."""
    scale = torch.where(amax > 0, amax / torch.full_like(amax, FP8_E4M3_MAX),
                        torch.ones_like(amax))
    q = (xf / scale).clamp(-FP8_E4M3_MAX, FP8_E4M3_MAX)
    return q.to(torch.float8_e4m3fn), scale


def quantize_rows_fp8_block128(x):
    """Reference for quant_rows_fp8_block128
    (csrc/gemm_tn_fp8_block_pipe.hip) and the CPU path: x [R, K], K % 128 ==
    0 -> (codes [R, K] e4m3, scales [K/128, R] f32). Every group of 128
    consecutive K elements of a row follows the rule of `quantize_rows_fp8`:

        amax  = max over the group of |f32(x[r, k])|
        scale = amax / 448            (true f32 division; 1 when amax == 0)
        code  = e4m3_rne(clamp(f32(x) / scale, -448, 448))   (true division)

    The scales are K-block-major, scales[kb, r]: the four accumulator rows of
    a GEMM lane are then 16 contiguous bytes. The kernel follows the same
    sequence and agrees bit for bit."""
    R, K = x.shape
    if K < FP8_BLOCK or K % FP8_BLOCK:
        raise ValueError(f"K must be a positive multiple of 128 (K={K})")
    xf = x.float().view(R, K // FP8_BLOCK, FP8_BLOCK)
    q, scale = _quantize_groups_fp8(xf, xf.abs().amax(dim=2, keepdim=True))
    return q.view(R, K), scale.view(R, K // FP8_BLOCK).t().contiguous()


def quantize_weight_fp8_block128(w):
    """w [N, K], N % 128 == 0 and K % 128 == 0 -> (codes [N, K] e4m3,
    scale_inv [N/128, K/128] f32): one scale per 128x128 block by the rule of
    `quantize_rows_fp8_block128` with amax taken over the block. This is the
    layout of the published block-FP8 checkpoints (`weight`,
    `weight_scale_inv`): dequantised weight = code * scale_inv[n // 128,
    k // 128]. Runs once at start-up, in plain torch on w's device."""
    N, K = w.shape
    if N < FP8_BLOCK or N % FP8_BLOCK or K < FP8_BLOCK or K % FP8_BLOCK:
        raise ValueError(
            f"N and K must be positive multiples of 128 (N={N}, K={K})")
    nb, kb = N // FP8_BLOCK, K // FP8_BLOCK
    wf = w.float().view(nb, FP8_BLOCK, kb, FP8_BLOCK)
    q, scale = _quantize_groups_fp8(wf, wf.abs().amax(dim=(1, 3),
                                                      keepdim=True))
    return q.view(N, K), scale.view(nb, kb).contiguous()


def fp8_block_linear(a_q, a_s, w_q, w_s):
    """Emulated block-scaled e4m3 GEMM -> f32 [R, N]: a_q [R, K] with a_s
    [K/128, R], w_q [N, K] with w_s [N/128, K/128]. For kb ascending

        acc += (a_q[:, kb] @ w_q[:, kb].T in f32)
               * (a_s[kb, :, None] * w_s[None, n // 128, kb])

    where [:, kb] is the kb-th group of 128 K elements and the factor is one
    f32 product. The kernel (csrc/gemm_tn_fp8_block_pipe.hip) may contract
    the multiply-add into an fma."""
    R, K = a_q.shape
    N = w_q.shape[0]
    af, wf = a_q.float(), w_q.float()
    acc = torch.zeros(R, N, dtype=torch.float32, device=a_q.device)
    for kb in range(K // FP8_BLOCK):
        ks = slice(kb * FP8_BLOCK, (kb + 1) * FP8_BLOCK)
        p = af[:, ks] @ wf[:, ks].T
        ws = w_s[:, kb].repeat_interleave(FP8_BLOCK)
        acc += p * (a_s[kb].unsqueeze(1) * ws.unsqueeze(0))
    return acc


def linear_fp8_block128(x, w_q, w_s, residual=None):
    """THE statement of the block-scaled dense projection
    (csrc/gemm_tn_fp8_block_pipe.hip): x [T, K] -> out [T, N] in x's dtype,
    for w_q [N, K] e4m3 + w_s [N/128, K/128] f32 (`weight`,
    `weight_scale_inv`):

        x_q, x_s = quantize_rows_fp8_block128(x)     (per row and K group)
        y        = fp8_block_linear(x_q, x_s, w_q, w_s)   (f32)
        y        = y + f32(residual)                  (when given)
        out      = y rounded once to x's dtype"""
    x_q, x_s = quantize_rows_fp8_block128(x)
    y = fp8_block_linear(x_q, x_s, w_q, w_s)
    if residual is not None:
        y = y + residual.float()
    return y.to(x.dtype)


def gate_up_silu_fp8_block128(x, w_q, w_s):
    """SwiGLU of the merged block-scaled gate_up projection: w_q [2I, K]
    (gate rows first) + w_s [2I/128, K/128], I % 128 == 0; returns [T, I] in
    x's dtype.

        y   = fp8_block_linear(quantize_rows_fp8_block128(x), w_q, w_s)
        out = silu(y[:, :I]) * y[:, I:] in f32, rounded once

    As in `gate_up_silu_fp8`, the two products are not rounded before the
    activation."""
    x_q, x_s = quantize_rows_fp8_block128(x)
    y = fp8_block_linear(x_q, x_s, w_q, w_s)
    inter = w_q.shape[0] // 2
    return (torch.nn.functional.silu(y[:, :inter]) * y[:, inter:]).to(x.dtype)


def grouped_gemm_fp8(out, a_q, a_scale, w_q, w_scale, row_tok, tile_off,
                     counts, max_tiles, gate_silu, bm: int = 64):
    """Reference for grouped_gemm_fp8 (csrc/grouped_gemm_fp8.hip) and the CPU
    path: the layout contract of `grouped_gemm` with the quantised arithmetic
    emulated — e4m3 codes, products and sums in fp32, scales after the sum,
    SwiGLU in fp32, then one rounding to out's dtype. Padding rows of `out`
    are left untouched."""
    E, N, _ = w_q.shape
    n_cols = N // 2 if gate_silu else N
    for e in range(E):
        c = int(counts[e])
        if c == 0:
            continue
        s0 = int(tile_off[e]) * bm
        if row_tok is not None:
            idx = row_tok[s0:s0 + c].long().clamp(min=0)
        else:
            idx = torch.arange(s0, s0 + c, device=a_q.device)
        # index the byte view: fp8 tensors have no gather kernels everywhere
        rows = a_q.view(torch.uint8)[idx].view(torch.float8_e4m3fn)
        y = fp8_linear(rows, a_scale[idx], w_q[e], w_scale[e])
        if gate_silu:
            y = torch.nn.functional.silu(y[:, :n_cols]) * y[:, n_cols:]
        out[s0:s0 + c] = y.to(out.dtype)
    return out


# the e2m1 grid, indexed by the 3 magnitude bits of a code (bit 3 = sign)
E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def quantize_weight_mxfp4(w):
    """THE statement of the MXFP4 weight format; quant_weight_mxfp4
    (csrc/grouped_gemm_mxfp4.hip), the GEMM kernel and the loader agree with
    it bit for bit. w [..., K] (finite) -> (codes uint8 [..., Kp/2],
    scales uint8 [..., Kp/32]), Kp = fp8_padded_k(K).

    Codes are OCP e2m1 (sign bit 3, magnitude bits index the grid
    {0, .5, 1, 1.5, 2, 3, 4, 6}), two per byte: element 2i in the low nibble
    of byte i. Scales are e8m0, value 2^(b-127); one covers 32 consecutive K
    elements. Rule (OCP MX v1.0), per 32-block, elements past K counting 0:

        amax = max |f32(w)|
        b    = clamp(floor(log2(amax)) - 2 + 127, 0, 254)   (127 if amax == 0)
        code = e2m1_rne(clamp(f32(w) / 2^(b-127), -6, 6))

    floor(log2(amax)) is read off the f32 exponent field (subnormal amax
    clamps to b = 0 either way); the division is the exact multiplication by
    2^(127-b); rounding is to nearest with ties to the even code (0.25 -> 0,
    0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); a value
    that rounds to zero gets code 0, never the negative zero 8. It follows
    that codes in [K, Kp) are 0 and that blocks wholly inside the padding
    tail (and all-zero blocks) hold b = 127 = 0x7f. There is no other weight
    scale."""
    *lead, K = w.shape
    Kp = fp8_padded_k(K)
    wf = torch.zeros(*lead, Kp, dtype=torch.float32, device=w.device)
    wf[..., :K] = w.float()
    blk = wf.view(*lead, Kp // 32, 32)
    amax = blk.abs().amax(dim=-1)
    ef = (amax.view(torch.int32) >> 23) & 0xff
    b = torch.where(amax > 0, (ef - 2).clamp(min=0), torch.full_like(ef, 127))
    inv = ((254 - b) << 23).view(torch.float32)            # 2^(127-b), exact
    x = (blk * inv.unsqueeze(-1)).clamp(-6.0, 6.0)
    m = x.abs()
    mag = ((m > 0.25).to(torch.uint8) + (m >= 0.75).to(torch.uint8)
           + (m > 1.25).to(torch.uint8) + (m >= 1.75).to(torch.uint8)
           + (m > 2.5).to(torch.uint8) + (m >= 3.5).to(torch.uint8)
           + (m > 5.0).to(torch.uint8))
    code = mag | (((x < 0) & (mag != 0)).to(torch.uint8) << 3)
    code = code.view(*lead, Kp // 2, 2)
    codes = code[..., 0] | (code[..., 1] << 4)
    return codes.contiguous(), b.to(torch.uint8).contiguous()


def dequantize_mxfp4(codes, scales):
    """(codes [..., Kp/2], scales [..., Kp/32]) -> f32 [..., Kp], exact: a
    grid value times a power of two."""
    *lead, kb = codes.shape
    grid = torch.tensor(E2M1_GRID + tuple(-v for v in E2M1_GRID),
                        dtype=torch.float32, device=codes.device)
    nib = torch.stack((codes & 0xf, codes >> 4), dim=-1).view(*lead, kb * 2)
    val = grid[nib.long()]
    # 2^(b-127) from the exponent field; b = 0 is the f32 subnormal 2^-127
    b = scales.to(torch.int32)
    sc = torch.where(b > 0, b << 23, torch.full_like(b, 0x00400000))
    sc = sc.view(torch.float32)
    return (val.view(*lead, kb // 16, 32) * sc.unsqueeze(-1)).view(
        *lead, kb * 2)


def mxfp4_linear(a_q, a_scale, codes, scales):
    """Emulated e4m3 x MXFP4 GEMM: (a_q @ dequant(W)^T in fp32)
    * a_scale[:, None] -> fp32 [rows, N]. The block scales act inside the sum
    (as in the MFMA), the row scale after it (the kernel epilogue)."""
    acc = a_q.float() @ dequantize_mxfp4(codes, scales).T
    return acc * a_scale.unsqueeze(1)


def grouped_gemm_mxfp4(out, a_q, a_scale, codes, scales, row_tok, tile_off,
                       counts, max_tiles, gate_silu, bm: int = 64):
    """Reference for grouped_gemm_mxfp4 (csrc/grouped_gemm_mxfp4.hip) and the
    CPU path: the layout contract of `grouped_gemm_fp8` with MXFP4 weights —
    e4m3 activation codes times exactly dequantised weights, products and
    sums in fp32, the row scale after the sum, SwiGLU in fp32, then one
    rounding to out's dtype. Padding rows of `out` are left untouched."""
    E, N, _ = codes.shape
    n_cols = N // 2 if gate_silu else N
    for e in range(E):
        c = int(counts[e])
        if c == 0:
            continue
        s0 = int(tile_off[e]) * bm
        if row_tok is not None:
            idx = row_tok[s0:s0 + c].long().clamp(min=0)
        else:
            idx = torch.arange(s0, s0 + c, device=a_q.device)
        rows = a_q.view(torch.uint8)[idx].view(torch.float8_e4m3fn)
        y = mxfp4_linear(rows, a_scale[idx], codes[e], scales[e])
        if gate_silu:
            y = torch.nn.functional.silu(y[:, :n_cols]) * y[:, n_cols:]
        out[s0:s0 + c] = y.to(out.dtype)
    return out


def apply_logit_penalties(logits, row_idx, hist, slot, hist_len, prompt_len,
                          rep, pres, freq, bias_tok, bias_val,
                          vocab_limit: int):
    """Reference for csrc/logit_penalties.hip (and the CPU path): in-place
    repetition / presence / frequency penalties + logit_bias on the rows in
    `row_idx`. For row r with history h = hist[slot[r], :hist_len[r]], prompt
    length P and every token t < vocab_limit:

        a(t) = t in h            c(t) = #{ j >= P : h[j] = t }
        y = f32(x[t])
        if a(t):    y = y / rep if y > 0 else y * rep
        y = y - freq * f32(c(t))
        if c(t)>0:  y = y - pres
        if t in bias: y = y + bias[t]      (first matching entry of the row)
        x[t] = y rounded to x's dtype

    Only touched elements (a(t) or t a bias key) are written. Each line is
    one separately rounded f32 torch op, the sequence the kernel follows, so
    the two agree bit for bit."""
    m = int(row_idx.numel())
    if m == 0:
        return logits
    dev = logits.device
    vl = min(int(vocab_limit), logits.shape[1])
    lcap = hist.shape[1]
    rows, slots = row_idx.tolist(), slot.tolist()
    lens, plens = hist_len.tolist(), prompt_len.tolist()
    n_bias = 0 if bias_tok is None else int(bias_tok.shape[1])
    for r in range(m):
        L = max(0, min(lens[r], lcap))
        P = max(0, min(plens[r], L))
        h = hist[slots[r], :L].long()
        out_pos = torch.arange(L, device=dev) >= P
        ok = (h >= 0) & (h < vl)
        h_all, h_out = h[ok], h[ok & out_pos]
        if n_bias:
            bt = bias_tok[r].long()
            b_ok = (bt >= 0) & (bt < vl)
            b_pos = torch.nonzero(b_ok).squeeze(1)
            bt = bt[b_ok]
        else:
            bt = h_all[:0]
        toks = torch.unique(torch.cat([h_all, bt]))     # sorted, distinct
        if toks.numel() == 0:
            continue
        cnt = torch.zeros(toks.numel(), dtype=torch.int64, device=dev)
        cnt.index_add_(0, torch.searchsorted(toks, h_out),
                       torch.ones_like(h_out))
        seen = torch.isin(toks, h_all)
        has_bias = torch.zeros_like(seen)
        bval = torch.zeros(toks.numel(), dtype=torch.float32, device=dev)
        if bt.numel():
            # first entry wins when a key is listed twice
            first = torch.full((toks.numel(),), n_bias, dtype=torch.int64,
                               device=dev)
            first.scatter_reduce_(0, torch.searchsorted(toks, bt), b_pos,
                                  reduce="amin")
            has_bias = first < n_bias
            bval = torch.where(has_bias,
                               bias_val[r].float()[first.clamp(max=n_bias - 1)],
                               bval)
        x = logits[rows[r]]
        y = x[toks].float()
        rp, pr, fq = rep[r].float(), pres[r].float(), freq[r].float()
        y = torch.where(seen, torch.where(y > 0, y / rp, y * rp), y)
        y = y - fq * cnt.float()
        y = torch.where(cnt > 0, y - pr, y)
        y = torch.where(has_bias, y + bval, y)
        x[toks] = y.to(logits.dtype)
    return logits
