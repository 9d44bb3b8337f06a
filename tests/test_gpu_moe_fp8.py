"""GPU tests for FP8 (e4m3) MoE expert weights: the row quantiser and the
block-scaled MFMA grouped GEMM (csrc/grouped_gemm_fp8.hip) against the torch
reference, the full layer, and the engine with hipGraph decode."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sutro_amd import ops
    from sutro_amd.ops import torch_ref

DEV = "cuda"
F8 = torch.float8_e4m3fn


def require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _segments(counts, bm):
    counts_t = torch.tensor(counts, dtype=torch.int32)
    padded = (counts_t + bm - 1) // bm * bm
    pad_off = torch.zeros(len(counts) + 1, dtype=torch.int32)
    pad_off[1:] = torch.cumsum(padded, 0)
    return counts_t, pad_off // bm, int(pad_off[-1]) // bm


def _quant_ref(x):
    """bf16 CPU rows -> (codes [R, Kp], scale [R]) by the torch reference."""
    R, K = x.shape
    q = torch.empty(R, torch_ref.fp8_padded_k(K), dtype=F8)
    s = torch.empty(R)
    torch_ref.quantize_rows_fp8(x, q, s)
    return q, s


def _codes(vals, Kp):
    """Exactly representable values [R, K] -> e4m3 codes [R, Kp], zero tail."""
    R, K = vals.shape
    q = torch.zeros(R, Kp, dtype=torch.uint8)
    c = vals.to(F8)
    assert torch.equal(c.float(), vals.float())
    q[:, :K] = c.view(torch.uint8)
    return q.view(F8)


def _run_both(a_q, a_s, w_q, w_s, row_tok, counts, bm, gate_silu, n_cols):
    """Kernel and CPU reference on the same operands -> (got, ref, tile_off)."""
    counts_t, tile_off, max_tiles = _segments(counts, bm)
    rows_max = max_tiles * bm + bm
    ref = torch.zeros(rows_max, n_cols, dtype=torch.bfloat16)
    torch_ref.grouped_gemm_fp8(ref, a_q, a_s, w_q, w_s, row_tok, tile_off,
                               counts_t, max_tiles, gate_silu, bm)
    out = torch.zeros(rows_max, n_cols, dtype=torch.bfloat16, device=DEV)
    ops.grouped_gemm_fp8(out, a_q.to(DEV), a_s.to(DEV), w_q.to(DEV),
                         w_s.to(DEV),
                         None if row_tok is None else row_tok.to(DEV),
                         tile_off.to(DEV), counts_t.to(DEV), max_tiles,
                         gate_silu, bm)
    assert torch.isfinite(out.float()).all()  # padding rows included
    return out.cpu(), ref, tile_off


def _live(t, tile_off, counts, bm):
    return torch.cat([t[int(tile_off[e]) * bm:int(tile_off[e]) * bm + c]
                      for e, c in enumerate(counts)]).float()


@pytest.mark.parametrize("K", [128, 192, 2880])
def test_quantize_rows_bit_equal(K):
    """(a) codes and scales bit-equal to the reference, zero tail included;
    K=2880 (gpt-oss width) is no multiple of 128; one all-zero row."""
    require_gpu()
    torch.manual_seed(K)
    R = 70
    x = (torch.randn(R, K) * torch.rand(R, 1) * 4).to(torch.bfloat16)
    x[11] = 0
    q_ref, s_ref = _quant_ref(x)
    Kp = q_ref.shape[1]
    assert Kp == (K + 127) // 128 * 128
    q = torch.full((R, Kp), 0x55, dtype=torch.uint8, device=DEV).view(F8)
    s = torch.full((R,), -1.0, device=DEV)
    ops.quantize_rows_fp8(x.to(DEV), q, s)
    assert torch.equal(s.cpu().view(torch.int32), s_ref.view(torch.int32))
    assert torch.equal(q.cpu().view(torch.uint8), q_ref.view(torch.uint8))
    assert s_ref[11].item() == 1.0
    assert (q.cpu().view(torch.uint8)[:, K:] == 0).all()


def test_quantize_rows_wide_row_bit_equal():
    """Rows above 4096 elements leave the kernel's register-cached path and
    are read twice; K=4104 is also no multiple of 128 (Kp=4224)."""
    require_gpu()
    torch.manual_seed(4104)
    R, K = 9, 4104
    x = (torch.randn(R, K) * torch.rand(R, 1) * 4).to(torch.bfloat16)
    x[2] = 0
    q_ref, s_ref = _quant_ref(x)
    assert q_ref.shape[1] == 4224
    q = torch.full((R, 4224), 0x55, dtype=torch.uint8, device=DEV).view(F8)
    s = torch.full((R,), -1.0, device=DEV)
    ops.quantize_rows_fp8(x.to(DEV), q, s)
    assert torch.equal(s.cpu().view(torch.int32), s_ref.view(torch.int32))
    assert torch.equal(q.cpu().view(torch.uint8), q_ref.view(torch.uint8))


def test_quantize_rows_row_limit():
    """Rows at and past row_limit[0] * limit_mul are left untouched."""
    require_gpu()
    torch.manual_seed(7)
    x = torch.randn(70, 192).to(torch.bfloat16)
    q_ref, s_ref = _quant_ref(x)
    q = torch.full((70, 256), 0x55, dtype=torch.uint8, device=DEV).view(F8)
    s = torch.full((70,), -1.0, device=DEV)
    lim = torch.tensor([3], dtype=torch.int32, device=DEV)
    ops.quantize_rows_fp8(x.to(DEV), q, s, row_limit=lim, limit_mul=16)
    qb = q.cpu().view(torch.uint8)
    assert torch.equal(qb[:48], q_ref.view(torch.uint8)[:48])
    assert torch.equal(s.cpu()[:48], s_ref[:48])
    assert (qb[48:] == 0x55).all() and (s.cpu()[48:] == -1.0).all()


@pytest.mark.parametrize("bm", [64, 128])
def test_lane_map_exact_integers(bm):
    """(b) operand lane map with exact integer data: all scales 1, each A row
    nonzero at one k (different per row) with an integer in [-4, 4], W an
    asymmetric integer pattern in n and k. Every fp32 sum is exact, so the
    kernel and the reference round the same value to bf16: bit-equal."""
    require_gpu()
    E, N, K = 5, 192, 256
    counts = [7, 0, 130, 64, 1]
    _, tile_off, max_tiles = _segments(counts, bm)
    rows = max_tiles * bm + bm
    r = torch.arange(rows)
    a = torch.zeros(rows, K)
    vals = torch.tensor([-4., -3., -2., -1., 1., 2., 3., 4.])
    a[r, (r * 37 + 5) % K] = vals[r % 8]      # 37 is coprime to 256
    n = torch.arange(N).view(1, N, 1)
    k = torch.arange(K).view(1, 1, K)
    e = torch.arange(E).view(E, 1, 1)
    w = ((3 * n + 5 * k + e) % 9 - 4).float()
    a_q, w_q = _codes(a, K), _codes(w.view(E * N, K), K).view(E, N, K)
    got, ref, tile_off = _run_both(a_q, torch.ones(rows), w_q,
                                   torch.ones(E, N), None, counts, bm, False,
                                   N)
    g, f = _live(got, tile_off, counts, bm), _live(ref, tile_off, counts, bm)
    assert f.abs().max() > 0
    assert torch.equal(g, f)


@pytest.mark.parametrize("K", [128, 192])
def test_grouped_gemm_fp8_plain_vs_ref(K):
    """(c) random data, plain stage. rtol 2^-7 is one bf16 ulp (accumulation
    order may flip one rounding); atol 2e-3 sits above the fp32
    accumulation-order bound K * 2^-24 * sum|ab| ~ 5e-4 at these magnitudes."""
    require_gpu()
    torch.manual_seed(K + 1)
    E, N, bm = 5, 192, 64
    counts = [7, 0, 130, 64, 1]
    _, _, max_tiles = _segments(counts, bm)
    rows = max_tiles * bm + bm
    a_q, a_s = _quant_ref(torch.randn(rows, K).to(torch.bfloat16))
    w_q, w_s = torch_ref.quantize_weight_fp8(
        (torch.randn(E, N, K) * 0.2).to(torch.bfloat16))
    got, ref, tile_off = _run_both(a_q, a_s, w_q, w_s, None, counts, bm,
                                   False, N)
    torch.testing.assert_close(_live(got, tile_off, counts, bm),
                               _live(ref, tile_off, counts, bm),
                               atol=2e-3, rtol=2.0 ** -7)


def test_grouped_gemm_fp8_plain_bm128_bn128_vs_ref():
    """The 8-wave 128x128 configuration on the plain stage (the cases above
    select 64x64 and 128x64), multi-tile segments, same bounds as (c)."""
    require_gpu()
    torch.manual_seed(9)
    E, N, K, bm = 4, 256, 256, 128
    counts = [300, 0, 129, 64]
    _, _, max_tiles = _segments(counts, bm)
    rows = max_tiles * bm + bm
    a_q, a_s = _quant_ref(torch.randn(rows, K).to(torch.bfloat16))
    w_q, w_s = torch_ref.quantize_weight_fp8(
        (torch.randn(E, N, K) * 0.2).to(torch.bfloat16))
    got, ref, tile_off = _run_both(a_q, a_s, w_q, w_s, None, counts, bm,
                                   False, N)
    torch.testing.assert_close(_live(got, tile_off, counts, bm),
                               _live(ref, tile_off, counts, bm),
                               atol=2e-3, rtol=2.0 ** -7)


# (bm, m): the three tile configurations — 64x64, 128x128, and 128x64 for an
# n_cols that is a multiple of 64 but not of 128
@pytest.mark.parametrize("bm,m", [(64, 128), (128, 128), (128, 192)])
def test_grouped_gemm_fp8_gather_silu_vs_ref(bm, m):
    """(d) gather + SwiGLU stage, row_tok with -1 padding. Tolerances of the
    bf16 kernel's test (__expf differs from torch's exp)."""
    require_gpu()
    torch.manual_seed(bm + m)
    E, K, T = 4, 192, 100
    counts = [65, 3, 0, 90]
    _, tile_off, max_tiles = _segments(counts, bm)
    rows_max = max_tiles * bm + bm
    x_q, x_s = _quant_ref(torch.randn(T, K).to(torch.bfloat16))
    w_q, w_s = torch_ref.quantize_weight_fp8(
        (torch.randn(E, 2 * m, K) * 0.2).to(torch.bfloat16))
    rng = np.random.default_rng(5)
    row_tok = torch.full((rows_max,), -1, dtype=torch.int32)
    for e, c in enumerate(counts):
        s0 = int(tile_off[e]) * bm
        row_tok[s0:s0 + c] = torch.from_numpy(
            rng.integers(0, T, size=c).astype(np.int32))
    got, ref, tile_off = _run_both(x_q, x_s, w_q, w_s, row_tok, counts, bm,
                                   True, m)
    torch.testing.assert_close(_live(got, tile_off, counts, bm),
                               _live(ref, tile_off, counts, bm),
                               atol=5e-2, rtol=5e-2)


def test_moe_fp8_layer_gpu_matches_loop():
    """(e) full layer in FP8 mode: grouped kernel path vs the segment-loop
    emulation, with and without the all-tokens-to-one-expert skew."""
    require_gpu()
    from sutro_amd.models.qwen3 import Qwen3MoE
    from sutro_amd.models.registry import ModelSpec

    spec = ModelSpec(name="tiny-moe-fp8-gpu", hidden_size=256, num_layers=1,
                     num_heads=4, num_kv_heads=2, head_dim=64,
                     intermediate_size=0, vocab_size=512, num_experts=8,
                     experts_per_token=2, moe_intermediate_size=256)
    torch.manual_seed(2)
    moe = Qwen3MoE(spec, torch.bfloat16).to(DEV)
    for p in moe.parameters():
        torch.nn.init.normal_(p, std=0.05)
    moe.quantize_experts_fp8()
    assert moe.gate_up.dtype == F8 and moe.down.dtype == F8
    x = (torch.randn(333, 256) * 0.5).to(torch.bfloat16).to(DEV)
    ref = moe._forward_loop(x).float()
    got = moe._forward_grouped(x).float()
    torch.testing.assert_close(got, ref, atol=3e-2, rtol=3e-2)
    with torch.no_grad():
        moe.router.weight[3] += 50.0  # every token -> expert 3 (skew)
    ref = moe._forward_loop(x).float()
    got = moe._forward_grouped(x).float()
    assert ref.abs().max() > 0
    torch.testing.assert_close(got, ref, atol=3e-2, rtol=3e-2)


def test_moe_fp8_engine_gpu_graph_decode():
    """(f) tiny MoE model in FP8 mode through the engine with hipGraph decode:
    rows finish, two seeded runs agree, and capture succeeded (a hidden host
    sync or an allocation inside capture would leave graph_runner None)."""
    require_gpu()
    from sutro_amd.engine.config import EngineConfig
    from sutro_amd.engine.engine import LLMEngine
    from sutro_amd.engine.request import SamplingParams
    from sutro_amd.models.qwen3 import Qwen3MoE
    from sutro_amd.models.registry import ModelSpec

    spec = ModelSpec(name="tiny-moe-fp8-e2e", hidden_size=256, num_layers=2,
                     num_heads=4, num_kv_heads=2, head_dim=64,
                     intermediate_size=0, vocab_size=2048, max_context=512,
                     tie_embeddings=True, num_experts=4, experts_per_token=2,
                     moe_intermediate_size=192)

    def run():
        cfg = EngineConfig(spec=spec, device=DEV, max_model_len=256,
                           num_kv_blocks=128, max_tokens_per_step=512,
                           seed=0, moe_weight_dtype="fp8_e4m3")
        eng = LLMEngine(cfg)
        assert eng.graph_runner is not None
        assert all(m.experts_fp8 for m in eng.model.modules()
                   if isinstance(m, Qwen3MoE))
        reqs = [eng.add_request(eng.tokenizer.encode(p),
                                SamplingParams(max_tokens=12, temperature=0.7,
                                               seed=3 + i))
                for i, p in enumerate(["moe fp8 row one", "moe fp8 row two"])]
        while eng.has_work():
            eng.step()
        assert all(r.finish_reason is not None for r in reqs)
        return [list(r.output_token_ids) for r in reqs]

    a = run()
    assert all(len(t) > 0 for t in a)
    assert a == run()
