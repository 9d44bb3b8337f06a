"""GPU tests for MXFP4 MoE expert weights: the weight quantiser and the
e4m3 x e2m1 block-scaled MFMA grouped GEMM (csrc/grouped_gemm_mxfp4.hip)
against the torch reference, the full layer, and the engine with hipGraph
decode."""

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


def _quant_rows_ref(x):
    """bf16 CPU rows -> (e4m3 codes [R, Kp], scale [R]) by the reference."""
    R, K = x.shape
    q = torch.empty(R, torch_ref.fp8_padded_k(K), dtype=F8)
    s = torch.empty(R)
    torch_ref.quantize_rows_fp8(x, q, s)
    return q, s


def _run_both(a_q, a_s, codes, scales, row_tok, counts, bm, gate_silu,
              n_cols):
    """Kernel and CPU reference on the same operands -> (got, ref, tile_off)."""
    counts_t, tile_off, max_tiles = _segments(counts, bm)
    rows_max = max_tiles * bm + bm
    ref = torch.zeros(rows_max, n_cols, dtype=torch.bfloat16)
    torch_ref.grouped_gemm_mxfp4(ref, a_q, a_s, codes, scales, row_tok,
                                 tile_off, counts_t, max_tiles, gate_silu, bm)
    out = torch.zeros(rows_max, n_cols, dtype=torch.bfloat16, device=DEV)
    ops.grouped_gemm_mxfp4(out, a_q.to(DEV), a_s.to(DEV), codes.to(DEV),
                           scales.to(DEV),
                           None if row_tok is None else row_tok.to(DEV),
                           tile_off.to(DEV), counts_t.to(DEV), max_tiles,
                           gate_silu, bm)
    assert torch.isfinite(out.float()).all()  # padding rows included
    return out.cpu(), ref, tile_off


def _live(t, tile_off, counts, bm):
    return torch.cat([t[int(tile_off[e]) * bm:int(tile_off[e]) * bm + c]
                      for e, c in enumerate(counts)]).float()


@pytest.mark.parametrize("K", [128, 160, 2880])
def test_quant_weight_bit_equal(K):
    """(a) codes and block scales bit-equal to the reference. K = 160 ends a
    row inside a K-tile, K = 2880 (gpt-oss width) pads to 2944; one all-zero
    row, one row whose block amax values are exact powers of two (the
    exponent must not round up), one with amax just below a power of two."""
    require_gpu()
    torch.manual_seed(K)
    R = 70
    x = (torch.randn(R, K) * torch.rand(R, 1) * 4).to(torch.bfloat16)
    x[11] = 0
    x[12] = x[12].clamp(-0.03, 0.03)          # below the smallest, 2^-4
    x[12, ::32] = torch.tensor([2.0 ** (i % 9 - 4) for i in range(K // 32)],
                               dtype=torch.bfloat16)
    x[13] = x[13].clamp(-0.9, 0.9)
    x[13, 5::32] = 1.9921875                  # bf16 just below 2
    c_ref, s_ref = torch_ref.quantize_weight_mxfp4(x)
    Kp = torch_ref.fp8_padded_k(K)
    assert c_ref.shape == (R, Kp // 2) and s_ref.shape == (R, Kp // 32)
    c, s = ops.quantize_weight_mxfp4(x.to(DEV))
    assert c.dtype == torch.uint8 and s.dtype == torch.uint8
    assert torch.equal(s.cpu(), s_ref)
    assert torch.equal(c.cpu(), c_ref)
    assert (s_ref[11] == 0x7f).all() and (c_ref[11] == 0).all()
    assert (s_ref[12, :K // 32].int() ==
            torch.tensor([127 + i % 9 - 4 - 2 for i in range(K // 32)])).all()
    assert (c.cpu()[:, K // 2:] == 0).all()
    assert (s.cpu()[:, K // 32:] == 0x7f).all()


@pytest.mark.parametrize("bm", [64, 128])
def test_lane_and_scale_maps_exact(bm):
    """(b) operand lane map, nibble order, scale-byte-to-block map, scale
    layout and swizzle, with exact data: each A row is nonzero at one k
    (different per row) with an integer in [-4, 4]; W codes follow an
    asymmetric pattern in (n, k, e) over the whole signed e2m1 grid; block
    scales an asymmetric pattern of powers of two 2^-3 .. 2^3 in
    (n, k/32, e). Every product is a single term a * grid * 2^s with at most
    5 significant bits, so the kernel and the reference hold the same fp32
    value and round it to the same bf16: bit-equal on the live rows."""
    require_gpu()
    E, N, K = 5, 192, 256
    counts = [7, 0, 130, 64, 1]
    _, tile_off, max_tiles = _segments(counts, bm)
    rows = max_tiles * bm + bm
    r = torch.arange(rows)
    a = torch.zeros(rows, K)
    vals = torch.tensor([-4., -3., -2., -1., 1., 2., 3., 4.])
    a[r, (r * 37 + 5) % K] = vals[r % 8]      # 37 is coprime to 256
    a_q = a.to(F8)
    assert torch.equal(a_q.float(), a)
    n = torch.arange(N).view(1, N, 1)
    k = torch.arange(K).view(1, 1, K)
    e = torch.arange(E).view(E, 1, 1)
    # all 16 codes; the k // 16 term makes every shift of k by a multiple of
    # 16 inside a K-tile change the code (5 * 16 = 0 mod 16 alone would not:
    # a permutation of 16-element runs must not go unseen)
    code = ((3 * n + 5 * k + 11 * (k // 16) + 7 * e) % 16).to(torch.uint8)
    codes = (code[..., 0::2] | (code[..., 1::2] << 4)).contiguous()
    kb = torch.arange(K // 32).view(1, 1, K // 32)
    scales = (127 - 3 + (2 * n + 3 * kb + e) % 7).to(torch.uint8).contiguous()
    # the packed pair decodes to the pattern it was built from
    grid = torch.tensor(torch_ref.E2M1_GRID + tuple(
        -v for v in torch_ref.E2M1_GRID))
    want_w = grid[code.long()] * torch.exp2(
        scales.float() - 127).repeat_interleave(32, dim=2)
    assert torch.equal(torch_ref.dequantize_mxfp4(codes, scales), want_w)
    got, ref, tile_off = _run_both(a_q, torch.ones(rows), codes, scales, None,
                                   counts, bm, False, N)
    g, f = _live(got, tile_off, counts, bm), _live(ref, tile_off, counts, bm)
    assert f.abs().max() > 0
    assert torch.equal(g, f)


def _plain_case(seed, E, N, K, bm, counts):
    torch.manual_seed(seed)
    _, _, max_tiles = _segments(counts, bm)
    rows = max_tiles * bm + bm
    a_q, a_s = _quant_rows_ref(torch.randn(rows, K).to(torch.bfloat16))
    codes, scales = torch_ref.quantize_weight_mxfp4(
        (torch.randn(E, N, K) * 0.2).to(torch.bfloat16))
    got, ref, tile_off = _run_both(a_q, a_s, codes, scales, None, counts, bm,
                                   False, N)
    torch.testing.assert_close(_live(got, tile_off, counts, bm),
                               _live(ref, tile_off, counts, bm),
                               atol=2e-3, rtol=2.0 ** -7)


@pytest.mark.parametrize("K", [128, 192])
def test_grouped_gemm_mxfp4_plain_vs_ref(K):
    """(c) random data, plain stage; the FP8 test's tolerances (rtol 2^-7 is
    one bf16 ulp, atol 2e-3 sits above the fp32 accumulation-order bound):
    the dequantised weights are exact in both, so only the order of the fp32
    sum differs."""
    require_gpu()
    _plain_case(K + 1, 5, 192, K, 64, [7, 0, 130, 64, 1])


def test_grouped_gemm_mxfp4_plain_bm128_bn128_vs_ref():
    """(c) the 8-wave 128x128 configuration, multi-tile segments."""
    require_gpu()
    _plain_case(9, 4, 256, 256, 128, [300, 0, 129, 64])


# (bm, m): the three tile configurations — 64x64, 128x128, and 128x64 for an
# n_cols that is a multiple of 64 but not of 128
@pytest.mark.parametrize("bm,m", [(64, 128), (128, 128), (128, 192)])
def test_grouped_gemm_mxfp4_gather_silu_vs_ref(bm, m):
    """(d) gather + SwiGLU stage, row_tok with -1 padding. Tolerances of the
    bf16 and FP8 kernels' tests (__expf differs from torch's exp)."""
    require_gpu()
    torch.manual_seed(bm + m)
    E, K, T = 4, 192, 100
    counts = [65, 3, 0, 90]
    _, tile_off, max_tiles = _segments(counts, bm)
    rows_max = max_tiles * bm + bm
    x_q, x_s = _quant_rows_ref(torch.randn(T, K).to(torch.bfloat16))
    codes, scales = torch_ref.quantize_weight_mxfp4(
        (torch.randn(E, 2 * m, K) * 0.2).to(torch.bfloat16))
    rng = np.random.default_rng(5)
    row_tok = torch.full((rows_max,), -1, dtype=torch.int32)
    for e, c in enumerate(counts):
        s0 = int(tile_off[e]) * bm
        row_tok[s0:s0 + c] = torch.from_numpy(
            rng.integers(0, T, size=c).astype(np.int32))
    got, ref, tile_off = _run_both(x_q, x_s, codes, scales, row_tok, counts,
                                   bm, True, m)
    torch.testing.assert_close(_live(got, tile_off, counts, bm),
                               _live(ref, tile_off, counts, bm),
                               atol=5e-2, rtol=5e-2)


def test_moe_mxfp4_layer_gpu_matches_loop():
    """(e) full layer in MXFP4 mode: grouped kernel path vs the segment-loop
    emulation, with and without the all-tokens-to-one-expert skew."""
    require_gpu()
    from sutro_amd.models.qwen3 import Qwen3MoE
    from sutro_amd.models.registry import ModelSpec

    spec = ModelSpec(name="tiny-moe-mx-gpu", hidden_size=256, num_layers=1,
                     num_heads=4, num_kv_heads=2, head_dim=64,
                     intermediate_size=0, vocab_size=512, num_experts=8,
                     experts_per_token=2, moe_intermediate_size=256)
    torch.manual_seed(2)
    moe = Qwen3MoE(spec, torch.bfloat16).to(DEV)
    for p in moe.parameters():
        torch.nn.init.normal_(p, std=0.05)
    moe.quantize_experts_mxfp4()
    assert moe.gate_up.dtype == torch.uint8 and moe.down.dtype == torch.uint8
    assert moe.experts_mxfp4 and not moe.experts_fp8
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


def test_moe_mxfp4_engine_gpu_graph_decode():
    """(f) tiny MoE model in MXFP4 mode through the engine with hipGraph
    decode: rows finish, two seeded runs agree, capture succeeded (a hidden
    host sync or an allocation inside capture would leave graph_runner None),
    and the experts are stored as uint8 at half a byte per weight (h and m
    are multiples of 128, so there is no padding)."""
    require_gpu()
    from sutro_amd.engine.config import EngineConfig
    from sutro_amd.engine.engine import LLMEngine
    from sutro_amd.engine.request import SamplingParams
    from sutro_amd.models.qwen3 import Qwen3MoE
    from sutro_amd.models.registry import ModelSpec

    E, h, m = 4, 256, 128
    spec = ModelSpec(name="tiny-moe-mx-e2e", hidden_size=h, num_layers=2,
                     num_heads=4, num_kv_heads=2, head_dim=64,
                     intermediate_size=0, vocab_size=2048, max_context=512,
                     tie_embeddings=True, num_experts=E, experts_per_token=2,
                     moe_intermediate_size=m)

    def run():
        cfg = EngineConfig(spec=spec, device=DEV, max_model_len=256,
                           num_kv_blocks=128, max_tokens_per_step=512,
                           seed=0, moe_weight_dtype="mxfp4")
        eng = LLMEngine(cfg)
        assert eng.graph_runner is not None
        moes = [mod for mod in eng.model.modules()
                if isinstance(mod, Qwen3MoE)]
        assert len(moes) == 2
        for mod in moes:
            assert mod.experts_mxfp4
            assert mod.gate_up.dtype == torch.uint8
            assert mod.down.dtype == torch.uint8
            assert mod.gate_up.numel() == E * 2 * m * h // 2
            assert mod.down.numel() == E * h * m // 2
            assert mod.gate_up_scales.dtype == torch.uint8
            assert mod.gate_up_scales.numel() == E * 2 * m * h // 32
        reqs = [eng.add_request(eng.tokenizer.encode(p),
                                SamplingParams(max_tokens=12, temperature=0.7,
                                               seed=3 + i))
                for i, p in enumerate(["moe mx row one", "moe mx row two"])]
        while eng.has_work():
            eng.step()
        assert all(r.finish_reason is not None for r in reqs)
        return [list(r.output_token_ids) for r in reqs]

    a = run()
    assert all(len(t) > 0 for t in a)
    assert a == run()
