"""GPU tests for block-scaled FP8 MoE experts: the grouped GEMM with 128x128
weight scales (csrc/grouped_gemm_fp8_block.hip), its quantising stage-1
epilogue, the layer and the engine with moe_weight_dtype="fp8_block128".

References: the f64 product of the dequantised operands, and the dense block
kernel (csrc/gemm_tn_fp8_block_pipe.hip) with the separate group quantiser,
which the grouped kernel must reproduce bit for bit."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sutro_amd import _C, ops
    from sutro_amd.ops import torch_ref
else:  # collected on CPU; every test is skipped by the marker filter anyway
    _C = ops = torch_ref = None

DEV = "cuda"
F8 = torch.float8_e4m3fn
# the plain-stage tolerance of tests/test_gpu_dense_fp8_block128.py
PLAIN_TOL = dict(atol=2e-3, rtol=2.0 ** -7)
MOE = "fp8_block128"


def require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _segments(counts, bm):
    """(tile_off, counts, max_tiles) on the device for segments padded to bm;
    max_tiles has one spare tile, so the grid's early exit runs too."""
    tiles = [(c + bm - 1) // bm for c in counts]
    off = [0]
    for t in tiles:
        off.append(off[-1] + t)
    return (torch.tensor(off, dtype=torch.int32, device=DEV),
            torch.tensor(counts, dtype=torch.int32, device=DEV), off[-1] + 1)


def _operands(R, E, N, K, seed, exact):
    """a_q [R, K] + a_s [K/128, R], w_q [E, N, K] + w_s [E, N/128, K/128] on
    the device, and their exact f64 dequantisations. exact: integer codes in
    [-3, 3] and power-of-two scales, distinct per (row, kb) and per (expert,
    N block, kb), so every f32 product and sum is exact; else random bf16
    data through the real quantisers."""
    g = torch.Generator().manual_seed(seed)
    if exact:
        a_q = torch.randint(-3, 4, (R, K), generator=g).float().to(F8)
        w_q = torch.randint(-3, 4, (E, N, K), generator=g).float().to(F8)
        kb = torch.arange(K // 128)
        a_s = 2.0 ** ((torch.arange(R)[None, :] + 2 * kb[:, None]) % 3
                      - 1).float()
        w_s = 2.0 ** ((torch.arange(E)[:, None, None] * 3
                       + torch.arange(N // 128)[None, :, None]
                       + kb[None, None, :]) % 4 - 2).float()
    else:
        a_q, a_s = torch_ref.quantize_rows_fp8_block128(
            (torch.randn(R, K, generator=g) * 2).bfloat16())
        pairs = [torch_ref.quantize_weight_fp8_block128(
            (torch.randn(N, K, generator=g) * 0.2).bfloat16())
            for _ in range(E)]
        w_q = torch.stack([q for q, _ in pairs])
        w_s = torch.stack([s for _, s in pairs])
    a64 = a_q.double() * a_s.double().t().repeat_interleave(128, 1)
    w64 = (w_q.double() * w_s.double().repeat_interleave(128, 1)
           .repeat_interleave(128, 2))
    return tuple(t.to(DEV) for t in (a_q, a_s, w_q, w_s, a64, w64))


@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("K", [128, 256, 384])
@pytest.mark.parametrize("bm", [64, 128])
def test_plain_stage_scale_maps_are_exact(bm, K, N):
    """Live rows equal the f64 evaluation rounded once to bf16, bit for bit:
    an index error in either scale map is a wrong value, not noise."""
    require_gpu()
    counts = (1, 0, 130)
    tile_off, cnt, max_tiles = _segments(counts, bm)
    rows = max_tiles * bm
    a_q, a_s, w_q, w_s, a64, w64 = _operands(rows, 3, N, K, bm + K + N, True)
    out = torch.zeros(rows, N, dtype=torch.bfloat16, device=DEV)
    ops.grouped_gemm_fp8_block128(out, a_q, a_s, w_q, w_s, tile_off, cnt,
                                  max_tiles, bm=bm)
    for e, c in enumerate(counts):
        s0 = int(tile_off[e]) * bm
        ref = a64[s0:s0 + c] @ w64[e].T
        assert torch.equal(ref.float().double(), ref)  # exact in f32 too
        assert c == 0 or ref.abs().max() > 0
        assert torch.equal(out[s0:s0 + c], ref.float().bfloat16()), (
            e, (out[s0:s0 + c] != ref.float().bfloat16()).sum().item())


@pytest.mark.parametrize("M", [1, 129, 300])
@pytest.mark.parametrize("bm", [64, 128])
def test_plain_stage_equals_the_dense_block_kernel(bm, M):
    """One expert, identity layout, full-range operands: the fold is the
    dense kernel's, so the outputs are the same bits."""
    require_gpu()
    K, N = 640, 384
    tile_off, cnt, max_tiles = _segments((M,), bm)
    rows = max_tiles * bm
    a_q, a_s, w_q, w_s, a64, w64 = _operands(rows, 1, N, K, M + bm, False)
    out = torch.zeros(rows, N, dtype=torch.bfloat16, device=DEV)
    ops.grouped_gemm_fp8_block128(out, a_q, a_s, w_q, w_s, tile_off, cnt,
                                  max_tiles, bm=bm)
    dense = _C.gemm_fp8_block_pipelined(a_q[:M], a_s[:, :M].contiguous(),
                                        w_q[0], w_s[0], None, 1)
    assert torch.equal(out[:M], dense)
    torch.testing.assert_close(out[:M].double(), a64[:M] @ w64[0].T,
                               **PLAIN_TOL)


@pytest.mark.parametrize("I", [128, 256])
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("bm", [64, 128])
def test_stage1_equals_dense_kernel_plus_quantiser(bm, K, I):
    """Gathered codes and scales, SwiGLU, and the quantising epilogue: per
    expert the live rows of act_q / act_s are the bits of the dense SwiGLU
    kernel's bf16 output put through the separate group quantiser."""
    require_gpu()
    counts, T = (65, 0, 3), 100
    tile_off, cnt, max_tiles = _segments(counts, bm)
    rows = max_tiles * bm
    x_q, x_s, w_q, w_s, _, _ = _operands(T, 3, 2 * I, K, bm + K + I, False)
    g = torch.Generator().manual_seed(7)
    row_tok = torch.full((rows,), -1, dtype=torch.int32)
    for e, c in enumerate(counts):
        s0 = int(tile_off[e]) * bm
        row_tok[s0:s0 + c] = torch.randint(0, T, (c,), generator=g).int()
    row_tok = row_tok.to(DEV)
    # a row stride that is not the row count, as in the layer's workspace
    act_q = torch.zeros(rows, I, dtype=torch.uint8, device=DEV).view(F8)
    act_s = torch.zeros(I // 128, rows + 4, device=DEV)[:, :rows]
    ops.grouped_gemm_fp8_block128_gate_q(act_q, act_s, x_q, x_s, w_q, w_s,
                                         row_tok, tile_off, cnt, max_tiles,
                                         bm=bm)
    for e, c in enumerate(counts):
        if c == 0:
            continue
        s0 = int(tile_off[e]) * bm
        idx = row_tok[s0:s0 + c].long()
        act = _C.gemm_fp8_block_gate_up_silu(
            x_q.view(torch.uint8)[idx].view(F8), x_s[:, idx].contiguous(),
            w_q[e], w_s[e])
        assert act.abs().max() > 0
        want_q, want_s = ops.quantize_rows_fp8_block128(act)
        assert torch.equal(act_s[:, s0:s0 + c], want_s), e
        assert torch.equal(act_q[s0:s0 + c].view(torch.uint8),
                           want_q.view(torch.uint8)), e


def _spec(layers, experts):
    from sutro_amd.models.registry import ModelSpec

    return ModelSpec(name="tiny-moe-fp8-block-gpu", hidden_size=256,
                     num_layers=layers, num_heads=4, num_kv_heads=2,
                     head_dim=64, intermediate_size=0, vocab_size=2048,
                     max_context=512, tie_embeddings=True,
                     num_experts=experts, experts_per_token=2,
                     moe_intermediate_size=128)


def test_layer_grouped_matches_loop():
    """Full layer, quantised at start-up: grouped kernel path vs the
    segment-loop statement, with and without the all-tokens-to-one-expert
    skew; the tolerance of test_moe_fp8_layer_gpu_matches_loop."""
    require_gpu()
    from sutro_amd.models.qwen3 import Qwen3MoE

    torch.manual_seed(2)
    moe = Qwen3MoE(_spec(1, 8), torch.bfloat16).to(DEV)
    for p in moe.parameters():
        torch.nn.init.normal_(p, std=0.05)
    moe.quantize_experts_fp8_block128()
    assert moe.experts_fp8_block128 and not moe.experts_fp8
    assert moe.gate_up.dtype == F8 and moe.down.dtype == F8
    x = (torch.randn(333, 256) * 0.5).to(torch.bfloat16).to(DEV)
    for skew in (False, True):
        if skew:
            with torch.no_grad():
                moe.router.weight[3] += 50.0  # every token -> expert 3
        ref = moe._forward_loop(x).float()
        got = moe._forward_grouped(x).float()
        assert ref.abs().max() > 0
        torch.testing.assert_close(got, ref, atol=3e-2, rtol=3e-2)


def test_engine_graph_decode_and_reload(tmp_path):
    """Tiny MoE model through the engine with hipGraph decode: capture
    succeeded, two seeded runs agree, and a second engine started from the
    saved quantised experts holds the same bytes and gives the same tokens."""
    require_gpu()
    from sutro_amd.engine.config import EngineConfig
    from sutro_amd.engine.engine import LLMEngine
    from sutro_amd.engine.request import SamplingParams
    from sutro_amd.models.loader import save_weights

    def run(weights_path=None):
        cfg = EngineConfig(spec=_spec(2, 4), device=DEV, max_model_len=256,
                           num_kv_blocks=128, max_tokens_per_step=512,
                           seed=0, moe_weight_dtype=MOE,
                           weights_path=weights_path)
        eng = LLMEngine(cfg)
        assert eng.graph_runner is not None
        assert all(layer.mlp.experts_fp8_block128
                   for layer in eng.model.layers)
        reqs = [eng.add_request(eng.tokenizer.encode(p),
                                SamplingParams(max_tokens=12, temperature=0.7,
                                               seed=3 + i))
                for i, p in enumerate(["moe block row one", "moe block two"])]
        while eng.has_work():
            eng.step()
        assert all(r.finish_reason is not None for r in reqs)
        return eng, [list(r.output_token_ids) for r in reqs]

    eng, a = run()
    assert all(len(t) > 0 for t in a)
    assert a == run()[1]
    path = str(tmp_path / "ckpt")
    save_weights(eng.model, path)
    eng_l, b = run(path)
    for la, lb in zip(eng.model.layers, eng_l.model.layers):
        for name in ("gate_up", "down"):
            assert torch.equal(getattr(la.mlp, name).view(torch.uint8),
                               getattr(lb.mlp, name).view(torch.uint8))
            assert torch.equal(getattr(la.mlp, name + "_scale_inv"),
                               getattr(lb.mlp, name + "_scale_inv"))
    assert b == a
