"""FP8 (e4m3) MoE expert weights on the CPU path: the quantiser, the emulated
arithmetic of the layer, expert storage, the config knob and the engine."""

import pytest
import torch

from sutro_amd import ops
from sutro_amd.engine.config import EngineConfig
from sutro_amd.engine.engine import LLMEngine
from sutro_amd.engine.request import SamplingParams
from sutro_amd.models.qwen3 import Qwen3MoE
from sutro_amd.models.registry import ModelSpec
from sutro_amd.ops import torch_ref

F8 = torch.float8_e4m3fn


def _quant(x):
    R, K = x.shape
    Kp = torch_ref.fp8_padded_k(K)
    q = torch.empty(R, Kp, dtype=F8)
    q.view(torch.uint8).fill_(0x55)  # the op must overwrite every byte
    s = torch.empty(R)
    ops.quantize_rows_fp8(x, q, s)
    return q, s


def test_quantize_rows_round_trip():
    """Per-row |dequant - x| <= 2^-4 * amax: half an e4m3 ulp in the top
    binade [256, 448] is 16 of 448 after scaling, below 2^-4 of amax; lower
    binades and subnormals only err less."""
    torch.manual_seed(0)
    x = torch.randn(70, 192).to(torch.bfloat16)
    x[5] = 0                      # all-zero row
    x[6] *= 1e-3                  # small row keeps its own scale
    x[7, 3] = 100.0               # outlier: the rest of the row goes subnormal
    q, s = _quant(x)
    assert q.shape == (70, 256) and q.dtype == F8
    xf = x.float()
    amax = xf.abs().amax(dim=1)
    deq = q.float()[:, :192] * s[:, None]
    err = (deq - xf).abs().amax(dim=1)
    assert (err <= amax * 2.0 ** -4).all(), (err / amax.clamp(min=1e-30)).max()
    # scale = amax / 448, the amax element lands on +-448 exactly
    assert torch.equal(s[amax > 0], (amax / torch.full_like(amax, 448.0))[amax > 0])
    assert (q.float().abs().amax(dim=1)[amax > 0] == 448.0).all()
    # all-zero row: scale 1, codes 0
    assert s[5].item() == 1.0
    assert (q.view(torch.uint8)[5] == 0).all()
    # K=192 -> Kp=256 with a zero tail
    assert (q.view(torch.uint8)[:, 192:] == 0).all()
    assert torch.isfinite(q.float()).all()


def test_quantize_weight_shapes():
    torch.manual_seed(1)
    w = torch.randn(3, 10, 192)
    w_q, sc = torch_ref.quantize_weight_fp8(w)
    assert w_q.shape == (3, 10, 256) and w_q.dtype == F8
    assert sc.shape == (3, 10) and sc.dtype == torch.float32
    torch.testing.assert_close(sc, w.abs().amax(dim=2) / 448.0, rtol=1e-6,
                               atol=0)


def _tiny_moe():
    spec = ModelSpec(name="tiny-moe-fp8", hidden_size=256, num_layers=1,
                     num_heads=4, num_kv_heads=2, head_dim=64,
                     intermediate_size=0, vocab_size=512, num_experts=8,
                     experts_per_token=2, moe_intermediate_size=256)
    torch.manual_seed(2)
    moe = Qwen3MoE(spec, torch.float32)
    for p in moe.parameters():
        torch.nn.init.normal_(p, std=0.05)
    return moe


def test_moe_fp8_close_to_unquantised():
    """FP8 layer vs the same module unquantised (fp32), normalised Frobenius
    error capped at 0.15 — a sanity bound: independent e4m3 rounding is about
    0.036 rms per operand, about 0.05 per GEMM and about 0.09 through SwiGLU
    and the second GEMM; a wrong scale or layout gives about 1.
    Measured: 0.0636 (routed), 0.0635 (all tokens to one expert), the same
    on the segment loop and the grouped path."""
    import copy

    moe = _tiny_moe()
    moe8 = copy.deepcopy(moe)
    moe8.quantize_experts_fp8()
    assert moe8.experts_fp8 and not moe.experts_fp8
    x = torch.randn(333, 256) * 0.5
    for skew in (False, True):
        if skew:
            with torch.no_grad():  # every token -> expert 3
                moe.router.weight[3] += 50.0
                moe8.router.weight[3] += 50.0
        y = moe._forward_loop(x)
        for fwd in (moe8._forward_loop, moe8._forward_grouped):
            y8 = fwd(x)
            err = ((y8 - y).norm() / y.norm()).item()
            print(f"fp8 MoE {fwd.__name__} skew={skew}: "
                  f"normalised Frobenius error {err:.4f}")
            assert err <= 0.15
        # the grouped path and the segment loop compute the same function
        torch.testing.assert_close(moe8._forward_grouped(x),
                                   moe8._forward_loop(x), atol=1e-4,
                                   rtol=1e-4)


def test_expert_storage_bytes():
    moe = _tiny_moe()
    E, h, m = 8, 256, 256
    moe.quantize_experts_fp8()
    moe.quantize_experts_fp8()  # idempotent
    for name, (N, K) in (("gate_up", (2 * m, h)), ("down", (h, m))):
        Kp = (K + 127) // 128 * 128
        w, s = getattr(moe, name), getattr(moe, name + "_scale")
        assert w.dtype == F8 and w.shape == (E, N, Kp)
        assert s.dtype == torch.float32 and s.shape == (E, N)
        assert w.numel() * w.element_size() == E * N * Kp
        assert s.numel() * s.element_size() == 4 * E * N
    # nothing but the router is left in the working dtype
    assert [n for n, _ in moe.named_parameters()] == ["router.weight"]
    big = [n for n, t in moe.state_dict().items()
           if t.dim() == 3 and t.dtype != F8]
    assert big == []


def test_expert_storage_pads_k():
    """m = 192 is no multiple of the 128-element K-tile: down pads to 256."""
    spec = ModelSpec(name="tiny-moe-pad", hidden_size=64, num_layers=1,
                     num_heads=2, num_kv_heads=1, head_dim=32,
                     intermediate_size=0, vocab_size=128, num_experts=4,
                     experts_per_token=2, moe_intermediate_size=192)
    torch.manual_seed(3)
    moe = Qwen3MoE(spec, torch.float32)
    for p in moe.parameters():
        torch.nn.init.normal_(p, std=0.1)
    x = torch.randn(21, 64)
    y = moe._forward_loop(x)
    moe.quantize_experts_fp8()
    assert moe.gate_up.shape == (4, 384, 128) and moe.down.shape == (4, 64, 256)
    assert (moe.down.view(torch.uint8)[:, :, 192:] == 0).all()
    y8 = moe._forward_grouped(x)
    assert ((y8 - y).norm() / y.norm()).item() <= 0.15
    torch.testing.assert_close(y8, moe._forward_loop(x), atol=1e-4, rtol=1e-4)


def _spec(moe: bool):
    if moe:
        return ModelSpec(name="tiny-moe-fp8-e2e", hidden_size=64, num_layers=2,
                         num_heads=4, num_kv_heads=2, head_dim=16,
                         intermediate_size=0, vocab_size=512, max_context=512,
                         tie_embeddings=True, num_experts=4,
                         experts_per_token=2, moe_intermediate_size=64)
    return ModelSpec(name="tiny-dense-fp8-e2e", hidden_size=64, num_layers=2,
                     num_heads=4, num_kv_heads=2, head_dim=16,
                     intermediate_size=128, vocab_size=512, max_context=512,
                     tie_embeddings=True)


def _generate(spec, **kw):
    cfg = EngineConfig(spec=spec, device="cpu", max_model_len=256,
                       num_kv_blocks=64, max_tokens_per_step=128, seed=0, **kw)
    eng = LLMEngine(cfg)
    reqs = [eng.add_request(eng.tokenizer.encode(p),
                            SamplingParams(max_tokens=8, temperature=0.7,
                                           seed=11 + i))
            for i, p in enumerate(["fp8 row one", "fp8 row two"])]
    while eng.has_work():
        eng.step()
    return eng, [list(r.output_token_ids) for r in reqs]


def test_config_rejects_unknown_dtype():
    with pytest.raises(ValueError):
        EngineConfig(spec=_spec(True), device="cpu", moe_weight_dtype="int4")
    assert EngineConfig(spec=_spec(True), device="cpu").moe_weight_dtype == "bf16"


def test_dense_spec_ignores_moe_weight_dtype():
    _, base = _generate(_spec(False))
    _, got = _generate(_spec(False), moe_weight_dtype="fp8_e4m3")
    assert got == base and all(len(t) > 0 for t in got)


def test_engine_kwargs_reach_the_config():
    from sutro_amd.service.models_map import resolve_engine_config

    cfg = resolve_engine_config("qwen-3-30b-a3b", device="cpu",
                                moe_weight_dtype="fp8_e4m3")
    assert cfg.moe_weight_dtype == "fp8_e4m3"


def test_cpu_engine_fp8_end_to_end():
    eng, a = _generate(_spec(True), moe_weight_dtype="fp8_e4m3")
    moes = [m for m in eng.model.modules() if isinstance(m, Qwen3MoE)]
    assert len(moes) == 2 and all(m.experts_fp8 for m in moes)
    assert all(len(t) > 0 for t in a)
    _, b = _generate(_spec(True), moe_weight_dtype="fp8_e4m3")
    assert a == b
