"""MXFP4 MoE expert weights on the CPU path: the reference quantiser (the one
statement of the format), the emulated arithmetic of the layer, expert
storage, the config knob, the engine and the checkpoint loader."""

import copy

import pytest
import torch

from sutro_amd import ops
from sutro_amd.engine.config import EngineConfig
from sutro_amd.engine.engine import LLMEngine
from sutro_amd.engine.request import SamplingParams
from sutro_amd.models.loader import save_weights
from sutro_amd.models.qwen3 import Qwen3MoE
from sutro_amd.models.registry import ModelSpec
from sutro_amd.ops import torch_ref

GRID = torch.tensor(torch_ref.E2M1_GRID)

# normalised Frobenius error of the MXFP4 layer against the unquantised one,
# measured on the CPU emulation (segment loop, routed) at the test's seed
MEASURED_LAYER_ERR = 0.2107


def test_grid_values_round_trip_exactly():
    """Every signed grid value times 2^s, for block exponents across the
    range, quantises to itself: the block holds a 4 or a 6 so amax fixes the
    shared exponent at s."""
    vals = torch.cat([GRID, -GRID])                       # 16 values
    for s in (-20, -3, 0, 1, 9):
        for top in (4.0, 6.0):
            blk = torch.zeros(32)
            blk[:16] = vals
            blk[16] = top
            w = (blk * 2.0 ** s).view(1, 1, 32)
            codes, scales = torch_ref.quantize_weight_mxfp4(w)
            assert codes.shape == (1, 1, 64) and scales.shape == (1, 1, 4)
            assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8
            assert scales[0, 0, 0].item() == 127 + s
            deq = torch_ref.dequantize_mxfp4(codes, scales)
            assert torch.equal(deq[0, 0, :32], w[0, 0])
            # K = 32 pads to Kp = 128: zero codes, unit scales
            assert (codes[0, 0, 16:] == 0).all()
            assert (scales[0, 0, 1:] == 0x7f).all()


def test_nibble_order_and_zero_block():
    w = torch.zeros(1, 2, 64)
    w[0, 0, 0] = 1.0      # element 0 -> low nibble of byte 0
    w[0, 0, 1] = -4.0     # element 1 -> high nibble of byte 0
    w[0, 0, 35] = 3.0     # second block: amax 3 -> b = 126, 3 / 0.5 = 6
    codes, scales = torch_ref.quantize_weight_mxfp4(w)
    # block 0: amax 4 -> 2^0; 1.0 is code 2, -4.0 is code 8 | 6
    assert scales[0, 0, 0].item() == 127
    assert codes[0, 0, 0].item() == (2 | (0xe << 4))
    assert scales[0, 0, 1].item() == 126
    assert codes[0, 0, 17].item() == (7 << 4)             # element 35
    # an all-zero row: unit scales, zero codes
    assert (scales[0, 1] == 0x7f).all() and (codes[0, 1] == 0).all()


def test_ties_round_to_even_and_small_values_have_no_sign():
    blk = torch.zeros(32)
    blk[0] = 4.0                                          # scale 2^0
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    want = torch.tensor([0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0])
    blk[1:8] = ties
    blk[8:15] = -ties
    blk[15] = -0.1                                        # rounds to +0
    blk[16] = 5.5                                         # above the tie: 6
    codes, scales = torch_ref.quantize_weight_mxfp4(blk.view(1, 32))
    deq = torch_ref.dequantize_mxfp4(codes, scales)[0]
    assert torch.equal(deq[1:8], want) and torch.equal(deq[8:15], -want)
    assert deq[16].item() == 6.0
    nib = torch.stack((codes[0] & 0xf, codes[0] >> 4), dim=-1).view(-1)
    assert nib[15].item() == 0 and nib[8].item() == 0     # never code 8
    # amax in [6, 8) * 2^s clamps to 6
    codes, scales = torch_ref.quantize_weight_mxfp4(
        torch.tensor([7.5] + [0.0] * 31).view(1, 32))
    assert torch_ref.dequantize_mxfp4(codes, scales)[0, 0].item() == 6.0


@pytest.mark.parametrize("K,Kp", [(2880, 2944), (40, 128)])
def test_padding_tail(K, Kp):
    """K = 2880 is 90 whole blocks in Kp = 2944; K = 40 ends inside its
    second block, whose amax runs over the 8 live elements only."""
    torch.manual_seed(K)
    w = torch.randn(2, 3, K)
    codes, scales = torch_ref.quantize_weight_mxfp4(w)
    assert codes.shape == (2, 3, Kp // 2) and scales.shape == (2, 3, Kp // 32)
    assert (codes[..., (K + 1) // 2:] == 0).all()
    assert (scales[..., (K + 31) // 32:] == 0x7f).all()
    assert (scales[..., :(K + 31) // 32] != 0x7f).any()
    deq = torch_ref.dequantize_mxfp4(codes, scales)
    assert (deq[..., K:] == 0).all()
    # per block |dequant - w| <= amax / 4: the block is scaled so that amax
    # lies in [4, 8); the widest rounding gap of the grid (4 -> 6) is 2, so
    # rounding errs by at most 1 <= amax / 4, and clamping x in (6, 8) to 6
    # errs by x - 6 <= amax - 6 <= amax / 4
    wp = torch.zeros(2, 3, Kp)
    wp[..., :K] = w
    err = (deq - wp).view(2, 3, Kp // 32, 32).abs().amax(dim=-1)
    amax = wp.view(2, 3, Kp // 32, 32).abs().amax(dim=-1)
    assert (err <= amax / 4).all()
    if K == 40:
        ref_b = torch.floor(torch.log2(w[..., 32:].abs().amax(dim=-1))) + 125
        assert torch.equal(scales[..., 1].float(), ref_b)


def test_ops_dispatch_matches_reference():
    torch.manual_seed(4)
    w = torch.randn(2, 5, 160)
    a, b = ops.quantize_weight_mxfp4(w)
    c, d = torch_ref.quantize_weight_mxfp4(w)
    assert torch.equal(a, c) and torch.equal(b, d)


def _tiny_moe():
    # the spec and seed of tests/test_moe_fp8.py
    spec = ModelSpec(name="tiny-moe-mxfp4", hidden_size=256, num_layers=1,
                     num_heads=4, num_kv_heads=2, head_dim=64,
                     intermediate_size=0, vocab_size=512, num_experts=8,
                     experts_per_token=2, moe_intermediate_size=256)
    torch.manual_seed(2)
    moe = Qwen3MoE(spec, torch.float32)
    for p in moe.parameters():
        torch.nn.init.normal_(p, std=0.05)
    return moe


def test_moe_mxfp4_close_to_unquantised():
    """MXFP4 layer vs the same module unquantised (fp32), normalised
    Frobenius error. The bound is 1.5 x the error of the CPU emulation
    measured at this seed on the routed segment loop, MEASURED_LAYER_ERR =
    0.2107; the margin covers the all-to-one-expert variant and the
    platform's BLAS summation order. Measured: 0.2107 (routed) and 0.2101
    (skewed), the same on the segment loop and the grouped path. (e2m1 with a
    power-of-two block scale errs by 0.117 rms per Gaussian weight, against
    0.036 for e4m3 — the FP8 layer measures 0.064; 0.12 per GEMM, twice
    through SwiGLU's product and once more in the second GEMM, gives 0.21.)"""
    moe = _tiny_moe()
    moe4 = copy.deepcopy(moe)
    moe4.quantize_experts_mxfp4()
    assert moe4.experts_mxfp4 and not moe4.experts_fp8
    assert not moe.experts_mxfp4
    x = torch.randn(333, 256) * 0.5
    for skew in (False, True):
        if skew:
            with torch.no_grad():  # every token -> expert 3
                moe.router.weight[3] += 50.0
                moe4.router.weight[3] += 50.0
        y = moe._forward_loop(x)
        for fwd in (moe4._forward_loop, moe4._forward_grouped):
            y4 = fwd(x)
            err = ((y4 - y).norm() / y.norm()).item()
            print(f"mxfp4 MoE {fwd.__name__} skew={skew}: "
                  f"normalised Frobenius error {err:.4f}")
            assert err <= 1.5 * MEASURED_LAYER_ERR
        # the grouped path and the segment loop compute the same function
        torch.testing.assert_close(moe4._forward_grouped(x),
                                   moe4._forward_loop(x), atol=1e-4,
                                   rtol=1e-4)


def test_expert_storage_idempotent_and_modes_do_not_mix():
    moe = _tiny_moe()
    E, h, m = 8, 256, 256
    moe.quantize_experts_mxfp4()
    before = {k: v.clone() for k, v in moe.state_dict().items()}
    moe.quantize_experts_mxfp4()  # idempotent
    after = moe.state_dict()
    assert before.keys() == after.keys()
    assert all(torch.equal(before[k], after[k]) for k in before)
    for name, (N, K) in (("gate_up", (2 * m, h)), ("down", (h, m))):
        w, s = getattr(moe, name), getattr(moe, name + "_scales")
        assert w.dtype == torch.uint8 and w.shape == (E, N, K // 2)
        assert s.dtype == torch.uint8 and s.shape == (E, N, K // 32)
    assert [n for n, _ in moe.named_parameters()] == ["router.weight"]
    with pytest.raises(RuntimeError):
        moe.quantize_experts_fp8()
    moe8 = _tiny_moe()
    moe8.quantize_experts_fp8()
    with pytest.raises(RuntimeError):
        moe8.quantize_experts_mxfp4()
    assert moe8.experts_fp8 and not moe8.experts_mxfp4


def test_expert_storage_pads_k():
    """m = 192 is no multiple of the 128-element K-tile: down pads to 256
    elements = 128 bytes, and the workspace follows the element count."""
    spec = ModelSpec(name="tiny-moe-mx-pad", hidden_size=64, num_layers=1,
                     num_heads=2, num_kv_heads=1, head_dim=32,
                     intermediate_size=0, vocab_size=128, num_experts=4,
                     experts_per_token=2, moe_intermediate_size=192)
    torch.manual_seed(3)
    moe = Qwen3MoE(spec, torch.float32)
    for p in moe.parameters():
        torch.nn.init.normal_(p, std=0.1)
    x = torch.randn(21, 64)
    moe.quantize_experts_mxfp4()
    assert moe.gate_up.shape == (4, 384, 64) and moe.down.shape == (4, 64, 128)
    assert moe.down_scales.shape == (4, 64, 8)
    assert (moe.down[:, :, 96:] == 0).all()
    assert (moe.down_scales[:, :, 6:] == 0x7f).all()
    torch.testing.assert_close(moe._forward_grouped(x), moe._forward_loop(x),
                               atol=1e-4, rtol=1e-4)


def _spec(moe: bool):
    if moe:
        return ModelSpec(name="tiny-moe-mx-e2e", hidden_size=64, num_layers=2,
                         num_heads=4, num_kv_heads=2, head_dim=16,
                         intermediate_size=0, vocab_size=512, max_context=512,
                         tie_embeddings=True, num_experts=4,
                         experts_per_token=2, moe_intermediate_size=64)
    return ModelSpec(name="tiny-dense-mx-e2e", hidden_size=64, num_layers=2,
                     num_heads=4, num_kv_heads=2, head_dim=16,
                     intermediate_size=128, vocab_size=512, max_context=512,
                     tie_embeddings=True)


def _engine(spec, **kw):
    cfg = EngineConfig(spec=spec, device="cpu", max_model_len=256,
                       num_kv_blocks=64, max_tokens_per_step=128, seed=0, **kw)
    return LLMEngine(cfg)


def _generate(spec, **kw):
    eng = _engine(spec, **kw)
    reqs = [eng.add_request(eng.tokenizer.encode(p),
                            SamplingParams(max_tokens=8, temperature=0.7,
                                           seed=11 + i))
            for i, p in enumerate(["mx row one", "mx row two"])]
    while eng.has_work():
        eng.step()
    return eng, [list(r.output_token_ids) for r in reqs]


def test_config_accepts_mxfp4_rejects_int4():
    cfg = EngineConfig(spec=_spec(True), device="cpu",
                       moe_weight_dtype="mxfp4")
    assert cfg.moe_weight_dtype == "mxfp4"
    with pytest.raises(ValueError):
        EngineConfig(spec=_spec(True), device="cpu", moe_weight_dtype="int4")


def test_cli_offers_mxfp4():
    from sutro_amd.cli import serve

    opt = next(p for p in serve.params if p.name == "moe_weight_dtype")
    assert "mxfp4" in opt.type.choices


def test_dense_spec_ignores_moe_weight_dtype():
    _, base = _generate(_spec(False))
    _, got = _generate(_spec(False), moe_weight_dtype="mxfp4")
    assert got == base and all(len(t) > 0 for t in got)


def test_cpu_engine_mxfp4_end_to_end():
    eng, a = _generate(_spec(True), moe_weight_dtype="mxfp4")
    moes = [m for m in eng.model.modules() if isinstance(m, Qwen3MoE)]
    assert len(moes) == 2 and all(m.experts_mxfp4 for m in moes)
    assert all(len(t) > 0 for t in a)
    _, b = _generate(_spec(True), moe_weight_dtype="mxfp4")
    assert a == b


def _expert_state(eng):
    return {k: v for k, v in eng.model.state_dict().items()
            if ".mlp.gate_up" in k or ".mlp.down" in k}


def test_loader_round_trips_quantised_experts(tmp_path):
    """Quantised experts are saved as the uint8 blocks/scales pair and come
    back byte-equal in a fresh mxfp4 engine; a bf16-mode load refuses them."""
    from safetensors import safe_open

    eng = _engine(_spec(True), moe_weight_dtype="mxfp4")
    path = save_weights(eng.model, str(tmp_path / "q"))
    with safe_open(path, framework="pt") as f:
        names = set(f.keys())
        blocks = f.get_tensor("layers.0.mlp.gate_up_blocks")
    assert {"layers.0.mlp.gate_up_blocks", "layers.0.mlp.gate_up_scales",
            "layers.1.mlp.down_blocks", "layers.1.mlp.down_scales"} <= names
    assert "layers.0.mlp.gate_up" not in names
    assert blocks.dtype == torch.uint8

    eng2 = _engine(_spec(True), moe_weight_dtype="mxfp4",
                   weights_path=str(tmp_path / "q"))
    want, got = _expert_state(eng), _expert_state(eng2)
    assert len(want) == 8 and want.keys() == got.keys()
    for k in want:
        assert got[k].dtype == torch.uint8 and torch.equal(got[k], want[k]), k
    with pytest.raises(ValueError):
        _engine(_spec(True), weights_path=str(tmp_path / "q"))


def test_loader_quantises_bf16_checkpoint_after_load(tmp_path):
    """A checkpoint with unquantised experts, loaded with the flag set,
    equals quantise-after-load."""
    plain = _engine(_spec(True))
    save_weights(plain.model, str(tmp_path / "p"))
    eng = _engine(_spec(True), moe_weight_dtype="mxfp4",
                  weights_path=str(tmp_path / "p"))
    got = _expert_state(eng)
    assert len(got) == 8
    for name, mod in plain.model.named_modules():
        if isinstance(mod, Qwen3MoE):
            for which in ("gate_up", "down"):
                c, s = torch_ref.quantize_weight_mxfp4(getattr(mod, which).data)
                assert torch.equal(got[f"{name}.{which}"], c)
                assert torch.equal(got[f"{name}.{which}_scales"], s)
