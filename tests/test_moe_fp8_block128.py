"""CPU tests for block-scaled FP8 MoE experts
(moe_weight_dtype="fp8_block128"): config and CLI, the loader for the
published per-expert pairs and the model's own stacked pairs (TP slicing on
the block grid, errors), and the layer's loop path against an f64 evaluation
of the dequantised weights."""

import pytest
import torch
import torch.nn.functional as F

from sutro_amd.engine.config import EngineConfig
from sutro_amd.models.loader import load_weights, save_weights
from sutro_amd.models.qwen3 import Qwen3MoE
from sutro_amd.models.registry import ModelSpec, tiny_spec_for_tests
from sutro_amd.ops import torch_ref
from sutro_amd.parallel.tp import TPContext

F8 = torch.float8_e4m3fn
MOE = "fp8_block128"
H, M = 128, 256


def _layer(tp=None, m=M, quantised=False):
    """a 2-expert MoE layer under the name `layers.0.mlp`"""
    spec = ModelSpec(name="tiny-moe-block", hidden_size=H, num_layers=1,
                     num_heads=4, num_kv_heads=2, head_dim=32,
                     intermediate_size=0, vocab_size=512, num_experts=2,
                     experts_per_token=1, moe_intermediate_size=m)
    moe = Qwen3MoE(spec, torch.float32, tp)
    if quantised:
        torch.manual_seed(1)
        for p in moe.parameters():
            torch.nn.init.normal_(p, std=0.05)
        moe.quantize_experts_fp8_block128()
    return torch.nn.ModuleDict(
        {"layers": torch.nn.ModuleList([torch.nn.ModuleDict({"mlp": moe})])})


def _published(model, tmp_path, drop=()):
    """write the quantised layer under the published per-expert names"""
    from safetensors.torch import save_file

    moe = model["layers"][0]["mlp"]
    m = moe.gate_up.shape[1] // 2
    state = {}
    for e in range(2):
        pre = f"model.layers.0.mlp.experts.{e}."
        for part, w, s in (
                ("gate", moe.gate_up[e, :m], moe.gate_up_scale_inv[e, :m // 128]),
                ("up", moe.gate_up[e, m:], moe.gate_up_scale_inv[e, m // 128:]),
                ("down", moe.down[e], moe.down_scale_inv[e])):
            state[pre + part + "_proj.weight"] = w.contiguous()
            state[pre + part + "_proj.weight_scale_inv"] = s.contiguous()
    for k in drop:
        del state[k]
    tmp_path.mkdir(exist_ok=True)
    save_file(state, str(tmp_path / "model.safetensors"))
    return str(tmp_path)


def _same(a, b):
    return a.dtype == b.dtype and torch.equal(
        a.view(torch.uint8) if a.dtype == F8 else a,
        b.view(torch.uint8) if b.dtype == F8 else b)


def test_config_and_cli_values(monkeypatch):
    from click.testing import CliRunner

    from sutro_amd import cli as cli_mod
    from sutro_amd.service import http_api

    spec = tiny_spec_for_tests()
    cfg = EngineConfig(spec=spec, device="cpu", moe_weight_dtype=MOE)
    assert cfg.moe_weight_dtype == MOE
    with pytest.raises(ValueError, match="fp8_block128"):
        EngineConfig(spec=spec, device="cpu", moe_weight_dtype="fp8_block")
    seen = {}
    monkeypatch.setattr(http_api, "run_server", lambda **kw: seen.update(kw))
    res = CliRunner().invoke(cli_mod.cli, ["serve", "--moe-weight-dtype", MOE])
    assert res.exit_code == 0, res.output
    assert seen["engine_kwargs"] == {"moe_weight_dtype": MOE}
    res = CliRunner().invoke(cli_mod.cli,
                             ["serve", "--moe-weight-dtype", "fp8_block"])
    assert res.exit_code != 0


@pytest.mark.parametrize("form", ["published", "stacked"])
def test_loader_installs_the_pairs_bit_for_bit(tmp_path, form):
    src = _layer(quantised=True)
    if form == "published":
        path = _published(src, tmp_path)
    else:
        path = str(tmp_path)
        save_weights(src, path)
    dst = _layer()
    load_weights(dst, path, strict=False, moe_weight_dtype=MOE)
    a, b = src["layers"][0]["mlp"], dst["layers"][0]["mlp"]
    assert b.experts_fp8_block128 and not b.experts_fp8
    assert not any("gate_up" in n or "down" in n
                   for n, _ in dst.named_parameters())
    for name in ("gate_up", "gate_up_scale_inv", "down", "down_scale_inv"):
        assert _same(getattr(a, name), getattr(b, name)), name


def test_loader_tp2_shards_are_block_grid_slices(tmp_path):
    """gate_up is cut along N per section (gate and up halved separately),
    down along K; codes and scales together."""
    src = _layer(quantised=True)
    full = src["layers"][0]["mlp"]
    path = _published(src, tmp_path)
    for rank in (0, 1):
        dst = _layer(TPContext(2, rank))
        load_weights(dst, path, strict=False, moe_weight_dtype=MOE)
        got = dst["layers"][0]["mlp"]
        rows = torch.cat([torch.arange(o + rank * 128, o + rank * 128 + 128)
                          for o in (0, M)])
        assert _same(got.gate_up, full.gate_up[:, rows])
        assert _same(got.gate_up_scale_inv,
                     full.gate_up_scale_inv[:, rows[::128] // 128])
        assert _same(got.down, full.down[:, :, rank * 128:(rank + 1) * 128])
        assert _same(got.down_scale_inv,
                     full.down_scale_inv[:, :, rank:rank + 1])


def test_loader_errors(tmp_path):
    src = _layer(m=128, quantised=True)
    path = _published(src, tmp_path / "a")
    # TP 2 of m = 128 puts the shard boundary at 64, off the block grid
    with pytest.raises(ValueError, match="128-wide scale blocks"):
        load_weights(_layer(TPContext(2, 1), m=128), path, strict=False,
                     moe_weight_dtype=MOE)
    # the same file under the per-channel mode: never an upcast of bare codes
    with pytest.raises(ValueError, match="FP8 tensor"):
        load_weights(_layer(m=128), path, strict=False,
                     moe_weight_dtype="fp8_e4m3")
    path = _published(src, tmp_path / "b", drop=(
        "model.layers.0.mlp.experts.1.up_proj.weight_scale_inv",))
    with pytest.raises(ValueError, match="incomplete FP8 pair"):
        load_weights(_layer(m=128), path, strict=False, moe_weight_dtype=MOE)


def test_loop_path_is_the_f64_evaluation_of_the_dequantised_weights():
    """_expert_mlp against f64 products of the dequantised weights with the
    layer's own quantised activations; the layer tolerance (atol = rtol =
    3e-2, tests/test_gpu_moe_fp8.py)."""
    moe = _layer(quantised=True)["layers"][0]["mlp"]
    x = torch.randn(37, H, generator=torch.Generator().manual_seed(0)) * 0.5

    def deq_w(q, s):
        return q.double() * s.double().repeat_interleave(
            128, 0).repeat_interleave(128, 1)

    def deq_a(rows):
        q, s = torch_ref.quantize_rows_fp8_block128(rows)
        return q.double() * s.double().t().repeat_interleave(128, 1)

    for e in range(2):
        y = deq_a(x) @ deq_w(moe.gate_up[e], moe.gate_up_scale_inv[e]).T
        act = (F.silu(y[:, :M]) * y[:, M:]).float()
        ref = deq_a(act) @ deq_w(moe.down[e], moe.down_scale_inv[e]).T
        got = moe._expert_mlp(x, e)
        assert ref.abs().max() > 0
        torch.testing.assert_close(got.double(), ref, atol=3e-2, rtol=3e-2)
