"""dense_act_quant on the CPU path: the config value and the CLI option, the
op against the composition it states, and the engine's tokens with the
activation quantiser fused into the norms against the separate pass."""

from dataclasses import replace

import pytest
import torch

from sutro_amd import ops
from sutro_amd.engine.config import EngineConfig
from sutro_amd.engine.engine import LLMEngine
from sutro_amd.engine.request import SamplingParams
from sutro_amd.models.registry import tiny_spec_for_tests
from sutro_amd.ops import torch_ref

DENSE = ("fp8_e4m3", "fp8_block128")


def _cfg(**kw):
    # every dense projection is whole 128x128 blocks (the spec of
    # tests/test_dense_fp8_block128.py)
    spec = replace(tiny_spec_for_tests(), hidden_size=128, num_heads=4,
                   num_kv_heads=4, head_dim=32, intermediate_size=256)
    return EngineConfig(spec=spec, device="cpu", max_model_len=256,
                        num_kv_blocks=64, max_tokens_per_step=128, seed=0,
                        **kw)


def test_config_values():
    assert _cfg().dense_act_quant == "separate"
    for dense in DENSE:
        assert _cfg(dense_weight_dtype=dense,
                    dense_act_quant="fused").dense_act_quant == "fused"
    with pytest.raises(ValueError, match="dense_act_quant"):
        _cfg(dense_weight_dtype="fp8_e4m3", dense_act_quant="norm")
    with pytest.raises(ValueError, match="dense_weight_dtype='bf16'"):
        _cfg(dense_act_quant="fused")


def test_cli_serve_carries_the_value(monkeypatch):
    from click.testing import CliRunner

    from sutro_amd import cli as cli_mod
    from sutro_amd.service import http_api
    from sutro_amd.service.models_map import resolve_engine_config

    seen = {}
    monkeypatch.setattr(http_api, "run_server", lambda **kw: seen.update(kw))
    res = CliRunner().invoke(cli_mod.cli, [
        "serve", "--dense-weight-dtype", "fp8_block128",
        "--dense-act-quant", "fused"])
    assert res.exit_code == 0, res.output
    assert seen["engine_kwargs"] == {"dense_weight_dtype": "fp8_block128",
                                     "dense_act_quant": "fused"}
    cfg = resolve_engine_config("qwen-3-0.6b", device="cpu",
                                **seen["engine_kwargs"])
    assert cfg.dense_act_quant == "fused"
    res = CliRunner().invoke(cli_mod.cli, ["serve", "--dense-act-quant", "x"])
    assert res.exit_code != 0


@pytest.mark.parametrize("with_residual", [True, False])
@pytest.mark.parametrize("mode", ["rows", "block128"])
def test_op_is_the_composition(mode, with_residual):
    g = torch.Generator().manual_seed(0)
    x = (3 * torch.randn(5, 256, generator=g)).bfloat16()
    res = (5 * torch.randn(5, 256, generator=g)).bfloat16()
    w = (1 + 0.1 * torch.randn(256, generator=g)).bfloat16()
    if with_residual:
        y, new_res = torch_ref.fused_add_rmsnorm(x, res, w, 1e-6)
    else:
        y, new_res = torch_ref.rmsnorm(x, w, 1e-6), x
    q, s = (torch_ref.quantize_act_fp8(y) if mode == "rows"
            else torch_ref.quantize_rows_fp8_block128(y))
    got_q, got_s, got_res = ops.rmsnorm_quant_fp8(
        x.clone(), res.clone() if with_residual else None, w, 1e-6, mode)
    assert torch.equal(got_q.view(torch.uint8), q.view(torch.uint8))
    assert torch.equal(got_s, s)
    assert torch.equal(got_res, new_res)


@pytest.mark.parametrize("dense", DENSE)
def test_engine_fused_equals_separate(dense, monkeypatch):
    calls = []
    real = ops.rmsnorm_quant_fp8
    monkeypatch.setattr(ops, "rmsnorm_quant_fp8",
                        lambda *a: calls.append(a[4]) or real(*a))
    out = {}
    for how in ("separate", "fused"):
        eng = LLMEngine(_cfg(dense_weight_dtype=dense, dense_act_quant=how))
        reqs = [eng.add_request(eng.tokenizer.encode(p),
                                SamplingParams(max_tokens=8, temperature=0.7,
                                               seed=5 + i))
                for i, p in enumerate(["act quant one", "act quant row two"])]
        while eng.has_work():
            eng.step()
        out[how] = ([list(r.output_token_ids) for r in reqs],
                    [r.cumulative_logprob for r in reqs])
        if how == "separate":
            assert not calls
    # the norms took the fused op, in the consumer's format
    assert calls and set(calls) == {
        "block128" if dense == "fp8_block128" else "rows"}
    assert all(out["fused"][0]) and out["fused"] == out["separate"]
