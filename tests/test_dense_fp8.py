"""FP8 (W8A8) dense weights on the CPU path: the config knob and the CLI
option, the stated arithmetic of the quantised layers, the quantise method,
closeness to the unquantised model, the engine, and the registry shapes."""

import pytest
import torch
import torch.nn.functional as F

from sutro_amd import ops
from sutro_amd.engine.config import EngineConfig
from sutro_amd.engine.engine import LLMEngine
from sutro_amd.engine.request import SamplingParams
from sutro_amd.models import qwen3
from sutro_amd.models.qwen3 import Qwen3Attention, Qwen3MLP, Qwen3MoE
from sutro_amd.models.registry import (MODEL_REGISTRY, ModelSpec,
                                       tiny_spec_for_tests)
from sutro_amd.ops import torch_ref

F8 = torch.float8_e4m3fn


def _cfg(spec, **kw):
    return EngineConfig(spec=spec, device="cpu", max_model_len=256,
                        num_kv_blocks=64, max_tokens_per_step=128, seed=0,
                        **kw)


# ---- config / CLI ----

def test_config_values():
    spec = tiny_spec_for_tests()
    assert EngineConfig(spec=spec, device="cpu").dense_weight_dtype == "bf16"
    assert _cfg(spec, dense_weight_dtype="bf16").dense_weight_dtype == "bf16"
    assert (_cfg(spec, dense_weight_dtype="fp8_e4m3").dense_weight_dtype
            == "fp8_e4m3")
    for bad in ("mxfp4", "fp8", "int8", ""):
        with pytest.raises(ValueError):
            _cfg(spec, dense_weight_dtype=bad)


def test_engine_kwargs_reach_the_config():
    from sutro_amd.service.models_map import resolve_engine_config

    cfg = resolve_engine_config("qwen-3-0.6b", device="cpu",
                                dense_weight_dtype="fp8_e4m3")
    assert cfg.dense_weight_dtype == "fp8_e4m3"
    assert cfg.moe_weight_dtype == "bf16"


def test_cli_serve_has_the_option(monkeypatch):
    from click.testing import CliRunner

    from sutro_amd import cli as cli_mod
    from sutro_amd.service import http_api

    res = CliRunner().invoke(cli_mod.cli, ["serve", "--help"])
    assert res.exit_code == 0 and "--dense-weight-dtype" in res.output

    seen = {}
    monkeypatch.setattr(http_api, "run_server",
                        lambda **kw: seen.update(kw))
    res = CliRunner().invoke(cli_mod.cli, [
        "serve", "--dense-weight-dtype", "fp8_e4m3",
        "--moe-weight-dtype", "mxfp4"])
    assert res.exit_code == 0, res.output
    assert seen["engine_kwargs"] == {"dense_weight_dtype": "fp8_e4m3",
                                     "moe_weight_dtype": "mxfp4"}
    seen.clear()
    assert CliRunner().invoke(cli_mod.cli, ["serve"]).exit_code == 0
    assert seen["engine_kwargs"] is None          # default: nothing changes
    res = CliRunner().invoke(cli_mod.cli,
                             ["serve", "--dense-weight-dtype", "mxfp4"])
    assert res.exit_code != 0


# ---- the stated arithmetic ----

def _quant_rows(x):
    q = torch.empty(x.shape[0], torch_ref.fp8_padded_k(x.shape[1]), dtype=F8)
    s = torch.empty(x.shape[0])
    torch_ref.quantize_rows_fp8(x, q, s)
    return q, s


def test_mlp_forward_is_the_stated_sequence():
    """quantise rows -> fp8_linear -> f32 SwiGLU -> one rounding -> quantise
    rows -> fp8_linear -> one rounding; hidden 192 pads K to 256."""
    torch.manual_seed(0)
    mlp = Qwen3MLP(192, 256, torch.float32)
    for p in mlp.parameters():
        torch.nn.init.normal_(p, std=0.05)
    w_gu = mlp.gate_up_proj.weight.data.clone()
    w_dn = mlp.down_proj.weight.data.clone()
    mlp.quantize_dense_fp8()
    x = torch.randn(37, 192) * 0.5

    gu_q, gu_s = torch_ref.quantize_weight_fp8(w_gu[None])
    dn_q, dn_s = torch_ref.quantize_weight_fp8(w_dn[None])
    assert gu_q.shape == (1, 512, 256)
    assert torch.equal(mlp.gate_up_proj.weight.view(torch.uint8),
                       gu_q[0].view(torch.uint8))
    assert torch.equal(mlp.gate_up_proj.weight_scale, gu_s[0])
    x_q, x_s = _quant_rows(x)
    y = torch_ref.fp8_linear(x_q, x_s, gu_q[0], gu_s[0])
    act = (F.silu(y[:, :256]) * y[:, 256:]).to(x.dtype)
    a_q, a_s = _quant_rows(act)
    want = torch_ref.fp8_linear(a_q, a_s, dn_q[0], dn_s[0]).to(x.dtype)
    got = mlp(x)
    assert want.abs().max() > 0
    assert torch.equal(got, want)
    # and through the ops, which state the same thing
    assert torch.equal(
        ops.gate_up_silu_fp8(x, mlp.gate_up_proj.weight,
                             mlp.gate_up_proj.weight_scale), act)
    res = torch.randn(37, 192)
    want_res = (torch_ref.fp8_linear(a_q, a_s, dn_q[0], dn_s[0])
                + res).to(x.dtype)
    assert torch.equal(
        ops.linear_fp8(act, mlp.down_proj.weight, mlp.down_proj.weight_scale,
                       residual=res), want_res)


def test_attention_projections_are_the_stated_sequence():
    torch.manual_seed(1)
    spec = tiny_spec_for_tests()
    attn = Qwen3Attention(spec, torch.float32, 0)
    for p in attn.parameters():
        torch.nn.init.normal_(p, std=0.1)
    weights = {n: getattr(attn, n).weight.data.clone()
               for n in ("qkv_proj", "o_proj")}
    attn.quantize_dense_fp8()
    for name, w in weights.items():
        lin = getattr(attn, name)
        x = torch.randn(19, w.shape[1])
        w_q, w_s = torch_ref.quantize_weight_fp8(w[None])
        x_q, x_s = _quant_rows(x)
        want = torch_ref.fp8_linear(x_q, x_s, w_q[0], w_s[0]).to(x.dtype)
        got = qwen3._dense_linear(lin, x)
        assert got.shape == (19, w.shape[0]) and want.abs().max() > 0
        assert torch.equal(got, want), name


# ---- the quantise method ----

def test_quantize_method():
    eng = LLMEngine(_cfg(tiny_spec_for_tests()))
    model = eng.model
    before = {n: t.dtype for n, t in model.state_dict().items()}
    model.quantize_dense_fp8()
    snap = {n: t.clone() for n, t in model.state_dict().items()}
    model.quantize_dense_fp8()        # idempotent: the bf16 weight is gone
    after = model.state_dict()
    assert set(after) == set(snap)
    for n, t in after.items():
        assert t.dtype == snap[n].dtype
        a = t.view(torch.uint8) if t.dtype == F8 else t
        b = snap[n].view(torch.uint8) if t.dtype == F8 else snap[n]
        assert torch.equal(a, b), n
    h, inter = 64, 128
    shapes = {"self_attn.qkv_proj": (64 + 2 * 32, h), "self_attn.o_proj": (h, 64),
              "mlp.gate_up_proj": (2 * inter, h), "mlp.down_proj": (h, inter)}
    for i in range(2):
        for name, (N, K) in shapes.items():
            w = after[f"layers.{i}.{name}.weight"]
            s = after[f"layers.{i}.{name}.weight_scale"]
            assert w.dtype == F8 and w.shape == (N, 128), name  # Kp = 128
            assert s.dtype == torch.float32 and s.shape == (N,), name
    # embedding (tied lm_head), norms: untouched
    for n, dt in before.items():
        if "_proj" not in n:
            assert after[n].dtype == dt, n
    assert after["embed_tokens.weight"].dtype == torch.float32
    assert model.compute_logits(torch.randn(2, h)).dtype == torch.float32


def test_quantize_refuses_foreign_storage():
    mlp = Qwen3MLP(64, 128, torch.float32)
    lin = mlp.down_proj
    w = lin.weight.data
    del lin._parameters["weight"]
    lin.register_buffer("weight", torch.zeros(w.shape, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        mlp.quantize_dense_fp8()


def test_save_weights_refuses_a_quantised_model(tmp_path):
    """The quantised projections are buffers: save_weights, which writes the
    parameters, must not emit a file without them."""
    from sutro_amd.models.loader import save_weights

    eng = LLMEngine(_cfg(tiny_spec_for_tests(), dense_weight_dtype="fp8_e4m3"))
    with pytest.raises(RuntimeError, match="fp8_e4m3"):
        save_weights(eng.model, str(tmp_path / "ckpt"))
    assert not (tmp_path / "ckpt").exists()


def test_lm_head_and_router_keep_their_dtype():
    spec = ModelSpec(name="tiny-moe-dense-fp8", hidden_size=64, num_layers=2,
                     num_heads=4, num_kv_heads=2, head_dim=16,
                     intermediate_size=0, vocab_size=512, max_context=512,
                     tie_embeddings=False, num_experts=4, experts_per_token=2,
                     moe_intermediate_size=64)
    eng = LLMEngine(_cfg(spec, dense_weight_dtype="fp8_e4m3"))
    assert eng.model.lm_head.weight.dtype == torch.float32
    for m in eng.model.modules():
        if isinstance(m, Qwen3MoE):
            assert m.router.weight.dtype == torch.float32
            assert not m.experts_fp8 and m.gate_up.dtype == torch.float32
        if isinstance(m, Qwen3Attention):
            assert m.qkv_proj.weight.dtype == F8
            assert m.o_proj.weight.dtype == F8


# ---- closeness to the unquantised model ----

def _prefill_logits(dense):
    eng = LLMEngine(_cfg(tiny_spec_for_tests(), dense_weight_dtype=dense))
    seen = []
    real = eng.model.compute_logits
    eng.model.compute_logits = lambda h: seen.append(real(h)) or seen[-1]
    for p in ("closeness row one", "a second and somewhat longer row",
              "three", "the fourth row of the closeness check"):
        eng.add_request(eng.tokenizer.encode(p),
                        SamplingParams(max_tokens=1, temperature=0.0))
    eng.step()
    assert len(seen) == 1 and seen[0].shape == (4, 512)
    return seen[0].float()


def test_logits_close_to_unquantised_model():
    """Tiny-spec engine, prefill logits of four rows, option on against
    option off (the reference is the unquantised model). Relative error =
    max |diff| / max |reference|."""
    ref = _prefill_logits("bf16")
    got = _prefill_logits("fp8_e4m3")
    rel = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f"dense fp8 vs unquantised logits: relative error {rel:.5f}")
    assert rel > 0                       # the option did change the path
    # measured on CPU at this seed: 0.11226 (eight e4m3 GEMMs of about 0.05
    # each on a 64-wide model); the bound is twice that
    assert rel <= 2 * 0.11226


# ---- engine ----

def _generate(spec, **kw):
    eng = LLMEngine(_cfg(spec, **kw))
    reqs = [eng.add_request(eng.tokenizer.encode(p),
                            SamplingParams(max_tokens=8, temperature=0.7,
                                           seed=11 + i))
            for i, p in enumerate(["dense fp8 row one", "dense fp8 row two"])]
    while eng.has_work():
        eng.step()
    return eng, [list(r.output_token_ids) for r in reqs]


def test_cpu_engine_deterministic():
    eng, a = _generate(tiny_spec_for_tests(), dense_weight_dtype="fp8_e4m3")
    mods = [m for m in eng.model.modules()
            if isinstance(m, (Qwen3Attention, Qwen3MLP))]
    assert len(mods) == 4
    for m in mods:
        lins = ((m.qkv_proj, m.o_proj) if isinstance(m, Qwen3Attention)
                else (m.gate_up_proj, m.down_proj))
        assert all(l.weight.dtype == F8 for l in lins)
    assert all(len(t) > 0 for t in a)
    _, b = _generate(tiny_spec_for_tests(), dense_weight_dtype="fp8_e4m3")
    assert a == b


def test_moe_spec_with_both_switches():
    spec = ModelSpec(name="tiny-moe-both-fp8", hidden_size=64, num_layers=2,
                     num_heads=4, num_kv_heads=2, head_dim=16,
                     intermediate_size=0, vocab_size=512, max_context=512,
                     tie_embeddings=True, num_experts=4, experts_per_token=2,
                     moe_intermediate_size=64)
    eng, toks = _generate(spec, dense_weight_dtype="fp8_e4m3",
                          moe_weight_dtype="fp8_e4m3")
    assert all(len(t) > 0 for t in toks)
    for m in eng.model.modules():
        if isinstance(m, Qwen3MoE):
            assert m.experts_fp8
        if isinstance(m, Qwen3Attention):
            assert m.qkv_proj.weight.dtype == F8


def test_embedding_spec_runs():
    import numpy as np

    spec = ModelSpec(name="tiny-emb-fp8", hidden_size=64, num_layers=2,
                     num_heads=4, num_kv_heads=2, head_dim=16,
                     intermediate_size=128, vocab_size=512, max_context=512,
                     tie_embeddings=True, embedding=True)
    eng = LLMEngine(_cfg(spec, dense_weight_dtype="fp8_e4m3"))
    assert eng.model.layers[0].mlp.down_proj.weight.dtype == F8
    reqs = [eng.add_request(eng.tokenizer.encode(t), SamplingParams())
            for t in ("hello", "another longer text input")]
    while eng.has_work():
        eng.step()
    for r in reqs:
        v = eng.embeddings[r.req_id]
        assert v.shape == (64,)
        assert abs(np.linalg.norm(v) - 1.0) < 1e-5


# ---- registry: pure arithmetic ----

@pytest.mark.parametrize("name", sorted(MODEL_REGISTRY))
def test_registry_projections_qualify(name):
    """At tp = recommended_tp every dense projection has a shape the kernel
    takes: N % 64 == 0 (qkv, o, down) and I % 128 == 0 (gate_up)."""
    spec = MODEL_REGISTRY[name]
    tp = spec.recommended_tp
    h = spec.hidden_size
    heads = spec.num_heads // tp
    kv = max(1, spec.num_kv_heads // tp)
    q_size, kv_size = heads * spec.head_dim, kv * spec.head_dim
    assert ops.linear_fp8_qualifies(q_size + 2 * kv_size, h), "qkv"
    assert ops.linear_fp8_qualifies(h, q_size), "o"
    assert (q_size + 2 * kv_size) % 64 == 0 and h % 64 == 0
    if spec.num_experts == 0:
        inter = spec.intermediate_size // tp
        assert inter % 128 == 0
        assert ops.gate_up_silu_fp8_qualifies(2 * inter, h), "gate_up"
        assert ops.linear_fp8_qualifies(h, inter), "down"
