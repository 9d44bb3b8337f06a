"""Block-scaled FP8 dense weights (128x128 weight blocks, 1x128 activation
groups) on the CPU path: the config value and the CLI option, the stated
arithmetic of the quantisers and of the layers, the quantise method, closeness
to the unquantised model, and the loader for pre-quantised checkpoints."""

import json
import os
from dataclasses import replace

import pytest
import torch
import torch.nn.functional as F

from sutro_amd import ops
from sutro_amd.engine.config import EngineConfig
from sutro_amd.engine.engine import LLMEngine
from sutro_amd.engine.request import SamplingParams
from sutro_amd.models import qwen3
from sutro_amd.models.loader import load_weights, save_weights
from sutro_amd.models.qwen3 import (Qwen3Attention, Qwen3MLP, Qwen3Model,
                                    Qwen3MoE)
from sutro_amd.models.registry import ModelSpec, tiny_spec_for_tests
from sutro_amd.ops import torch_ref
from sutro_amd.parallel.tp import TPContext

F8 = torch.float8_e4m3fn
BLOCK = "fp8_block128"


def _spec():
    """Every dense projection is whole 128x128 blocks: qkv [384, 128],
    o [128, 128], gate_up [512, 128], down [128, 256]."""
    return replace(tiny_spec_for_tests(), hidden_size=128, num_heads=4,
                   num_kv_heads=4, head_dim=32, intermediate_size=256)


def _cfg(spec, **kw):
    kw.setdefault("seed", 0)
    return EngineConfig(spec=spec, device="cpu", max_model_len=256,
                        num_kv_blocks=64, max_tokens_per_step=128, **kw)


def _bits(t):
    return t.view(torch.uint8) if t.dtype == F8 else t


# ---- config / CLI ----

def test_config_values():
    spec = tiny_spec_for_tests()
    assert _cfg(spec, dense_weight_dtype=BLOCK).dense_weight_dtype == BLOCK
    assert _cfg(spec, dense_weight_dtype="fp8_e4m3").dense_weight_dtype \
        == "fp8_e4m3"
    for bad in ("fp8", "int8", "", "fp8_block", "mxfp4"):
        with pytest.raises(ValueError):
            _cfg(spec, dense_weight_dtype=bad)


def test_engine_kwargs_reach_the_config():
    from sutro_amd.service.models_map import resolve_engine_config

    cfg = resolve_engine_config("qwen-3-0.6b", device="cpu",
                                dense_weight_dtype=BLOCK)
    assert cfg.dense_weight_dtype == BLOCK


def test_cli_serve_carries_the_value(monkeypatch):
    from click.testing import CliRunner

    from sutro_amd import cli as cli_mod
    from sutro_amd.service import http_api

    seen = {}
    monkeypatch.setattr(http_api, "run_server",
                        lambda **kw: seen.update(kw))
    res = CliRunner().invoke(cli_mod.cli,
                             ["serve", "--dense-weight-dtype", BLOCK])
    assert res.exit_code == 0, res.output
    assert seen["engine_kwargs"] == {"dense_weight_dtype": BLOCK}
    res = CliRunner().invoke(cli_mod.cli,
                             ["serve", "--dense-weight-dtype", "fp8"])
    assert res.exit_code != 0


# ---- the stated arithmetic ----

def _e4m3(x):
    return x.to(F8).float()


def test_row_quantiser_on_a_hand_built_input():
    """Three groups in a row: all zero, amax exactly 448, and an ordinary
    one; the scales come out K-block-major."""
    x = torch.zeros(2, 384)
    x[0, 128:256] = torch.linspace(-448.0, 440.0, 128)     # amax == 448
    x[0, 256:] = torch.linspace(-1.0, 3.0, 128)
    x[1, :128] = 0.5
    x[1, 300] = -7.0
    q, s = torch_ref.quantize_rows_fp8_block128(x)
    assert q.shape == (2, 384) and q.dtype == F8
    assert s.shape == (3, 2) and s.dtype == torch.float32
    three = torch.tensor(3.0) / torch.tensor(448.0)
    seven = torch.tensor(7.0) / torch.tensor(448.0)
    half = torch.tensor(0.5) / torch.tensor(448.0)
    assert torch.equal(s, torch.stack([
        torch.stack([torch.tensor(1.0), half]),             # zero group -> 1
        torch.stack([torch.tensor(1.0), torch.tensor(1.0)]),  # 448 / 448
        torch.stack([three, seven])]))
    qf = q.float()
    assert torch.equal(qf[0, :128], torch.zeros(128))
    # scale 1: the codes are the e4m3 roundings of the values themselves
    assert torch.equal(qf[0, 128:256], _e4m3(x[0, 128:256]))
    assert qf[0, 128] == -448.0
    assert torch.equal(qf[0, 256:], _e4m3((x[0, 256:] / three)
                                          .clamp(-448.0, 448.0)))
    assert qf[0, 383] == 448.0
    assert torch.equal(qf[1, :128], torch.full((128,), 448.0))
    assert torch.equal(qf[1, 128:256], torch.zeros(128))
    assert qf[1, 300] == -448.0 and qf[1, 256:].abs().sum() == 448.0
    # the op states the same thing on CPU
    q2, s2 = ops.quantize_rows_fp8_block128(x)
    assert torch.equal(_bits(q2), _bits(q)) and torch.equal(s2, s)
    with pytest.raises(ValueError):
        torch_ref.quantize_rows_fp8_block128(torch.zeros(2, 192))


def test_weight_quantiser_on_a_hand_built_input():
    """2 x 2 blocks: all zero, amax exactly 448, and two ordinary ones whose
    maxima sit in different rows and columns of the block."""
    w = torch.zeros(256, 256)
    w[:128, 128:] = torch.linspace(-448.0, 100.0, 128 * 128).view(128, 128)
    w[128:, :128] = torch.linspace(-2.0, 1.0, 128 * 128).view(128, 128).t()
    w[200, 130] = 5.0
    q, s = torch_ref.quantize_weight_fp8_block128(w)
    assert q.shape == (256, 256) and q.dtype == F8 and s.shape == (2, 2)
    two = torch.tensor(2.0) / torch.tensor(448.0)
    five = torch.tensor(5.0) / torch.tensor(448.0)
    assert torch.equal(s, torch.stack([
        torch.stack([torch.tensor(1.0), torch.tensor(1.0)]),
        torch.stack([two, five])]))
    qf = q.float()
    assert torch.equal(qf[:128, :128], torch.zeros(128, 128))
    assert torch.equal(qf[:128, 128:], _e4m3(w[:128, 128:]))
    assert torch.equal(qf[128:, :128],
                       _e4m3((w[128:, :128] / two).clamp(-448.0, 448.0)))
    assert qf[200, 130] == 448.0
    assert qf[128:, 128:].abs().sum() == 448.0
    with pytest.raises(ValueError):
        torch_ref.quantize_weight_fp8_block128(torch.zeros(192, 128))


def test_quantisers_reproduce_the_input_within_half_an_ulp():
    """code * scale is within e4m3's half-ulp of the group maximum: the
    largest binade [256, 448] has ulp 32, so |err| <= 16 * scale =
    amax / 28."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(33, 384, generator=g) * torch.logspace(-3, 2, 33)[:, None]
    q, s = torch_ref.quantize_rows_fp8_block128(x)
    deq = q.float().view(33, 3, 128) * s.t()[:, :, None]
    amax = x.view(33, 3, 128).abs().amax(dim=2, keepdim=True)
    slack = 1 + 2.0 ** -20     # the f32 roundings of this check itself
    assert ((deq - x.view(33, 3, 128)).abs() <= amax / 28 * slack).all()
    assert (q.float().view(33, 3, 128).abs().amax(dim=2) == 448).all()

    w = torch.randn(256, 384, generator=g) * 0.05
    wq, ws = torch_ref.quantize_weight_fp8_block128(w)
    deq = wq.float().view(2, 128, 3, 128) * ws[:, None, :, None]
    wb = w.view(2, 128, 3, 128)
    amax = wb.abs().amax(dim=(1, 3), keepdim=True)
    assert ((deq - wb).abs() <= amax / 28 * slack).all()
    assert (wq.float().view(2, 128, 3, 128).abs().amax(dim=(1, 3))
            == 448).all()


def _block_linear_f64(a_q, a_s, w_q, w_s):
    """The formula of torch_ref.fp8_block_linear, evaluated in f64."""
    a, w = a_q.double(), w_q.double()
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float64)
    for kb in range(a.shape[1] // 128):
        ks = slice(kb * 128, (kb + 1) * 128)
        f = (a_s[kb].double()[:, None]
             * w_s[:, kb].double().repeat_interleave(128)[None, :])
        acc += (a[:, ks] @ w[:, ks].T) * f
    return acc


def test_block_linear_equals_its_f64_evaluation():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(19, 640, generator=g)
    w = torch.randn(256, 640, generator=g) / 640 ** 0.5
    a_q, a_s = torch_ref.quantize_rows_fp8_block128(x)
    w_q, w_s = torch_ref.quantize_weight_fp8_block128(w)
    got = torch_ref.fp8_block_linear(a_q, a_s, w_q, w_s)
    ref = _block_linear_f64(a_q, a_s, w_q, w_s)
    assert got.dtype == torch.float32 and got.shape == (19, 256)
    assert ref.abs().max() > 1
    # f32 rounding only. The standard bound of a length-n f32 sum of
    # products, n * 2^-24 * sum |terms|, with n = 128 products + 5 fold-ins
    # + the factor product and the scaling multiply of each K group
    sum_abs = _block_linear_f64(a_q.float().abs(), a_s, w_q.float().abs(),
                                w_s)
    assert ((got.double() - ref).abs() <= 140 * 2.0 ** -24 * sum_abs).all()


# ---- model: the stated sequence ----

def test_mlp_forward_is_the_stated_sequence():
    torch.manual_seed(0)
    mlp = Qwen3MLP(128, 256, torch.float32)
    for p in mlp.parameters():
        torch.nn.init.normal_(p, std=0.05)
    w_gu = mlp.gate_up_proj.weight.data.clone()
    w_dn = mlp.down_proj.weight.data.clone()
    mlp.quantize_dense_fp8_block128()
    gu_q, gu_s = torch_ref.quantize_weight_fp8_block128(w_gu)
    dn_q, dn_s = torch_ref.quantize_weight_fp8_block128(w_dn)
    assert torch.equal(_bits(mlp.gate_up_proj.weight), _bits(gu_q))
    assert torch.equal(mlp.gate_up_proj.weight_scale_inv, gu_s)
    assert gu_s.shape == (4, 1) and dn_s.shape == (1, 2)
    assert not hasattr(mlp.gate_up_proj, "weight_scale")

    x = torch.randn(37, 128) * 0.5
    x_q, x_s = torch_ref.quantize_rows_fp8_block128(x)
    y = torch_ref.fp8_block_linear(x_q, x_s, gu_q, gu_s)
    act = (F.silu(y[:, :256]) * y[:, 256:]).to(x.dtype)
    a_q, a_s = torch_ref.quantize_rows_fp8_block128(act)
    want = torch_ref.fp8_block_linear(a_q, a_s, dn_q, dn_s).to(x.dtype)
    got = mlp(x)
    assert want.abs().max() > 0
    assert torch.equal(got, want)
    assert torch.equal(ops.gate_up_silu_fp8_block128(x, gu_q, gu_s), act)
    res = torch.randn(37, 128)
    want_res = (torch_ref.fp8_block_linear(a_q, a_s, dn_q, dn_s)
                + res).to(x.dtype)
    assert torch.equal(
        ops.linear_fp8_block128(act, dn_q, dn_s, residual=res), want_res)


def test_attention_projections_are_the_stated_sequence():
    torch.manual_seed(1)
    attn = Qwen3Attention(_spec(), torch.float32, 0)
    for p in attn.parameters():
        torch.nn.init.normal_(p, std=0.1)
    weights = {n: getattr(attn, n).weight.data.clone()
               for n in ("qkv_proj", "o_proj")}
    attn.quantize_dense_fp8_block128()
    for name, w in weights.items():
        lin = getattr(attn, name)
        assert lin.weight.dtype == F8 and lin.weight_scale_inv is not None
        x = torch.randn(19, w.shape[1])
        w_q, w_s = torch_ref.quantize_weight_fp8_block128(w)
        x_q, x_s = torch_ref.quantize_rows_fp8_block128(x)
        want = torch_ref.fp8_block_linear(x_q, x_s, w_q, w_s).to(x.dtype)
        got = qwen3._dense_linear(lin, x)
        assert got.shape == (19, w.shape[0]) and want.abs().max() > 0
        assert torch.equal(got, want), name


# ---- the quantise method ----

def test_quantize_method_is_idempotent_and_frees_the_weight():
    model = LLMEngine(_cfg(_spec())).model
    before = {n: t.dtype for n, t in model.state_dict().items()}
    model.quantize_dense_fp8_block128()
    snap = {n: t.clone() for n, t in model.state_dict().items()}
    model.quantize_dense_fp8_block128()
    after = model.state_dict()
    assert set(after) == set(snap)
    for n, t in after.items():
        assert t.dtype == snap[n].dtype
        assert torch.equal(_bits(t), _bits(snap[n])), n
    shapes = {"self_attn.qkv_proj": (384, 128), "self_attn.o_proj": (128, 128),
              "mlp.gate_up_proj": (512, 128), "mlp.down_proj": (128, 256)}
    names = {n for n, _ in model.named_parameters()}
    for i in range(2):
        for name, (N, K) in shapes.items():
            w = after[f"layers.{i}.{name}.weight"]
            s = after[f"layers.{i}.{name}.weight_scale_inv"]
            assert w.dtype == F8 and w.shape == (N, K), name
            assert s.dtype == torch.float32
            assert s.shape == (N // 128, K // 128), name
            # the unquantised parameter is gone
            assert f"layers.{i}.{name}.weight" not in names
    for n, dt in before.items():
        if "_proj" not in n:
            assert after[n].dtype == dt, n


def test_quantize_refuses_foreign_storage():
    mlp = Qwen3MLP(128, 256, torch.float32)
    lin = mlp.down_proj
    w = lin.weight.data
    del lin._parameters["weight"]
    lin.register_buffer("weight", torch.zeros(w.shape, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        mlp.quantize_dense_fp8_block128()


def test_lm_head_and_router_keep_their_dtype():
    spec = ModelSpec(name="tiny-moe-dense-fp8-block", hidden_size=128,
                     num_layers=2, num_heads=4, num_kv_heads=4, head_dim=32,
                     intermediate_size=0, vocab_size=512, max_context=512,
                     tie_embeddings=False, num_experts=4, experts_per_token=2,
                     moe_intermediate_size=64)
    eng = LLMEngine(_cfg(spec, dense_weight_dtype=BLOCK))
    assert eng.model.lm_head.weight.dtype == torch.float32
    assert not hasattr(eng.model.lm_head, "weight_scale_inv")
    for m in eng.model.modules():
        if isinstance(m, Qwen3MoE):
            assert m.router.weight.dtype == torch.float32
            assert not m.experts_fp8 and m.gate_up.dtype == torch.float32
        if isinstance(m, Qwen3Attention):
            assert m.qkv_proj.weight.dtype == F8
            assert m.o_proj.weight_scale_inv.shape == (1, 1)


def test_projections_that_do_not_qualify_stay_as_they_are():
    """tiny_spec_for_tests() has hidden 64: nothing is a whole block."""
    eng = LLMEngine(_cfg(tiny_spec_for_tests(), dense_weight_dtype=BLOCK))
    for m in eng.model.modules():
        if isinstance(m, torch.nn.Linear):
            assert m.weight.dtype == torch.float32
            assert not hasattr(m, "weight_scale_inv")
    req = eng.add_request(eng.tokenizer.encode("still runs"),
                          SamplingParams(max_tokens=4, temperature=0.0))
    while eng.has_work():
        eng.step()
    assert len(req.output_token_ids) > 0


# ---- closeness to the unquantised model ----

def _prefill_logits(dense):
    eng = LLMEngine(_cfg(_spec(), dense_weight_dtype=dense))
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
    """Prefill logits of four rows, option on against option off (the
    reference is the unquantised model). Relative error = max |diff| /
    max |reference|."""
    ref = _prefill_logits("bf16")
    got = _prefill_logits(BLOCK)
    chan = _prefill_logits("fp8_e4m3")
    rel = ((got - ref).abs().max() / ref.abs().max()).item()
    rel_chan = ((chan - ref).abs().max() / ref.abs().max()).item()
    print(f"dense fp8 vs unquantised logits on the 128-wide spec: "
          f"block128 {rel:.5f}, per-channel {rel_chan:.5f}")
    assert rel > 0                       # the option did change the path
    # measured on CPU at this seed: 0.12073 (per-channel on the same spec:
    # 0.21073); the bound is twice the measured value
    assert rel <= 2 * 0.12073


# ---- loader ----

def _quantised_model(seed=0):
    eng = LLMEngine(_cfg(_spec(), dense_weight_dtype=BLOCK, seed=seed))
    return eng.model


def _fresh_model(tp=None):
    return Qwen3Model(_spec(), torch.float32, 256, tp or TPContext())


def _proj_buffers(model):
    return {n: t for n, t in model.state_dict().items() if "_proj" in n}


def test_save_and_reload_is_bit_equal(tmp_path):
    src = _quantised_model()
    path = str(tmp_path / "ckpt")
    save_weights(src, path)
    dst = _fresh_model()
    with pytest.raises(ValueError, match="fp8_block128"):
        load_weights(_fresh_model(), path)               # default: bf16
    n = load_weights(dst, path, dense_weight_dtype=BLOCK)
    assert n > 0
    a, b = _proj_buffers(src), _proj_buffers(dst)
    assert set(a) == set(b) and len(a) == 16
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(_bits(a[k]),
                                                        _bits(b[k])), k
    # nothing unquantised is left on the projections, and the rest loaded
    assert not any("_proj" in n for n, _ in dst.named_parameters())
    for k, v in src.state_dict().items():
        assert torch.equal(_bits(v), _bits(dst.state_dict()[k])), k
    dst.quantize_dense_fp8_block128()                    # a no-op
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(_proj_buffers(dst)[k])), k


def _split_state(model):
    """The model's tensors under the published split HF names."""
    out = {}
    for k, v in model.state_dict().items():
        v = v.detach().clone()
        hk = "lm_head.weight" if k == "lm_head.weight" else "model." + k
        base, leaf = hk.rsplit(".", 1)
        if base.endswith("qkv_proj"):
            pre = base[: -len("qkv_proj")]
            cut = (128, 128, 128) if leaf == "weight" else (1, 1, 1)
            for nm, t in zip(("q_proj", "k_proj", "v_proj"),
                             v.split(cut, dim=0)):
                out[f"{pre}{nm}.{leaf}"] = t.contiguous()
        elif base.endswith("gate_up_proj"):
            pre = base[: -len("gate_up_proj")]
            for nm, t in zip(("gate_proj", "up_proj"), v.chunk(2, dim=0)):
                out[f"{pre}{nm}.{leaf}"] = t.contiguous()
        else:
            out[hk] = v.contiguous()
    return out


def _write(tmp_path, name, state, config=None):
    from safetensors.torch import save_file

    d = tmp_path / name
    os.makedirs(d)
    save_file(state, str(d / "model.safetensors"))
    if config is not None:
        (d / "config.json").write_text(json.dumps(config))
    return str(d)


GOOD_QC = {"quantization_config": {"quant_method": "fp8", "fmt": "e4m3",
                                   "weight_block_size": [128, 128]}}


def test_split_hf_names_load_to_the_same_buffers(tmp_path):
    src = _quantised_model()
    state = _split_state(src)
    assert "model.layers.1.self_attn.q_proj.weight_scale_inv" in state
    assert state["model.layers.0.mlp.up_proj.weight"].dtype == F8
    path = _write(tmp_path, "split", state, GOOD_QC)
    dst = _fresh_model()
    load_weights(dst, path, dense_weight_dtype=BLOCK)
    a, b = _proj_buffers(src), _proj_buffers(dst)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_tp2_shards_are_slices_of_the_full_tensors(tmp_path):
    """Column-parallel qkv / gate_up cut N/128 per section, row-parallel o /
    down cut K/128. The spec doubles the widths so every half is a block."""
    spec = replace(_spec(), hidden_size=256, num_heads=8, num_kv_heads=8,
                   intermediate_size=512)
    full = Qwen3Model(spec, torch.float32, 256, TPContext())
    full.init_random_weights(3)
    full.quantize_dense_fp8_block128()
    path = str(tmp_path / "ckpt")
    save_weights(full, path)
    fs = full.state_dict()
    for rank in (0, 1):
        shard = Qwen3Model(spec, torch.float32, 256, TPContext(2, rank))
        load_weights(shard, path, dense_weight_dtype=BLOCK)
        ss = shard.state_dict()
        pre = "layers.1."
        # qkv: rows [q | k | v], each section halved
        w, s = fs[pre + "self_attn.qkv_proj.weight"], \
            fs[pre + "self_attn.qkv_proj.weight_scale_inv"]
        rows = torch.cat([torch.arange(o + rank * 128, o + rank * 128 + 128)
                          for o in (0, 256, 512)])
        assert torch.equal(_bits(ss[pre + "self_attn.qkv_proj.weight"]),
                           _bits(w)[rows])
        assert torch.equal(ss[pre + "self_attn.qkv_proj.weight_scale_inv"],
                           s[rows[::128] // 128])
        # gate_up: [gate | up], each halved
        w, s = fs[pre + "mlp.gate_up_proj.weight"], \
            fs[pre + "mlp.gate_up_proj.weight_scale_inv"]
        rows = torch.cat([torch.arange(o + rank * 256, o + rank * 256 + 256)
                          for o in (0, 512)])
        assert torch.equal(_bits(ss[pre + "mlp.gate_up_proj.weight"]),
                           _bits(w)[rows])
        assert torch.equal(ss[pre + "mlp.gate_up_proj.weight_scale_inv"],
                           s[rows[::128] // 128])
        # row-parallel: columns
        for name, kw in (("self_attn.o_proj", 128), ("mlp.down_proj", 256)):
            w, s = fs[pre + name + ".weight"], \
                fs[pre + name + ".weight_scale_inv"]
            cols = slice(rank * kw, (rank + 1) * kw)
            assert torch.equal(_bits(ss[pre + name + ".weight"]),
                               _bits(w)[:, cols]), name
            assert torch.equal(
                ss[pre + name + ".weight_scale_inv"],
                s[:, rank * kw // 128:(rank + 1) * kw // 128]), name


def test_tp_boundary_off_the_block_grid_is_an_error(tmp_path):
    """_spec() at TP=2: o_proj's K shard is 64 wide."""
    path = str(tmp_path / "ckpt")
    save_weights(_quantised_model(), path)
    shard = Qwen3Model(_spec(), torch.float32, 256, TPContext(2, 1))
    with pytest.raises(ValueError, match="_proj.weight"):
        load_weights(shard, path, dense_weight_dtype=BLOCK)


@pytest.mark.parametrize("strict", [True, False])
def test_e4m3_weight_with_another_dtype_is_an_error(tmp_path, strict):
    path = str(tmp_path / "ckpt")
    save_weights(_quantised_model(), path)
    for dense in ("bf16", "fp8_e4m3"):
        with pytest.raises(ValueError, match="fp8_block128"):
            load_weights(_fresh_model(), path, strict=strict,
                         dense_weight_dtype=dense)


def test_incomplete_pairs_and_bad_scales_are_errors(tmp_path):
    state = _split_state(_quantised_model())
    k_scale = "model.layers.0.self_attn.k_proj.weight_scale_inv"
    cases = {}
    s = dict(state); del s[k_scale]
    cases["no_scale"] = s
    s = dict(state); del s["model.layers.0.mlp.down_proj.weight"]
    cases["no_codes"] = s
    s = dict(state); del s["model.layers.1.mlp.up_proj.weight"]
    del s["model.layers.1.mlp.up_proj.weight_scale_inv"]
    cases["no_up_part"] = s
    s = dict(state); s[k_scale] = torch.ones(1, 2)
    cases["scale_shape"] = s
    s = dict(state); s[k_scale] = torch.ones(1, 1, dtype=torch.float16)
    cases["scale_dtype"] = s
    for name, st in cases.items():
        path = _write(tmp_path, name, st)
        with pytest.raises(ValueError):
            load_weights(_fresh_model(), path, dense_weight_dtype=BLOCK)
    # the untouched state loads
    load_weights(_fresh_model(), _write(tmp_path, "good", state),
                 dense_weight_dtype=BLOCK)


@pytest.mark.parametrize("qc", [
    {"quant_method": "fp8", "weight_block_size": [64, 64]},
    {"quant_method": "fp8"},
    {"quant_method": "awq", "weight_block_size": [128, 128]},
    {"quant_method": "mxfp4"},
])
def test_quantization_config_must_match(tmp_path, qc):
    state = _split_state(_quantised_model())
    path = _write(tmp_path, "bad", state, {"quantization_config": qc})
    with pytest.raises(ValueError, match="quantization_config"):
        load_weights(_fresh_model(), path, dense_weight_dtype=BLOCK)
    # a config.json without the entry is fine
    path = _write(tmp_path, "plain", state, {"hidden_size": 128})
    load_weights(_fresh_model(), path, dense_weight_dtype=BLOCK)


def test_save_weights_still_refuses_per_channel(tmp_path):
    eng = LLMEngine(_cfg(_spec(), dense_weight_dtype="fp8_e4m3"))
    with pytest.raises(RuntimeError, match="fp8_e4m3"):
        save_weights(eng.model, str(tmp_path / "ckpt"))


def _generate(**kw):
    eng = LLMEngine(_cfg(_spec(), dense_weight_dtype=BLOCK, **kw))
    reqs = [eng.add_request(eng.tokenizer.encode(p),
                            SamplingParams(max_tokens=8, temperature=0.7,
                                           seed=11 + i))
            for i, p in enumerate(["block fp8 row one", "block fp8 row two"])]
    while eng.has_work():
        eng.step()
    return eng, ([list(r.output_token_ids) for r in reqs],
                 [r.cumulative_logprob for r in reqs])


def test_engine_from_bf16_and_from_quantised_checkpoint_agree(tmp_path):
    """A bf16 checkpoint quantised at start-up and the saved quantised file
    give the same model, hence the same tokens and logprobs."""
    src = LLMEngine(_cfg(_spec(), seed=5))
    bf16_path = str(tmp_path / "bf16")
    save_weights(src.model, bf16_path)
    eng_a, out_a = _generate(weights_path=bf16_path)
    assert eng_a.model.layers[0].mlp.down_proj.weight.dtype == F8
    q_path = str(tmp_path / "fp8")
    save_weights(eng_a.model, q_path)
    eng_b, out_b = _generate(weights_path=q_path)
    assert eng_b.model.layers[1].self_attn.qkv_proj.weight_scale_inv \
        .shape == (3, 1)
    assert all(len(t) > 0 for t in out_a[0])
    assert out_a == out_b
