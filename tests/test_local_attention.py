"""Local attention on the CPU path: sliding-window attention and attention
sinks in the reference op, the config switch and CLI flag, the model and
engine with the switch off and on, the shared-prefix fallback, the loader and
TP sharding of the sinks."""

import dataclasses
import math
import multiprocessing as mp
import os
import warnings

import pytest
import torch

from sutro_amd import ops
from sutro_amd.engine.config import EngineConfig
from sutro_amd.engine.engine import LLMEngine
from sutro_amd.engine.request import SamplingParams
from sutro_amd.models.qwen3 import Qwen3Model
from sutro_amd.models.registry import (MODEL_REGISTRY, ModelSpec,
                                       get_model_spec, tiny_spec_for_tests)
from sutro_amd.ops import torch_ref as R

BS = 32


# ---- the reference op against a dense statement ----

def _paged_case(seq_lens, new_counts, hq, hk, d=16, seed=0):
    """Scattered paged cache holding `seq_lens` positions per sequence, and
    the q rows of each one's last `new_counts` positions."""
    g = torch.Generator().manual_seed(seed)
    nblk = [(L + BS - 1) // BS for L in seq_lens]
    total = sum(nblk) + 2
    perm = torch.randperm(total, generator=g).tolist()
    kc = torch.randn(total, hk, BS, d, generator=g)
    vc = torch.randn(total, hk, BS, d, generator=g)
    bt = torch.zeros(len(seq_lens), max(nblk), dtype=torch.int32)
    i = 0
    for s, n in enumerate(nblk):
        bt[s, :n] = torch.tensor(perm[i:i + n], dtype=torch.int32)
        i += n
    q = torch.randn(sum(new_counts), hq, d, generator=g)
    qlocs = torch.tensor([0] + torch.tensor(new_counts).cumsum(0).tolist(),
                         dtype=torch.int32)
    sl = torch.tensor(seq_lens, dtype=torch.int32)
    return q, kc, vc, bt, sl, qlocs


def _dense_attention(q, kc, vc, bt, sl, qlocs, scale, window, sinks):
    """The semantics written out once more, one (sequence, head) at a time:
    gather K/V to [L, D], band mask, the sink as an extra logit column,
    softmax, drop the column, times V."""
    hq, hk = q.shape[1], kc.shape[1]
    out = torch.empty_like(q)
    for s in range(sl.numel()):
        L = int(sl[s])
        q0, q1 = int(qlocs[s]), int(qlocs[s + 1])
        nq = q1 - q0
        pages = bt[s, :(L + BS - 1) // BS].long()
        for h in range(hq):
            kh = h // (hq // hk)
            K = kc[pages, kh].reshape(-1, kc.shape[-1])[:L]
            V = vc[pages, kh].reshape(-1, vc.shape[-1])[:L]
            i = torch.arange(L - nq, L).unsqueeze(1)
            j = torch.arange(L).unsqueeze(0)
            vis = j <= i
            if window > 0:
                vis = vis & (j > i - window)
            logits = (q[q0:q1, h] @ K.T) * scale
            logits = logits.masked_fill(~vis, float("-inf"))
            if sinks is not None:
                col = sinks[h].expand(nq, 1)
                p = torch.softmax(torch.cat([logits, col], 1), 1)[:, :L]
            else:
                p = torch.softmax(logits, 1)
            out[q0:q1, h] = p @ V
    return out


@pytest.mark.parametrize("hq,hk", [(2, 2), (4, 2), (8, 1)])
@pytest.mark.parametrize("window", [1, 5, 32, 33, 70, 77])
def test_reference_matches_dense_statement(window, hq, hk):
    # L = 70: a decode row, a whole-prompt prefill, two chunks with ctx > 0
    seq_lens, new_counts = [70, 70, 70, 70], [1, 70, 37, 5]
    q, kc, vc, bt, sl, ql = _paged_case(seq_lens, new_counts, hq, hk)
    scale = 1.0 / math.sqrt(q.shape[-1])
    for sinks in (None, torch.randn(hq, generator=torch.Generator()
                                    .manual_seed(1))):
        got = R.paged_attention(q, kc, vc, bt, sl, ql, scale, window=window,
                                sinks=sinks)
        ref = _dense_attention(q, kc, vc, bt, sl, ql, scale, window, sinks)
        assert torch.allclose(got, ref, atol=1e-5, rtol=0), (
            (got - ref).abs().max())
    if window >= 70:   # W >= L is no window
        full = R.paged_attention(q, kc, vc, bt, sl, ql, scale)
        win = R.paged_attention(q, kc, vc, bt, sl, ql, scale, window=window)
        assert torch.allclose(full, win, atol=1e-5, rtol=0)


def test_neutral_values_change_nothing():
    q, kc, vc, bt, sl, ql = _paged_case([70, 33, 9], [1, 33, 4], 4, 2)
    plain = R.paged_attention(q, kc, vc, bt, sl, ql, 0.25)
    assert torch.equal(plain, R.paged_attention(q, kc, vc, bt, sl, ql, 0.25,
                                                window=0, sinks=None))
    assert torch.equal(plain, ops.paged_attention(q, kc, vc, bt, sl, ql, 0.25,
                                                  window=0, sinks=None))
    assert torch.equal(plain, ops.paged_attention(q, kc, vc, bt, sl, ql, 0.25))


def test_ops_passes_window_and_sinks_through():
    q, kc, vc, bt, sl, ql = _paged_case([70, 33], [1, 33], 4, 2)
    sinks = torch.tensor([0.5, -1.0, 2.0, 0.0])
    assert torch.equal(
        ops.paged_attention(q, kc, vc, bt, sl, ql, 0.25, window=7,
                            sinks=sinks),
        R.paged_attention(q, kc, vc, bt, sl, ql, 0.25, window=7, sinks=sinks))
    with pytest.raises(ValueError):
        R.paged_attention(q, kc, vc, bt, sl, ql, 0.25, window=-1)
    with pytest.raises(ValueError):
        R.paged_attention(q, kc, vc, bt, sl, ql, 0.25, sinks=sinks[:3])


def test_sink_sanity():
    q, kc, vc, bt, sl, ql = _paged_case([70, 40], [1, 40], 4, 2)
    scale = 1.0 / math.sqrt(q.shape[-1])   # unit-scale scores
    plain = R.paged_attention(q, kc, vc, bt, sl, ql, scale, window=9)
    low = R.paged_attention(q, kc, vc, bt, sl, ql, scale, window=9,
                            sinks=torch.full((4,), -1e4))
    assert torch.allclose(plain, low, atol=1e-6, rtol=0)
    high = R.paged_attention(q, kc, vc, bt, sl, ql, scale, window=9,
                             sinks=torch.full((4,), 30.0))
    assert torch.isfinite(high).all()
    # every weight is at most exp(s - 30) with s of order 1
    assert high.abs().max() < 1e-6 < plain.abs().max()


# ---- config, CLI, registry ----

def _spec(window=8, pattern=2, sinks=True, **kw):
    return dataclasses.replace(tiny_spec_for_tests(), sliding_window=window,
                               sliding_window_pattern=pattern,
                               attention_sinks=sinks, **kw)


def _cfg(spec, **kw):
    kw.setdefault("max_model_len", 256)
    kw.setdefault("num_kv_blocks", 64)
    kw.setdefault("max_tokens_per_step", 128)
    return EngineConfig(spec=spec, device="cpu", seed=0, **kw)


def test_config_values():
    spec = _spec()
    assert EngineConfig(spec=spec, device="cpu").local_attention is False
    assert _cfg(spec, local_attention=True).local_attention is True
    for bad in ("on", 1, None, "True"):
        with pytest.raises(ValueError):
            _cfg(spec, local_attention=bad)
    # a pattern without a window, or a negative one, cannot be switched on
    for w, p in ((0, 2), (-4, 2), (8, -1)):
        _cfg(_spec(window=w, pattern=p))   # ignored while off
        with pytest.raises(ValueError):
            _cfg(_spec(window=w, pattern=p), local_attention=True)
    # a spec with neither runs as always, switch on or off
    assert _cfg(tiny_spec_for_tests(), local_attention=True).local_attention


def test_layer_pattern():
    s2 = _spec(window=8, pattern=2, num_layers=4)
    assert [s2.layer_window(i) for i in range(4)] == [8, 0, 8, 0]
    s6 = _spec(window=16, pattern=6, num_layers=12)
    assert [s6.layer_window(i) for i in range(12)] == [16] * 5 + [0] + [16] * 5 + [0]
    assert [_spec(pattern=0).layer_window(i) for i in range(2)] == [0, 0]
    assert [_spec(pattern=1).layer_window(i) for i in range(2)] == [0, 0]
    assert not tiny_spec_for_tests().has_local_attention
    assert _spec(window=0, pattern=0).has_local_attention   # sinks alone
    assert not _spec(window=0, pattern=0).has_windowed_layer


def test_registry_specs():
    for name in ("gpt-oss-20b", "gpt-oss-120b", "gpt-oss-20b-thinking",
                 "gpt-oss-120b-no-thinking"):
        s = get_model_spec(name)
        assert (s.sliding_window, s.sliding_window_pattern,
                s.attention_sinks) == (128, 2, True), name
        assert s.layer_window(0) == 128 and s.layer_window(1) == 0
    for name, s in MODEL_REGISTRY.items():
        if not name.startswith("gpt-oss"):
            assert not s.has_local_attention, name


def test_engine_kwargs_reach_the_config():
    from sutro_amd.service.models_map import resolve_engine_config

    cfg = resolve_engine_config("gpt-oss-20b", device="cpu",
                                local_attention=True)
    assert cfg.local_attention is True
    assert cfg.spec.sliding_window == 128 and cfg.spec.attention_sinks
    assert not resolve_engine_config("gpt-oss-20b",
                                     device="cpu").local_attention


def test_cli_serve_has_the_flag(monkeypatch):
    from click.testing import CliRunner

    from sutro_amd import cli as cli_mod
    from sutro_amd.service import http_api

    res = CliRunner().invoke(cli_mod.cli, ["serve", "--help"])
    assert res.exit_code == 0 and "--local-attention" in res.output
    seen = {}
    monkeypatch.setattr(http_api, "run_server", lambda **kw: seen.update(kw))
    res = CliRunner().invoke(cli_mod.cli, ["serve", "--local-attention"])
    assert res.exit_code == 0, res.output
    assert seen["engine_kwargs"] == {"local_attention": True}
    seen.clear()
    assert CliRunner().invoke(cli_mod.cli, ["serve"]).exit_code == 0
    assert seen["engine_kwargs"] is None


def test_prefill_tile_step():
    # Qwen3-32B's layout (G 8, head_dim 128) keeps what it yields today
    today = ops.prefill_tile_step(64, 8, 128)
    assert ops.prefill_tile_step(64, 8, 128, local_attention=False) == today
    assert ops.prefill_tile_step(64, 8, 128, 4096) == today
    # any windowed / sink layer: the reference kernel's 32 rows
    assert ops.prefill_tile_step(64, 8, 128, local_attention=True) == 32
    assert ops.prefill_tile_step(64, 8, 128, 4096, local_attention=True) == 32
    ops.set_attn_prefill("pipe,64")
    try:
        assert ops.prefill_tile_step(64, 8, 128) == 64
        assert ops.prefill_tile_step(64, 8, 128, local_attention=True) == 32
    finally:
        ops.set_attn_prefill(None)
    on = LLMEngine(_cfg(_spec(), local_attention=True))
    off = LLMEngine(_cfg(_spec()))
    assert on.local_attention and not off.local_attention
    assert not LLMEngine(_cfg(tiny_spec_for_tests(),
                              local_attention=True)).local_attention


# ---- engine ----

PROMPTS = [list(range(3, 3 + n)) for n in (5, 23, 40)]


def _generate(eng, prompts=PROMPTS, max_tokens=10, temperature=0.8):
    reqs = [eng.add_request(list(p), SamplingParams(
        max_tokens=max_tokens, temperature=temperature, seed=11 + i))
        for i, p in enumerate(prompts)]
    for _ in range(5000):
        if not eng.has_work():
            break
        eng.step()
    assert all(r.finished for r in reqs)
    return ([list(r.output_token_ids) for r in reqs],
            [r.cumulative_logprob for r in reqs], reqs)


def _set_sinks(eng, value):
    n = 0
    with torch.no_grad():
        for name, p in eng.model.named_parameters():
            if name.endswith(".sinks"):
                p.fill_(value)
                n += 1
    return n


def test_switch_off_changes_nothing():
    plain = LLMEngine(_cfg(tiny_spec_for_tests()))
    off = LLMEngine(_cfg(_spec()))
    assert not any("sinks" in k for k in off.model.state_dict())
    assert list(off.model.state_dict()) == list(plain.model.state_dict())
    assert all(layer.self_attn.window == 0 and layer.self_attn.sinks is None
               for layer in off.model.layers)
    toks_p, lps_p, _ = _generate(plain)
    toks_o, lps_o, _ = _generate(off)
    assert toks_p == toks_o and lps_p == lps_o


def test_switch_on_builds_windows_and_sinks():
    eng = LLMEngine(_cfg(_spec(), local_attention=True))
    attn = [layer.self_attn for layer in eng.model.layers]
    assert [a.window for a in attn] == [8, 0]
    for a in attn:
        assert a.sinks.dtype == torch.float32 and a.sinks.shape == (4,)
        # drawn by the per-name generator, not the norm weights' ones
        assert a.sinks.std() > 0.1
    assert not torch.equal(attn[0].sinks, attn[1].sinks)
    again = LLMEngine(_cfg(_spec(), local_attention=True))
    assert torch.equal(again.model.layers[0].self_attn.sinks, attn[0].sinks)
    # the other weights do not move
    off = LLMEngine(_cfg(_spec()))
    sd_on, sd_off = eng.model.state_dict(), off.model.state_dict()
    assert set(sd_on) - set(sd_off) == {"layers.0.self_attn.sinks",
                                        "layers.1.self_attn.sinks"}
    assert all(torch.equal(sd_on[k], v) for k, v in sd_off.items())


def test_window_wider_than_the_row_and_no_sink_is_the_old_model():
    """Rows that never outgrow W with a sink of -1e4 (weight exp(-1e4) = 0):
    the switch-off tokens."""
    spec = _spec(window=64)
    short = [p for p in PROMPTS]            # <= 40 + 10 tokens < 64
    off = _generate(LLMEngine(_cfg(spec)), short)
    on_eng = LLMEngine(_cfg(spec, local_attention=True))
    assert _set_sinks(on_eng, -1e4) == 2
    on = _generate(on_eng, short)
    assert on[0] == off[0]
    assert on[1] == pytest.approx(off[1], abs=1e-4)


def _layer_attn_outputs(eng, prompt):
    """Outputs of every layer's attention block for one whole-prompt prefill."""
    seen = {}
    hooks = [layer.self_attn.register_forward_hook(
        lambda m, a, out, i=i: seen.setdefault(i, out.detach().clone()))
        for i, layer in enumerate(eng.model.layers)]
    eng.add_request(list(prompt), SamplingParams(max_tokens=1, temperature=0))
    eng.step()
    for h in hooks:
        h.remove()
    return seen


def test_window_changes_the_windowed_layer_past_w():
    spec, prompt = _spec(window=8), list(range(3, 3 + 40))
    off = _layer_attn_outputs(LLMEngine(_cfg(spec)), prompt)
    on_eng = LLMEngine(_cfg(spec, local_attention=True))
    _set_sinks(on_eng, -1e4)
    on = _layer_attn_outputs(on_eng, prompt)
    assert off[0].shape == on[0].shape == (40, spec.hidden_size)
    # layer 0 is windowed: positions 0..7 see the same keys, later ones fewer
    assert torch.allclose(on[0][:8], off[0][:8], atol=1e-5, rtol=0)
    diff = (on[0][8:] - off[0][8:]).abs().amax(dim=1)
    assert (diff > 1e-4).all(), diff
    # layer 1 is full attention; its input already differs past W, not before
    assert torch.allclose(on[1][:8], off[1][:8], atol=1e-5, rtol=0)


def test_sinks_change_every_layer():
    spec, prompt = _spec(window=0, pattern=0), list(range(3, 3 + 12))
    off = _layer_attn_outputs(LLMEngine(_cfg(spec)), prompt)
    on = _layer_attn_outputs(LLMEngine(_cfg(spec, local_attention=True)),
                             prompt)
    assert (on[0] - off[0]).abs().max() > 1e-4


def test_chunked_prefill_matches_unchunked():
    spec = _spec(window=8)
    prompts = [list(range(3, 3 + 50)), list(range(9, 9 + 21))]
    whole = _generate(LLMEngine(_cfg(spec, local_attention=True)), prompts,
                      temperature=0)
    eng = LLMEngine(_cfg(spec, local_attention=True, max_tokens_per_step=16,
                         min_prefill_batch_tokens=0))
    req = eng.add_request(list(prompts[0]), SamplingParams(max_tokens=1))
    eng.step()
    assert req.num_computed_tokens == 16      # it does chunk
    eng.abort_request(req)
    while eng.has_work():
        eng.step()
    chunked = _generate(eng, prompts, temperature=0)
    assert chunked[0] == whole[0]
    assert chunked[1] == whole[1]


def test_preemption_matches_roomy_run():
    spec = _spec(window=8)

    def run(num_blocks):
        eng = LLMEngine(_cfg(spec, local_attention=True, max_num_seqs=8,
                             max_model_len=512, min_prefill_batch_tokens=0,
                             num_kv_blocks=num_blocks))
        prompts = [list(range(3, 3 + 40 + i)) for i in range(6)]
        toks, lps, reqs = _generate(eng, prompts, max_tokens=24,
                                    temperature=0.9)
        return toks, lps, sum(r.alloc_gen for r in reqs)

    tight_t, tight_l, n_preempt = run(8)
    roomy_t, roomy_l, _ = run(256)
    assert n_preempt > 0, "the tight run must preempt"
    assert tight_t == roomy_t
    # The tokens are exact. The cumulative logprobs are not bit-equal, with
    # the switch off either: a preempted row is recomputed in a batch of
    # another shape, and the f32 GEMMs sum in a shape-dependent order
    # (measured 1e-6..3e-6 here, the same on the parent). Bound: 24 tokens,
    # each logprob a few f32 roundings of logits of magnitude < 16
    # (ulp 2e-6), so 24 * 1e-5.
    assert tight_l == pytest.approx(roomy_l, abs=2.4e-4)


def test_shared_prefix_decode_falls_back():
    spec = _spec(window=8)
    kw = dict(local_attention=True, enable_prefix_caching=True)
    with pytest.warns(UserWarning, match="local attention"):
        shared = LLMEngine(_cfg(spec, prefix_decode="shared", **kw))
    assert shared.prefix_shared is False
    assert "per_row" in shared.prefix_decode_fallback
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        per_row = LLMEngine(_cfg(spec, prefix_decode="per_row", **kw))
        # with the switch off the spec's window does not trigger the fallback
        quiet = LLMEngine(_cfg(spec, prefix_decode="shared",
                               enable_prefix_caching=True))
    assert per_row.prefix_decode_fallback is None
    assert quiet.prefix_decode_fallback is None
    head = list(range(3, 3 + 70))              # two full shared blocks
    prompts = [head + [100 + i, 101 + i] for i in range(4)]
    a = _generate(shared, prompts)
    b = _generate(per_row, prompts)
    assert a[0] == b[0] and a[1] == b[1]
    # block-hash reuse itself stays on
    assert shared.cfg.enable_prefix_caching and shared.kv.prefix_caching


# ---- loader, TP ----

def test_save_load_roundtrips_sinks(tmp_path):
    pytest.importorskip("safetensors")
    from sutro_amd.models.loader import load_weights, save_weights

    spec = _spec()
    src = Qwen3Model(spec, torch.float32, 128, local_attention=True)
    src.init_random_weights(5)
    save_weights(src, str(tmp_path))
    dst = Qwen3Model(spec, torch.float32, 128, local_attention=True)
    dst.init_random_weights(6)
    assert not torch.equal(dst.layers[0].self_attn.sinks,
                           src.layers[0].self_attn.sinks)
    load_weights(dst, str(tmp_path))
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v), k

    # the same file into a model built without sinks
    plain = Qwen3Model(spec, torch.float32, 128)
    plain.init_random_weights(7)
    with pytest.raises(ValueError, match="sinks"):
        load_weights(plain, str(tmp_path), strict=True)
    load_weights(plain, str(tmp_path), strict=False)
    assert torch.equal(plain.layers[1].self_attn.o_proj.weight,
                       src.layers[1].self_attn.o_proj.weight)

    # and a file without sinks into a model that has them
    other = tmp_path / "plain"
    save_weights(plain, str(other))
    with pytest.raises(ValueError, match="sinks"):
        load_weights(dst, str(other), strict=True)


def test_load_shards_sinks_with_the_q_heads(tmp_path):
    pytest.importorskip("safetensors")
    from safetensors.torch import save_file

    from sutro_amd.models.loader import load_weights
    from sutro_amd.parallel.tp import TPContext

    spec = _spec()
    full = Qwen3Model(spec, torch.float32, 128, local_attention=True)
    full.init_random_weights(0)
    # the names a gpt-oss checkpoint uses
    state = {"model." + k: v.detach().clone().contiguous()
             for k, v in full.named_parameters()}
    assert "model.layers.0.self_attn.sinks" in state
    save_file(state, str(tmp_path / "model.safetensors"))
    for r in range(2):
        shard = Qwen3Model(spec, torch.float32, 128, TPContext(size=2, rank=r),
                           local_attention=True)
        shard.init_random_weights(0)
        init = shard.layers[0].self_attn.sinks.detach().clone()
        assert torch.equal(init, full.layers[0].self_attn.sinks[2 * r:2 * r + 2])
        with torch.no_grad():
            shard.layers[0].self_attn.sinks.zero_()
        load_weights(shard, str(tmp_path))
        assert torch.equal(shard.layers[0].self_attn.sinks, init)


def _tp_worker(rank, world, port, result_q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist

        dist.init_process_group("gloo", rank=rank, world_size=world)
        eng = LLMEngine(_cfg(_spec(), local_attention=True, tp_size=world))
        result_q.put((rank, _tp_rows(eng)))
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        result_q.put((rank, f"ERROR: {type(e).__name__}: {e}"))


def _tp_rows(eng):
    reqs = [eng.add_request(eng.tokenizer.encode(t),
                            SamplingParams(max_tokens=8, temperature=0))
            for t in ("tensor parallel row with a window", "row b")]
    while eng.has_work():
        eng.step()
    return [list(r.output_token_ids) for r in reqs]


def test_tp2_greedy_matches_tp1_with_sinks():
    ref = _tp_rows(LLMEngine(_cfg(_spec(), local_attention=True)))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, 29561, q))
             for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(2):
        rank, outs = q.get(timeout=300)
        assert not isinstance(outs, str), outs
        results[rank] = outs
    for p in procs:
        p.join(timeout=60)
    assert results[0] == results[1] == ref
