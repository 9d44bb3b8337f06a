"""Split-KV decode: config, CLI, routing rule and the CPU engine path."""

import warnings

import pytest

from sutro_amd import ops
from sutro_amd.engine.config import EngineConfig
from sutro_amd.engine.engine import LLMEngine
from sutro_amd.engine.request import SamplingParams
from sutro_amd.models.registry import ModelSpec

SPEC = ModelSpec(name="split-cpu", hidden_size=64, num_layers=2, num_heads=4,
                 num_kv_heads=2, head_dim=64, intermediate_size=128,
                 vocab_size=512, max_context=512, tie_embeddings=True)


def _cfg(**kw):
    return EngineConfig(spec=SPEC, device="cpu", max_model_len=256,
                        num_kv_blocks=64, seed=0, **kw)


def test_config_validation():
    assert _cfg().decode_kv_splits == "off"
    assert _cfg(decode_kv_splits="auto").decode_kv_splits == "auto"
    for bad in ("on", 4, None, ""):
        with pytest.raises(ValueError, match="decode_kv_splits"):
            _cfg(decode_kv_splits=bad)


def test_cli_flag_reaches_engine_kwargs(monkeypatch):
    from click.testing import CliRunner

    from sutro_amd import cli as cli_mod
    from sutro_amd.service import http_api
    from sutro_amd.service.models_map import resolve_engine_config

    seen = {}
    monkeypatch.setattr(http_api, "run_server", lambda **kw: seen.update(kw))
    res = CliRunner().invoke(cli_mod.cli, ["serve", "--decode-kv-splits", "auto"])
    assert res.exit_code == 0, res.output
    assert seen["engine_kwargs"] == {"decode_kv_splits": "auto"}
    assert resolve_engine_config("qwen-3-32b", device="cpu",
                                 **seen["engine_kwargs"]).decode_kv_splits == "auto"
    assert CliRunner().invoke(
        cli_mod.cli, ["serve", "--decode-kv-splits", "4"]).exit_code != 0


def test_rule_is_off_at_the_operating_point_bounded_and_monotone():
    s_max = ops.DECODE_SPLIT_RULE["s_max"]
    assert s_max <= ops.DECODE_SPLIT_S_MAX == 16
    for hk in (1, 2, 8):
        for pages in (1, 32, 256, 1024):
            assert ops.decode_kv_splits(2048, hk, pages) == 1
            got = [ops.decode_kv_splits(n, hk, pages) for n in range(1, 2100)]
            assert all(1 <= s <= s_max for s in got)
            assert all(a >= b for a, b in zip(got, got[1:]))
    # the force switch: off, a fixed S, and S = 1 still routing (> 1)
    try:
        ops.set_decode_kv_splits("off")
        assert ops.decode_kv_splits(1, 8, 1024) == 1
        ops.set_decode_kv_splits(4)
        assert ops.decode_kv_splits(2048, 8, 1) == 4
        ops.set_decode_kv_splits("1")
        assert ops.decode_kv_splits(1, 8, 1024) == 2
        with pytest.raises(ValueError):
            ops.set_decode_kv_splits(17)
    finally:
        ops.set_decode_kv_splits(None)


def _generate(**kw):
    eng = LLMEngine(_cfg(**kw))
    reqs = [eng.add_request(list(range(5 + i, 5 + i + n)),
                            SamplingParams(max_tokens=6, temperature=0.7,
                                           seed=i))
            for i, n in enumerate((3, 40, 150))]
    while eng.has_work():
        eng.step()
    return eng, [list(r.output_token_ids) for r in reqs]


def test_cpu_engine_auto_equals_off():
    eng, toks = _generate(decode_kv_splits="auto")
    assert eng.decode_split and eng.decode_kv_splits_fallback is None
    assert toks == _generate()[1]


def test_shared_prefix_decode_keeps_splitting_off():
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        eng = LLMEngine(_cfg(decode_kv_splits="auto", prefix_decode="shared",
                             enable_prefix_caching=True))
    assert not eng.decode_split
    assert "prefix_decode='shared'" in eng.decode_kv_splits_fallback
    assert any("decode_kv_splits" in str(w.message) for w in caught)
