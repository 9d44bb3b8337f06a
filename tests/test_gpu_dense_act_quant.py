"""The engine with dense_act_quant="fused" on the GPU (the norms emit codes
and scales, csrc/rmsnorm_quant_fp8.hip), under hipGraph decode and eager:
the tokens and logprobs of the separate quantiser pass."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _generate(dense, how, eager=False):
    from sutro_amd.engine.config import EngineConfig
    from sutro_amd.engine.engine import LLMEngine
    from sutro_amd.engine.request import SamplingParams
    from sutro_amd.models.registry import ModelSpec

    # the two-layer spec of tests/test_gpu_dense_fp8_block128.py
    spec = ModelSpec(name="dense-act-quant-gpu", hidden_size=256,
                     num_layers=2, num_heads=4, num_kv_heads=2, head_dim=128,
                     intermediate_size=512, vocab_size=512, max_context=512,
                     tie_embeddings=True)
    eng = LLMEngine(EngineConfig(
        spec=spec, device=DEV, max_model_len=256, num_kv_blocks=128,
        max_tokens_per_step=512, seed=0, dense_weight_dtype=dense,
        dense_act_quant=how, enforce_eager=eager))
    assert (eng.graph_runner is None) == eager
    assert all(layer.dense_act_quant == how for layer in eng.model.layers)
    reqs = [eng.add_request(eng.tokenizer.encode(p),
                            SamplingParams(max_tokens=12, temperature=0.7,
                                           seed=3 + i))
            for i, p in enumerate(["act quant row one", "act quant row two"])]
    while eng.has_work():
        eng.step()
    assert all(r.finish_reason is not None for r in reqs)
    return ([list(r.output_token_ids) for r in reqs],
            [r.cumulative_logprob for r in reqs])


@pytest.mark.parametrize("dense", ["fp8_e4m3", "fp8_block128"])
def test_fused_equals_separate_under_graph_and_eager(dense, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from sutro_amd import ops

    separate = _generate(dense, "separate")
    calls = []
    real = ops.rmsnorm_quant_fp8
    monkeypatch.setattr(ops, "rmsnorm_quant_fp8",
                        lambda *a: calls.append(a[4]) or real(*a))
    fused = _generate(dense, "fused")
    assert calls and set(calls) == {
        "block128" if dense == "fp8_block128" else "rows"}
    assert all(fused[0]) and fused == separate
    assert fused == _generate(dense, "fused", eager=True)
