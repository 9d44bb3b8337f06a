"""torch_ref.moe_route (the statement of csrc/moe_route.hip and its CPU path)
against a plain statement written here, the present torch routing on tie-free
logits, and the moe_routing setting end to end on CPU."""

import pytest
import torch

from sutro_amd.engine.config import EngineConfig
from sutro_amd.models.qwen3 import Qwen3MoE
from sutro_amd.models.registry import ModelSpec
from sutro_amd.ops import torch_ref


def plain_route(logits, k, base, E_l, bm):
    """f64 softmax, top-k by (value desc, index asc), renormalise; layout by
    Python-level stable ordering."""
    T, E = logits.shape
    rows_max = T * k + E_l * bm
    w = torch.zeros(T, k, dtype=torch.float64)
    sel = []
    for t in range(T):
        row = logits[t].double()
        probs = torch.softmax(row, 0)
        top = sorted(range(E), key=lambda e: (-row[e].item(), e))[:k]
        p = torch.stack([probs[e] for e in top])
        w[t] = p / p.sum()
        sel.append(top)
    local = [(sel[t][j] - base, t * k + j) for t in range(T) for j in range(k)
             if 0 <= sel[t][j] - base < E_l]
    counts = [sum(1 for e, _ in local if e == x) for x in range(E_l)]
    padded = [(c + bm - 1) // bm * bm for c in counts]
    pad_off = [sum(padded[:e]) for e in range(E_l + 1)]
    padpos = torch.full((T * k,), rows_max - 1, dtype=torch.long)
    row_tok = torch.full((rows_max,), -1, dtype=torch.int32)
    seen = [0] * E_l
    for e, f in sorted(local):
        padpos[f] = pad_off[e] + seen[e]
        row_tok[pad_off[e] + seen[e]] = f // k
        seen[e] += 1
    for t in range(T):
        for j in range(k):
            if not 0 <= sel[t][j] - base < E_l:
                w[t, j] = 0.0
    return (w, padpos.view(T, k), row_tok,
            torch.tensor([o // bm for o in pad_off], dtype=torch.int32),
            torch.tensor(counts, dtype=torch.int32))


def tie_free(T, E, seed):
    g = torch.Generator().manual_seed(seed)
    vals = torch.linspace(-3.0, 3.0, E)
    return torch.stack([vals[torch.randperm(E, generator=g)]
                        for _ in range(T)])


def check(got, want):
    # weights: f32 exp, k <= 4 adds and a divide, each within an ulp (6e-8)
    # of the f64 statement, plus the rounded logit difference: under 2e-6
    torch.testing.assert_close(got[0].double(), want[0], atol=0, rtol=2e-6)
    for g, w in zip(got[1:], want[1:]):
        assert g.dtype == w.dtype and torch.equal(g, w)


@pytest.mark.parametrize("E,k,base,E_l,bm", [
    (8, 2, 0, 8, 64), (32, 4, 0, 32, 128), (32, 4, 16, 8, 64)])
def test_ref_tie_free_matches_statement_and_torch_routing(E, k, base, E_l, bm):
    T = 97
    logits = tie_free(T, E, seed=E + k)
    got = torch_ref.moe_route(logits, k, base, E_l, bm)
    check(got, plain_route(logits, k, base, E_l, bm))
    # the tensors the present _forward_grouped code builds
    spec = ModelSpec(name="route-ref", hidden_size=16, num_layers=1,
                     num_heads=2, num_kv_heads=1, head_dim=8,
                     intermediate_size=0, vocab_size=64, num_experts=E,
                     experts_per_token=k, moe_intermediate_size=16)
    moe = Qwen3MoE(spec, torch.float32)
    moe.expert_base, moe.experts_per_rank = base, E_l
    rows_max = T * k + E_l * bm
    ws = {"row_tok": torch.empty(rows_max, dtype=torch.int32)}
    w_t, pp_t, row_tok_t, tile_off_t, counts_t = moe._route_torch(logits, ws,
                                                                  bm)
    torch.testing.assert_close(got[0], w_t, atol=0, rtol=2e-6)
    assert torch.equal(got[1], pp_t)
    assert torch.equal(got[2][:rows_max - 1], row_tok_t[:rows_max - 1])
    assert torch.equal(got[3], tile_off_t) and torch.equal(got[4], counts_t)


def test_ref_ties_follow_the_stated_rule():
    g = torch.Generator().manual_seed(7)
    four = torch.tensor([-1.0, 0.0, 0.5, 2.0])
    logits = four[torch.randint(0, 4, (70, 32), generator=g)]
    logits[5] = 0.25                       # an all-equal row
    logits = logits.bfloat16()
    for base, E_l in ((0, 32), (8, 16)):
        check(torch_ref.moe_route(logits, 4, base, E_l, 64),
              plain_route(logits, 4, base, E_l, 64))
    _, idx = torch_ref.moe_route_select(logits, 4)
    assert idx[5].tolist() == [0, 1, 2, 3]


def test_config_validation():
    spec = ModelSpec(name="route-cfg", hidden_size=32, num_layers=1,
                     num_heads=2, num_kv_heads=1, head_dim=16,
                     intermediate_size=64, vocab_size=128)
    assert EngineConfig(spec=spec, device="cpu").moe_routing == "torch"
    assert EngineConfig(spec=spec, device="cpu",
                        moe_routing="fused").moe_routing == "fused"
    with pytest.raises(ValueError, match="moe_routing"):
        EngineConfig(spec=spec, device="cpu", moe_routing="hip")


def test_fused_routing_generates_on_cpu():
    from sutro_amd.engine.engine import LLMEngine
    from sutro_amd.engine.request import SamplingParams

    spec = ModelSpec(name="tiny-moe-route", hidden_size=64, num_layers=2,
                     num_heads=4, num_kv_heads=2, head_dim=16,
                     intermediate_size=0, vocab_size=512, max_context=512,
                     tie_embeddings=True, num_experts=4, experts_per_token=2,
                     moe_intermediate_size=64)
    eng = LLMEngine(EngineConfig(spec=spec, device="cpu", max_model_len=256,
                                 num_kv_blocks=64, max_tokens_per_step=128,
                                 moe_routing="fused"))
    mlp = eng.model.layers[0].mlp
    assert mlp.moe_routing == "fused"
    x = torch.randn(9, 64)
    torch.testing.assert_close(mlp._forward_grouped(x), mlp._forward_loop(x),
                               atol=1e-4, rtol=1e-4)
    outs = eng.generate(["route row one", "route row two"],
                        sampling=SamplingParams(max_tokens=6, temperature=0))
    assert len(outs) == 2 and eng.total_output_tokens > 0
