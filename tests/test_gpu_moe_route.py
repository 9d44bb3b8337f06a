"""The fused MoE routing kernels (csrc/moe_route.hip) against
torch_ref.moe_route on the same logits: integer outputs and the selection bit
for bit, weights against an f64 statement with the present f32 torch routing
as the yardstick; determinism, hipGraph replay, the layer and the engine.
A block owns 128 tokens: T = 129 is one token past a block, 4100 spans 33."""

import pytest
import torch

from sutro_amd import ops
from sutro_amd.engine.config import EngineConfig
from sutro_amd.engine.engine import LLMEngine
from sutro_amd.engine.request import SamplingParams
from sutro_amd.models.qwen3 import Qwen3MoE
from sutro_amd.models.registry import ModelSpec
from sutro_amd.ops import torch_ref

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="no GPU")]
DEV = "cuda"


def tie_free(T, E, scale, seed):
    """each row a random permutation of E distinct bf16-exact values"""
    g = torch.Generator().manual_seed(seed)
    vals = torch.linspace(-scale, scale, E).bfloat16().float()
    assert vals.unique().numel() == E
    return vals[torch.argsort(torch.rand(T, E, generator=g), dim=-1)]


def check_against_ref(logits, k, base, E_l, bm):
    """integer outputs and selected experts bit-equal to torch_ref on the
    same logits, zeros for non-local assignments exact; returns (w, w_ref)"""
    T = logits.shape[0]
    ws = ops.moe_route_workspace(T, k, E_l, DEV, bm)
    got = ops.moe_route(logits.to(DEV), k, base, E_l, bm, ws)
    torch.cuda.synchronize()
    ref = torch_ref.moe_route(logits, k, base, E_l, bm)
    _, idx_ref = torch_ref.moe_route_select(logits, k)
    assert torch.equal(ws["route_idx"][:T * k].cpu().view(T, k).long(),
                       idx_ref)
    for name, g, r in zip(("padpos", "row_tok", "tile_off", "counts"),
                          got[1:], ref[1:]):
        assert g.dtype == r.dtype, name
        assert torch.equal(g.cpu(), r), name
    w = got[0].cpu()
    assert torch.equal(w == 0, ref[0] == 0)
    return w, ref[0]


@pytest.mark.parametrize("T", [1, 63, 129, 4100])
@pytest.mark.parametrize("E,k", [(8, 2), (32, 4), (64, 4), (128, 8)])
def test_random_logits_grid(E, k, T):
    g = torch.Generator().manual_seed(1000 * E + T)
    logits = torch.randn(T, E, generator=g) * 2
    for dtype in (torch.bfloat16, torch.float32):
        for bm in (64, 128):
            w, w_ref = check_against_ref(logits.to(dtype), k, 0, E, bm)
            # two f32 evaluations of the same formula: a few ulp apart
            torch.testing.assert_close(w, w_ref, atol=0, rtol=2e-6)


# family -> the smallest (E, k, T) at which it can fail
@pytest.mark.parametrize("family", ["ties", "one_expert", "ep"])
def test_input_families(family):
    g = torch.Generator().manual_seed(11)
    base, E_l = 0, 32
    if family == "ties":
        # four distinct bf16 values and one all-equal row; T past one block
        E, k, T = 32, 4, 129
        logits = torch.tensor([-1.0, 0.0, 0.5, 2.0])[
            torch.randint(0, 4, (T, E), generator=g)]
        logits[5] = 0.25
    elif family == "one_expert":
        # every assignment on one expert, the others empty: 300 rows cross
        # the blocks, the waves and several tiles
        E, k, T, E_l = 8, 1, 300, 8
        logits = torch.randn(T, E, generator=g)
        logits[:, 3] += 50.0
    else:
        # EP: non-local assignments on both sides of the local range
        E, k, T = 32, 4, 257
        base, E_l = E // 2, E // 4
        logits = torch.randn(T, E, generator=g) * 2
    for bm in (64, 128):
        check_against_ref(logits.bfloat16(), k, base, E_l, bm)


@pytest.mark.parametrize("scale", [4.0, 80.0])   # 80: max subtraction matters
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("E,k", [(8, 2), (128, 8)])
def test_weights_against_f64(E, k, dtype, scale):
    """Largest relative deviation from the f64 statement at most 4x that of
    the present f32 path (torch_ref.topk_softmax_router) on the same
    tie-free logits, floor 1e-6. Measured on MI355X (capture R1): fused
    <= 1.76e-7, torch path <= 1.46e-7."""
    T = 257
    logits = tie_free(T, E, scale, seed=E + int(scale))
    if dtype == "f32":
        logits = logits * 1.0371          # no longer bf16-exact, still distinct
    else:
        logits = logits.bfloat16()
    l64 = logits.double()
    vals, idx = torch.sort(l64, dim=-1, descending=True, stable=True)
    p = torch.softmax(l64, -1).gather(1, idx[:, :k])
    w64 = p / p.sum(-1, keepdim=True)

    def deviation(w):
        # relative; the guard keeps f32-denormal weights out of the ratio
        return ((w.double() - w64).abs() / w64.clamp_min(1e-30)).max().item()

    w_torch, idx_torch = torch_ref.topk_softmax_router(logits, k)
    assert torch.equal(idx_torch, idx[:, :k])
    w, _ = check_against_ref(logits, k, 0, E, 64)
    dev_fused, dev_torch = deviation(w), deviation(w_torch)
    print(f"moe_route weights E={E} k={k} {dtype} scale={scale}: "
          f"fused {dev_fused:.3e} torch {dev_torch:.3e}")
    assert dev_fused <= max(4 * dev_torch, 1e-6)


def test_deterministic_and_graph_replay():
    E, k, T, bm = 128, 8, 257, 64
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randn(T, E, generator=g) * 2).bfloat16().to(DEV)
               for _ in range(4)]

    def eager(logits):
        return [t.clone() for t in ops.moe_route(logits, k, 0, E, bm)]

    first, again = eager(batches[0]), eager(batches[0])
    assert all(torch.equal(a, b) for a, b in zip(first, again))

    ws = ops.moe_route_workspace(T, k, E, DEV, bm)
    static = batches[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.moe_route(static, k, 0, E, bm, ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.moe_route(static, k, 0, E, bm, ws)
    for logits in batches[1:]:
        static.copy_(logits)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager(logits)))


def _layer(experts, k, seed, routing="fused"):
    spec = ModelSpec(name="tiny-moe-route-gpu", hidden_size=256, num_layers=1,
                     num_heads=4, num_kv_heads=2, head_dim=64,
                     intermediate_size=0, vocab_size=512, num_experts=experts,
                     experts_per_token=k, moe_intermediate_size=128)
    torch.manual_seed(seed)
    moe = Qwen3MoE(spec, torch.bfloat16, moe_routing=routing).to(DEV)
    for p in moe.parameters():
        torch.nn.init.normal_(p, std=0.05)
    return moe


@pytest.mark.parametrize("experts_dtype", ["bf16", "fp8_e4m3",
                                           "fp8_block128"])
def test_fused_layer_matches_loop(experts_dtype):
    moe = _layer(8, 2, seed=2)
    if experts_dtype == "fp8_e4m3":
        moe.quantize_experts_fp8()
    elif experts_dtype == "fp8_block128":
        moe.quantize_experts_fp8_block128()
    x = (torch.randn(333, 256) * 0.5).to(torch.bfloat16).to(DEV)
    # bf16 experts also at a skewed routing: every token -> expert 3
    for skew in (False, True) if experts_dtype == "bf16" else (False,):
        if skew:
            with torch.no_grad():
                moe.router.weight[3] += 50.0
        ref = moe._forward_loop(x).float()
        got = moe._forward_grouped(x).float()
        assert ref.abs().max() > 0
        torch.testing.assert_close(got, ref, atol=3e-2, rtol=3e-2)


def test_fused_layer_matches_torch_layer_tie_free():
    """Router logits made tie-free by construction: token t carries a one-hot
    selector in the first 128 hidden dims, where router column p is a
    permutation of distinct values (the product is exact), and noise in the
    rest, which the router ignores."""
    T, E = 333, 8
    moe = _layer(E, 2, seed=3)
    cols = tie_free(128, E, 3.0, seed=9).t()              # [E, 128]
    with torch.no_grad():
        moe.router.weight.zero_()
        moe.router.weight[:, :128] = cols.to(DEV)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(T, 256, generator=g) * 0.5
    x[:, :128] = 0
    x[torch.arange(T), torch.randint(0, 128, (T,), generator=g)] = 1.0
    x = x.bfloat16().to(DEV)
    logits = moe.router(x).float()
    assert all(row.unique().numel() == E for row in logits.cpu())
    fused = moe._forward_grouped(x).float().clone()
    moe.moe_routing = "torch"
    plain = moe._forward_grouped(x).float()
    assert plain.abs().max() > 0
    torch.testing.assert_close(fused, plain, atol=3e-2, rtol=3e-2)


def test_engine_fused_graph_decode_matches_eager():
    spec = ModelSpec(name="tiny-moe-route-e2e", hidden_size=256, num_layers=2,
                     num_heads=4, num_kv_heads=2, head_dim=64,
                     intermediate_size=0, vocab_size=2048, max_context=512,
                     tie_embeddings=True, num_experts=8, experts_per_token=2,
                     moe_intermediate_size=192)

    def run(eager):
        eng = LLMEngine(EngineConfig(
            spec=spec, device=DEV, max_model_len=256, num_kv_blocks=128,
            max_tokens_per_step=512, seed=0, moe_routing="fused",
            enforce_eager=eager))
        assert (eng.graph_runner is None) == eager
        assert all(m.moe_routing == "fused" for m in eng.model.modules()
                   if isinstance(m, Qwen3MoE))
        reqs = [eng.add_request(eng.tokenizer.encode(p),
                                SamplingParams(max_tokens=10, temperature=0))
                for p in ["moe route row one", "moe route row two"]]
        while eng.has_work():
            eng.step()
        return [list(r.output_token_ids) for r in reqs]

    graphed = run(False)
    assert all(len(t) > 0 for t in graphed)
    assert graphed == run(True)
