"""GPU tests for FP8 (W8A8) dense weights: the pipelined block-scaled MFMA
GEMM (csrc/gemm_tn_fp8_pipe.hip), its residual and SwiGLU epilogues, the ops
under hipGraph capture and the engine with dense_weight_dtype="fp8_e4m3".

On-device oracle: ops.grouped_gemm_fp8 with one expert. It feeds the same
instruction the same fragments in ascending K into one accumulator per
fragment and applies the same epilogue expression, so the outputs must be
bit-equal."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sutro_amd import _C, ops
    from sutro_amd.ops import torch_ref
else:  # collected on CPU; every test is skipped by the marker filter anyway
    _C = ops = torch_ref = None

DEV = "cuda"
F8 = torch.float8_e4m3fn
# the plain-stage tolerance of tests/test_gpu_moe_fp8.py
PLAIN_TOL = dict(atol=2e-3, rtol=2.0 ** -7)


def require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _quantized(M, N, K, seed):
    """Random bf16 operands through the row quantiser -> device tensors
    (a_q [M, Kp], a_s [M], w_q [N, Kp], w_s [N])."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    w = (torch.randn(N, K, device=DEV, generator=g) / K ** 0.5).bfloat16()
    Kp = torch_ref.fp8_padded_k(K)
    out = []
    for t in (x, w):
        q = torch.empty(t.shape[0], Kp, dtype=F8, device=DEV)
        s = torch.empty(t.shape[0], dtype=torch.float32, device=DEV)
        ops.quantize_rows_fp8(t, q, s)
        out += [q, s]
    return out


def _oracle(a_q, a_s, w_q, w_s, gate_silu, bm=128):
    """grouped_gemm_fp8 with E = 1: tile_off = [0, ceil(M / bm)], counts =
    [M]; the gather stage (gate_silu) takes an identity row_tok."""
    M, Kp = a_q.shape
    N = w_q.shape[0]
    tiles = (M + bm - 1) // bm
    rows = tiles * bm
    n_cols = N // 2 if gate_silu else N
    tile_off = torch.tensor([0, tiles], dtype=torch.int32, device=DEV)
    counts = torch.tensor([M], dtype=torch.int32, device=DEV)
    out = torch.zeros(rows, n_cols, dtype=torch.bfloat16, device=DEV)
    if gate_silu:
        row_tok = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
        row_tok[:M] = torch.arange(M, dtype=torch.int32, device=DEV)
        a_p, s_p = a_q, a_s
    else:
        row_tok = None
        a_p = torch.zeros(rows, Kp, dtype=torch.uint8, device=DEV)
        a_p[:M] = a_q.view(torch.uint8)
        a_p = a_p.view(F8)
        s_p = torch.ones(rows, dtype=torch.float32, device=DEV)
        s_p[:M] = a_s
    ops.grouped_gemm_fp8(out, a_p, s_p, w_q.view(1, N, Kp), w_s.view(1, N),
                         row_tok, tile_off, counts, tiles, gate_silu, bm)
    return out[:M]


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (512, 512, 384)])
def test_exact_integers(M, N, K):
    """Codes drawn from {-2..2} and power-of-two scales, distinct per row
    and per column: every f32 sum and product is exact in any order, so the
    kernel and torch_ref round the same value to bf16. Pins the operand lane
    map and the scale indexing (a swapped or broadcast scale fails)."""
    require_gpu()
    g = torch.Generator().manual_seed(M + K)
    a = torch.randint(-2, 3, (M, K), generator=g).float()
    w = torch.randint(-2, 3, (N, K), generator=g).float()
    a_s = 2.0 ** ((torch.arange(M) % 5) - 2).float()
    w_s = 2.0 ** ((torch.arange(N) % 7) - 3).float()
    a_q, w_q = a.to(F8), w.to(F8)
    assert torch.equal(a_q.float(), a) and torch.equal(w_q.float(), w)
    ref = torch_ref.fp8_linear(a_q, a_s, w_q, w_s).to(torch.bfloat16)
    assert ref.float().abs().max() > 0
    for xswz in (0, 1):
        out = _C.gemm_fp8_pipelined(a_q.to(DEV), a_s.to(DEV), w_q.to(DEV),
                                    w_s.to(DEV), None, xswz)
        assert out.shape == (M, N) and out.dtype == torch.bfloat16
        assert torch.equal(out.cpu(), ref), (xswz, (out.cpu() != ref).sum())


@pytest.mark.parametrize("M,N,K", [
    (256, 256, 128),    # one K-tile: prologue and epilogue only
    (256, 256, 256),
    (256, 512, 384),    # odd tile count
    (512, 1024, 200),   # K tail, Kp = 256
    (384, 256, 1024),   # M edge (half a tile)
    (130, 256, 256),    # M edge inside the first half-tile
    (1, 256, 256),
    (512, 960, 640),    # N edge inside a tile
])
def test_plain_equals_oracle(M, N, K):
    require_gpu()
    a_q, a_s, w_q, w_s = _quantized(M, N, K, 11)
    oracle = _oracle(a_q, a_s, w_q, w_s, False)
    ref = torch_ref.fp8_linear(a_q.cpu(), a_s.cpu(), w_q.cpu(), w_s.cpu())
    for xswz in (0, 1):
        out = _C.gemm_fp8_pipelined(a_q, a_s, w_q, w_s, None, xswz)
        assert out.shape == (M, N)
        assert torch.equal(out, oracle), (M, N, K, xswz,
                                          (out != oracle).sum().item())
        torch.testing.assert_close(out.cpu().float(), ref, **PLAIN_TOL)


def test_residual_epilogue():
    """f32 fp8_linear + residual, rounded once."""
    require_gpu()
    M, N, K = 300, 512, 384
    a_q, a_s, w_q, w_s = _quantized(M, N, K, 12)
    res = torch.randn(M, N, device=DEV).bfloat16()
    out = _C.gemm_fp8_pipelined(a_q, a_s, w_q, w_s, res, 1)
    ref = (torch_ref.fp8_linear(a_q.cpu(), a_s.cpu(), w_q.cpu(), w_s.cpu())
           + res.cpu().float())
    torch.testing.assert_close(out.cpu().float(), ref, **PLAIN_TOL)


@pytest.mark.parametrize("M,I,K", [
    (256, 128, 128),
    (384, 256, 384),
    (130, 128, 256),
    (512, 384, 5120),   # the flagship K
])
def test_swiglu_equals_oracle(M, I, K):
    """Bit-equal to the grouped kernel's gate/up stage: same accumulators,
    same epilogue expression."""
    require_gpu()
    a_q, a_s, w_q, w_s = _quantized(M, 2 * I, K, 13)
    oracle = _oracle(a_q, a_s, w_q, w_s, True)
    for xswz in (0, 1):
        out = _C.gemm_fp8_gate_up_silu(a_q, a_s, w_q, w_s, xswz)
        assert out.shape == (M, I)
        assert torch.equal(out, oracle), (M, I, K, xswz,
                                          (out != oracle).sum().item())


def test_ordering_screen():
    """A misplaced LDS read passes most runs: repeat both kernels with other
    work filling the stream between calls and require every result to equal
    the first and the oracle, bit for bit."""
    require_gpu()
    a_q, a_s, w_q, w_s = _quantized(512, 1024, 1024, 14)
    plain_ref = _oracle(a_q, a_s, w_q, w_s, False)
    fused_ref = _oracle(a_q, a_s, w_q, w_s, True)
    filler = torch.empty(1 << 24, device=DEV)
    for it in range(10):
        filler.normal_()
        p = _C.gemm_fp8_pipelined(a_q, a_s, w_q, w_s, None, 1)
        filler.normal_()
        f = _C.gemm_fp8_gate_up_silu(a_q, a_s, w_q, w_s, 1)
        assert torch.equal(p, plain_ref), it
        assert torch.equal(f, fused_ref), it


def test_ops_graph_capture():
    """ops.gate_up_silu_fp8 and ops.linear_fp8 (quantiser + GEMM, fresh
    allocator tensors) captured at M = 128 and replayed with two inputs."""
    require_gpu()
    M, I, K = 128, 256, 512
    _, _, gu_q, gu_s = _quantized(8, 2 * I, K, 15)
    _, _, dn_q, dn_s = _quantized(8, K, I, 16)

    def fwd(x):
        return ops.linear_fp8(ops.gate_up_silu_fp8(x, gu_q, gu_s), dn_q, dn_s)

    static_x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fwd(static_x)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = fwd(static_x)
    for seed in (21, 22):
        g = torch.Generator(device=DEV)
        g.manual_seed(seed)
        xin = torch.randn(M, K, device=DEV, generator=g).bfloat16()
        static_x.copy_(xin)
        graph.replay()
        torch.cuda.synchronize()
        eager = fwd(xin)
        assert eager.shape == (M, K) and eager.float().abs().max() > 0
        assert torch.equal(static_out, eager), seed


def _engine(dense, eager):
    from sutro_amd.engine.config import EngineConfig
    from sutro_amd.engine.engine import LLMEngine
    from sutro_amd.models.registry import ModelSpec

    spec = ModelSpec(name="dense-fp8-gpu", hidden_size=256, num_layers=2,
                     num_heads=4, num_kv_heads=2, head_dim=128,
                     intermediate_size=512, vocab_size=1024, max_context=512,
                     tie_embeddings=True)
    cfg = EngineConfig(spec=spec, device=DEV, max_model_len=256,
                       num_kv_blocks=128, max_tokens_per_step=512, seed=0,
                       dense_weight_dtype=dense, enforce_eager=eager)
    return LLMEngine(cfg)


def _generate(eng):
    from sutro_amd.engine.request import SamplingParams

    reqs = [eng.add_request(eng.tokenizer.encode(p),
                            SamplingParams(max_tokens=12, temperature=0.7,
                                           seed=3 + i))
            for i, p in enumerate(["dense fp8 row one", "dense fp8 row two"])]
    while eng.has_work():
        eng.step()
    assert all(r.finish_reason is not None for r in reqs)
    return ([list(r.output_token_ids) for r in reqs],
            [r.cumulative_logprob for r in reqs])


def test_engine_graph_decode_equals_eager():
    """hipGraph decode and eager decode give the same tokens and logprobs;
    capture succeeded (a hidden host sync or an allocation the capture cannot
    take would leave graph_runner None)."""
    require_gpu()
    eng = _engine("fp8_e4m3", eager=False)
    assert eng.graph_runner is not None
    layer = eng.model.layers[0]
    assert layer.self_attn.qkv_proj.weight.dtype == F8
    assert layer.mlp.down_proj.weight.dtype == F8
    toks_g, lps_g = _generate(eng)
    toks_e, lps_e = _generate(_engine("fp8_e4m3", eager=True))
    assert all(len(t) > 0 for t in toks_g)
    assert toks_g == toks_e
    assert lps_g == lps_e


@pytest.mark.parametrize("dense,per_layer", [("fp8_e4m3", 4), ("bf16", 0)])
def test_engine_fp8_gemm_calls(dense, per_layer):
    """A counting wrapper around the two bindings: one forward (the prefill
    step) makes four FP8 GEMM calls per layer (qkv, o, gate_up, down) with
    the option on and none with it off."""
    require_gpu()
    from sutro_amd.engine.request import SamplingParams

    eng = _engine(dense, eager=True)
    calls = {"linear": 0, "gate_up": 0}
    real_l, real_g = _C.gemm_fp8_pipelined, _C.gemm_fp8_gate_up_silu

    def count_l(*a, **kw):
        calls["linear"] += 1
        return real_l(*a, **kw)

    def count_g(*a, **kw):
        calls["gate_up"] += 1
        return real_g(*a, **kw)

    _C.gemm_fp8_pipelined, _C.gemm_fp8_gate_up_silu = count_l, count_g
    try:
        eng.add_request(eng.tokenizer.encode("count the fp8 gemm calls"),
                        SamplingParams(max_tokens=4, temperature=0.0))
        eng.step()  # the prefill: one forward
    finally:
        _C.gemm_fp8_pipelined, _C.gemm_fp8_gate_up_silu = real_l, real_g
    layers = eng.spec.num_layers
    assert calls["linear"] + calls["gate_up"] == per_layer * layers
    if per_layer:
        assert calls == {"linear": 3 * layers, "gate_up": layers}
