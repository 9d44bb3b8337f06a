"""GPU tests for block-scaled FP8 dense weights: the group quantiser and the
pipelined GEMM with in-loop scales (csrc/gemm_tn_fp8_block_pipe.hip), its
residual and SwiGLU epilogues, the ops under hipGraph capture, and the engine
with dense_weight_dtype="fp8_block128", quantised at start-up and loaded
pre-quantised.

The reference throughout is the f64 evaluation of the formula stated in
torch_ref.fp8_block_linear on the same codes and scales."""

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
# the plain-stage tolerance of tests/test_gpu_dense_fp8.py
PLAIN_TOL = dict(atol=2e-3, rtol=2.0 ** -7)

# every edge of the schedule: 1, 2, 3 and 5 K-tiles (both buffers, the odd
# tail, the clamped prefetch past the end); a lone row, a one-row second
# half, a full tile, two tiles with a ragged edge; a second half-tile wholly
# past the edge, one tile, a ragged N tile
KS = (128, 256, 384, 640)
MS = (1, 129, 256, 300)
NS = (128, 256, 384)
IS = (128, 256)


def require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _f64_linear(a_q, a_s, w_q, w_s):
    """torch_ref.fp8_block_linear's formula in f64, on the device."""
    a, w = a_q.float().double(), w_q.float().double()
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float64,
                      device=a.device)
    for kb in range(a.shape[1] // 128):
        ks = slice(kb * 128, (kb + 1) * 128)
        f = (a_s[kb].double()[:, None]
             * w_s[:, kb].double().repeat_interleave(128)[None, :])
        acc += (a[:, ks] @ w[:, ks].T) * f
    return acc


# ---- the group quantiser ----

@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("R", [1, 63, 257])
def test_quantiser_is_bit_equal_to_the_statement(R, K):
    """Includes an all-zero row, an all-zero group, a row of +-max-finite
    bf16 and magnitudes across many binades."""
    require_gpu()
    g = torch.Generator().manual_seed(R * 1000 + K)
    x = torch.randn(R, K, generator=g) * torch.logspace(-6, 6, R)[:, None]
    x[R // 2] = 0
    x[0, :128] = 0
    big = torch.finfo(torch.bfloat16).max
    x[R - 1] = big
    x[R - 1, ::3] = -big
    x = x.bfloat16()
    want_q, want_s = torch_ref.quantize_rows_fp8_block128(x)
    got_q, got_s = ops.quantize_rows_fp8_block128(x.to(DEV))
    assert got_q.shape == (R, K) and got_q.dtype == F8
    assert got_s.shape == (K // 128, R) and got_s.dtype == torch.float32
    assert torch.equal(got_s.cpu(), want_s)
    assert torch.equal(got_q.cpu().view(torch.uint8),
                       want_q.view(torch.uint8))


# ---- the scale maps, exactly ----

def _exact_operands(M, N, K, seed, a_shift=0):
    """Integer codes in [-3, 3] and power-of-two scales, distinct per
    (row, kb) and per (N block, kb): every f32 product and sum is exact."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    w = torch.randint(-3, 4, (N, K), generator=g).float()
    kb = torch.arange(K // 128)
    r = torch.arange(M)
    nb = torch.arange(N // 128)
    a_s = 2.0 ** ((r[None, :] + 2 * kb[:, None]) % 3 - 1 + a_shift).float()
    w_s = 2.0 ** ((nb[:, None] + kb[None, :]) % 4 - 2).float()
    a_q, w_q = a.to(F8), w.to(F8)
    assert torch.equal(a_q.float(), a) and torch.equal(w_q.float(), w)
    return a_q.to(DEV), a_s.to(DEV), w_q.to(DEV), w_s.to(DEV)


@pytest.mark.parametrize("K", KS)
def test_plain_scale_maps_are_exact(K):
    """The output must equal the f64 reference rounded once to bf16, bit for
    bit: an index error in either scale map is a wrong value, not noise."""
    require_gpu()
    for M in MS:
        for N in NS:
            a_q, a_s, w_q, w_s = _exact_operands(M, N, K, M + N + K)
            ref = _f64_linear(a_q, a_s, w_q, w_s)
            assert ref.abs().max() > 0
            # exact in f32 too, so the one rounding is the bf16 one
            assert torch.equal(ref.float().double(), ref)
            ref = ref.float().bfloat16()
            for xswz in (0, 1):
                out = _C.gemm_fp8_block_pipelined(a_q, a_s, w_q, w_s, None,
                                                  xswz)
                assert out.shape == (M, N) and out.dtype == torch.bfloat16
                assert torch.equal(out, ref), (
                    M, N, K, xswz, (out != ref).sum().item())


@pytest.mark.parametrize("K", KS)
def test_swiglu_scale_maps_are_exact(K):
    """Gate and up products are exact in f32; the activation is not (the
    kernel's exp is an f32 approximation, a few 2^-24 relative at the |g| <
    64 used here). So: every element within one bf16 ulp of the f64
    reference rounded once, and bit-equal wherever that reference is not
    within 2^-14 relative of a bf16 rounding boundary. A wrong scale index
    changes a value by a factor of two or more."""
    require_gpu()
    for M in MS:
        for inter in IS:
            # activation scales 2^-5 smaller: |g| stays in silu's live range
            a_q, a_s, w_q, w_s = _exact_operands(M, 2 * inter, K,
                                                 M + inter + K, a_shift=-5)
            y = _f64_linear(a_q, a_s, w_q, w_s)
            assert torch.equal(y.float().double(), y)
            gate, up = y[:, :inter], y[:, inter:]
            assert 0 < gate.abs().max() < 64
            ref64 = gate / (1 + torch.exp(-gate)) * up
            ref = ref64.float().bfloat16()
            # bf16 ulp at the reference: |ref| = m * 2^e with m in [0.5, 1)
            ulp = torch.ldexp(torch.ones_like(ref64),
                              torch.frexp(ref.float().abs())[1] - 8)
            frac = (ref64 / ulp) % 1.0            # 0.5 = a rounding boundary
            clear = (frac - 0.5).abs() > 2.0 ** -14 * ref64.abs() / ulp
            for xswz in (0, 1):
                out = _C.gemm_fp8_block_gate_up_silu(a_q, a_s, w_q, w_s, xswz)
                assert out.shape == (M, inter)
                diff = (out.double() - ref.double()).abs()
                assert (diff <= ulp).all(), (M, inter, K, xswz)
                assert torch.equal(out[clear], ref[clear]), (
                    M, inter, K, xswz, (out != ref)[clear].sum().item())
                assert clear.float().mean() > 0.9


# ---- random data ----

def _random_operands(M, N, K, seed):
    """Full-range codes from the real quantisers; outputs are O(1)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    w = (torch.randn(N, K, device=DEV, generator=g) / K ** 0.5)
    a_q, a_s = ops.quantize_rows_fp8_block128(x)
    w_q, w_s = torch_ref.quantize_weight_fp8_block128(w)
    return a_q, a_s, w_q, w_s


@pytest.mark.parametrize("M,N,K", [
    (1, 128, 128), (129, 384, 256), (256, 256, 384), (300, 384, 640),
    (300, 128, 128), (1, 256, 640),
])
def test_plain_random(M, N, K):
    require_gpu()
    a_q, a_s, w_q, w_s = _random_operands(M, N, K, 11)
    ref = _f64_linear(a_q, a_s, w_q, w_s).float()
    for xswz in (0, 1):
        out = _C.gemm_fp8_block_pipelined(a_q, a_s, w_q, w_s, None, xswz)
        torch.testing.assert_close(out.float(), ref, **PLAIN_TOL)


@pytest.mark.parametrize("M,I,K", [
    (1, 128, 256), (129, 256, 384), (300, 128, 640), (256, 256, 128),
])
def test_swiglu_random(M, I, K):
    require_gpu()
    a_q, a_s, w_q, w_s = _random_operands(M, 2 * I, K, 13)
    y = _f64_linear(a_q, a_s, w_q, w_s)
    ref = (torch.nn.functional.silu(y[:, :I]) * y[:, I:]).float()
    for xswz in (0, 1):
        out = _C.gemm_fp8_block_gate_up_silu(a_q, a_s, w_q, w_s, xswz)
        torch.testing.assert_close(out.float(), ref, **PLAIN_TOL)


def test_residual_epilogue():
    """The plain f32 result plus the residual, rounded once: reproduced from
    the f64 reference within the plain tolerance, and exactly on operands
    whose sums are exact."""
    require_gpu()
    M, N, K = 300, 384, 384
    a_q, a_s, w_q, w_s = _random_operands(M, N, K, 12)
    res = torch.randn(M, N, device=DEV).bfloat16()
    out = _C.gemm_fp8_block_pipelined(a_q, a_s, w_q, w_s, res, 1)
    ref = (_f64_linear(a_q, a_s, w_q, w_s) + res.double()).float()
    torch.testing.assert_close(out.float(), ref, **PLAIN_TOL)
    # exact operands, a residual of small dyadics: sum exact, one rounding
    a_q, a_s, w_q, w_s = _exact_operands(M, N, K, 5)
    res = (torch.randint(-64, 65, (M, N), device=DEV).float() / 8).bfloat16()
    y = _f64_linear(a_q, a_s, w_q, w_s) + res.double()
    assert torch.equal(y.float().double(), y)
    out = _C.gemm_fp8_block_pipelined(a_q, a_s, w_q, w_s, res, 1)
    assert torch.equal(out, y.float().bfloat16())
    # and through the op
    x = torch.randn(M, K, device=DEV).bfloat16()
    plain = ops.linear_fp8_block128(x, w_q, w_s)
    x_q, x_s = ops.quantize_rows_fp8_block128(x)
    y = _f64_linear(x_q, x_s, w_q, w_s)
    torch.testing.assert_close(plain.float(), y.float(), **PLAIN_TOL)
    torch.testing.assert_close(
        ops.linear_fp8_block128(x, w_q, w_s, residual=res).float(),
        (y + res.double()).float(), **PLAIN_TOL)


def test_ordering_screen():
    """A misplaced LDS read passes most runs: repeat both kernels with other
    work filling the stream between calls and require every result to equal
    the first, bit for bit, and the first to match the reference."""
    require_gpu()
    a_q, a_s, w_q, w_s = _random_operands(512, 1024, 1024, 14)
    y = _f64_linear(a_q, a_s, w_q, w_s)
    plain0 = _C.gemm_fp8_block_pipelined(a_q, a_s, w_q, w_s, None, 1)
    fused0 = _C.gemm_fp8_block_gate_up_silu(a_q, a_s, w_q, w_s, 1)
    torch.testing.assert_close(plain0.float(), y.float(), **PLAIN_TOL)
    torch.testing.assert_close(
        fused0.float(),
        (torch.nn.functional.silu(y[:, :512]) * y[:, 512:]).float(),
        **PLAIN_TOL)
    filler = torch.empty(1 << 24, device=DEV)
    for it in range(10):
        filler.normal_()
        p = _C.gemm_fp8_block_pipelined(a_q, a_s, w_q, w_s, None, 1)
        filler.normal_()
        f = _C.gemm_fp8_block_gate_up_silu(a_q, a_s, w_q, w_s, 1)
        assert torch.equal(p, plain0), it
        assert torch.equal(f, fused0), it


def test_ops_graph_capture():
    """ops.gate_up_silu_fp8_block128 and ops.linear_fp8_block128 (quantiser +
    GEMM, fresh allocator tensors) captured at M = 128 and replayed with two
    inputs."""
    require_gpu()
    M, I, K = 128, 256, 512
    g = torch.Generator(device=DEV)
    g.manual_seed(15)
    gu_q, gu_s = torch_ref.quantize_weight_fp8_block128(
        torch.randn(2 * I, K, device=DEV, generator=g) / K ** 0.5)
    dn_q, dn_s = torch_ref.quantize_weight_fp8_block128(
        torch.randn(K, I, device=DEV, generator=g) / I ** 0.5)

    def fwd(x):
        return ops.linear_fp8_block128(
            ops.gate_up_silu_fp8_block128(x, gu_q, gu_s), dn_q, dn_s)

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
        g.manual_seed(seed)
        xin = torch.randn(M, K, device=DEV, generator=g).bfloat16()
        static_x.copy_(xin)
        graph.replay()
        torch.cuda.synchronize()
        eager = fwd(xin)
        assert eager.shape == (M, K) and eager.float().abs().max() > 0
        assert torch.equal(static_out, eager), seed


# ---- engine ----

def _engine(eager, weights_path=None):
    from sutro_amd.engine.config import EngineConfig
    from sutro_amd.engine.engine import LLMEngine
    from sutro_amd.models.registry import ModelSpec

    spec = ModelSpec(name="dense-fp8-block-gpu", hidden_size=256,
                     num_layers=2, num_heads=4, num_kv_heads=2, head_dim=128,
                     intermediate_size=512, vocab_size=512, max_context=512,
                     tie_embeddings=True)
    cfg = EngineConfig(spec=spec, device=DEV, max_model_len=256,
                       num_kv_blocks=128, max_tokens_per_step=512, seed=0,
                       dense_weight_dtype="fp8_block128", enforce_eager=eager,
                       weights_path=weights_path)
    return LLMEngine(cfg)


def _generate(eng):
    from sutro_amd.engine.request import SamplingParams

    reqs = [eng.add_request(eng.tokenizer.encode(p),
                            SamplingParams(max_tokens=12, temperature=0.7,
                                           seed=3 + i))
            for i, p in enumerate(["block fp8 row one", "block fp8 row two"])]
    while eng.has_work():
        eng.step()
    assert all(r.finish_reason is not None for r in reqs)
    return ([list(r.output_token_ids) for r in reqs],
            [r.cumulative_logprob for r in reqs])


def test_engine_graph_decode_equals_eager(tmp_path):
    """hipGraph decode and eager decode give the same tokens and logprobs,
    the projections carry `weight_scale_inv`, and a model saved, reloaded
    pre-quantised and run gives the same tokens as the one quantised at
    start-up."""
    require_gpu()
    from sutro_amd.models.loader import save_weights

    eng = _engine(eager=False)
    assert eng.graph_runner is not None
    for layer in eng.model.layers:
        for lin in (layer.self_attn.qkv_proj, layer.self_attn.o_proj,
                    layer.mlp.gate_up_proj, layer.mlp.down_proj):
            assert lin.weight.dtype == F8
            N, K = lin.weight.shape
            assert lin.weight_scale_inv.shape == (N // 128, K // 128)
            assert lin.weight_scale_inv.is_cuda
    toks_g, lps_g = _generate(eng)
    eng_e = _engine(eager=True)
    toks_e, lps_e = _generate(eng_e)
    assert all(len(t) > 0 for t in toks_g)
    assert toks_g == toks_e
    assert lps_g == lps_e

    path = str(tmp_path / "ckpt")
    save_weights(eng_e.model, path)
    eng_l = _engine(eager=True, weights_path=path)
    assert not any("_proj" in n for n, _ in eng_l.model.named_parameters())
    a, b = eng_e.model.state_dict(), eng_l.model.state_dict()
    for k in a:
        if "_proj" in k:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8))
    toks_l, lps_l = _generate(eng_l)
    assert toks_l == toks_e
    assert lps_l == lps_e
