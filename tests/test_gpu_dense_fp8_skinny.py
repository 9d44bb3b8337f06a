"""The weight-streaming small-M FP8 GEMM (csrc/gemm_tn_fp8_skinny.hip), the
block-per-row activation quantiser and their routing in ops.linear_fp8.
References: torch_ref on the CPU. GPU tests carry the gpu marker; the two
routing tests at the end run anywhere."""

import pytest
import torch

from sutro_amd import ops
from sutro_amd.ops import torch_ref

if torch.cuda.is_available():
    from sutro_amd import _C
    from test_gpu_dense_fp8 import (PLAIN_TOL, _engine, _generate, _quantized,
                                    require_gpu)

gpu = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn


def _ref(a_q, a_s, w_q, w_s):
    return torch_ref.fp8_linear(a_q.cpu(), a_s.cpu(), w_q.cpu(), w_s.cpu())


@gpu
@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("M,N,K", [
    (1, 64, 128), (16, 64, 128), (17, 64, 128), (64, 64, 128), (65, 64, 128),
    (256, 64, 128),                                   # every M, one K-tile
    (1, 64, 384), (1, 64, 1152), (1, 64, 200),        # every K
    (1, 192, 128), (65, 192, 1152),
])
def test_exact_integers(M, N, K, waves):
    """Codes in {-2..2}, power-of-two scales distinct per row and column:
    every partial sum is exact in any order, so the output equals the
    reference bit for bit. Pins the swapped-operand lane map, the scale
    indexing and the cross-wave reduction (K = 128 leaves waves empty)."""
    require_gpu()
    g = torch.Generator().manual_seed(M + N + K)
    Kp = torch_ref.fp8_padded_k(K)
    a = torch.zeros(M, Kp)
    w = torch.zeros(N, Kp)
    a[:, :K] = torch.randint(-2, 3, (M, K), generator=g).float()
    w[:, :K] = torch.randint(-2, 3, (N, K), generator=g).float()
    a_s = 2.0 ** ((torch.arange(M) % 5) - 2).float()
    w_s = 2.0 ** ((torch.arange(N) % 7) - 3).float()
    a_q, w_q = a.to(F8), w.to(F8)
    ref = torch_ref.fp8_linear(a_q, a_s, w_q, w_s).to(torch.bfloat16)
    assert ref.float().abs().max() > 0
    out = _C.gemm_fp8_skinny(a_q.to(DEV), a_s.to(DEV), w_q.to(DEV),
                             w_s.to(DEV), None, waves)
    assert out.shape == (M, N) and out.dtype == torch.bfloat16
    assert torch.equal(out.cpu(), ref), (out.cpu() != ref).sum()


@gpu
@pytest.mark.parametrize("M,N,K", [(1, 64, 128), (17, 192, 1152),
                                   (64, 256, 4096), (200, 128, 640)])
def test_random_codes(M, N, K):
    """Full-range codes against the f32 reference and the 256-row kernel,
    both within the plain-stage tolerance. Not bit-equal to the latter: it
    sums the K-tiles ascending into one accumulator, this kernel sums W
    interleaved partial sums, and f32 addition is not associative."""
    require_gpu()
    a_q, a_s, w_q, w_s = _quantized(M, N, K, 31)
    out = _C.gemm_fp8_skinny(a_q, a_s, w_q, w_s)
    torch.testing.assert_close(out.cpu().float(), _ref(a_q, a_s, w_q, w_s),
                               **PLAIN_TOL)
    pipe = _C.gemm_fp8_pipelined(a_q, a_s, w_q, w_s, None, 1)
    torch.testing.assert_close(out.float(), pipe.float(), **PLAIN_TOL)


@gpu
def test_residual_epilogue():
    """f32 fp8_linear + residual, rounded once."""
    require_gpu()
    M, N, K = 50, 128, 384
    a_q, a_s, w_q, w_s = _quantized(M, N, K, 32)
    res = torch.randn(M, N, device=DEV).bfloat16()
    out = _C.gemm_fp8_skinny(a_q, a_s, w_q, w_s, res)
    ref = _ref(a_q, a_s, w_q, w_s) + res.cpu().float()
    torch.testing.assert_close(out.cpu().float(), ref, **PLAIN_TOL)


@gpu
def test_row_invariance():
    """A token's bits depend neither on the other tokens of the call nor on
    its row index or chunk: the K split is a function of Kp alone."""
    require_gpu()
    a_q, a_s, w_q, w_s = _quantized(200, 128, 1152, 33)
    full = _C.gemm_fp8_skinny(a_q, a_s, w_q, w_s)
    for r in (0, 63, 64, 199):
        alone = _C.gemm_fp8_skinny(a_q[r:r + 1].contiguous(),
                                   a_s[r:r + 1].contiguous(), w_q, w_s)
        assert torch.equal(alone[0], full[r]), r
        a40, s40 = a_q[:40].clone(), a_s[:40].clone()
        a40[5], s40[5] = a_q[r], a_s[r]
        at5 = _C.gemm_fp8_skinny(a40, s40, w_q, w_s)
        assert torch.equal(at5[5], full[r]), r


@gpu
@pytest.mark.parametrize("K", [8, 200, 5120, 25600])
@pytest.mark.parametrize("R", [1, 3, 64])
def test_block_row_quantiser(R, K):
    """The block-per-row kernel (variant 1) writes the reference's bits,
    including an all-zero row and a row of +-max-finite bf16, and leaves
    rows past row_limit untouched."""
    require_gpu()
    g = torch.Generator().manual_seed(R * K)
    x = torch.randn(R, K, generator=g).bfloat16()
    x[R // 2] = 0
    big = torch.finfo(torch.bfloat16).max
    x[R - 1] = torch.where(torch.arange(K) % 2 == 0, big, -big).bfloat16()
    Kp = torch_ref.fp8_padded_k(K)
    for limit in (None, torch.tensor([R - 1], dtype=torch.int32)):
        q_ref = torch.full((R, Kp), 0x55, dtype=torch.uint8).view(F8)
        s_ref = torch.full((R,), -1.0)
        torch_ref.quantize_rows_fp8(x, q_ref, s_ref, limit)
        q = torch.full((R, Kp), 0x55, dtype=torch.uint8, device=DEV).view(F8)
        s = torch.full((R,), -1.0, device=DEV)
        ops.quantize_rows_fp8(x.to(DEV), q, s,
                              None if limit is None else limit.to(DEV), 1, 1)
        assert torch.equal(q.cpu().view(torch.uint8), q_ref.view(torch.uint8))
        assert torch.equal(s.cpu(), s_ref)


@gpu
def test_ops_graph_capture():
    """ops.linear_fp8 on the forced skinny path captured at M = 32: ten
    replays with other work in the stream equal the eager result."""
    require_gpu()
    M, N, K = 32, 256, 1152
    _, _, w_q, w_s = _quantized(8, N, K, 34)
    x = torch.randn(M, K, device=DEV).bfloat16()
    ops.set_linear_fp8_skinny(True)
    try:
        eager = ops.linear_fp8(x, w_q, w_s)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.linear_fp8(x, w_q, w_s)  # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = ops.linear_fp8(x, w_q, w_s)
        filler = torch.empty(1 << 22, device=DEV)
        for it in range(10):
            filler.normal_()
            static_out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_out, eager), it
    finally:
        ops.set_linear_fp8_skinny(None)
    ref = torch_ref.linear_fp8(x.cpu(), w_q.cpu(), w_s.cpu())
    torch.testing.assert_close(eager.cpu().float(), ref.float(), **PLAIN_TOL)


@gpu
@pytest.mark.parametrize("mode", [True, None])
def test_engine(mode, monkeypatch):
    """The tiny FP8 engine: with the skinny path forced, graph decode equals
    eager decode and the binding is reached; with the rule in charge (the
    tiny shapes are not in it) it is never called."""
    require_gpu()
    calls = []
    real = _C.gemm_fp8_skinny
    monkeypatch.setattr(_C, "gemm_fp8_skinny",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    ops.set_linear_fp8_skinny(mode)
    try:
        eng = _engine("fp8_e4m3", eager=False)
        assert eng.graph_runner is not None
        toks_g, lps_g = _generate(eng)
        toks_e, lps_e = _generate(_engine("fp8_e4m3", eager=True))
    finally:
        ops.set_linear_fp8_skinny(None)
    assert all(len(t) > 0 for t in toks_g)
    assert toks_g == toks_e and lps_g == lps_e
    assert (len(calls) > 0) == bool(mode)


def test_routing_follows_rule(monkeypatch):
    monkeypatch.setattr(ops, "_FP8_SKINNY_FORCE", None)
    monkeypatch.setattr(ops, "FP8_SKINNY_RULE", {(5120, 8192): 64})
    assert ops.linear_fp8_skinny_routed(5120, 8192, 1)
    assert ops.linear_fp8_skinny_routed(5120, 8192, 64)
    assert not ops.linear_fp8_skinny_routed(5120, 8192, 65)
    assert not ops.linear_fp8_skinny_routed(10240, 5120, 8)   # unlisted
    monkeypatch.setattr(ops, "FP8_SKINNY_RULE", {(5120, 8192): 512})
    assert not ops.linear_fp8_skinny_routed(5120, 8192, 257)  # kernel limit


def test_routing_force_and_restore(monkeypatch):
    monkeypatch.setattr(ops, "_FP8_SKINNY_FORCE", None)
    monkeypatch.setattr(ops, "FP8_SKINNY_RULE", {(5120, 8192): 64})
    ops.set_linear_fp8_skinny(True)
    assert ops.linear_fp8_skinny_routed(64, 128, 256)
    assert not ops.linear_fp8_skinny_routed(64, 128, 257)
    ops.set_linear_fp8_skinny(False)
    assert not ops.linear_fp8_skinny_routed(5120, 8192, 8)
    ops.set_linear_fp8_skinny(None)
    assert ops.linear_fp8_skinny_routed(5120, 8192, 8)
    assert not ops.linear_fp8_skinny_routed(64, 128, 8)
