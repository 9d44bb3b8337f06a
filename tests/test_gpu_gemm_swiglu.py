"""Pipelined TN GEMM (csrc/gemm_tn_pipe.hip) and its SwiGLU epilogue.

Oracles: the pipelined kernel keeps every accumulator's MFMA order, so its
plain output equals the double-buffered gemm_tn kernel's bit for bit; the
fused kernel rounds both products to bf16 before the activation, so it equals
"plain kernel, then silu_mul" bit for bit."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sutro_amd import _C, ops
else:  # collected on CPU; every test is skipped by the marker filter anyway
    _C = ops = None

DEV = "cuda"


def require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _operands(M, N, K, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = torch.randn(M, K, device=DEV, generator=g).bfloat16()
    w = (torch.randn(N, K, device=DEV, generator=g) / K ** 0.5).bfloat16()
    return x, w


def _old_kernel(x, w, swz, xswz):
    """gemm_tn (256x256 tile) on x zero-padded to a multiple of 256 rows;
    returns the valid rows."""
    M = x.shape[0]
    Mp = (M + 255) // 256 * 256
    if Mp != M:
        xp = torch.zeros(Mp, x.shape[1], dtype=x.dtype, device=x.device)
        xp[:M] = x
        x = xp
    return _C.gemm_tn(x, w, None, 256, 256, swz, xswz)[:M]


@pytest.mark.parametrize("M,N,K", [
    (256, 256, 64),     # one K-tile: prologue and epilogue only
    (256, 256, 128),
    (256, 512, 192),    # odd tile count
    (512, 1000, 640),   # N edge
    (384, 256, 1024),   # M edge (half a tile)
    (130, 256, 256),    # M edge inside the first half-tile
])
def test_pipelined_equals_old_kernel(M, N, K):
    require_gpu()
    x, w = _operands(M, N, K, 11)
    ref = x.float() @ w.t().float()
    scale = ref.abs().max().item()
    for swz in (0, 1, 2):
        for xswz in (0, 1):
            out = _C.gemm_tn_pipelined(x, w, None, swz, xswz)
            old = _old_kernel(x, w, swz, xswz)
            assert out.shape == (M, N)
            assert torch.equal(out, old), (M, N, K, swz, xswz,
                                           (out != old).sum().item())
            rel = (out.float() - ref).abs().max().item() / scale
            assert rel < 2e-2, (M, N, K, swz, xswz, rel)


def test_pipelined_residual_epilogue():
    require_gpu()
    x, w = _operands(300, 520, 384, 12)
    res = torch.randn(300, 520, device=DEV).bfloat16()
    out = _C.gemm_tn_pipelined(x, w, res, 2, 1)
    ref = x.float() @ w.t().float() + res.float()
    rel = (out.float() - ref).abs().max().item() / ref.abs().max().item()
    assert rel < 2e-2, rel


@pytest.mark.parametrize("M,I,K", [
    (256, 128, 64),
    (384, 256, 192),
    (130, 128, 128),
    (512, 384, 5120),   # the flagship K
])
def test_fused_equals_plain_then_silu_mul(M, I, K):
    require_gpu()
    x, w = _operands(M, 2 * I, K, 13)
    lib = ops.silu_mul(F.linear(x, w))
    for swz in (0, 1, 2):
        for xswz in (0, 1):
            fused = _C.gemm_gate_up_silu(x, w, swz, xswz)
            two_step = ops.silu_mul(_C.gemm_tn_pipelined(x, w, None, swz, xswz))
            assert fused.shape == (M, I)
            assert torch.equal(fused, two_step), (
                M, I, K, swz, xswz, (fused != two_step).sum().item())
            assert torch.allclose(fused.float(), lib.float(), atol=3e-2,
                                  rtol=3e-2), (
                M, I, K, swz, xswz, (fused.float() - lib.float()).abs().max())


@pytest.mark.parametrize("M,N,K", [(512, 1024, 1024), (2048, 1024, 5120)])
def test_ordering_screen(M, N, K):
    """A misplaced LDS read passes most runs: repeat both kernels with other
    work filling the stream between calls and require every result to equal
    the first and the old-kernel oracle, bit for bit."""
    require_gpu()
    x, w = _operands(M, N, K, 14)
    plain_ref = _old_kernel(x, w, 2, 1)
    fused_ref = ops.silu_mul(plain_ref)
    filler = torch.empty(1 << 24, device=DEV)
    first_p = first_f = None
    for it in range(20):
        filler.normal_()
        p = _C.gemm_tn_pipelined(x, w, None, 2, 1)
        filler.normal_()
        f = _C.gemm_gate_up_silu(x, w, 2, 1)
        if it == 0:
            first_p, first_f = p, f
            assert torch.equal(p, plain_ref)
            assert torch.equal(f, fused_ref)
        else:
            assert torch.equal(p, first_p), it
            assert torch.equal(f, first_f), it


def test_routing_rule():
    """The committed rule: fused from the measured threshold up, except the
    held-back decode buckets; other shapes and smaller M on the library pair.
    Which path ran is read off a counting wrapper around the binding."""
    require_gpu()
    (K, N), (min_m, held_back) = next(iter(ops.GATE_UP_FUSED_RULE.items()))
    calls = []
    real = _C.gemm_gate_up_silu

    def counting(x, w, *a, **kw):
        calls.append(x.shape[0])
        return real(x, w, *a, **kw)

    x_all, w = _operands(2 * min_m, N, K, 16)
    _C.gemm_gate_up_silu = counting
    try:
        expect = []
        for M in [min_m - 128, min_m, min_m + 1, 2 * min_m] + sorted(held_back):
            out = ops.gate_up_silu(x_all[:M].contiguous(), w)
            assert out.shape == (M, N // 2)
            if M >= min_m and M not in held_back:
                expect.append(M)
        assert calls == expect
        ops.gate_up_silu(x_all[:min_m, :256].contiguous(),
                         w[:512, :256].contiguous())   # unlisted shape
        assert calls == expect
    finally:
        _C.gemm_gate_up_silu = real


def test_gate_up_silu_graph_capture():
    require_gpu()
    M, I, K = 128, 256, 512
    _, w = _operands(M, 2 * I, K, 15)
    ops.set_gate_up_fused(True)
    try:
        static_x = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.gate_up_silu(static_x, w)  # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = ops.gate_up_silu(static_x, w)
        for seed in (21, 22):
            xin, _ = _operands(M, 8, K, seed)
            static_x.copy_(xin)
            graph.replay()
            torch.cuda.synchronize()
            eager = ops.gate_up_silu(xin, w)
            assert torch.equal(static_out, eager), seed
    finally:
        ops.set_gate_up_fused(None)


def test_model_fused_vs_library_path():
    """One forward of a 300-token prefill plus 8 decode rows through a small
    dense model, fused gate_up forced on and then off."""
    require_gpu()
    from sutro_amd.engine.batch import ForwardBatch
    from sutro_amd.engine.kv_cache import PagedKVCache
    from sutro_amd.models.qwen3 import Qwen3Model
    from sutro_amd.models.registry import ModelSpec

    spec = ModelSpec(name="swiglu-test", hidden_size=256, num_layers=2,
                     num_heads=4, num_kv_heads=2, head_dim=128,
                     intermediate_size=512, vocab_size=1024, max_context=512,
                     tie_embeddings=True)
    with torch.device(DEV):
        model = Qwen3Model(spec, torch.bfloat16, 512)
    model.init_random_weights(seed=3)

    bs, P, D, ctx = 32, 300, 8, 4  # decode rows sit at position ctx
    pre_blocks = (P + bs - 1) // bs
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, spec.vocab_size, (P + D,), generator=g)
    positions = list(range(P)) + [ctx] * D
    tables = torch.zeros(1 + D, pre_blocks, dtype=torch.int32)
    tables[0] = torch.arange(1, pre_blocks + 1, dtype=torch.int32)
    slots = [int(tables[0, p // bs]) * bs + p % bs for p in range(P)]
    for d in range(D):
        tables[1 + d, 0] = pre_blocks + 1 + d
        slots.append((pre_blocks + 1 + d) * bs + ctx)
    qlocs = [0, P] + [P + d + 1 for d in range(D)]

    def run(fused):
        ops.set_gate_up_fused(fused)
        try:
            kv = PagedKVCache(num_layers=2, num_blocks=pre_blocks + D + 2,
                              num_kv_heads=2, block_size=bs, head_dim=128,
                              dtype=torch.bfloat16, device=DEV)
            fb = ForwardBatch(
                input_ids=ids.to(DEV),
                positions=torch.tensor(positions, dtype=torch.long, device=DEV),
                slot_mapping=torch.tensor(slots, dtype=torch.long, device=DEV),
                block_tables=tables.to(DEV),
                seq_lens=torch.tensor([P] + [ctx + 1] * D, dtype=torch.int32,
                                      device=DEV),
                query_start_locs=torch.tensor(qlocs, dtype=torch.int32,
                                              device=DEV),
                num_decodes_tail=D,
                logits_idx=torch.tensor([P - 1] + list(range(P, P + D)),
                                        dtype=torch.long, device=DEV),
                max_seq_len=P, max_query_len=P,
                tile_seq=torch.zeros(len(range(0, P, 32)), dtype=torch.int32,
                                     device=DEV),
                tile_q0=torch.arange(0, P, 32, dtype=torch.int32, device=DEV),
                prefill_token_count=P)
            return model(fb, kv).float()
        finally:
            ops.set_gate_up_fused(None)

    calls = []
    real = _C.gemm_gate_up_silu

    def counting(x, w, *a, **kw):
        calls.append(tuple(x.shape))
        return real(x, w, *a, **kw)

    _C.gemm_gate_up_silu = counting
    try:
        on = run(True)
        assert calls == [(P + D, 256)] * 2   # one fused call per layer
        off = run(False)
        assert len(calls) == 2               # forced off: library pair only
    finally:
        _C.gemm_gate_up_silu = real
    assert on.shape == (P + D, 256)
    assert torch.isfinite(on).all()
    assert torch.allclose(on, off, atol=3e-2, rtol=3e-2), (on - off).abs().max()
