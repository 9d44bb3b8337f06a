"""Persistent form of the fused gate_up + SwiGLU kernel (csrc/
gemm_tn_pipe.hip: seam prefetch, grouped tile order, wide epilogue stores).

Oracles: every variant keeps each accumulator's MFMA order and the epilogue's
arithmetic, so it must equal the one-tile-per-block kernel with its default
arguments and "plain pipelined GEMM, then silu_mul" bit for bit: no
tolerance anywhere in this file."""

import pytest
import torch

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


def _oracles(x, w, swz):
    v1 = _C.gemm_gate_up_silu(x, w, swz, 1)
    two_step = ops.silu_mul(_C.gemm_tn_pipelined(x, w, None, swz, 1))
    assert torch.equal(v1, two_step)
    return v1


# M, I, K, num_blocks, group_m values, swizzles
CASES = [
    (256, 128, 128, 1, (1,), (2,)),        # one tile, KT = 2
    (130, 256, 128, 1, (1,), (0, 1, 2)),   # two tiles on one block at the
                                           # shortest K: the seam prefetch
                                           # starts in the first K-tile
    (300, 384, 256, 2, (1, 2, 8), (2,)),   # three tiles per block; M-edge tile
                                           # whose second A half is all past
                                           # the end
    (520, 640, 384, 4, (2,), (2,)),        # 15 tiles as 4/4/4/3; remainder
                                           # group of one M-tile
    (256, 256, 128, 8, (1,), (2,)),        # blocks without a tile
    (512, 384, 5120, 3, (8,), (2,)),       # the flagship K
]


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("M,I,K,num_blocks,group_ms,swzs", CASES)
def test_persistent_equals_one_tile_kernel(M, I, K, num_blocks, group_ms,
                                           swzs, wide):
    require_gpu()
    x, w = _operands(M, 2 * I, K, 31)
    for swz in swzs:
        ref = _oracles(x, w, swz)
        for group_m in group_ms:
            got = _C.gemm_gate_up_silu(x, w, swz, 1, 1, group_m, num_blocks,
                                       wide)
            assert got.shape == (M, I)
            assert torch.equal(got, ref), (
                M, I, K, swz, group_m, num_blocks, wide,
                (got != ref).sum().item())
            # the one-tile kernel in the same grouped order
            v1g = _C.gemm_gate_up_silu(x, w, swz, 1, 0, group_m)
            assert torch.equal(v1g, ref), (M, I, K, swz, group_m)


def test_default_grid_and_plain_block_order():
    """num_blocks = 0 (one block per CU), -1 (one per tile) and the order
    without the XCD spans."""
    require_gpu()
    x, w = _operands(520, 2 * 640, 384, 32)
    ref = _oracles(x, w, 2)
    for xswz in (0, 1):
        for wide in (False, True):
            got = _C.gemm_gate_up_silu(x, w, 2, xswz, 1, 2, 0, wide)
            assert torch.equal(got, ref), (xswz, wide)
    got = _C.gemm_gate_up_silu(x, w, 2, 0, 1, 2, 4, False)
    assert torch.equal(got, ref)
    # num_blocks = -1: one block per tile on the persistent kernel's code
    for wide in (False, True):
        got = _C.gemm_gate_up_silu(x, w, 2, 1, 1, 2, -1, wide)
        assert torch.equal(got, ref), wide


@pytest.mark.parametrize("M,I,K", [
    (2400, 256, 128),   # MT = 10 on 8 labels: one whole row each + 2 leftover
    (520, 640, 384),    # MT = 3 < 8 labels: leftover rows only
    (4360, 128, 128),   # MT = 18: bands of 2 rows, M edge in a leftover row
])
def test_banded_order(M, I, K):
    """group_m < 0: every XCD label walks its own band of M-tiles; both
    kernels, several grids, narrow and wide stores."""
    require_gpu()
    x, w = _operands(M, 2 * I, K, 37)
    ref = _oracles(x, w, 2)
    for group_m in (-8, -1):
        assert torch.equal(_C.gemm_gate_up_silu(x, w, 2, 1, 0, group_m), ref)
        for num_blocks in (0, 3, 16, -1):
            for wide in (False, True):
                got = _C.gemm_gate_up_silu(x, w, 2, 1, 1, group_m,
                                           num_blocks, wide)
                assert torch.equal(got, ref), (group_m, num_blocks, wide)
    with pytest.raises(RuntimeError, match="xcd_swz"):
        _C.gemm_gate_up_silu(x, w, 2, 0, 0, -8)


def test_persistent_rejects_odd_k_tile_count():
    require_gpu()
    x, w = _operands(256, 256, 192, 33)
    with pytest.raises(RuntimeError, match="K % 128 == 0"):
        _C.gemm_gate_up_silu(x, w, 2, 1, 1, 0, 0, False)
    # the one-tile kernel still takes it
    assert _C.gemm_gate_up_silu(x, w, 2, 1).shape == (256, 128)


def test_persistent_ordering_screen():
    """A misplaced seam read passes most runs: 5 blocks walk 7/7/6/6/6 tiles;
    repeat with other work filling the stream between the calls and require
    every result to equal the first and the oracle, bit for bit."""
    require_gpu()
    M, I, K = 2048, 512, 5120
    x, w = _operands(M, 2 * I, K, 34)
    ref = _oracles(x, w, 2)
    filler = torch.empty(1 << 24, device=DEV)
    first = None
    for it in range(20):
        filler.normal_()
        wide = bool(it & 1)
        got = _C.gemm_gate_up_silu(x, w, 2, 1, 1, 8, 5, wide)
        if first is None:
            first = got
        assert torch.equal(got, first), it
        assert torch.equal(got, ref), it


def test_persistent_graph_capture():
    require_gpu()
    M, I, K = 300, 256, 512
    _, w = _operands(M, 2 * I, K, 35)
    ops.set_gate_up_fused(True)
    ops.set_gate_up_variant("persistent,2,wide")
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
        for seed in (41, 42):
            xin, _ = _operands(M, 8, K, seed)
            static_x.copy_(xin)
            graph.replay()
            torch.cuda.synchronize()
            ops.set_gate_up_variant("v1")
            eager = ops.gate_up_silu(xin, w)
            ops.set_gate_up_variant("persistent,2,wide")
            assert torch.equal(static_out, eager), seed
    finally:
        ops.set_gate_up_variant(None)
        ops.set_gate_up_fused(None)


def test_variant_routing():
    """The variant table is consulted only for shapes GATE_UP_FUSED_RULE
    routes to the fused kernel; the held-back buckets and smaller M stay on
    the library pair whatever the table says; every fused call still goes
    through _C.gemm_gate_up_silu; a forced variant reaches the binding."""
    require_gpu()
    (K, N), (min_m, held_back) = next(iter(ops.GATE_UP_FUSED_RULE.items()))
    fused_calls, looked_up = [], []
    real, real_lookup = _C.gemm_gate_up_silu, ops.gate_up_variant

    def counting(x, w, *a, **kw):
        fused_calls.append((x.shape[0],) + tuple(a))
        return real(x, w, *a, **kw)

    def lookup(k, two_i, m):
        looked_up.append(m)
        return real_lookup(k, two_i, m)

    x_all, w = _operands(2 * min_m, N, K, 36)
    saved = dict(ops.GATE_UP_VARIANT_RULE)
    _C.gemm_gate_up_silu, ops.gate_up_variant = counting, lookup
    try:
        ops.GATE_UP_VARIANT_RULE.clear()
        ops.GATE_UP_VARIANT_RULE[(K, N)] = [(2 * min_m, None, 1, 8, True)]
        ms = [min_m - 128, min_m, 2 * min_m] + sorted(held_back)
        routed = [m for m in ms if m >= min_m and m not in held_back]
        outs = {}
        for M in ms:
            outs[M] = ops.gate_up_silu(x_all[:M].contiguous(), w)
        assert looked_up == routed
        assert fused_calls == [
            (min_m,), (2 * min_m, 2, 1, 1, 8, 0, True)]
        ops.gate_up_silu(x_all[:min_m, :256].contiguous(),
                         w[:512, :256].contiguous())   # unlisted shape
        assert looked_up == routed
        # SUTRO_GATE_UP_VARIANT=v1 / set_gate_up_variant("v1") wins over the
        # table, and the result is the same either way
        ops.set_gate_up_variant("v1")
        del fused_calls[:]
        v1 = ops.gate_up_silu(x_all, w)
        assert fused_calls == [(2 * min_m,)]
        assert torch.equal(v1, outs[2 * min_m])
    finally:
        ops.set_gate_up_variant(None)
        ops.GATE_UP_VARIANT_RULE.clear()
        ops.GATE_UP_VARIANT_RULE.update(saved)
        _C.gemm_gate_up_silu, ops.gate_up_variant = real, real_lookup
