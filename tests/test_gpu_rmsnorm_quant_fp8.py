"""GPU tests for ops.rmsnorm_quant_fp8 (csrc/rmsnorm_quant_fp8.hip): bit
equality with the two-kernel sequence it replaces, an f64 reference with a
bound derived from the number formats, and hipGraph replay."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sutro_amd import ops
    from sutro_amd.ops import torch_ref
else:  # collected on CPU; every test is skipped by the marker filter anyway
    ops = torch_ref = None

DEV = "cuda"
EPS = 1e-6
# rows: one partly filled wave; K % 8 only (zero tail to 256); NCH = 1 full;
# NCH = 2 with one live chunk; the hot width; NCH = 8. 2050 rows pass the
# 2048-block grid cap (grid-stride loop, both LDS buffers).
C_ROWS = (128, 136, 2048, 2056, 5120, 16384)
C_BLOCK = (128, 2048, 2176, 5120, 16384)
CASES = [(mode, R, C)
         for mode, cs in (("rows", C_ROWS), ("block128", C_BLOCK))
         for C in cs for R in (1, 3, 2050) if R < 2050 or C <= 256]


def _inputs(R, C, seed=0):
    """Row 0 all zeros (amax 0 -> scale 1, codes 0); one element of row 1 at
    300, which crushes the rest of its row or group into e4m3 subnormals."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = 3 * torch.randn(R, C, device=DEV, generator=g)
    res = 5 * torch.randn(R, C, device=DEV, generator=g)
    w = 1 + 0.1 * torch.randn(C, device=DEV, generator=g)
    x[0] = 0
    res[0] = 0
    if R > 1:
        x[1, C // 3] = 300
    return x.bfloat16(), res.bfloat16(), w.bfloat16()


def _separate(x, res, w, mode):
    """today's sequence, on clones: norm kernel, then the quantiser op"""
    x = x.clone()
    if res is None:
        y, new_res = ops.rmsnorm(x, w, EPS), x
    else:
        y, new_res = ops.fused_add_rmsnorm(x, res.clone(), w, EPS)
    if mode == "block128":
        return (*ops.quantize_rows_fp8_block128(y), new_res)
    return (*torch_ref.quantize_act_fp8(y, ops.quantize_rows_fp8), new_res)


def _fused(x, res, w, mode):
    return ops.rmsnorm_quant_fp8(x.clone(), None if res is None
                                 else res.clone(), w, EPS, mode)


def _assert_same(got, want):
    for name, a, b in zip(("codes", "scales", "residual"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        if a.dtype == torch.float8_e4m3fn:
            a, b = a.view(torch.uint8), b.view(torch.uint8)
        assert torch.equal(a, b), name


@pytest.mark.parametrize("with_residual", [True, False])
@pytest.mark.parametrize("mode,R,C", CASES)
def test_bit_equal_to_the_separate_sequence(mode, R, C, with_residual):
    x, res, w = _inputs(R, C)
    if not with_residual:
        res = None
    _assert_same(_fused(x, res, w, mode), _separate(x, res, w, mode))


@pytest.mark.parametrize("mode,R,C", CASES)
def test_against_f64_reference(mode, R, C):
    """|code * s - y| <= |y| (2^-4 + 2^-7) + s 2^-9 for every element, s the
    scale written for it: e4m3's half-ulp for normal codes, the bf16 rounding
    of y plus the f32 arithmetic (together <= 2^-8), and twice the subnormal
    half-step. The scale itself within 2^-7 of amax(|y|) / 448."""
    x, res, w = _inputs(R, C)
    q, s, _ = _fused(x, res, w, mode)
    r = x.double() + res.double()
    y = r * torch.rsqrt((r * r).mean(dim=1, keepdim=True) + EPS) * w.double()
    if mode == "rows":
        assert not q.view(torch.uint8)[:, C:].any()
        s_got = s.double()[:, None]
        amax = y.abs().amax(dim=1, keepdim=True)
        s_el = s_got.expand(R, C)
    else:
        s_got = s.double().t()
        amax = y.abs().view(R, C // 128, 128).amax(dim=2)
        s_el = s_got.repeat_interleave(128, dim=1)
    s_ref = torch.where(amax > 0, amax / 448, torch.ones_like(amax))
    err = (q[:, :C].double() * s_el - y).abs()
    bound = y.abs() * (2.0 ** -4 + 2.0 ** -7) + s_el * 2.0 ** -9
    print("max err / bound:", (err / bound).max().item())
    assert (err <= bound).all()
    assert ((s_got - s_ref).abs() <= 2.0 ** -7 * s_got).all()


@pytest.mark.parametrize("mode", ["rows", "block128"])
def test_graph_replay_equals_eager(mode):
    R, C = 5, 2176 if mode == "block128" else 2056
    sx, sres, w = _inputs(R, C)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.rmsnorm_quant_fp8(sx, sres, w, EPS, mode)  # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = ops.rmsnorm_quant_fp8(sx, sres, w, EPS, mode)
    for seed in (21, 22):
        x, res, _ = _inputs(R, C, seed)
        sx.copy_(x)
        sres.copy_(res)
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(static_out, _fused(x, res, w, mode))
