"""CPU check of the fused gate_up kernel's index flow (tools/
sim_gemm_swiglu.py follows csrc/gemm_tn_pipe.hip lane by lane) against
silu_mul(x @ w.T) with the two-step rounding (GEMM output rounded to bf16,
then the activation)."""

import importlib.util
import pathlib

import numpy as np
import pytest
import torch

from sutro_amd.ops import torch_ref as R

_spec = importlib.util.spec_from_file_location(
    "sim_gemm_swiglu",
    pathlib.Path(__file__).parent.parent / "tools" / "sim_gemm_swiglu.py")
sim = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sim)


def _case(M, I, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(2 * I, K, generator=g) / K ** 0.5).bfloat16()
    return x, w


@pytest.mark.parametrize("M,I,K", [(256, 128, 64), (384, 256, 192),
                                   (130, 128, 128)])
def test_fused_index_flow_matches_silu_mul(M, I, K):
    x, w = _case(M, I, K, 3)
    ref = R.silu_mul((x.float() @ w.float().t()).bfloat16()).float().numpy()
    xn, wn = x.float().numpy(), w.float().numpy()
    # both landing extremes of the staged half-tiles (at issue / only at the
    # counted wait) on the default swizzle; the other modes once each
    runs = [(2, False), (2, True)]
    if (M, I, K) == (130, 128, 128):
        runs += [(0, True), (1, True)]
    for mode, lazy in runs:
        got = sim.sim(mode, 2, xn, wn, lazy)
        assert got.shape == (M, I)
        assert not np.isnan(got).any(), "an output element was never stored"
        # one bf16 ulp: torch's fp32 matmul / exp may round a tie differently
        # from the simulation's float64 sums; a wrong index is O(1) off
        np.testing.assert_allclose(got, ref, rtol=2.0 ** -7, atol=2.0 ** -14)


def test_plain_index_flow_with_edges():
    """Plain epilogue, M edge inside the second half-tile and N edge with a
    B half wholly past the end (N = 300: tile 1 holds 44 columns)."""
    x, w = _case(300, 150, 128, 4)
    xn, wn = x.float().numpy(), w.float().numpy()
    ref = sim.reference(0, xn, wn)
    for lazy in (False, True):
        got = sim.sim(2, 0, xn, wn, lazy)
        assert np.array_equal(got, ref)
