"""CPU check of the persistent gate_up kernel's index flow: tools/
sim_gemm_swiglu.py follows one block of csrc/gemm_tn_pipe.hip's persistent
kernel over its whole tile list (seam staging through the tail slots, staged
loads pending across the epilogue, grouped tile order) against
silu_mul(x @ w.T) with the two-step rounding. In the lazy landing mode a seam
read placed before its data lands reads the previous tile and fails here."""

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


# the first four shapes of tests/test_gpu_gemm_swiglu_persistent.py
@pytest.mark.parametrize("M,I,K,num_blocks,group_ms,modes", [
    (256, 128, 128, 1, (1,), (2,)),
    (130, 256, 128, 1, (1,), (0, 1, 2)),
    (300, 384, 256, 2, (1, 2, 8), (2,)),
    (520, 640, 384, 4, (2,), (2,)),
])
def test_persistent_index_flow_matches_silu_mul(M, I, K, num_blocks, group_ms,
                                                modes):
    x, w = _case(M, I, K, 5)
    ref = R.silu_mul((x.float() @ w.float().t()).bfloat16()).float().numpy()
    xn, wn = x.float().numpy(), w.float().numpy()
    for mode in modes:
        for group_m in group_ms:
            for lazy in (False, True):
                got = sim.sim_persistent(mode, xn, wn, num_blocks, group_m,
                                         lazy)
                assert got.shape == (M, I)
                assert not np.isnan(got).any(), \
                    "an output element was never stored"
                # one bf16 ulp: torch's fp32 matmul / exp may round a tie
                # differently from the simulation's float64 sums; a wrong
                # index or a stale tile is O(1) off
                np.testing.assert_allclose(got, ref, rtol=2.0 ** -7,
                                           atol=2.0 ** -14)


def test_one_tile_kernel_in_grouped_order():
    x, w = _case(520, 384, 128, 6)
    xn, wn = x.float().numpy(), w.float().numpy()
    plain = sim.sim(2, 2, xn, wn, True)
    assert not np.isnan(plain).any()
    assert np.array_equal(sim.sim(2, 2, xn, wn, True, group_m=2), plain)


@pytest.mark.parametrize("MT", [1, 5, 8, 9, 64, 121])
@pytest.mark.parametrize("group_m", [-8, -3])
@pytest.mark.parametrize("num_blocks", [1, 5, 256])
def test_banded_order_visits_every_tile_once(MT, group_m, num_blocks):
    NT = 200
    tiles = MT * NT
    per_block = [sim.block_coords(bid, num_blocks, MT, NT, group_m)
                 for bid in range(num_blocks)]
    walked = [c for cs in per_block for c in cs]
    assert len(walked) == tiles and len(set(walked)) == tiles
    assert all(0 <= m < MT and 0 <= n < NT for m, n in walked)
    # the same tile counts as the plain order's balanced spans
    assert [len(cs) for cs in per_block] == [
        len(sim.block_tiles(bid, num_blocks, tiles))
        for bid in range(num_blocks)]
    # the one-tile kernel's blocks cover the grid too
    one = [sim.one_tile_coords(bid, tiles, MT, NT, group_m)
           for bid in range(tiles)]
    assert len(set(one)) == tiles
    assert all(0 <= m < MT and 0 <= n < NT for m, n in one)
    if num_blocks == 256 and MT >= 8:
        # while in their bands, the 8 labels sit at the same N-tile
        a = MT // 8
        for i in range(0, a * NT, 97):
            nts = {sim.tile_mn_banded(xl, i, 8, MT, NT, group_m)[1]
                   for xl in range(8)}
            assert len(nts) == 1


def test_banded_index_flow():
    """MT = 10 on 8 labels (one whole row each, two leftover rows) through
    the persistent walk and the one-tile kernel, lazy landing."""
    x, w = _case(2400, 256, 128, 8)
    xn, wn = x.float().numpy(), w.float().numpy()
    ref = sim.sim(2, 2, xn, wn, True)
    assert not np.isnan(ref).any()
    assert np.array_equal(sim.sim(2, 2, xn, wn, True, group_m=-8), ref)
    assert np.array_equal(sim.sim_persistent(2, xn, wn, 16, -8, True), ref)
    assert np.array_equal(sim.sim_persistent(2, xn, wn, 3, -2, True), ref)


@pytest.mark.parametrize("MT", [1, 5, 8, 121])
@pytest.mark.parametrize("group_m", [1, 4, 8, 16])
@pytest.mark.parametrize("num_blocks", [1, 5, 256])
def test_grouped_order_visits_every_tile_once(MT, group_m, num_blocks):
    NT = 200
    tiles = MT * NT
    for xcd_swz in (0, 1):
        walked = [t for bid in range(num_blocks)
                  for t in sim.block_tiles(bid, num_blocks, tiles, xcd_swz)]
        assert sorted(walked) == list(range(tiles))
        counts = [len(sim.block_tiles(bid, num_blocks, tiles, xcd_swz))
                  for bid in range(num_blocks)]
        if num_blocks <= 8 or num_blocks % 8 == 0:
            assert max(counts) - min(counts) <= 1
    coords = [sim.tile_mn(t, MT, NT, group_m) for t in range(tiles)]
    assert len(set(coords)) == tiles
    assert all(0 <= m < MT and 0 <= n < NT for m, n in coords)
    if group_m >= MT:   # today's order: m fastest over all M-tiles
        assert coords == [(t % MT, t // MT) for t in range(tiles)]
    else:               # a full group's first tiles are group_m x (NT) blocks
        head = coords[:group_m * min(4, NT)]
        assert head == [(i % group_m, i // group_m) for i in range(len(head))]
