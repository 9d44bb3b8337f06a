"""CPU check of the pipelined prefill attention kernel's work assignment
(tools/sim_attn_prefill_pipe.py follows csrc/attn_prefill.hip's index
arithmetic): at every tile granularity each (sequence, 32-row sub-tile, head)
is covered exactly once with the rows, causal bound and page count of the
reference kernel, and no block reads a block-table column at or beyond its
sequence's page count."""

import importlib.util
import pathlib

import pytest

_spec = importlib.util.spec_from_file_location(
    "sim_attn_prefill_pipe",
    pathlib.Path(__file__).parent.parent / "tools" / "sim_attn_prefill_pipe.py")
sim = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sim)

# (ctx, new): fresh prompts around every tile edge, chunk continuations
CASES = [(0, n) for n in (1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 200)]
CASES += [(1, 1), (32, 33), (40, 64), (100, 29), (31, 128)]


def _batch():
    new_counts = [n for _, n in CASES]
    qlocs = [0]
    for n in new_counts:
        qlocs.append(qlocs[-1] + n)
    seq_lens = [c + n for c, n in CASES]
    return new_counts, qlocs, seq_lens


@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("R", sim.GRANULARITIES)
def test_tile_mapping_matches_reference(G, R):
    if sim.pipe_config(G, R) is None:
        assert G * (R // 32) > 16
        return
    new_counts, qlocs, seq_lens = _batch()
    ref = sim.reference_tiles(new_counts, qlocs, seq_lens)
    seen = {}
    ts, tq = sim.build_tiles(new_counts, R)
    assert len(ts) == sum((n + R - 1) // R for n in new_counts)
    for s, q0 in zip(ts, tq):
        plan = sim.block_plan(G, R, s, q0, qlocs, seq_lens)
        assert plan is not None
        n_pages = (seq_lens[s] + sim.BS - 1) // sim.BS
        # never a column at or beyond the sequence's page count, prefetch
        # included, and never beyond what the block itself stages
        assert plan["pages"] <= n_pages
        assert all(0 <= c < plan["pages"] for c in plan["bt_reads"])
        # every staged page's column is read before it is loaded
        assert set(plan["bt_reads"]) == set(range(plan["pages"]))
        heads = set()
        for g, subs in plan["waves"]:
            for row_base, nq, qabs_base, nt_w in subs:
                if nq <= 0:
                    assert nt_w == 0   # idle wave: joins barriers only
                    continue
                assert nt_w <= plan["pages"]
                key = (s, row_base, g)
                assert key not in seen
                seen[key] = (nq, qabs_base, nt_w)
                heads.add(g)
        assert heads == set(range(G))
        # the block's page count is its last active sub-tile's
        assert plan["pages"] == max(x[3] for _, subs in plan["waves"]
                                    for x in subs)
    assert len(seen) == len(ref) * G
    for (s, row_base, g), v in seen.items():
        assert ref[(s, row_base)] == v


def test_pad_tile_is_skipped():
    # dummy sequence of the prefill graph runner: no rows, length 0
    qlocs, seq_lens = [0, 37, 37], [40, 0]
    for R in sim.GRANULARITIES:
        assert sim.block_plan(4, R, 1, 0, qlocs, seq_lens) is None


def test_supported_configurations():
    assert sim.pipe_config(8, 32) == (8, 1)
    assert sim.pipe_config(8, 64) == (8, 2)
    assert sim.pipe_config(8, 128) is None
    assert sim.pipe_config(4, 128) == (8, 2)
    assert sim.pipe_config(1, 128) == (4, 1)
    assert sim.pipe_config(3, 32) is None
    # 16 heads per kv head would need 16 waves for one sub-tile
    for rows in sim.GRANULARITIES:
        assert sim.pipe_config(16, rows) is None


def test_python_mirror_agrees_with_sim():
    from sutro_amd import ops
    for g in (1, 2, 3, 4, 8, 16):
        for d in (64, 128):
            for rows in sim.GRANULARITIES:
                assert ops.attn_prefill_pipe_supported(g * 2, 2, d, rows) == (
                    sim.pipe_config(g, rows) is not None), (g, d, rows)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("NW", [1, 2, 4, 8])
def test_v_staging_covers_page_without_bank_conflicts(D, NW):
    NT = NW * 64
    items = sim.v_stage_items(D, NT)
    cells = {(kvp, c4) for _, kvp, c4 in items}
    assert len(items) == len(cells) == 16 * (D // 4)
    for banks in sim.v_write_banks(D, NT):
        assert len(banks) == len(set(banks))
