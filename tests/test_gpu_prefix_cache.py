"""GPU tests for the prefix KV cache: the shared-prefix decode attention
kernels (csrc/attn_decode_prefix.hip + the CONT instantiation of the per-row
MFMA kernel) against the per-row kernel (bit-equal) and the fp32 reference,
and the engine with hipGraph decode in "shared" and "per_row" mode."""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sutro_amd import ops
    from sutro_amd.ops import torch_ref

DEV = "cuda"
F8 = torch.float8_e4m3fn
BS = 32


def require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---- kernel tests ----

# batch row -> (group, positions beyond the prefix). Group A shares P = 3
# pages, group B is a single row with P = 1, row 1 has P = 0 and no tile.
GROUP_PAGES = {"A": [29, 17, 5], "B": [11], None: []}   # descending, gaps
ROWS = [("A", 1), (None, 45), ("A", 31), ("B", 33), ("A", 32), ("A", 33),
        ("A", 65)]
NUM_TILES = 5          # tile 1 and the trailing tiles 3, 4 stay all -1
NUM_BLOCKS, BT_WIDTH = 40, 8


@functools.lru_cache(maxsize=None)
def _case(D, kv_fp8, Hq, Hk):
    """Inputs, the per-row kernel's output and the fp32 reference, computed
    once per parameter set and shared by the three kernel tests."""
    torch.manual_seed(D + 7 * Hq + Hk + (1000 if kv_fp8 else 0))
    n = len(ROWS)
    R = ops.prefix_tile_rows(Hq, Hk)
    k = torch.randn(NUM_BLOCKS, Hk, BS, D) * 0.5
    v = torch.randn(NUM_BLOCKS, Hk, BS, D) * 0.5
    kd = k.to(F8) if kv_fp8 else k.bfloat16()
    vd = v.to(F8) if kv_fp8 else v.bfloat16()
    q = torch.randn(n, Hq, D).bfloat16()
    private = [p for p in range(NUM_BLOCKS - 1, 0, -1)
               if all(p not in g for g in GROUP_PAGES.values())]
    bt = torch.zeros(n, BT_WIDTH, dtype=torch.int32)
    lens, rpp = [], []
    for i, (grp, beyond) in enumerate(ROWS):
        shared = GROUP_PAGES[grp]
        L = len(shared) * BS + beyond
        pages = (L + BS - 1) // BS
        row = shared + [private.pop(0) for _ in range(pages - len(shared))]
        bt[i, :pages] = torch.tensor(row, dtype=torch.int32)
        lens.append(L)
        rpp.append(len(shared))
    # group A's five rows spread over the whole tile (every column block,
    # with -1 gaps between them); group B's single row in the last slot
    tiles = torch.full((NUM_TILES, R), -1, dtype=torch.int32)
    rows_a = [i for i, (g, _) in enumerate(ROWS) if g == "A"]
    for j, i in enumerate(rows_a):
        tiles[0, (j * (R - 1)) // (len(rows_a) - 1)] = i
    tiles[2, R - 1] = [g for g, _ in ROWS].index("B")
    sl = torch.tensor(lens, dtype=torch.int32)
    ql = torch.arange(n + 1, dtype=torch.int32)
    scale = 1.0 / math.sqrt(D)
    g = dict(q=q.to(DEV), k=kd.to(DEV), v=vd.to(DEV), bt=bt.to(DEV),
             sl=sl.to(DEV), ql=ql.to(DEV), scale=scale, n=n,
             rpp=torch.tensor(rpp, dtype=torch.int32, device=DEV),
             tiles=tiles.to(DEV))
    g["per_row"] = ops.paged_attention(g["q"], g["k"], g["v"], g["bt"],
                                       g["sl"], g["ql"], scale,
                                       num_decodes_tail=n).cpu()
    g["fp32"] = torch_ref.paged_attention(q.float(), kd.float(), vd.float(),
                                          bt, sl, ql, scale)
    return g


KERNEL_PARAMS = [(D, f8, hq, hk) for D in (64, 128) for f8 in (False, True)
                 for hq, hk in ((8, 1), (4, 2), (12, 4))]
param_kernel = pytest.mark.parametrize("D,kv_fp8,Hq,Hk", KERNEL_PARAMS)


def _shared(g, rpp, tiles):
    out = ops.paged_attention_decode_shared(g["q"], g["k"], g["v"], g["bt"],
                                            g["sl"], g["scale"], rpp, tiles)
    torch.cuda.synchronize()
    return out.cpu()


@param_kernel
def test_shared_bit_equal_to_per_row(D, kv_fp8, Hq, Hk):
    """Two groups (P = 3 spread over every column block, P = 1 single row),
    one row in no tile, suffixes of 1/31/32/33 positions, descending shared
    page ids, empty tiles in the middle and at the end: the output equals the
    per-row kernel's bit for bit. (With G = 2 a column block holds 8 rows,
    more than the 7 here; the spread over four blocks covers that path.)"""
    require_gpu()
    g = _case(D, kv_fp8, Hq, Hk)
    got = _shared(g, g["rpp"], g["tiles"])
    assert torch.equal(got, g["per_row"]), (
        (got.float() - g["per_row"].float()).abs().max())


@param_kernel
def test_shared_matches_fp32_reference(D, kv_fp8, Hq, Hk):
    require_gpu()
    g = _case(D, kv_fp8, Hq, Hk)
    got = _shared(g, g["rpp"], g["tiles"]).float()
    err = (got - g["fp32"]).abs().max()
    assert torch.allclose(got, g["fp32"], atol=3e-2, rtol=3e-2), err


@param_kernel
def test_shared_with_no_prefix_is_per_row(D, kv_fp8, Hq, Hk):
    """Every row_prefix_pages = 0 and all tiles empty: the CONT kernel alone
    is the per-row kernel."""
    require_gpu()
    g = _case(D, kv_fp8, Hq, Hk)
    got = _shared(g, torch.zeros_like(g["rpp"]),
                  torch.full_like(g["tiles"], -1))
    assert torch.equal(got, g["per_row"])


# ---- engine tests ----

PREFIX_LEN, NUM_ROWS = 96, 12


def _spec():
    from sutro_amd.models.registry import ModelSpec

    return ModelSpec(name="tiny-prefix-gpu", hidden_size=256, num_layers=2,
                     num_heads=4, num_kv_heads=2, head_dim=64,
                     intermediate_size=512, vocab_size=2048, max_context=512,
                     tie_embeddings=True)


def _prompts():
    import random

    rng = random.Random(5)
    prefix = [rng.randrange(3, 2000) for _ in range(PREFIX_LEN)]
    return [prefix + [rng.randrange(3, 2000)
                      for _ in range(rng.randint(5, 39))]
            for _ in range(NUM_ROWS)]


def _run_engine(prefix_caching, prefix_decode):
    """12 rows behind one 96-token prefix, admitted over several steps
    (128-token step budget), half greedy and half seeded at temperature 0.7,
    hipGraph decode. Returns what the tests compare."""
    from sutro_amd.engine.config import EngineConfig
    from sutro_amd.engine.engine import LLMEngine
    from sutro_amd.engine.request import SamplingParams

    cfg = EngineConfig(spec=_spec(), device=DEV, max_model_len=256,
                       num_kv_blocks=128, max_num_seqs=16,
                       max_tokens_per_step=128, seed=0,
                       enable_prefix_caching=prefix_caching,
                       prefix_decode=prefix_decode)
    eng = LLMEngine(cfg)
    reqs = []
    for i, p in enumerate(_prompts()):
        sp = (SamplingParams(max_tokens=24, temperature=0.0) if i % 2 == 0
              else SamplingParams(max_tokens=24, temperature=0.7, seed=11 + i))
        reqs.append(eng.add_request(p, sp))
    tables_ok = True
    steps = 0
    while eng.has_work():
        eng.step()
        steps += 1
        assert steps < 2000
        if prefix_caching:
            for r in eng.scheduler.running:
                t = eng.kv.block_tables[r.req_id]
                nhit = r.prefix_hit_tokens // BS
                tables_ok &= all(eng.kv.allocator.is_registered(b)
                                 for b in t[:nhit])
                tables_ok &= eng.kv.prefix_blocks.get(r.req_id, 0) >= nhit
    return dict(
        tokens=[list(r.output_token_ids) for r in reqs],
        logprobs=[r.cumulative_logprob for r in reqs],
        finished=[r.finish_reason is not None for r in reqs],
        hits=[r.prefix_hit_tokens for r in reqs],
        hit_tokens=eng.prefix_hit_tokens,
        tile_steps=eng.prefix_tile_steps,
        graph=eng.graph_runner is not None,
        shared=eng.prefix_shared,
        tables_ok=tables_ok,
    )


@functools.lru_cache(maxsize=None)
def _engine_run(prefix_caching, prefix_decode):
    return _run_engine(prefix_caching, prefix_decode)


def test_engine_shared_equals_per_row():
    """Both with the cache on: the shared route is bit-identical attention,
    so tokens AND cumulative logprobs are equal, greedy and seeded rows."""
    require_gpu()
    shared = _engine_run(True, "shared")
    per_row = _engine_run(True, "per_row")
    assert shared["shared"] and not per_row["shared"]
    assert shared["tokens"] == per_row["tokens"]
    assert shared["logprobs"] == per_row["logprobs"]
    assert shared["hits"] == per_row["hits"]


def test_engine_shared_runs_tiles_under_graph():
    require_gpu()
    first = _engine_run(True, "shared")
    assert first["graph"]
    assert all(first["finished"])
    assert first["hit_tokens"] > 0
    assert first["tile_steps"] > 0
    again = _run_engine(True, "shared")
    assert again["tokens"] == first["tokens"]
    assert again["logprobs"] == first["logprobs"]
    assert again["tile_steps"] == first["tile_steps"]


def test_engine_cache_on_vs_off():
    """The prefill GEMMs see another M with the cache on and may differ in
    the last bits, so tokens are not compared across on/off: both complete,
    hit rows' tables begin with registered blocks, and the cache-on greedy
    outputs reproduce."""
    require_gpu()
    off = _engine_run(False, "per_row")
    on = _engine_run(True, "per_row")
    assert all(off["finished"]) and all(on["finished"])
    assert off["hit_tokens"] == 0 and on["hit_tokens"] > 0
    assert all(h % BS == 0 and h <= PREFIX_LEN for h in on["hits"])
    assert on["tables_ok"]
    again = _run_engine(True, "per_row")
    greedy = range(0, NUM_ROWS, 2)
    assert [again["tokens"][i] for i in greedy] == \
        [on["tokens"][i] for i in greedy]
