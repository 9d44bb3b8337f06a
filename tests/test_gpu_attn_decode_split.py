"""GPU tests for split-KV MFMA decode attention (csrc/attn_decode_split.hip)
against torch_ref.paged_attention in float64 on the same rounded inputs, and
against the per-row kernel where equality is derivable."""

import functools
import gc
import math
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sutro_amd import _C, ops
    from sutro_amd.ops import torch_ref as R

DEV = "cuda"
BS = 32
P, W = 4, 4   # SPLIT_MIN_PAGES, SPLIT_W of the kernel file


def require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def boundary_lens(S):
    """Every boundary of the chunking at S block-splits: page edges, one
    wave's minimum, one block, all S blocks, and ~3x that (per_wave >
    MIN_PAGES, a ragged last wave); the short rows leave waves and blocks
    empty in the same launch."""
    a, b, c = BS * P, BS * P * W, BS * P * W * S
    return (1, 31, 32, 33, a - 1, a, a + 1, b, b + 1, c - 1, c + 33,
            3 * c + 77)


@functools.lru_cache(maxsize=2)
def _batch(lens, Hq, Hk, D, kv8, seed=5):
    """A scattered paged cache, one decode row per length, and the float64
    reference (with and without sinks), computed once."""
    torch.manual_seed(seed)
    n = len(lens)
    pages = [(L + BS - 1) // BS for L in lens]
    perm = torch.randperm(sum(pages) + 3)
    dt = torch.float8_e4m3fn if kv8 else torch.bfloat16
    kc = torch.zeros(sum(pages) + 3, Hk, BS, D, dtype=dt, device=DEV)
    vc = torch.zeros_like(kc)
    bt = torch.zeros(n, max(pages), dtype=torch.int32)
    i = 0
    for s, (L, np_) in enumerate(zip(lens, pages)):
        bt[s, :np_] = perm[i:i + np_].to(torch.int32)
        i += np_
        pos = torch.arange(L)
        slots = bt[s, pos // BS].long() * BS + pos % BS
        R.write_kv_cache(torch.randn(L, Hk, D).bfloat16().to(DEV),
                         torch.randn(L, Hk, D).bfloat16().to(DEV), kc, vc,
                         slots.to(DEV))
    q = torch.randn(n, Hq, D).bfloat16().to(DEV)
    sl = torch.tensor(lens, dtype=torch.int32)
    ql = torch.arange(n + 1, dtype=torch.int32)
    sinks = torch.randn(Hq) * 2
    scale = 1.0 / math.sqrt(D)
    ref = [R.paged_attention(q.cpu().double(), kc.cpu().float().double(),
                             vc.cpu().float().double(), bt, sl, ql, scale,
                             sinks=sk) for sk in (None, sinks)]
    return dict(q=q, kc=kc, vc=vc, bt=bt.to(DEV), sl=sl.to(DEV),
                ql=ql.to(DEV), scale=scale, sinks=sinks.to(DEV), ref=ref,
                lens=lens)


def _run(b, S, rows=None, sinks=None, ws=None):
    """Decode rows `rows` (default: all) of batch b. S = 0: the per-row
    kernel; S >= 1: the split kernels forced to S block-splits."""
    rows = slice(None) if rows is None else rows
    q, bt, sl = b["q"][rows], b["bt"][rows], b["sl"][rows]
    n = q.shape[0]
    ops.set_decode_kv_splits(S or None)
    try:
        return ops.paged_attention(
            q, b["kc"], b["vc"], bt, sl, b["ql"][:n + 1], b["scale"],
            num_decodes_tail=n, sinks=sinks, kv_splits=2 if S else 1,
            split_workspace=ws)
    finally:
        ops.set_decode_kv_splits(None)


def _close(got, ref):
    err = (got.double().cpu() - ref).abs().max().item()
    print("max abs err", err)
    assert torch.allclose(got.double().cpu(), ref, atol=3e-2, rtol=3e-2), err


@pytest.mark.parametrize("S", [1, 2, 3, 16])
@pytest.mark.parametrize("Hq,Hk", [(16, 2), (6, 2)])
@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_split_matches_f64_reference(D, kv8, Hq, Hk, S):
    require_gpu()
    b = _batch(boundary_lens(S), Hq, Hk, D, kv8)
    _close(_run(b, S), b["ref"][0])


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("D,kv8", [(128, False), (64, True)])
def test_one_part_rows_equal_the_per_row_kernel(D, kv8, S):
    """npages <= MIN_PAGES: one non-empty wave, weight e(0) = 1, the per-row
    kernel's epilogue: the same bits, beside longer rows or not."""
    require_gpu()
    b = _batch(boundary_lens(4), 16, 2, D, kv8)
    short = [i for i, L in enumerate(b["lens"]) if L <= BS * P]
    assert len(short) == 6
    want = _run(b, 0)[short]
    assert torch.equal(_run(b, S)[short], want)
    assert torch.equal(_run(b, S, rows=short), want)


@pytest.mark.parametrize("S", [1, 4])
def test_row_invariance_and_no_unwritten_slot_read(S):
    require_gpu()
    b = _batch(boundary_lens(4), 16, 2, 128, False)
    n, long_row = len(b["lens"]), len(b["lens"]) - 1
    outs = []
    for _ in range(2):
        ws = ops.alloc_decode_split_workspace(n, 16, 128, S, DEV)
        for t in ws:
            t.fill_(float("nan"))
        outs.append(_run(b, S, ws=ws))
    assert torch.equal(outs[0], outs[1]) and not outs[0].isnan().any()
    alone = _run(b, S, rows=slice(long_row, long_row + 1))
    assert torch.equal(alone[0], outs[0][long_row])


@pytest.mark.parametrize("D,kv8,Hq", [(128, False, 16), (64, True, 6)])
def test_sinks(D, kv8, Hq):
    require_gpu()
    b = _batch(boundary_lens(4), Hq, 2, D, kv8)   # length 1 .. several blocks
    _close(_run(b, 4, sinks=b["sinks"]), b["ref"][1])
    # one non-empty part: the per-row kernel's sink route, bit for bit
    assert torch.equal(_run(b, 4, sinks=b["sinks"])[:4],
                       _run(b, 0, sinks=b["sinks"])[:4])


def test_graph_replay_follows_changed_lengths():
    require_gpu()
    b = _batch(boundary_lens(4), 16, 2, 128, False)
    n = len(b["lens"])
    st = dict(b, bt=b["bt"].clone(), sl=b["sl"].clone())
    ws = ops.alloc_decode_split_workspace(n, 16, 128, 4, DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(st, 4, ws=ws)
    torch.cuda.current_stream().wait_stream(side)
    from sutro_amd.engine.graph_runner import capture_gc_guard

    g = torch.cuda.CUDAGraph()
    with capture_gc_guard(), torch.cuda.graph(g):
        out = _run(st, 4, ws=ws)
    # rows take other lengths and tables in place; q stays
    for order in (torch.arange(n - 1, -1, -1), torch.arange(n),
                  torch.arange(n).roll(5)):
        idx = order.to(DEV)
        st["bt"].copy_(b["bt"][idx])
        st["sl"].copy_(b["sl"][idx])
        g.replay()
        assert torch.equal(out, _run(dict(b, bt=b["bt"][idx], sl=b["sl"][idx]), 4))


def test_argument_checks():
    require_gpu()
    assert _C.decode_split_constants() == (
        W, P, ops.DECODE_SPLIT_S_MAX) == (
        ops.DECODE_SPLIT_WAVES, ops.DECODE_SPLIT_MIN_PAGES, 16)
    b = _batch(boundary_lens(4), 16, 2, 128, False)
    n = len(b["lens"])
    with pytest.raises(ValueError, match="window"):
        ops.paged_attention(b["q"], b["kc"], b["vc"], b["bt"], b["sl"],
                            b["ql"], b["scale"], num_decodes_tail=n,
                            window=64, kv_splits=2)
    small = ops.alloc_decode_split_workspace(n, 16, 128, 3, DEV)
    with pytest.raises(RuntimeError, match="workspace too small"):
        _run(b, 4, ws=small)


def _engine(eager, **kw):
    from sutro_amd.engine.config import EngineConfig
    from sutro_amd.engine.engine import LLMEngine
    from sutro_amd.models.registry import ModelSpec

    spec = ModelSpec(name="split-gpu", hidden_size=256, num_layers=4,
                     num_heads=8, num_kv_heads=2, head_dim=64,
                     intermediate_size=512, vocab_size=1024, max_context=1024,
                     tie_embeddings=True, **kw.pop("spec_kw", {}))
    eng = LLMEngine(EngineConfig(
        spec=spec, device=DEV, max_model_len=1024, num_kv_blocks=256,
        max_tokens_per_step=2048, max_num_seqs=16, seed=0,
        decode_kv_splits="auto",
        enforce_eager=eager, **kw))
    assert eng.decode_split and (eager or eng.graph_runner is not None)
    return eng


def _engine_run(eager, **kw):
    from sutro_amd.engine.request import SamplingParams

    eng = _engine(eager, **kw)
    # 5 .. 19 pages: several waves and, at S = 4, several blocks non-empty
    reqs = [eng.add_request(list(range(3 + i, 3 + i + n)),
                            SamplingParams(max_tokens=24, temperature=0.7,
                                           seed=3 + i))
            for i, n in enumerate((150, 257, 300, 600))]
    while eng.has_work():
        eng.step()
    return ([list(r.output_token_ids) for r in reqs],
            [r.cumulative_logprob for r in reqs])


@pytest.mark.parametrize("kw", [
    {}, {"kv_dtype": "fp8_e4m3"},
    {"local_attention": True,
     "spec_kw": dict(sliding_window=32, sliding_window_pattern=2,
                     attention_sinks=True)}], ids=["bf16", "fp8", "local"])
def test_engine_graph_decode_equals_eager(kw):
    require_gpu()
    ops.set_decode_kv_splits(4)
    try:
        graph = _engine_run(False, **dict(kw))
        eager = _engine_run(True, **dict(kw))
    finally:
        ops.set_decode_kv_splits(None)
        gc.collect()   # the dropped engines' hipGraphs die here, not later
    assert all(len(t) > 0 for t in graph[0])
    assert graph == eager


def test_capture_destroys_dropped_graphs_first_and_keeps_gc_out():
    """A dropped engine is cyclic garbage that owns hipGraphs, and destroying
    one inside a later capture aborts the process: the next engine's capture
    collects it before it starts and runs with the collector off."""
    require_gpu()
    old = _engine(False)
    dead = weakref.ref(old.graph_runner.graphs[8])
    del old
    try:
        new = _engine(False)
        assert dead() is None and gc.isenabled()
        del new
    finally:
        gc.collect()
