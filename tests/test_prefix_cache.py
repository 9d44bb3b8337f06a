"""Block-hash prefix KV cache (CPU): engine equality with the cache on and
off, the block-aligned hit cap, preemption + eviction, scheduler/allocator
invariants under random interleavings, the graph runner's shared-prefix
staging, and the shared-prefix decode op's CPU path."""

import random

import numpy as np
import torch
from hypothesis import given, settings, strategies as st

from sutro_amd import ops
from sutro_amd.engine.batch import ScheduledBatch
from sutro_amd.engine.config import EngineConfig
from sutro_amd.engine.engine import LLMEngine
from sutro_amd.engine.kv_cache import PagedKVCache
from sutro_amd.engine.request import FinishReason, Request, SamplingParams
from sutro_amd.engine.scheduler import Scheduler
from sutro_amd.models.registry import tiny_spec_for_tests

BS = 32


def _engine(prefix, **kw):
    kw.setdefault("max_model_len", 256)
    cfg = EngineConfig(spec=tiny_spec_for_tests(), device="cpu",
                       enable_prefix_caching=prefix, **kw)
    return LLMEngine(cfg)


def _drain(eng):
    while eng.has_work():
        eng.step()


def _shared_prefix_prompts():
    random.seed(0)
    prefix = [random.randrange(3, 250) for _ in range(96)]
    return [prefix + [random.randrange(3, 250)
                      for _ in range(random.randint(5, 39))]
            for _ in range(16)]


def _run_shared_prefix(prefix_caching):
    eng = _engine(prefix_caching, max_num_seqs=16, max_tokens_per_step=96)
    reqs = [eng.add_request(p, SamplingParams(max_tokens=16, temperature=0.0))
            for p in _shared_prefix_prompts()]
    _drain(eng)
    return eng, reqs


def test_engine_equality_cache_on_vs_off():
    """16 rows behind one 96-token prefix, a step budget that cannot hold the
    first wave: later waves hit, and a hit is a re-chunked prefill — token
    for token the same output, logprobs within 1e-4."""
    off, r_off = _run_shared_prefix(False)
    on, r_on = _run_shared_prefix(True)
    for a, b in zip(r_off, r_on):
        assert a.finish_reason is not None and b.finish_reason is not None
        assert a.output_token_ids == b.output_token_ids
        assert abs(a.cumulative_logprob - b.cumulative_logprob) <= 1e-4
    assert on.prefix_hit_tokens > 0
    assert on.prefix_hit_tokens % BS == 0
    assert on.prefix_hit_tokens == sum(r.prefix_hit_tokens for r in r_on)
    assert on.prefix_query_tokens == sum(r.num_prompt_tokens for r in r_on)
    for r in r_on:
        assert r.prefix_hit_tokens % BS == 0
        assert r.prefix_hit_tokens <= r.num_prompt_tokens - 1
    # job accounting: submitted prompt tokens, cache or no cache
    assert on.total_prompt_tokens == off.total_prompt_tokens
    assert on.total_output_tokens == off.total_output_tokens


def test_flag_off_builds_no_index():
    eng, reqs = _run_shared_prefix(False)
    assert not eng.cfg.enable_prefix_caching
    assert not eng.kv.prefix_caching
    assert not hasattr(eng.kv.allocator, "_index")
    assert not hasattr(eng.kv.allocator, "ref")
    assert eng.prefix_hit_tokens == 0 and eng.prefix_query_tokens == 0
    assert eng.kv.prefix_blocks == {}
    assert all(r.prefix_hit_tokens == 0 for r in reqs)


def test_engine_kwargs_reach_the_config():
    """The service and SDK hand engine_kwargs to resolve_engine_config;
    embedding specs force the cache off."""
    from sutro_amd.service.models_map import resolve_engine_config

    kw = {"enable_prefix_caching": True, "prefix_decode": "shared"}
    cfg = resolve_engine_config("qwen-3-0.6b", device="cpu", **kw)
    assert cfg.enable_prefix_caching and cfg.prefix_decode == "shared"
    emb = resolve_engine_config("qwen-3-embedding-0.6b", device="cpu", **kw)
    assert emb.spec.embedding and not emb.enable_prefix_caching
    # "shared" on CPU is the ordinary path
    eng = _engine(True, prefix_decode="shared", max_num_seqs=4)
    assert not eng.prefix_shared


def test_exact_block_prompts():
    """A 64-token prompt equal to a cached one matches one block only (a
    prompt token must be left to compute) and decodes the same; prompts of
    at most one block never hit."""
    random.seed(3)
    p64 = [random.randrange(3, 250) for _ in range(64)]
    sp = SamplingParams(max_tokens=8, temperature=0.0)

    ref = _engine(False, max_num_seqs=4)
    r_ref = ref.add_request(p64, sp)
    _drain(ref)

    eng = _engine(True, max_num_seqs=4)
    first = eng.add_request(p64, sp)
    _drain(eng)
    assert first.prefix_hit_tokens == 0
    again = eng.add_request(p64, sp)
    _drain(eng)
    assert again.prefix_hit_tokens == 32
    assert first.output_token_ids == r_ref.output_token_ids
    assert again.output_token_ids == r_ref.output_token_ids
    for short in (p64[:32], p64[:20], p64[:1]):
        r = eng.add_request(short, sp)
        _drain(eng)
        assert r.prefix_hit_tokens == 0
    # one token past the block: the whole first block is reusable
    r33 = eng.add_request(p64[:33], sp)
    _drain(eng)
    assert r33.prefix_hit_tokens == 32


def _run_tight(prefix_caching):
    random.seed(1)
    pre = [[random.randrange(3, 250) for _ in range(64)] for _ in range(3)]
    prompts = [pre[i % 3] + [random.randrange(3, 250)
                             for _ in range(random.randint(5, 39))]
               for i in range(18)]
    eng = _engine(prefix_caching, max_num_seqs=8, max_tokens_per_step=128,
                  num_kv_blocks=20)
    counts = {"preempt": 0, "evict": 0}
    preempt = eng.scheduler._preempt_one

    def counting_preempt(*a):
        done = preempt(*a)
        counts["preempt"] += bool(done)
        return done

    eng.scheduler._preempt_one = counting_preempt
    if prefix_caching:
        evict = eng.kv.allocator._evict_one

        def counting_evict():
            counts["evict"] += 1
            evict()

        eng.kv.allocator._evict_one = counting_evict
    reqs = [eng.add_request(p, SamplingParams(max_tokens=48, temperature=0.7,
                                              seed=100 + i))
            for i, p in enumerate(prompts)]
    _drain(eng)
    return eng, reqs, counts


def test_preemption_and_eviction():
    """A cache too small for the job preempts rows and evicts cached blocks;
    seeded rows still produce the uncached outputs, and nothing leaks."""
    off, r_off, _ = _run_tight(False)
    on, r_on, counts = _run_tight(True)
    assert counts["preempt"] > 0 and counts["evict"] > 0
    assert on.prefix_hit_tokens > 0
    for a, b in zip(r_off, r_on):
        assert b.finish_reason is not None
        assert a.output_token_ids == b.output_token_ids
    alloc = on.kv.allocator
    assert int(alloc.ref.sum()) == 0 and int(alloc.ref.min()) == 0
    assert not on.kv.block_tables and not on.kv.prefix_blocks
    assert set(alloc._free).isdisjoint(alloc._evictable)
    # everything but the engine's scratch block is free or evictable
    assert len(alloc._free) + len(alloc._evictable) == alloc.num_blocks - 1
    assert alloc.num_free == alloc.num_blocks - 1
    assert on.scratch_block not in alloc._free
    assert on.scratch_block not in alloc._evictable


# ---- property test: scheduler + allocator invariants ----

def _check_prefix_invariants(kv, live_reqs):
    alloc = kv.allocator
    held = {}
    for t in kv.block_tables.values():
        assert len(set(t)) == len(t), "block twice in one table"
        for b in t:
            held[b] = held.get(b, 0) + 1
    for b in range(alloc.num_blocks):
        assert int(alloc.ref[b]) == held.get(b, 0), "refcount != holders"
    free, evictable = alloc._free, list(alloc._evictable)
    assert len(set(free)) == len(free), "block double-freed"
    assert set(free).isdisjoint(held), "block free and referenced"
    assert set(evictable).isdisjoint(held), "block evictable and referenced"
    assert set(free).isdisjoint(evictable)
    assert len(free) + len(evictable) + len(held) == alloc.num_blocks
    assert alloc.num_free == len(free) + len(evictable)
    # index: registered <-> keyed, unregistered blocks at count 0 are free,
    # and no entry outlives its parent
    assert len(alloc._index) == len(alloc._key_of)
    for key, b in alloc._index.items():
        assert alloc._key_of[b] == key
        assert key[0] < 0 or key[0] in alloc._key_of, "orphaned index entry"
        assert b not in free
    for b in evictable:
        assert b in alloc._key_of
    for b, cnt in held.items():
        if cnt > 1:
            assert b in alloc._key_of, "unregistered block shared"
    # a row's leading prefix blocks are registered and hold its prompt
    bs = kv.block_size
    for req in live_reqs:
        table = kv.block_tables.get(req.req_id)
        if table is None:
            continue
        n = kv.prefix_blocks.get(req.req_id, 0)
        assert n * bs >= req.prefix_hit_tokens
        assert n <= len(table)
        parent = -1
        for i in range(n):
            key = alloc._key_of[table[i]]
            assert key[0] == parent
            assert key[1] == tuple(req.prompt_token_ids[i * bs:(i + 1) * bs])
            parent = table[i]


@settings(max_examples=40, deadline=None)
@given(st.data())
def test_prefix_cache_random_interleaving(data):
    num_blocks = data.draw(st.integers(6, 40), label="blocks")
    max_seqs = data.draw(st.integers(1, 10), label="max_seqs")
    budget = data.draw(st.integers(8, 128), label="budget")
    cfg = EngineConfig(spec=tiny_spec_for_tests(), device="cpu",
                       max_num_seqs=max_seqs, max_model_len=256,
                       max_tokens_per_step=budget, min_prefill_batch_tokens=0,
                       num_kv_blocks=num_blocks, enable_prefix_caching=True)
    kv = PagedKVCache(num_layers=1, num_blocks=num_blocks, num_kv_heads=1,
                      block_size=cfg.kv_block_size, head_dim=8,
                      dtype=torch.float32, device="cpu", prefix_caching=True)
    sch = Scheduler(cfg, kv)
    bs = kv.block_size
    # three prefixes that themselves share their first block
    stems = [list(range(3, 35)) + [40 + k] * 70 for k in range(3)]
    rid = [0]
    all_reqs = []

    def submit():
        stem = stems[data.draw(st.integers(0, 2), label="stem")]
        plen = data.draw(st.integers(1, 100), label="plen")
        tail = data.draw(st.integers(0, 20), label="tail")
        mt = data.draw(st.integers(1, 12), label="max_tokens")
        r = Request(req_id=rid[0],
                    prompt_token_ids=stem[:plen] + [200 + rid[0]] * tail,
                    sampling=SamplingParams(max_tokens=mt))
        rid[0] += 1
        all_reqs.append(r)
        sch.add_request(r, priority=data.draw(st.integers(0, 1), label="pri"))

    def run_step():
        sb = sch.schedule()
        for req, c in zip(sb.reqs, sb.num_new_tokens):
            table = kv.block_tables[req.req_id]
            assert req.num_computed_tokens + c <= len(table) * bs
            assert req.prefix_hit_tokens <= req.num_prompt_tokens - 1
            assert req.prefix_hit_tokens % bs == 0
            # no slot written this step lies in a registered block
            for pos in range(req.num_computed_tokens,
                             req.num_computed_tokens + c):
                assert not kv.allocator.is_registered(table[pos // bs])
        _check_prefix_invariants(kv, all_reqs)
        # emulate the engine: advance, register, sample, finish
        for req, c in zip(sb.reqs, sb.num_new_tokens):
            req.num_computed_tokens += c
        for req in sb.reqs[: sb.num_prefills]:
            kv.register_computed(req.req_id, req.prompt_token_ids,
                                 req.num_computed_tokens)
        for req in sb.reqs:
            if not req.in_prefill and req.num_computed_tokens == req.total_len:
                req.output_token_ids.append(65)
                if len(req.output_token_ids) >= req.sampling.max_tokens:
                    sch.finish(req, FinishReason.LENGTH)
        _check_prefix_invariants(kv, all_reqs)

    for _ in range(data.draw(st.integers(5, 30), label="n_ops")):
        op = data.draw(st.sampled_from(["submit", "submit", "abort", "step",
                                        "step", "step"]), label="op")
        if op == "submit" and rid[0] < 24:
            submit()
        elif op == "abort":
            live = [r for r in all_reqs if r.finish_reason is None]
            if live:
                sch.abort_request(data.draw(st.sampled_from(live),
                                            label="victim"))
                _check_prefix_invariants(kv, all_reqs)
            else:
                run_step()
        else:
            run_step()
    for _ in range(800):
        if not sch.has_work():
            break
        run_step()
    assert not sch.has_work()
    assert all(r.finish_reason is not None for r in all_reqs)
    assert int(kv.allocator.ref.sum()) == 0
    assert kv.allocator.num_free == kv.allocator.num_blocks


# ---- graph runner staging (no capture) ----

def test_graph_fill_host_shared_tiles():
    """`_fill_host` over shared tables fills bt/slots as before and, in
    shared mode, tiles whose rows have identical leading P entries; every
    row with P > 0 sits in exactly one tile; padding rows get P = 0."""
    from sutro_amd.engine.graph_runner import DecodeGraphRunner
    from sutro_amd.engine.prefix_groups import max_tiles

    bs, B, W, R = 4, 16, 16, 4
    kv = PagedKVCache(num_layers=1, num_blocks=64, num_kv_heads=1,
                      block_size=bs, head_dim=8, dtype=torch.float32,
                      device="cpu", prefix_caching=True)
    scratch = kv.allocator.allocate(1)[0]

    class EngStub:
        prefix_tile_steps = 0

    EngStub.kv = kv
    EngStub.scratch_block = scratch

    r = DecodeGraphRunner.__new__(DecodeGraphRunner)
    r.engine = EngStub()
    r.h_ids = torch.zeros(B, dtype=torch.long)
    r.h_pos = torch.zeros(B, dtype=torch.long)
    r.h_slots = torch.zeros(B, dtype=torch.long)
    r.h_bt = torch.zeros(B, W, dtype=torch.int32)
    r.h_sl = torch.ones(B, dtype=torch.int32)
    r._row_req = np.full(B, -1, dtype=np.int64)
    r._row_nb = np.zeros(B, dtype=np.int32)
    r._row_gen = np.zeros(B, dtype=np.int64)
    r._arange = np.arange(B, dtype=np.int64)
    r.prefix_shared = True
    r.h_tile_rows = torch.full((max_tiles(B, R), R), -1, dtype=torch.int32)
    r.h_rpp = torch.zeros(B, dtype=torch.int32)

    stem_a = list(range(10, 22))          # 3 full blocks
    stem_b = stem_a[:4] + list(range(50, 58))   # shares block 0 with stem_a
    next_id = [0]

    def admit(prompt, n_out):
        """Admit through the cache as the scheduler does, prefill, register,
        and leave the row mid-decode with n_out sampled tokens."""
        req = Request(req_id=next_id[0], prompt_token_ids=list(prompt),
                      sampling=SamplingParams(max_tokens=64))
        next_id[0] += 1
        matched = kv.match_prefix(req.prompt_token_ids)
        if matched:
            kv.seed(req.req_id, matched)
            req.prefix_hit_tokens = len(matched) * bs
        kv.grow(req.req_id, req.num_prompt_tokens + n_out)
        kv.register_computed(req.req_id, req.prompt_token_ids,
                             req.num_prompt_tokens)
        req.output_token_ids = [60 + i for i in range(n_out)]
        req.num_computed_tokens = req.total_len - 1
        return req

    def check(reqs, bucket):
        sb = ScheduledBatch(reqs=reqs, num_new_tokens=[1] * len(reqs),
                            num_prefills=0)
        r._fill_host(sb, bucket)
        n = len(reqs)
        bt, rpp = r.h_bt.numpy(), r.h_rpp.numpy()
        tiles = r.h_tile_rows.numpy()
        for i, req in enumerate(reqs):
            p = req.num_computed_tokens
            table = kv.block_tables[req.req_id]
            assert r.h_pos[i].item() == p and r.h_sl[i].item() == p + 1
            assert r.h_slots[i].item() == table[p // bs] * bs + p % bs
            assert bt[i, :len(table)].tolist() == table
            # the slot written this step is never in a shared block
            assert kv.allocator.ref[table[p // bs]] == 1
            assert not kv.allocator.is_registered(table[p // bs])
            # a position beyond the prefix, and only registered pages in it
            assert 0 <= rpp[i] <= kv.prefix_blocks.get(req.req_id, 0)
            assert p + 1 > rpp[i] * bs
        assert (rpp[n:] == 0).all()
        seen = []
        used = 0
        for t in range(tiles.shape[0]):
            rows = [int(x) for x in tiles[t] if x >= 0]
            if not rows:
                continue
            used += 1
            assert all(0 <= x < n for x in rows)
            P = int(rpp[rows[0]])
            assert P > 0
            for x in rows:
                assert int(rpp[x]) == P
                assert bt[x, :P].tolist() == bt[rows[0], :P].tolist()
            seen.extend(rows)
        assert len(seen) == len(set(seen)), "row in two tiles"
        assert sorted(seen) == [i for i in range(n) if rpp[i] > 0]
        assert used == r.tiles_used
        return rpp[:n].tolist(), used

    # the first row of each stem computes it; later rows hit
    a0 = admit(stem_a + [90], 1)
    assert a0.prefix_hit_tokens == 0
    rows_a = [admit(stem_a + [91 + i] * (1 + i), 1 + i) for i in range(6)]
    assert all(q.prefix_hit_tokens == 12 for q in rows_a)
    b0 = admit(stem_b + [80], 2)
    assert b0.prefix_hit_tokens == 4          # block 0 of stem_a
    rows_b = [admit(stem_b + [81 + i], 1) for i in range(2)]
    assert all(q.prefix_hit_tokens == 12 for q in rows_b)
    lone = admit(list(range(150, 163)), 1)    # shares with nobody

    reqs = [a0] + rows_a + [b0] + rows_b + [lone]
    rpp, used = check(reqs, 16)
    # 7 rows on stem_a (two tiles of R=4), 3 on stem_b, the loner alone
    assert rpp == [3] * 7 + [3] * 3 + [0]
    assert used == 3

    # rows leave: a group of one is not worth a tile and runs P = 0; the
    # survivors of stem_a still share
    for q in rows_b:
        kv.release(q.req_id)
    for q in rows_a[3:]:
        kv.release(q.req_id)
    reqs = [a0] + rows_a[:3] + [b0, lone]
    rpp, used = check(reqs, 8)
    assert rpp == [3, 3, 3, 3, 0, 0] and used == 1

    # decode on: tables grow, nothing written lands in a shared block
    for q in reqs:
        q.output_token_ids.append(77)
        q.num_computed_tokens += 1
        kv.grow(q.req_id, q.total_len)
    check(reqs, 8)


# ---- the op's CPU path ----

def test_paged_attention_decode_shared_cpu_equals_paged_attention():
    torch.manual_seed(0)
    n, Hq, Hk, D, nb = 5, 4, 2, 16, 24
    R = ops.prefix_tile_rows(Hq, Hk)
    k = torch.randn(nb, Hk, BS, D)
    v = torch.randn(nb, Hk, BS, D)
    q = torch.randn(n, Hq, D)
    bt = torch.zeros(n, 4, dtype=torch.int32)
    shared = [7, 3]
    lens = [65, 90, 64 + 32, 40, 70]
    rpp = [2, 2, 2, 0, 0]
    own = iter(range(10, 24))
    for i in range(n):
        pages = (lens[i] + BS - 1) // BS
        row = (shared[:rpp[i]] + [next(own) for _ in range(pages - rpp[i])])
        bt[i, :pages] = torch.tensor(row, dtype=torch.int32)
    seq_lens = torch.tensor(lens, dtype=torch.int32)
    tiles = torch.full((3, R), -1, dtype=torch.int32)
    tiles[0, :3] = torch.tensor([0, 1, 2], dtype=torch.int32)
    out = ops.paged_attention_decode_shared(
        q, k, v, bt, seq_lens, 0.25, torch.tensor(rpp, dtype=torch.int32),
        tiles)
    ref = ops.paged_attention(q, k, v, bt, seq_lens,
                              torch.arange(n + 1, dtype=torch.int32), 0.25,
                              num_decodes_tail=n)
    assert torch.equal(out, ref)
