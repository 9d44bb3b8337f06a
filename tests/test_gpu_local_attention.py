"""Sliding-window attention and attention sinks on the GPU: the MFMA decode
kernel and the reference prefill kernel against the f32 reference
(sutro_amd.ops.torch_ref.paged_attention), bit-equality of the neutral and the
page-aligned cases with the plain call, routing, and the engine under
hipGraph."""

import dataclasses
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sutro_amd import ops
    from sutro_amd.ops import torch_ref as R
else:  # collected on CPU; every test is skipped by the marker filter anyway
    ops = R = None

DEV = "cuda"
BS = 32
F8 = torch.float8_e4m3fn

# every boundary of the page loop's start and of the first page's mask
LENS_W128 = [1, 31, 32, 33, 127, 128, 129, 160, 161, 300]
LENS_W48 = [47, 48, 49, 80, 81, 100]


def require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_SETUPS = {}


def _setup(seq_lens, new_counts, hq, hk, d, fp8, seed=0):
    """A paged cache on the GPU with shuffled block tables, every slot that
    no sequence owns (spare blocks, the tail of a last page) holding large
    finite values, plus the f32 CPU image of what the kernels read."""
    key = (tuple(seq_lens), tuple(new_counts), hq, hk, d, fp8, seed)
    if key in _SETUPS:
        return _SETUPS[key]
    g = torch.Generator().manual_seed(seed)
    nblk = [(L + BS - 1) // BS for L in seq_lens]
    total = sum(nblk) + 5
    big = 448.0 if fp8 else 1.0e4
    kc = torch.full((total, hk, BS, d), big)
    vc = torch.full((total, hk, BS, d), -big)
    perm = torch.randperm(total, generator=g).tolist()
    bt = torch.zeros(len(seq_lens), max(nblk), dtype=torch.int32)
    i = 0
    for s, (L, n) in enumerate(zip(seq_lens, nblk)):
        blocks = perm[i:i + n]
        i += n
        bt[s, :n] = torch.tensor(blocks, dtype=torch.int32)
        for pg, b in enumerate(blocks):
            m = min(BS, L - pg * BS)
            kc[b, :, :m] = torch.randn(hk, m, d, generator=g)
            vc[b, :, :m] = torch.randn(hk, m, d, generator=g)
    cdt = F8 if fp8 else torch.bfloat16
    kc_q, vc_q = kc.to(cdt), vc.to(cdt)
    q = torch.randn(sum(new_counts), hq, d, generator=g).to(torch.bfloat16)
    ql = torch.tensor([0] + torch.tensor(new_counts).cumsum(0).tolist(),
                      dtype=torch.int32)
    sl = torch.tensor(seq_lens, dtype=torch.int32)
    st = dict(q=q.to(DEV), kc=kc_q.to(DEV), vc=vc_q.to(DEV), bt=bt.to(DEV),
              sl=sl.to(DEV), ql=ql.to(DEV), q_c=q.float(), kc_c=kc_q.float(),
              vc_c=vc_q.float(), bt_c=bt, sl_c=sl, ql_c=ql,
              scale=1.0 / math.sqrt(d), new_counts=list(new_counts))
    _SETUPS[key] = st
    return st


def _sinks(kind, hq):
    if kind == "none":
        return None
    if kind == "normal":
        return torch.randn(hq, generator=torch.Generator().manual_seed(3))
    s = torch.zeros(hq)        # "extreme"
    s[0], s[hq - 1] = 8.0, -30.0
    return s


def _tiles(new_counts, n_prefill, step=32):
    ts, tq = [], []
    for s in range(n_prefill):
        for j in range(0, new_counts[s], step):
            ts.append(s)
            tq.append(j)
    return (torch.tensor(ts, dtype=torch.int32, device=DEV),
            torch.tensor(tq, dtype=torch.int32, device=DEV))


def _gpu(st, n_prefill, n_decode, window=None, sinks=None, **kw):
    ts, tq = _tiles(st["new_counts"], n_prefill, kw.pop("step", 32))
    extra = {}
    if window is not None:
        extra["window"] = window
    if sinks is not None:
        extra["sinks"] = sinks.to(DEV)
    out = ops.paged_attention(
        st["q"], kw.pop("kc", st["kc"]), kw.pop("vc", st["vc"]),
        kw.pop("bt", st["bt"]), kw.pop("sl", st["sl"]), st["ql"], st["scale"],
        num_decodes_tail=n_decode, tile_seq=ts, tile_q0=tq,
        prefill_token_count=int(sum(st["new_counts"][:n_prefill])),
        **extra, **kw)
    torch.cuda.synchronize()
    return out


def _ref(st, window, sinks):
    return R.paged_attention(st["q_c"], st["kc_c"], st["vc_c"], st["bt_c"],
                             st["sl_c"], st["ql_c"], st["scale"],
                             window=window, sinks=sinks)


def _close(got, ref, tol):
    got = got.float().cpu()
    err = (got - ref).abs().max().item()
    print(f"max abs err {err:.4g} (tol {tol})")
    assert torch.isfinite(got).all()
    assert torch.allclose(got, ref, atol=tol, rtol=tol), err


# ---- 1. decode against the reference ----

@pytest.mark.parametrize("sink_kind", ["none", "normal", "extreme"])
@pytest.mark.parametrize("hq,hk", [(8, 1), (4, 2), (6, 2)])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("d", [64, 128])
def test_decode_matches_ref(d, fp8, hq, hk, sink_kind):
    require_gpu()
    lens = LENS_W128 + LENS_W48     # one batch of 16 rows under both windows
    st = _setup(lens, [1] * len(lens), hq, hk, d, fp8)
    sinks = _sinks(sink_kind, hq)
    for window in (128, 48):
        got = _gpu(st, 0, len(lens), window=window, sinks=sinks)
        _close(got, _ref(st, window, sinks), 3e-2)
    if sinks is not None:           # sinks without a window
        _close(_gpu(st, 0, len(lens), sinks=sinks), _ref(st, 0, sinks), 3e-2)


# ---- 2. bit-equality ----

@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("d", [64, 128])
def test_decode_window_covering_the_row_is_the_plain_call(d, fp8):
    require_gpu()
    lens = LENS_W128 + LENS_W48
    st = _setup(lens, [1] * len(lens), 8, 1, d, fp8)
    plain = _gpu(st, 0, len(lens))
    for window in (300, 301, 1 << 20):
        assert torch.equal(_gpu(st, 0, len(lens), window=window), plain)


@pytest.mark.parametrize("window,lens", [(128, [128, 160, 192, 288, 320]),
                                         (48, [48, 80, 112, 144])])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("d", [64, 128])
def test_decode_page_aligned_window_is_the_plain_call_on_its_pages(
        d, fp8, window, lens):
    """L - W a multiple of 32: the windowed call walks pages (L-W)/32.. with
    nothing masked in the first, which is the plain call on those pages with
    seq_lens = W, through the same per-page body."""
    require_gpu()
    st = _setup(lens, [1] * len(lens), 4, 2, d, fp8, seed=1)
    got = _gpu(st, 0, len(lens), window=window)
    bt = torch.zeros_like(st["bt_c"])
    for s, L in enumerate(lens):
        first = (L - window) // BS
        n = (L + BS - 1) // BS - first
        bt[s, :n] = st["bt_c"][s, first:first + n]
    sl = torch.full((len(lens),), window, dtype=torch.int32)
    plain = _gpu(st, 0, len(lens), bt=bt.to(DEV), sl=sl.to(DEV))
    assert torch.equal(got, plain)


# ---- 3. the reference prefill kernel ----

PREFILL_CASES = [(0, 96, 40), (70, 96, 40), (200, 33, 128), (0, 20, 128)]


@pytest.mark.parametrize("with_sinks", [False, True], ids=["nosink", "sinks"])
@pytest.mark.parametrize("ctx,nq,window", PREFILL_CASES)
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("d", [64, 128])
def test_prefill_matches_ref(d, fp8, ctx, nq, window, with_sinks):
    require_gpu()
    hq, hk = 8, 2
    st = _setup([ctx + nq], [nq], hq, hk, d, fp8, seed=2)
    sinks = _sinks("normal", hq) if with_sinks else None
    # pages below every row's window: never walked, so what their V holds
    # cannot matter. bf16: inf; e4m3 has no inf, its NaN code stands in.
    vc = st["vc"].clone()
    dead = max(0, ctx - window + 1) // BS
    for pg in range(dead):
        blk = int(st["bt_c"][0, pg])
        if fp8:
            vc[blk].view(torch.uint8).fill_(0x7F)
        else:
            vc[blk].fill_(float("inf"))
    got = _gpu(st, 1, 0, window=window, sinks=sinks, vc=vc)
    _close(got, _ref(st, window, sinks), 5e-2)


def test_prefill_page_masked_for_later_rows_weighs_zero():
    """ctx 70, W 40, no sinks: tile 0's first row (position 70) starts its
    window at 31, on page 0; for its rows past position 71 that page is fully
    masked while their state is still m = -1e30. Rows whose window does not
    reach page 0 must not depend on it: scaling page 0's V changes nothing
    for them, bit for bit."""
    require_gpu()
    ctx, nq, window = 70, 96, 40
    st = _setup([ctx + nq], [nq], 8, 2, 64, False, seed=2)
    base = _gpu(st, 1, 0, window=window)
    vc = st["vc"].clone()
    vc[int(st["bt_c"][0, 0])] *= 1024.0
    got = _gpu(st, 1, 0, window=window, vc=vc)
    # rows at position >= 32 + 40 - 1 = 71 see nothing of page 0
    first_free = 71 - ctx
    assert torch.equal(got[first_free:], base[first_free:])
    assert not torch.equal(got[:first_free], base[:first_free])


# ---- 4. mixed batch ----

@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("d", [64, 128])
def test_mixed_batch(d, fp8):
    require_gpu()
    seq_lens = [50, 130, 33, 65, 129, 40, 200]
    new_counts = [50, 45, 1, 1, 1, 1, 1]     # 2 prefill chunks + 5 decodes
    st = _setup(seq_lens, new_counts, 8, 2, d, fp8, seed=4)
    sinks = _sinks("normal", 8)
    got = _gpu(st, 2, 5, window=40, sinks=sinks)
    _close(got, _ref(st, 40, sinks), 5e-2)


# ---- 5. routing ----

def test_forced_pipelined_prefill_still_runs_the_reference_kernel():
    require_gpu()
    st = _setup([70 + 96], [96], 8, 1, 128, False, seed=2)
    sinks = _sinks("normal", 8)
    want = _gpu(st, 1, 0, window=40, sinks=sinks)
    ops.set_attn_prefill("pipe,64")
    try:
        assert ops.prefill_tile_rows(8, 1, 128) == 64
        got = _gpu(st, 1, 0, window=40, sinks=sinks)
        assert torch.equal(got, want)
        for kw in (dict(window=40), dict(sinks=sinks)):
            with pytest.raises(RuntimeError, match="32 rows"):
                _gpu(st, 1, 0, step=64, tile_rows=64, **kw)
        # without either, 64-row tile lists still run the pipelined kernel
        plain64 = _gpu(st, 1, 0, step=64, tile_rows=64)
    finally:
        ops.set_attn_prefill(None)
    _close(plain64, _ref(st, 0, None), 5e-2)


def test_valu_fallback_refuses_a_window(monkeypatch):
    require_gpu()
    st = _setup([100, 33], [1, 1], 8, 1, 64, False, seed=5)
    monkeypatch.setenv("SUTRO_DECODE_VALU", "1")
    _gpu(st, 0, 2)                                   # plain call: VALU kernel
    for kw in (dict(window=48), dict(sinks=_sinks("normal", 8))):
        with pytest.raises(RuntimeError, match="SUTRO_DECODE_VALU"):
            _gpu(st, 0, 2, **kw)


def test_binding_checks_its_arguments():
    require_gpu()
    st = _setup([100, 33], [1, 1], 8, 1, 64, False, seed=5)
    good = _sinks("normal", 8)
    with pytest.raises(ValueError):
        _gpu(st, 0, 2, window=-1)
    for bad in (good[:7], good.repeat(2), good.double(),
                good.to(DEV).repeat(2)[::2]):     # wrong size, dtype, strided
        with pytest.raises(RuntimeError, match="sinks"):
            _gpu(st, 0, 2, sinks=bad)
    with pytest.raises(RuntimeError, match="sinks"):   # host tensor
        ops.paged_attention(st["q"], st["kc"], st["vc"], st["bt"], st["sl"],
                            st["ql"], st["scale"], num_decodes_tail=2,
                            sinks=good)


# ---- 6. the engine ----

def _engine(eager, kv_dtype):
    from sutro_amd.engine.config import EngineConfig
    from sutro_amd.engine.engine import LLMEngine
    from sutro_amd.models.registry import ModelSpec

    spec = ModelSpec(name="local-attn-gpu", hidden_size=256, num_layers=4,
                     num_heads=8, num_kv_heads=1, head_dim=64,
                     intermediate_size=512, vocab_size=1024, max_context=512,
                     tie_embeddings=True, sliding_window=32,
                     sliding_window_pattern=2, attention_sinks=True)
    cfg = EngineConfig(spec=spec, device=DEV, max_model_len=256,
                       num_kv_blocks=128, max_tokens_per_step=512, seed=0,
                       local_attention=True, kv_dtype=kv_dtype,
                       enforce_eager=eager)
    return LLMEngine(cfg)


def _generate(eng):
    from sutro_amd.engine.request import SamplingParams

    prompts = [list(range(3 + i, 3 + i + n))
               for i, n in enumerate((10, 31, 33, 64, 90))]
    reqs = [eng.add_request(p, SamplingParams(max_tokens=40, temperature=0.7,
                                              seed=3 + i))
            for i, p in enumerate(prompts)]
    while eng.has_work():
        eng.step()
    assert all(r.finish_reason is not None for r in reqs)
    return ([list(r.output_token_ids) for r in reqs],
            [r.cumulative_logprob for r in reqs])


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8_e4m3"])
def test_engine_graph_decode_equals_eager(kv_dtype):
    require_gpu()
    eng = _engine(False, kv_dtype)
    assert eng.graph_runner is not None and eng.local_attention
    attn = [layer.self_attn for layer in eng.model.layers]
    assert [a.window for a in attn] == [32, 0, 32, 0]
    assert all(a.sinks.dtype == torch.float32 and a.sinks.is_cuda
               for a in attn)
    toks_g, lps_g = _generate(eng)
    toks_e, lps_e = _generate(_engine(True, kv_dtype))
    assert all(len(t) > 0 for t in toks_g)
    assert toks_g == toks_e
    assert lps_g == lps_e


def test_engine_window_is_live_on_the_gpu():
    """The switch changes what a windowed model generates once rows outgrow
    the window (otherwise the graph test above could pass with it ignored)."""
    require_gpu()
    from sutro_amd.engine.config import EngineConfig
    from sutro_amd.engine.engine import LLMEngine

    on = _engine(True, "bf16")
    off = LLMEngine(dataclasses.replace(on.cfg, local_attention=False))
    assert _generate(on)[0] != _generate(off)[0]
