"""Pipelined prefill attention (attn_prefill_pipe_kernel) against the
reference kernel (attn_prefill_kernel) on the same inputs: the two must
return identical bits at every tile granularity, head layout, head_dim and KV
dtype; one case per granularity also against the fp32 PyTorch reference."""

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

# fresh prompts around every tile edge (1 row: shorter than a sub-tile; 65,
# 129, 200: last group partial), then chunk continuations (ctx, new)
FRESH = [1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 200]
CONT = [(1, 1), (32, 33), (40, 64), (100, 29), (31, 128)]
NEW_COUNTS = FRESH + [n for _, n in CONT]
SEQ_LENS = FRESH + [c + n for c, n in CONT]
HEADS = [(8, 2), (16, 2), (8, 8)]       # G = 4, 8, 1


def require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bf(x):
    return x.to(torch.bfloat16).to(DEV)


def _attn_setup(seq_lens, new_counts, Hq=8, Hk=2, D=128, bs=32, seed=5,
                kv_dtype=torch.bfloat16):
    """Scattered paged cache + q batch, as tests/test_gpu_kernels.py builds
    them: page table permuted at random, 3 spare pages."""
    torch.manual_seed(seed)
    S = len(seq_lens)
    total_blocks = sum((L + bs - 1) // bs for L in seq_lens) + 3
    perm = torch.randperm(total_blocks).tolist()
    kc = torch.zeros(total_blocks, Hk, bs, D, dtype=kv_dtype, device=DEV)
    vc = torch.zeros_like(kc)
    tables = []
    i = 0
    for L in seq_lens:
        n = (L + bs - 1) // bs
        tables.append(perm[i:i + n])
        i += n
    max_b = max(len(t) for t in tables)
    bt = torch.zeros(S, max_b, dtype=torch.int32)
    for s, t in enumerate(tables):
        bt[s, :len(t)] = torch.tensor(t, dtype=torch.int32)
    qs = []
    for s, L in enumerate(seq_lens):
        K = bf(torch.randn(L, Hk, D))
        V = bf(torch.randn(L, Hk, D))
        slots = torch.tensor(
            [tables[s][p // bs] * bs + p % bs for p in range(L)], dtype=torch.long)
        R.write_kv_cache(K, V, kc, vc, slots.to(DEV))
        qs.append(bf(torch.randn(new_counts[s], Hq, D)))
    q = torch.cat(qs, 0)
    qlocs = torch.tensor([0] + list(torch.tensor(new_counts).cumsum(0)),
                         dtype=torch.int32)
    sl = torch.tensor(seq_lens, dtype=torch.int32)
    return q, kc, vc, bt.to(DEV), sl.to(DEV), qlocs.to(DEV), sl, qlocs, bt


def _tiles(new_counts, rows, n_prefills=None):
    ts, tq = [], []
    for s, c in enumerate(new_counts[:n_prefills]):
        for j in range(0, c, rows):
            ts.append(s)
            tq.append(j)
    return (torch.tensor(ts, dtype=torch.int32, device=DEV),
            torch.tensor(tq, dtype=torch.int32, device=DEV))


def _run(setup, rows, variant, new_counts=NEW_COUNTS, n_decodes=0):
    q, kc, vc, bt, sl, ql = setup[:6]
    n_pf = len(new_counts) - n_decodes
    ts, tq = _tiles(new_counts, rows, n_pf)
    scale = 1.0 / math.sqrt(q.shape[2])
    return ops.paged_attention(
        q, kc, vc, bt, sl, ql, scale, num_decodes_tail=n_decodes,
        tile_seq=ts, tile_q0=tq,
        prefill_token_count=int(sum(new_counts[:n_pf])),
        tile_rows=rows, prefill_variant=variant)


_CACHE = {}


def _case(hq, hk, D, fp8):
    """Inputs and the reference kernel's output, computed once per layout."""
    key = (hq, hk, D, fp8)
    if key not in _CACHE:
        setup = _attn_setup(
            SEQ_LENS, NEW_COUNTS, Hq=hq, Hk=hk, D=D, seed=5 + hq + D,
            kv_dtype=torch.float8_e4m3fn if fp8 else torch.bfloat16)
        _CACHE[key] = (setup, _run(setup, 32, "v1"))
    return _CACHE[key]


@pytest.mark.parametrize("rows", [32, 64, 128])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16kv", "e4m3kv"])
@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("hq,hk", HEADS)
def test_pipe_bit_identical_to_reference(hq, hk, D, fp8, rows):
    require_gpu()
    if not ops.attn_prefill_pipe_supported(hq, hk, D, rows):
        # the only layout here the kernel does not take: 8 heads per kv head
        # at 128 rows would be 32 (head, sub-tile) pairs per block
        assert (hq // hk) * (rows // 32) > 16
        with pytest.raises(RuntimeError):
            _run(_case(hq, hk, D, fp8)[0], rows, "pipe")
        return
    setup, ref = _case(hq, hk, D, fp8)
    got = _run(setup, rows, "pipe")
    assert torch.equal(got, ref), (
        (got.float() - ref.float()).abs().max().item())


@pytest.mark.parametrize("rows", [32, 64, 128])
def test_pipe_matches_torch_ref(rows):
    require_gpu()
    setup, _ = _case(8, 2, 128, False)
    q, kc, vc = setup[:3]
    sl_c, ql_c, bt_c = setup[6:]
    got = _run(setup, rows, "pipe")
    ref = R.paged_attention(q.float().cpu(), kc.float().cpu(), vc.float().cpu(),
                            bt_c, sl_c, ql_c, 1.0 / math.sqrt(128))
    err = (got.float().cpu() - ref).abs().max()
    assert torch.allclose(got.float().cpu(), ref, atol=5e-2, rtol=5e-2), err


@pytest.mark.parametrize("rows", [32, 64, 128])
def test_pipe_mixed_prefill_decode_batch(rows):
    require_gpu()
    seq_lens = [50, 90, 33, 65, 129]
    new_counts = [50, 40, 1, 1, 1]  # 2 prefills + 3 decodes
    setup = _attn_setup(seq_lens, new_counts)
    ref = _run(setup, 32, "v1", new_counts, n_decodes=3)
    got = _run(setup, rows, "pipe", new_counts, n_decodes=3)
    assert torch.equal(got, ref)
    q, kc, vc = setup[:3]
    sl_c, ql_c, bt_c = setup[6:]
    cpu = R.paged_attention(q.float().cpu(), kc.float().cpu(), vc.float().cpu(),
                            bt_c, sl_c, ql_c, 1.0 / math.sqrt(128))
    assert torch.allclose(got.float().cpu(), cpu, atol=5e-2, rtol=5e-2)


def test_pipe_rejects_sixteen_heads_per_kv_head():
    """G = 16 is not built (a wave owns one head, 8 waves at most): the
    extension's own check, its Python mirror and the call all say so."""
    require_gpu()
    from sutro_amd import _C
    for rows in (32, 64, 128):
        assert not _C.attn_prefill_pipe_supported(32, 2, 128, rows)
        assert not ops.attn_prefill_pipe_supported(32, 2, 128, rows)
    setup = _attn_setup([40, 7], [40, 7], Hq=32, Hk=2)
    with pytest.raises(RuntimeError):
        _run(setup, 32, "pipe", [40, 7])


def test_reference_kernel_rejects_wide_tiles():
    require_gpu()
    setup, _ = _case(8, 2, 128, False)
    with pytest.raises(RuntimeError):
        _run(setup, 64, "v1")
