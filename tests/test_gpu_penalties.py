"""GPU tests for csrc/logit_penalties.hip: the kernel must equal the torch
reference (computed on CPU from copies) bit for bit over the WHOLE logits
tensor -- penalised elements match, every other element keeps its bits."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sutro_amd import ops
    from sutro_amd.ops import torch_ref as R
else:  # collected on CPU; every test is skipped by the marker filter anyway
    ops = R = None

DEV = "cuda"
N, V, VL = 8, 151936, 151000
ROWS = [0, 2, 3, 6, 7]
B = 512
LCAP = 8196


def require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_LOGITS = {}


def _logits(dtype):
    """[8, 151936] randn*3 with a few -inf, built once per dtype (read-only:
    every test works on copies)."""
    if dtype not in _LOGITS:
        g = torch.Generator().manual_seed(1234)
        x = torch.randn(N, V, generator=g) * 3
        for r in range(N):
            x[r, [0, 7, 4096 + r, VL - 1, VL, V - 1]] = float("-inf")
        x[3, 100] = 0.0
        x[3, 101] = -0.0
        _LOGITS[dtype] = x.to(dtype)
    return _LOGITS[dtype]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class Case:
    """Host-side description of one call (all CPU tensors)."""

    def __init__(self, rows, hists, plens, rep, pres, freq, bias, lcap=LCAP,
                 n_slots=8):
        m = len(rows)
        self.row_idx = torch.tensor(rows, dtype=torch.int32)
        # slots deliberately not in row order; unused slots / tails hold
        # stale tokens that must be ignored
        slots = [(3 * j + 1) % n_slots for j in range(m)]
        self.slot = torch.tensor(slots, dtype=torch.int32)
        self.hist = torch.full((n_slots, lcap), 12345, dtype=torch.int32)
        for s, h in zip(slots, hists):
            self.hist[s, :len(h)] = torch.tensor(h, dtype=torch.int32)
        self.hist_len = torch.tensor([len(h) for h in hists], dtype=torch.int32)
        self.prompt_len = torch.tensor(plens, dtype=torch.int32)
        self.rep = torch.tensor(rep, dtype=torch.float32)
        self.pres = torch.tensor(pres, dtype=torch.float32)
        self.freq = torch.tensor(freq, dtype=torch.float32)
        nb = max((len(b) for b in bias), default=0)
        if nb:
            self.bias_tok = torch.full((m, nb), -1, dtype=torch.int32)
            self.bias_val = torch.zeros((m, nb), dtype=torch.float32)
            for r, b in enumerate(bias):
                for k, (t, v) in enumerate(b):
                    self.bias_tok[r, k], self.bias_val[r, k] = t, v
        else:
            self.bias_tok = self.bias_val = None

    def args(self, dev):
        mv = lambda t: None if t is None else t.to(dev)
        return [mv(t) for t in (self.row_idx, self.hist, self.slot,
                                self.hist_len, self.prompt_len, self.rep,
                                self.pres, self.freq, self.bias_tok,
                                self.bias_val)]


def _reference(case, logits_cpu):
    want = logits_cpu.clone()
    R.apply_logit_penalties(want, *case.args("cpu"), VL)
    return want


def _run_gpu(case, logits_cpu, **kw):
    got = logits_cpu.clone().to(DEV)
    ops.apply_logit_penalties(got, *case.args(DEV), vocab_limit=VL, **kw)
    torch.cuda.synchronize()
    return got.cpu()


def _check(case, dtype, **kw):
    src = _logits(dtype)
    want = _reference(case, src)
    got = _run_gpu(case, src, **kw)
    assert torch.equal(_bits(got), _bits(want))
    untouched = [r for r in range(N) if r not in case.row_idx.tolist()]
    assert torch.equal(_bits(got[untouched]), _bits(src[untouched]))
    assert torch.equal(_bits(got[:, VL:]), _bits(src[:, VL:]))
    assert not torch.equal(_bits(got), _bits(src)), "case must change logits"
    return got


def _mixed_case(lcap=LCAP, n_rows=5):
    """Lengths {0, 1, 65, 300, 2048} (empty history, wave boundary 64|65);
    n_rows=4 drops the longest."""
    rng = np.random.RandomState(7)
    h0 = []
    h1 = [4242]
    # tokens in [vl, V) plus the ids 0 and vl-1
    h65 = ([0, VL - 1, VL, V - 1, VL + 17] * 13)[:65]
    # all distinct, colliding modulo 2048 / 8192 / 16384: c + k*2048
    h300 = [5 + 2048 * k for k in range(73)] + [9 + 16384 * k for k in range(9)]
    h300 += [11 + 8192 * k for k in range(1, 18, 2)]
    h300 += [t for t in range(20000, 20400) if t % 2048 not in (5, 9, 11)][
        :300 - len(h300)]
    assert len(h300) == 300 == len(set(h300))
    # heavy duplication: 50 distinct ids
    ids50 = rng.choice(VL, size=50, replace=False)
    h2048 = ids50[rng.randint(0, 50, size=2048)].tolist()
    hists = [h0, h1, h65, h300, h2048]
    plens = [0, 1, 65 // 3, 0, 2048 // 3]
    rep = [1.3, 0.7, 1.0, 1.3, 0.7]
    pres = [0.5, 0.0, -1.5, 2.0, -0.25]
    freq = [0.0, -0.5, 1.25, 0.3, -2.0]
    full = [(int(t), float(v)) for t, v in zip(
        rng.choice(VL, size=B - 4, replace=False),
        rng.uniform(-100, 100, size=B - 4))]
    # keys also in the history, a key >= vl, -inf columns, id 0
    full += [(int(ids50[0]), 3.5), (V - 2, 50.0), (7, 100.0), (0, -100.0)]
    bias = [
        full[:100],                                  # empty history, bias only
        [(4242, -7.0)],                              # 1 entry, also in history
        [],                                          # no bias (-1 padding)
        [(5, 1.0), (5 + 2048, -1.0), (VL, 9.0), (100, 0.25), (101, 0.0)],
        full,                                        # 512 entries
    ]
    k = n_rows
    return Case(ROWS[:k], hists[:k], plens[:k], rep[:k], pres[:k], freq[:k],
                bias[:k], lcap=lcap)


def _big_case():
    """Largest table half full: 8192 - B all-distinct tokens (+ B bias keys),
    next to a row of the same length over 50 ids (counts in the hundreds)."""
    rng = np.random.RandomState(11)
    L = 8192 - B
    distinct = rng.choice(VL, size=L + B, replace=False)
    h_a = distinct[:L].tolist()
    ids50 = rng.choice(VL, size=50, replace=False)
    h_b = ids50[rng.randint(0, 50, size=L)].tolist()
    bias_a = [(int(t), float(v)) for t, v in zip(
        distinct[L:], rng.uniform(-100, 100, size=B))]
    bias_b = [(int(ids50[1]), -2.0), (VL + 5, 1.0)]
    return Case([6, 1], [h_a, h_b], [L // 3, L], [1.3, 0.7], [0.5, -0.5],
                [0.7, 1.1], [bias_a, bias_b])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_penalties_mixed_histories(dtype):
    require_gpu()
    _check(_mixed_case(), dtype)


def test_penalties_unaligned_pool_and_small_table():
    """A pool whose rows are not 16-byte aligned takes the scalar load path.
    Histories up to 300 with a 5-wide bias block fit the smallest table
    (2048 entries); the 2048-token row needs the middle one."""
    require_gpu()
    _check(_mixed_case(lcap=2049), torch.bfloat16)
    for lcap in (301, 304):
        case = _mixed_case(lcap=lcap, n_rows=4)
        case.bias_tok = case.bias_tok[:, :5].contiguous()
        case.bias_val = case.bias_val[:, :5].contiguous()
        _check(case, torch.bfloat16)
    # prompt_len == hist_len: repetition only, no counts
    case.prompt_len = case.hist_len.clone()
    _check(case, torch.float32)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_penalties_largest_table_half_full(dtype):
    require_gpu()
    _check(_big_case(), dtype)


def test_penalties_oversize_history_falls_back():
    require_gpu()
    rng = np.random.RandomState(3)
    h = rng.randint(0, V, size=8193).tolist()
    case = Case([4, 0], [h, [1, 2, 3]], [100, 1], [1.3, 1.0], [0.5, 0.0],
                [0.25, 1.0], [[(9, 2.0)], []])
    _check(case, torch.bfloat16)


def test_penalties_repeatable():
    require_gpu()
    case = _mixed_case()
    src = _logits(torch.bfloat16)
    a = _run_gpu(case, src)
    b = _run_gpu(case, src)
    assert torch.equal(_bits(a), _bits(b))
    # the host-provided length bound picks the same table as the read-back
    c = _run_gpu(case, src, max_hist_len=2048)
    assert torch.equal(_bits(a), _bits(c))


def test_penalties_empty_call_is_noop():
    require_gpu()
    src = _logits(torch.bfloat16)
    got = src.clone().to(DEV)
    e_i = torch.zeros(0, dtype=torch.int32, device=DEV)
    e_f = torch.zeros(0, dtype=torch.float32, device=DEV)
    ops.apply_logit_penalties(
        got, e_i, torch.zeros((1, 4), dtype=torch.int32, device=DEV), e_i,
        e_i, e_i, e_f, e_f, e_f, vocab_limit=VL)
    assert torch.equal(_bits(got.cpu()), _bits(src))


def test_engine_penalties_gpu_graph_decode():
    """End to end through the decode hipGraph: the penalty op edits the
    graph's static logits buffer in place before the fused sampler reads it."""
    require_gpu()
    from sutro_amd.engine.config import EngineConfig
    from sutro_amd.engine.engine import LLMEngine
    from sutro_amd.engine.request import SamplingParams
    from sutro_amd.engine.tokenizer import EOS_ID
    from sutro_amd.models.registry import get_model_spec

    cfg = EngineConfig(spec=get_model_spec("qwen-3-0.6b"), device="cuda",
                       max_model_len=512, num_kv_blocks=512,
                       max_tokens_per_step=2048, max_num_seqs=64)
    eng = LLMEngine(cfg)
    assert eng.graph_runner is not None
    T = 1000
    assert T != EOS_ID

    def run(sps):
        reqs = [eng.add_request(eng.tokenizer.render_prompt(f"row {i}"), sp)
                for i, sp in enumerate(sps)]
        while eng.has_work():
            eng.step()
        return reqs

    greedy = dict(max_tokens=12, temperature=0.0)
    first = run([SamplingParams(**greedy, logit_bias={T: 100.0})
                 if i % 2 == 0 else SamplingParams(**greedy)
                 for i in range(8)])
    for i, r in enumerate(first):
        if i % 2 == 0:
            assert r.output_token_ids == [T] * 12
    plain = [r for i, r in enumerate(first) if i % 2 == 1]
    firsts = [(r.output_token_ids or [EOS_ID])[0] for r in plain]
    # second run: the same prompts with their unbiased first token banned
    sps = [SamplingParams(**greedy, logit_bias={T: 100.0}) for _ in range(8)]
    for j, g in enumerate(firsts):
        sps[2 * j + 1] = SamplingParams(**greedy, logit_bias={g: -100.0})
    second = run(sps)
    for j, g in enumerate(firsts):
        assert (second[2 * j + 1].output_token_ids or [EOS_ID])[0] != g
    assert eng.penalties.num_free == eng.penalties.capacity
