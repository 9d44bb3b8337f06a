"""Repetition / presence / frequency penalties and logit_bias (CPU).

Covers the shared semantics (torch reference vs a per-token brute force),
SamplingParams validation, the engine's device-history invariant, end-to-end
behaviour, and replay equivalence (preemption, async_decode, slot release).
"""

import json
import math

import numpy as np
import pytest
import torch

from sutro_amd import ops
from sutro_amd.engine.config import EngineConfig
from sutro_amd.engine.request import SamplingParams
from sutro_amd.engine.tokenizer import EOS_ID
from sutro_amd.models.registry import tiny_spec_for_tests
from sutro_amd.ops import torch_ref

V, VL = 97, 90


# ---- 1. reference against brute force ----

def _brute_force(logits, row_idx, hist, slot, hist_len, prompt_len, rep, pres,
                 freq, bias, vl):
    """Per-token Python loop over the semantics block; np.float32 scalars so
    every operation is rounded on its own."""
    out = logits.clone()
    f = np.float32
    with np.errstate(all="ignore"):
        for r, row in enumerate(row_idx):
            h = hist[slot[r]][:hist_len[r]]
            P = prompt_len[r]
            for t in range(vl):
                a = t in h
                c = sum(1 for j in range(P, len(h)) if h[j] == t)
                in_bias = t in bias[r]
                if not (a or in_bias):
                    continue
                y = f(logits[row, t].float().item())
                if a:
                    y = y / f(rep[r]) if y > 0 else y * f(rep[r])
                y = f(y - f(f(freq[r]) * f(c)))
                if c > 0:
                    y = f(y - f(pres[r]))
                if in_bias:
                    y = f(y + f(bias[r][t]))
                out[row, t] = torch.tensor(float(y)).to(logits.dtype)
    return out


def _make_logits(n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, V, generator=g) * 3
    x[:, 5] = float("-inf")
    x[:, 40] = float("-inf")
    x[0, 7] = 0.0
    return x.to(dtype)


def _hist_cases():
    rng = np.random.RandomState(0)
    h40 = rng.randint(0, 30, size=40).tolist()   # duplicates
    h40[3], h40[25], h40[39] = 5, 93, 96          # a -inf column, two >= vl
    h40[10], h40[30] = 40, 40                     # -inf column, prompt + output
    return [[], [17], h40]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("params", [
    (1.3, 0.5, 0.7), (0.7, -1.5, -0.3), (1.0, 0.0, 0.0), (1.0, 2.0, 0.0),
    (2.0, 0.0, -2.0)])
def test_reference_matches_brute_force(dtype, params):
    rep_v, pres_v, freq_v = params
    hists = _hist_cases()
    biases = [{}, {3: 1.5, 94: 7.0, 17: -100.0},
              {5: 4.0, 2: 100.0, 89: -0.25, 96: 1.0}]
    lcap = 44
    rows, slots, lens, plens, bias = [], [], [], [], []
    pool = []
    n = 0
    for hi, h in enumerate(hists):
        L = len(h)
        for P in sorted({0, L // 2, L}):
            pool.append(h + [11] * (lcap - L))   # stale tail must be ignored
            slots.append(len(pool) - 1)
            lens.append(L)
            plens.append(P)
            bias.append(biases[(hi + P) % 3])
            rows.append(n)
            n += 2                                # odd rows stay untouched
    m = len(rows)
    logits = _make_logits(n, dtype, seed=m)
    B = max(len(b) for b in bias)
    btok = torch.full((m, B), -1, dtype=torch.int32)
    bval = torch.zeros((m, B), dtype=torch.float32)
    for r, b in enumerate(bias):
        for k, (t, v) in enumerate(b.items()):
            btok[r, k], bval[r, k] = t, v
    rep, pres, freq = [rep_v] * m, [pres_v] * m, [freq_v] * m
    want = _brute_force(logits, rows, pool, slots, lens, plens, rep, pres,
                        freq, bias, VL)
    got = logits.clone()
    ops.apply_logit_penalties(
        got, torch.tensor(rows, dtype=torch.int32),
        torch.tensor(pool, dtype=torch.int32),
        torch.tensor(slots, dtype=torch.int32),
        torch.tensor(lens, dtype=torch.int32),
        torch.tensor(plens, dtype=torch.int32),
        torch.tensor(rep), torch.tensor(pres), torch.tensor(freq),
        btok, bval, vocab_limit=VL)
    # bitwise: equal values AND equal zero signs / infinities
    assert torch.equal(got, want)
    assert torch.equal(got.view(torch.int32 if dtype == torch.float32
                                else torch.int16),
                       want.view(torch.int32 if dtype == torch.float32
                                 else torch.int16))
    # untouched rows and the columns >= vl keep their bits
    assert torch.equal(got[1::2], logits[1::2])
    assert torch.equal(got[:, VL:], logits[:, VL:])
    if (rep_v, pres_v, freq_v) != (1.0, 0.0, 0.0):
        assert not torch.equal(got, logits)


def test_reference_no_bias_and_empty_call():
    logits = _make_logits(2, torch.float32, seed=1)
    before = logits.clone()
    e_i = torch.zeros(0, dtype=torch.int32)
    e_f = torch.zeros(0)
    torch_ref.apply_logit_penalties(
        logits, e_i, torch.zeros((1, 4), dtype=torch.int32), e_i, e_i, e_i,
        e_f, e_f, e_f, None, None, VL)
    assert torch.equal(logits, before)
    one = torch.tensor([1], dtype=torch.int32)
    torch_ref.apply_logit_penalties(
        logits, one, torch.tensor([[9, 9, 8, 0]], dtype=torch.int32),
        torch.tensor([0], dtype=torch.int32),
        torch.tensor([3], dtype=torch.int32),
        torch.tensor([1], dtype=torch.int32),
        torch.tensor([1.0]), torch.tensor([0.0]), torch.tensor([1.0]),
        None, None, VL)
    want = before.clone()
    want[1, 9] -= 1.0   # one output occurrence (position 1)
    want[1, 8] -= 1.0
    assert torch.equal(logits, want)


# ---- 2. from_dict / validation ----

def test_from_dict_accepts_penalty_keys():
    sp = SamplingParams.from_dict({
        "repetition_penalty": 1.1, "presence_penalty": -2, "frequency_penalty": 2,
        "logit_bias": {"17": 5, "3": -100.0}, "some_unknown_key": 1})
    assert sp.repetition_penalty == 1.1
    assert sp.presence_penalty == -2.0 and sp.frequency_penalty == 2.0
    assert sp.logit_bias == {17: 5.0, 3: -100.0}
    assert all(isinstance(k, int) for k in sp.logit_bias)
    assert sp.penalised


@pytest.mark.parametrize("bad", [
    {"repetition_penalty": 0}, {"repetition_penalty": -1.0},
    {"repetition_penalty": float("nan")}, {"repetition_penalty": float("inf")},
    {"presence_penalty": 2.5}, {"frequency_penalty": -2.01},
    {"frequency_penalty": float("nan")},
    {"logit_bias": {"5": 101}}, {"logit_bias": {"-1": 1.0}},
    {"logit_bias": {-1: 1.0}}, {"logit_bias": {"abc": 1.0}},
    {"logit_bias": {"5": float("nan")}}, {"logit_bias": [1, 2]},
    {"logit_bias": {str(i): 0.5 for i in range(513)}},
])
def test_from_dict_rejects_bad_values(bad):
    with pytest.raises(ValueError):
        SamplingParams.from_dict(bad)


def test_neutral_values_are_not_penalised():
    assert not SamplingParams().penalised
    sp = SamplingParams.from_dict({
        "repetition_penalty": 1.0, "presence_penalty": 0.0,
        "frequency_penalty": 0, "logit_bias": {}})
    assert not sp.penalised
    assert SamplingParams.from_dict(
        {"logit_bias": {str(i): 0.5 for i in range(512)}}).penalised
    assert SamplingParams.from_dict({"presence_penalty": 0.1}).penalised


def test_submit_job_rejects_bad_penalty(sutro_home):
    from sutro_amd.service.jobs import JobService

    svc = JobService(home=sutro_home, device="cpu")
    with pytest.raises(ValueError):
        svc.submit_job({"model": "qwen-3-4b", "inputs": ["a"],
                        "sampling_params": {"repetition_penalty": 0}})
    with pytest.raises(ValueError):
        svc.submit_job({"model": "qwen-3-4b", "inputs": ["a"],
                        "sampling_params": {"logit_bias": {"7": 1000}}})


# ---- engine helpers ----

def _engine(**kw):
    from sutro_amd.engine.engine import LLMEngine

    cfg = EngineConfig(spec=tiny_spec_for_tests(), device="cpu",
                       max_num_seqs=kw.pop("max_num_seqs", 8),
                       max_model_len=512,
                       max_tokens_per_step=kw.pop("max_tokens_per_step", 128),
                       min_prefill_batch_tokens=0,
                       num_kv_blocks=kw.pop("num_kv_blocks", 256),
                       seed=3, **kw)
    return LLMEngine(cfg)


def _drain(eng, limit=3000):
    for _ in range(limit):
        if not eng.scheduler.has_work():
            break
        eng.step()
    eng.step()  # flush lagged async tokens
    assert not eng.scheduler.has_work()


def _prompt(i, n=20):
    return [3 + (7 * i + j) % 200 for j in range(n + i)]


# ---- 3. engine history invariant ----

def test_engine_history_invariant(tiny_engine, monkeypatch):
    eng = tiny_engine
    real_op = ops.apply_logit_penalties
    real_sample = eng.sampler.sample
    current = {}
    calls = []

    def sample_spy(logits, reqs, *a, **kw):
        current["reqs"] = list(reqs)
        return real_sample(logits, reqs, *a, **kw)

    def op_spy(logits, row_idx, hist, slot, hist_len, prompt_len, *a, **kw):
        reqs = current["reqs"]
        rows = row_idx.tolist()
        assert len(set(rows)) == len(rows)
        # only (and all of) the penalised rows of this batch
        assert rows == [i for i, r in enumerate(reqs) if r.sampling.penalised]
        for j, i in enumerate(rows):
            req = reqs[i]
            L = int(hist_len[j])
            assert L == req.total_len
            assert int(prompt_len[j]) == req.num_prompt_tokens
            assert (hist[int(slot[j]), :L].tolist()
                    == req.prompt_token_ids + req.output_token_ids)
        calls.append(len(rows))
        return real_op(logits, row_idx, hist, slot, hist_len, prompt_len,
                       *a, **kw)

    monkeypatch.setattr(eng.sampler, "sample", sample_spy)
    monkeypatch.setattr(ops, "apply_logit_penalties", op_spy)
    sps = [
        SamplingParams(max_tokens=10, temperature=0.8, seed=1),
        SamplingParams(max_tokens=14, temperature=0.8, seed=2,
                       repetition_penalty=1.3),
        SamplingParams(max_tokens=6, temperature=0.0,
                       frequency_penalty=0.5, presence_penalty=0.2),
        SamplingParams(max_tokens=12, temperature=0.9, seed=4),
        SamplingParams(max_tokens=9, temperature=0.0,
                       logit_bias={50: 3.0, 51: -3.0}),
    ]
    reqs = [eng.add_request(_prompt(i), sp) for i, sp in enumerate(sps)]
    _drain(eng)
    assert all(r.finished for r in reqs)
    assert calls and max(calls) == 3
    assert eng.penalties.hist is not None
    assert eng.penalties.num_free == eng.penalties.capacity


def test_no_penalised_request_no_pool_no_call(tiny_engine, monkeypatch):
    eng = tiny_engine

    def boom(*a, **kw):
        raise AssertionError("penalty op called without a penalised row")

    monkeypatch.setattr(ops, "apply_logit_penalties", boom)
    for i in range(3):
        eng.add_request(_prompt(i), SamplingParams(max_tokens=6, seed=i))
    _drain(eng)
    assert eng.penalties.hist is None
    assert eng.penalties.num_free == eng.penalties.capacity


# ---- 4. behaviour ----

def _first_step_logits(prompt):
    """Raw first-step logits of a fresh tiny engine for `prompt`."""
    eng = _engine()
    grabbed = []
    real = eng.sampler.sample

    def spy(logits, reqs, *a, **kw):
        grabbed.append(logits[0].float().clone())
        return real(logits, reqs, *a, **kw)

    eng.sampler.sample = spy
    req = eng.add_request(prompt, SamplingParams(max_tokens=1, temperature=0.0))
    _drain(eng)
    return grabbed[0], req


def test_bias_forces_token():
    T = 77
    assert T != EOS_ID
    eng = _engine()
    req = eng.add_request(_prompt(0), SamplingParams(
        max_tokens=12, temperature=0.0, logit_bias={T: 100.0}))
    _drain(eng)
    assert req.output_token_ids == [T] * 12


def test_bias_bans_greedy_token():
    logits, _ = _first_step_logits(_prompt(1))
    g = int(logits.argmax())
    eng = _engine()
    plain = eng.add_request(_prompt(1), SamplingParams(max_tokens=3,
                                                       temperature=0.0))
    banned = eng.add_request(_prompt(1), SamplingParams(
        max_tokens=3, temperature=0.0, logit_bias={g: -100.0}))
    _drain(eng)
    first_plain = (plain.output_token_ids or [EOS_ID])[0]
    assert first_plain == g or g == EOS_ID
    assert (banned.output_token_ids or [EOS_ID])[0] != g


def test_frequency_penalty_alternates_two_biased_tokens():
    logits, _ = _first_step_logits(_prompt(2))
    # the two ordinary tokens whose raw first-step logits are closest
    order = torch.argsort(logits[3:400]) + 3
    vals = logits[order]
    k = int((vals[1:] - vals[:-1]).argmin())
    t2, t1 = int(order[k]), int(order[k + 1])
    assert abs(float(logits[t1] - logits[t2])) < 0.5
    eng = _engine()
    req = eng.add_request(_prompt(2), SamplingParams(
        max_tokens=12, temperature=0.0, frequency_penalty=2.0,
        logit_bias={t1: 100.0, t2: 99.5}))
    _drain(eng)
    out = req.output_token_ids
    assert len(out) == 12
    assert set(out) == {t1, t2}
    assert abs(out.count(t1) - out.count(t2)) <= 1


# ---- 5. replay ----

def _penalised_job(num_blocks=256, async_mode=False, cancel=False):
    eng = _engine(num_kv_blocks=num_blocks, async_decode=async_mode)
    reqs = []
    for i in range(6):
        sp = SamplingParams(max_tokens=24, temperature=0.9, seed=1000 + i)
        if i % 3 == 0:
            sp.repetition_penalty = 1.4
            sp.logit_bias = {60 + i: 2.0}
        elif i % 3 == 1:
            sp.frequency_penalty = 0.8
            sp.presence_penalty = 0.4
        reqs.append(eng.add_request(list(range(3, 3 + 40 + i)), sp))
    if cancel:
        victim = reqs[3]
        for _ in range(200):
            eng.step()
            if len(victim.output_token_ids) >= 3:
                break
        assert not victim.finished and victim.output_token_ids
        eng.abort_request(victim)
    _drain(eng)
    return eng, reqs


def test_preemption_preserves_penalised_outputs():
    tight_eng, tight = _penalised_job(num_blocks=8)
    _, roomy = _penalised_job(num_blocks=256)
    assert sum(r.alloc_gen for r in tight) > 0, "must exercise preemption"
    assert ([r.output_token_ids for r in tight]
            == [r.output_token_ids for r in roomy])
    assert tight_eng.penalties.num_free == tight_eng.penalties.capacity


def test_penalties_change_seeded_outputs():
    """The replay tests would pass vacuously if the penalties were dropped."""
    _, pen = _penalised_job()
    eng = _engine()
    plain = [eng.add_request(list(range(3, 3 + 40 + i)), SamplingParams(
        max_tokens=24, temperature=0.9, seed=1000 + i)) for i in range(6)]
    _drain(eng)
    assert pen[2].output_token_ids == plain[2].output_token_ids  # plain row
    assert any(pen[i].output_token_ids != plain[i].output_token_ids
               for i in (0, 1, 3, 4))


def test_async_decode_matches_sync_with_penalised_rows():
    _, sync = _penalised_job(async_mode=False)
    eng, asy = _penalised_job(async_mode=True)
    assert eng.cfg.async_decode
    assert ([r.output_token_ids for r in asy]
            == [r.output_token_ids for r in sync])


def test_pool_is_free_after_finish_and_cancel():
    eng, reqs = _penalised_job(cancel=True)
    assert reqs[3].finish_reason.value == "abort"
    assert all(r.finished for r in reqs)
    assert eng.penalties.hist is not None
    assert eng.penalties.num_free == eng.penalties.capacity == 8


# ---- 6. guided rows ----

def test_guided_rows_with_repetition_penalty_stay_schema_valid():
    from sutro_amd.engine.tokenizer import get_tokenizer

    schema = {"type": "object",
              "properties": {"v": {"type": "integer", "minimum": 0,
                                   "maximum": 9}}}
    eng = _engine()
    fsm_id = eng.register_fsm(schema)
    reqs = [eng.add_request(
        list(range(3, 3 + 30 + i)),
        SamplingParams(max_tokens=20, temperature=0.9, seed=500 + i,
                       repetition_penalty=1.5, frequency_penalty=0.5),
        fsm_id=fsm_id) for i in range(4)]
    _drain(eng)
    assert eng.penalties.hist is not None
    tok = get_tokenizer()
    for r in reqs:
        parsed = json.loads(tok.decode(r.output_token_ids))
        assert 0 <= parsed["v"] <= 9
        assert not math.isnan(r.cumulative_logprob)
