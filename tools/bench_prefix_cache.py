"""A/B of the prefix KV cache on a shared-prefix workload, all in ONE process.

Workload: N rows, each a shared S-token prefix plus a unique U-token part,
generating up to O tokens (greedy).
Configurations: cache off, cache on with prefix_decode="per_row", cache on
with "shared". The three engines share one model (random weights); they
alternate round by round on the same prompts (a fresh prefix every round, so
no round starts with the previous round's blocks cached); round 0 warms up.
Every step is timed between device synchronisations; median (min-max) over
the rounds is reported.

    python tools/bench_prefix_cache.py [--model qwen-3-32b] [--rows 2048]
        [--prefix 128,512,0] [--unique 64] [--out-tokens 32] [--rounds 3]
Writes bench_outputs/prefix_cache_bench.txt (or under $BENCH_OUT).

Kernel times of the decode attention kernels come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/bench_prefix_cache.py
--rounds 1 --only shared` run (and `--only per_row`)."""

import argparse
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from sutro_amd.engine.config import EngineConfig  # noqa: E402
from sutro_amd.engine.engine import LLMEngine  # noqa: E402
from sutro_amd.engine.request import SamplingParams  # noqa: E402
from sutro_amd.models.registry import get_model_spec  # noqa: E402

CONFIGS = [
    ("off", dict(enable_prefix_caching=False)),
    ("per_row", dict(enable_prefix_caching=True, prefix_decode="per_row")),
    ("shared", dict(enable_prefix_caching=True, prefix_decode="shared")),
]


def prompts(n, s, u, seed, vocab):
    rng = random.Random(seed)
    hi = min(vocab, 30000)
    prefix = [rng.randrange(3, hi) for _ in range(s)]
    return [prefix + [rng.randrange(3, hi) for _ in range(u)] for _ in range(n)]


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def run_once(eng, rows, out_tokens):
    sp = SamplingParams(max_tokens=out_tokens, temperature=0.0,
                        stop_token_ids=[])
    hit0, query0 = eng.prefix_hit_tokens, eng.prefix_query_tokens
    for p in rows:
        eng.add_request(p, sp, priority=1)
    computed = out = peak = 0
    decode_ms = []
    _sync()
    t0 = time.perf_counter()
    while eng.has_work():
        ts = time.perf_counter()
        st = eng.step()
        _sync()
        dt = (time.perf_counter() - ts) * 1e3
        computed += st.prefill_tokens
        out += st.output_tokens
        peak = max(peak, len(eng.scheduler.running))
        if st.prefill_tokens == 0 and st.scheduled_tokens > 0:
            decode_ms.append(dt)
    wall = time.perf_counter() - t0
    query = eng.prefix_query_tokens - query0
    return dict(
        tok_s=out / wall, rows_h=len(rows) / wall * 3600.0,
        computed=computed, submitted=sum(len(p) for p in rows),
        hit_rate=(eng.prefix_hit_tokens - hit0) / query if query else 0.0,
        peak=peak,
        decode_ms=statistics.median(decode_ms) if decode_ms else float("nan"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="qwen-3-32b")
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--prefix", default="128,512,0", help="S values")
    ap.add_argument("--unique", type=int, default=64)
    ap.add_argument("--out-tokens", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-num-seqs", type=int, default=2048)
    ap.add_argument("--kv-blocks", type=int, default=None,
                    help="per engine (default: fits the largest point)")
    ap.add_argument("--device", default="cuda",
                    help="'cpu' only checks that the tool runs")
    ap.add_argument("--only", default=None, choices=[c for c, _ in CONFIGS])
    args = ap.parse_args()

    s_values = [int(s) for s in args.prefix.split(",")]
    longest = max(s_values) + args.unique + args.out_tokens
    max_len = (longest + 31) // 32 * 32 + 32
    blocks = args.kv_blocks or (
        min(args.rows, args.max_num_seqs) * (max_len // 32) + 64)
    spec = get_model_spec(args.model)
    configs = [c for c in CONFIGS if args.only in (None, c[0])]
    engines, model = {}, None
    for name, kw in configs:
        cfg = EngineConfig(spec=spec, device=args.device, max_model_len=max_len,
                           max_num_seqs=args.max_num_seqs,
                           num_kv_blocks=blocks, **kw)
        engines[name] = LLMEngine(cfg, model=model)
        model = engines[name].model

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"model={args.model} rows={args.rows} U={args.unique} "
         f"O={args.out_tokens} rounds={args.rounds} kv_blocks={blocks} "
         f"device={torch.cuda.get_device_name(0) if torch.cuda.is_available() else 'cpu'}")
    for s in s_values:
        res = {name: [] for name in engines}
        for r in range(args.rounds + 1):  # round 0 warms up
            rows = prompts(args.rows, s, args.unique, 1000 * s + r,
                           spec.vocab_size)
            for name, eng in engines.items():
                m = run_once(eng, rows, args.out_tokens)
                if r:
                    res[name].append(m)
        emit(f"S={s}")
        for name, ms in res.items():
            if not ms:
                continue

            def med(k):
                v = [m[k] for m in ms]
                return statistics.median(v), min(v), max(v)

            tok, lo, hi = med("tok_s")
            dms, dlo, dhi = med("decode_ms")
            emit(f"  {name:8s} {tok:9.1f} out tok/s ({lo:.1f}-{hi:.1f}, "
                 f"spread {(hi - lo) / tok * 100:4.1f}%)  "
                 f"{med('rows_h')[0]:11.0f} rows/h  prefill computed "
                 f"{ms[-1]['computed']}/{ms[-1]['submitted']}  hit rate "
                 f"{ms[-1]['hit_rate'] * 100:5.1f}%  peak rows "
                 f"{ms[-1]['peak']}  decode {dms:.2f} ms/step "
                 f"({dlo:.2f}-{dhi:.2f})")

    outd = os.environ.get("BENCH_OUT", "bench_outputs")
    os.makedirs(outd, exist_ok=True)
    with open(os.path.join(outd, "prefix_cache_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
