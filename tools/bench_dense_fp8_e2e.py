"""End-to-end effect of dense_weight_dtype on decode: bench.py has no switch
for it, so this builds the engine directly with each of its values ("bf16",
"fp8_e4m3", "fp8_block128"), at
bench.py's default operating point (Qwen3-32B, 2048 rows, prompt 128, 128 new
tokens), and reports ms per decode step and resident KV blocks for each.

Per setting: a fresh engine kept saturated the way bench.py keeps it (rows
of `--prompt-len` random tokens, finished rows — random weights do sample
EOS — replaced from the same seeded stream, default admission policy). Steps
run until the first one without prefill work, then `--warmup` more, then
`--steps` steps are timed one by one between device syncs. Only pure decode
steps (no prefill tokens: one hipGraph replay of the whole batch) enter the
median; the tool fails if fewer than half of the timed steps are such.
Every loop is bounded and progress is printed as it goes. Each setting runs
in a fresh process, so the memory figures of one do not depend on the other.

KV blocks: `kv_blocks` is what the engine allocated (capped at max_num_seqs
rows of max_model_len), `kv_blocks_fit` what the memory free after load
would hold before that cap; `allocated_after_init_gb` is the allocator's
figure once the engine is up (weights, KV, workspaces, graph pools).

    python tools/bench_dense_fp8_e2e.py [--steps 32] [--warmup 8]
Without a GPU it runs the same procedure on a tiny model (a check of the
tool, not a measurement).
Writes bench_outputs/dense_fp8_e2e.csv (or under $BENCH_OUT)."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from sutro_amd.engine.config import EngineConfig  # noqa: E402
from sutro_amd.engine.engine import LLMEngine  # noqa: E402
from sutro_amd.engine.request import SamplingParams  # noqa: E402
from sutro_amd.models.registry import (get_model_spec,  # noqa: E402
                                       tiny_spec_for_tests)


SETTINGS = ("bf16", "fp8_e4m3", "fp8_block128")


def run(args, dense, gpu):
    cfg = EngineConfig(
        spec=get_model_spec(args.model) if gpu else tiny_spec_for_tests(),
        device="cuda" if gpu else "cpu",
        max_model_len=max(256, args.prompt_len + args.max_new + 32),
        max_num_seqs=args.batch, max_tokens_per_step=args.tokens_per_step,
        seed=0, num_kv_blocks=None if gpu else 512,
        dense_weight_dtype=dense)

    def sync():
        if gpu:
            torch.cuda.synchronize()

    t0 = time.time()
    eng = LLMEngine(cfg)
    init_s = time.time() - t0
    fit, free, alloc = eng.kv.num_blocks, 0, 0
    if gpu:
        alloc = torch.cuda.memory_allocated()
        free, total = torch.cuda.mem_get_info()
        kv_bytes = sum(t.numel() * t.element_size()
                       for t in list(eng.kv.k_cache) + list(eng.kv.v_cache))
        headroom = int((1.0 - cfg.gpu_memory_utilization) * total)
        fit = cfg.derive_num_kv_blocks(max(0, free + kv_bytes - headroom))
    print(f"[{dense}] engine up in {init_s:.1f} s, {eng.kv.num_blocks} KV "
          f"blocks allocated, {fit} fit", flush=True)

    rng = np.random.default_rng(1234)
    hi = eng.tokenizer.vocab_size
    sch = eng.scheduler
    arrival = [0]

    def refill():
        while (len(sch.running) + len(sch.waiting_p0) + len(sch.waiting_p1)
               < args.batch):
            ids = [1] + rng.integers(3, hi, size=args.prompt_len - 1).tolist()
            eng.add_request(ids, SamplingParams(max_tokens=args.max_new,
                                                temperature=0.8, top_p=0.95),
                            priority=1, arrival_idx=arrival[0])
            arrival[0] += 1

    waves = args.batch * args.prompt_len // args.tokens_per_step + 1
    for i in range(4 * waves):
        refill()
        st = eng.step()
        if st.prefill_tokens == 0:
            break
    else:
        raise RuntimeError(f"still prefilling after {4 * waves} steps")
    print(f"[{dense}] first pure decode step after {i} steps, "
          f"{len(sch.running)} rows running", flush=True)
    for _ in range(args.warmup):
        refill()
        eng.step()
    ms, rows, mixed = [], [], 0
    for _ in range(args.steps):
        refill()
        sync()
        t = time.time()
        st = eng.step()
        sync()
        dt = (time.time() - t) * 1e3
        if st.prefill_tokens == 0:
            ms.append(dt)
            rows.append(st.scheduled_tokens)
        else:
            mixed += 1
    if len(ms) * 2 < args.steps:
        raise RuntimeError(f"only {len(ms)} of {args.steps} timed steps were "
                           "pure decode")
    out = dict(dense_weight_dtype=dense,
               ms_per_decode_step=statistics.median(ms), ms_min=min(ms),
               ms_max=max(ms), decode_steps=len(ms), mixed_steps=mixed,
               rows_min=min(rows), rows_max=max(rows),
               kv_blocks=eng.kv.num_blocks, kv_blocks_fit=fit,
               engine_init_s=init_s, free_after_init_gb=free / 2 ** 30,
               allocated_after_init_gb=alloc / 2 ** 30,
               graph=getattr(eng, "graph_runner", None) is not None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="qwen-3-32b")
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--max-new", type=int, default=128)
    ap.add_argument("--tokens-per-step", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--only", choices=list(SETTINGS), default=None,
                    help="run one setting in this process and print its "
                         "result as a JSON line (what the tool starts, one "
                         "fresh process per setting, so that the memory "
                         "figures of one do not depend on the other)")
    args = ap.parse_args()
    gpu = torch.cuda.is_available()
    if not gpu:
        args.batch = min(args.batch, 32)
        args.prompt_len = min(args.prompt_len, 16)
        args.tokens_per_step = min(args.tokens_per_step, 128)
    cols = ["dense_weight_dtype", "ms_per_decode_step", "ms_min", "ms_max",
            "decode_steps", "mixed_steps", "rows_min", "rows_max",
            "kv_blocks", "kv_blocks_fit", "engine_init_s",
            "free_after_init_gb", "allocated_after_init_gb", "graph"]
    if args.only:
        print("RESULT " + json.dumps(run(args, args.only, gpu)), flush=True)
        return
    lines = [",".join(cols)]
    for dense in SETTINGS:
        r = None
        with subprocess.Popen([sys.executable, __file__, "--only", dense]
                              + sys.argv[1:], stdout=subprocess.PIPE,
                              text=True) as child:
            for line in child.stdout:
                if line.startswith("RESULT "):
                    r = json.loads(line[len("RESULT "):])
                else:
                    print(line, end="", flush=True)
        if child.returncode != 0 or r is None:
            raise SystemExit(f"the {dense} run failed "
                             f"(exit {child.returncode}); stopping")
        print(r, flush=True)
        lines.append(",".join(f"{r[c]:.2f}" if isinstance(r[c], float)
                              else str(r[c]) for c in cols))
    outd = os.environ.get("BENCH_OUT", "bench_outputs")
    os.makedirs(outd, exist_ok=True)
    with open(os.path.join(outd, "dense_fp8_e2e.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
