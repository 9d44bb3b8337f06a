"""Micro-benchmark of split-KV decode attention (csrc/attn_decode_split.hip)
against the per-row MFMA decode kernel (csrc/attn_decode_mfma.hip), all in ONE
process: the measurement behind ops.DECODE_SPLIT_RULE (profiles/PROFILES.md,
capture S1).

Per head layout, KV dtype, decode batch n_dec and context it times
  row   the per-row kernel (kv_splits = 1, what the engine runs by default),
  S1    the split kernel forced to one block-split (intra-block split only,
        direct store), and
  S2 .. S16  the split + merge kernels at that many block-splits,
and reports the median (min-max) time per call and the ratio to `row`.

Method of tools/bench_dense_fp8.py: variants alternate round by round, one
warm-up round, median (min-max) over the rounds. A window is one hipGraph of
back-to-back calls, so the time is the kernels' and not the host's (the
engine's decode steps are replayed graphs too). Every row of a call has the
full context; the calls of a window walk KV sets scattered over one pool, as
many as it takes to stream 512 MiB between two visits of a set, so no call
finds its pages in the last-level cache (cells of 4 GiB and more use one
set). Cells whose pool would not fit --pool-gib are dropped and named.

    python tools/bench_attn_decode_split.py [--rounds 5] [--pool-gib 72]
        [--layouts 64/8/128,16/2/128,64/8/64] [--n-dec 1,8,64,512,2048]
        [--ctx 1024,8192,32768] [--kv bf16,e4m3]
Writes bench_outputs/attn_decode_split_bench.csv (or under $BENCH_OUT)."""

import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from sutro_amd import ops  # noqa: E402

BS = 32
VARIANTS = [("row", 0), ("S1", 1), ("S2", 2), ("S4", 4), ("S8", 8),
            ("S16", 16)]
ROTATE_BYTES = 512 << 20
ONE_SET_BYTES = 4 << 30
MAX_SETS = 512
WINDOW_US = 5000.0


def fill(pool):
    """Gaussian codes, one 16M-element chunk repeated (timing only)."""
    chunk = torch.randn(1 << 24, device=pool.device).to(torch.bfloat16)
    flat = pool.view(-1)
    for i in range(0, flat.numel(), chunk.numel()):
        n = min(chunk.numel(), flat.numel() - i)
        flat[i:i + n].copy_(chunk[:n])


def call(q, kc, vc, bt, sl, ql, scale, s, ws):
    return ops.paged_attention(q, kc, vc, bt, sl, ql, scale,
                               num_decodes_tail=q.shape[0],
                               kv_splits=2 if s else 1, split_workspace=ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pool-gib", type=float, default=72.0)
    ap.add_argument("--layouts", default="64/8/128,16/2/128,64/8/64")
    ap.add_argument("--n-dec", default="1,8,64,512,2048")
    ap.add_argument("--ctx", default="1024,8192,32768")
    ap.add_argument("--kv", default="bf16,e4m3")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = "cuda"
    n_decs = [int(x) for x in args.n_dec.split(",")]
    ctxs = [int(x) for x in args.ctx.split(",")]
    out_dir = os.environ.get("BENCH_OUT", "bench_outputs")
    os.makedirs(out_dir, exist_ok=True)
    csv = open(os.path.join(out_dir, "attn_decode_split_bench.csv"), "w")
    csv.write("layout,kv,n_dec,ctx,sets,calls,variant,median_us,min_us,"
              "max_us,ratio_to_row\n")

    for layout in args.layouts.split(","):
        hq, hk, d = (int(x) for x in layout.split("/"))
        scale = 1.0 / math.sqrt(d)
        for kv in args.kv.split(","):
            es = 1 if kv == "e4m3" else 2
            page_bytes = 2 * hk * BS * d * es          # K and V
            cells = []
            for n in n_decs:
                for ctx in ctxs:
                    foot = n * (ctx // BS) * page_bytes
                    sets = 1 if foot >= ONE_SET_BYTES else min(
                        MAX_SETS, max(2, -(-ROTATE_BYTES // foot)))
                    if sets * foot > args.pool_gib * (1 << 30):
                        print(f"# dropped (pool): {layout} {kv} n_dec={n} "
                              f"ctx={ctx}", flush=True)
                        continue
                    cells.append((n, ctx, sets))
            nblk = max(n * (ctx // BS) * sets for n, ctx, sets in cells)
            dt = torch.float8_e4m3fn if kv == "e4m3" else torch.bfloat16
            kc = torch.empty(nblk, hk, BS, d, dtype=torch.bfloat16
                             if es == 2 else torch.uint8, device=dev)
            vc = torch.empty_like(kc)
            if es == 2:
                fill(kc), fill(vc)
            else:   # any byte but the two e4m3 NaN codes
                kc.random_(0, 0x7F), vc.random_(0, 0x7F)
                kc, vc = kc.view(dt), vc.view(dt)
            perm = torch.randperm(nblk, device=dev).to(torch.int32)
            for n, ctx, sets in cells:
                pages = ctx // BS
                q = torch.randn(n, hq, d, device=dev).to(torch.bfloat16)
                bts = perm[:sets * n * pages].view(sets, n, pages).contiguous()
                sl = torch.full((n,), ctx, dtype=torch.int32, device=dev)
                ql = torch.arange(n + 1, dtype=torch.int32, device=dev)
                ws = ops.alloc_decode_split_workspace(n, hq, d, 16, dev)
                graphs, calls = {}, max(sets, 3)
                for name, s in VARIANTS:
                    ops.set_decode_kv_splits(s or None)
                    # eager warm-up, timed, sizes the window
                    t0 = torch.cuda.Event(enable_timing=True)
                    t1 = torch.cuda.Event(enable_timing=True)
                    call(q, kc, vc, bts[0], sl, ql, scale, s, ws)
                    t0.record()
                    call(q, kc, vc, bts[-1], sl, ql, scale, s, ws)
                    t1.record()
                    torch.cuda.synchronize()
                    if name == "row":
                        est = t0.elapsed_time(t1) * 1000.0
                        reps = max(1, min(8, int(WINDOW_US / (est * calls))))
                        calls *= reps
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        for c in range(calls):
                            call(q, kc, vc, bts[c % sets], sl, ql, scale, s, ws)
                    graphs[name] = g
                ops.set_decode_kv_splits(None)
                times = {name: [] for name, _ in VARIANTS}
                for rnd in range(args.rounds + 1):
                    for name, _ in VARIANTS:
                        t0 = torch.cuda.Event(enable_timing=True)
                        t1 = torch.cuda.Event(enable_timing=True)
                        t0.record()
                        graphs[name].replay()
                        t1.record()
                        torch.cuda.synchronize()
                        if rnd:   # round 0 warms up
                            times[name].append(
                                t0.elapsed_time(t1) * 1000.0 / calls)
                base = statistics.median(times["row"])
                line = [f"{layout} {kv:4s} n_dec={n:<5d} ctx={ctx:<6d}"]
                for name, _ in VARIANTS:
                    t = times[name]
                    med = statistics.median(t)
                    csv.write(f"{layout},{kv},{n},{ctx},{sets},{calls},{name},"
                              f"{med:.2f},{min(t):.2f},{max(t):.2f},"
                              f"{med / base:.3f}\n")
                    line.append(f"{name} {med:9.1f} ({min(t):.1f}-{max(t):.1f})"
                                f" x{med / base:.2f}")
                csv.flush()
                print(" | ".join(line), flush=True)
                del graphs, ws, bts, q
            del kc, vc, perm
            torch.cuda.empty_cache()
    csv.close()


if __name__ == "__main__":
    main()
