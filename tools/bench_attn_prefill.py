"""Micro-benchmark of prefill attention (reference kernel against the
pipelined kernel at each tile granularity) and, with --glue, of the wave's two
streaming kernels (fused_add_rmsnorm, qkv_prep), all in ONE process by the
method of tools/bench_gate_up.py.

Variants alternate round by round; each round times a window of back-to-back
calls per variant between device events; round 0 warms up; median (min-max)
over the rounds is reported. Every table ends with a plain device copy that
moves the same number of bytes (half read, half written): the floor of this
process on this device, not a data-sheet figure. Two sets of the streamed
operand (q for attention, x / residual / qkv for the others) rotate call by
call; the K/V pages, the weights and the cos/sin table are the same on every
call, so at the smaller shapes (KV of the continuation shape is 201 MB) they
can stay in the last-level cache, for every variant alike.

    python tools/bench_attn_prefill.py [--rounds 5] [--calls 20] [--glue]
Writes bench_outputs/attn_prefill_bench.txt (or under $BENCH_OUT)."""

import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from sutro_amd import ops  # noqa: E402
from sutro_amd.ops import torch_ref as R  # noqa: E402

HQ, HK, D, BS = 64, 8, 128, 32
NSETS = 2

# (label, shape class, [(ctx, new)] per sequence)
SHAPES = [
    ("wave 242 x 128 fresh", "prefill", [(0, 128)] * 242),
    ("64 x 512 fresh", "prefill", [(0, 512)] * 64),
    ("seeded step 1792 x 1 new, ctx 128-255", "single",
     [(128 + (i * 37) % 128, 1) for i in range(1792)]),
    ("continuation 128 x (ctx 256, new 128)", "prefill", [(256, 128)] * 128),
]


def window(fn, calls):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for c in range(calls):
        fn(c % NSETS)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1000.0 / calls  # us per call


def run_table(emit, title, variants, nbytes, rounds, calls):
    half = nbytes // 2
    src = [torch.empty(half, dtype=torch.uint8, device="cuda").random_(0, 255)
           for _ in range(NSETS)]
    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
    variants = variants + [("device copy, same bytes",
                            lambda i: dst.copy_(src[i]))]
    times = {name: [] for name, _ in variants}
    for r in range(rounds + 1):  # round 0 warms up
        for name, fn in variants:
            t = window(fn, calls if r else 3)
            if r:
                times[name].append(t)
    emit(f"{title}  ({nbytes / 1e6:.0f} MB per call)")
    for name, _ in variants:
        ts = times[name]
        med = statistics.median(ts)
        emit(f"  {name:30s} {med:9.1f} us ({min(ts):.1f}-{max(ts):.1f})"
             f"  {nbytes / med / 1e6:6.2f} TB/s")
    del src, dst
    torch.cuda.empty_cache()


def attn_inputs(seqs, gen):
    S = len(seqs)
    new = [n for _, n in seqs]
    lens = [c + n for c, n in seqs]
    pages = [(L + BS - 1) // BS for L in lens]
    nb = sum(pages)
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(1))
    bt = torch.zeros(S, max(pages), dtype=torch.int32)
    i = 0
    for s, n in enumerate(pages):
        bt[s, :n] = perm[i:i + n].to(torch.int32)
        i += n
    kc = torch.randn(nb, HK, BS, D, device="cuda", generator=gen).bfloat16()
    vc = torch.randn(nb, HK, BS, D, device="cuda", generator=gen).bfloat16()
    T = sum(new)
    qs = [torch.randn(T, HQ, D, device="cuda", generator=gen).bfloat16()
          for _ in range(NSETS)]
    qlocs = torch.tensor([0] + list(torch.tensor(new).cumsum(0)),
                         dtype=torch.int32, device="cuda")
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    nbytes = 2 * T * HQ * D * 2 + 2 * nb * HK * BS * D * 2
    return qs, kc, vc, bt.cuda(), sl, qlocs, new, T, nbytes


def attn_tables(emit, rounds, calls):
    gen = torch.Generator(device="cuda")
    scale = 1.0 / math.sqrt(D)
    for label, cls, seqs in SHAPES:
        gen.manual_seed(len(seqs))
        qs, kc, vc, bt, sl, ql, new, T, nbytes = attn_inputs(seqs, gen)

        def make(rows, variant):
            ts, tq = [], []
            for s, c in enumerate(new):
                for j in range(0, c, rows):
                    ts.append(s)
                    tq.append(j)
            ts = torch.tensor(ts, dtype=torch.int32, device="cuda")
            tq = torch.tensor(tq, dtype=torch.int32, device="cuda")
            return lambda i: ops.paged_attention(
                qs[i], kc, vc, bt, sl, ql, scale, 0, ts, tq, T,
                tile_rows=rows, prefill_variant=variant)

        vs = [("reference (32 rows)", make(32, "v1"))]
        for rows in ops.PREFILL_TILE_ROWS:
            if ops.attn_prefill_pipe_supported(HQ, HK, D, rows):
                vs.append((f"pipelined, {rows} rows", make(rows, "pipe")))
        ref = vs[0][1](0)
        for name, fn in vs[1:]:
            assert torch.equal(fn(0), ref), name
        run_table(emit, f"attn_prefill [{cls}] {label}", vs, nbytes, rounds,
                  calls)
        del qs, kc, vc
        torch.cuda.empty_cache()


def glue_tables(emit, rounds, calls):
    C = 5120
    gen = torch.Generator(device="cuda")
    for rows in (30976, 2048):
        gen.manual_seed(rows)
        xs = [torch.randn(rows, C, device="cuda", generator=gen).bfloat16()
              for _ in range(NSETS)]
        rs = [torch.randn(rows, C, device="cuda", generator=gen).bfloat16()
              for _ in range(NSETS)]
        w = torch.ones(C, device="cuda", dtype=torch.bfloat16)
        run_table(emit, f"fused_add_rmsnorm rows={rows} C={C}",
                  [("reference",
                    lambda i: ops.fused_add_rmsnorm(xs[i], rs[i], w, 1e-6,
                                                    variant="v1")),
                   ("row in registers",
                    lambda i: ops.fused_add_rmsnorm(xs[i], rs[i], w, 1e-6,
                                                    variant="reg"))],
                  4 * rows * C * 2, rounds, calls)
        del xs, rs
        torch.cuda.empty_cache()

        nb = (rows + BS - 1) // BS
        qkvs = [torch.randn(rows, (HQ + 2 * HK) * D, device="cuda",
                            generator=gen).bfloat16() for _ in range(NSETS)]
        kc = torch.zeros(nb, HK, BS, D, device="cuda", dtype=torch.bfloat16)
        vc = torch.zeros_like(kc)
        pos = (torch.arange(rows, device="cuda") % 128).long()
        slots = torch.randperm(nb * BS, device="cuda")[:rows].long()
        cs = R.rope_cos_sin(256, D, 1e6).cuda()
        qw = torch.ones(D, device="cuda", dtype=torch.bfloat16)
        kw = torch.ones(D, device="cuda", dtype=torch.bfloat16)
        run_table(emit, f"qkv_prep rows={rows} Hq={HQ} Hk={HK} D={D}",
                  [("qkv_prep v2",
                    lambda i: ops.fused_qkv_prep(qkvs[i], HQ, HK, D, pos,
                                                 slots, kc, vc, cs, qw, kw,
                                                 1e-6))],
                  2 * rows * (HQ + 2 * HK) * D * 2, rounds, calls)
        del qkvs, kc, vc
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--glue", action="store_true",
                    help="also time fused_add_rmsnorm and qkv_prep")
    ap.add_argument("--glue-only", action="store_true")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"rounds={args.rounds} calls/window={args.calls} input sets={NSETS}"
         f" device={torch.cuda.get_device_name(0)}"
         f" Hq={HQ} Hk={HK} D={D} bf16 KV")
    if not args.glue_only:
        attn_tables(emit, args.rounds, args.calls)
    if args.glue or args.glue_only:
        glue_tables(emit, args.rounds, args.calls)
    outd = os.environ.get("BENCH_OUT", "bench_outputs")
    os.makedirs(outd, exist_ok=True)
    with open(os.path.join(outd, "attn_prefill_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
