"""Micro-benchmark of the norm in front of a dense FP8 projection: the fused
kernel (ops.rmsnorm_quant_fp8, csrc/rmsnorm_quant_fp8.hip) against the
two-kernel sequence it replaces, in ONE process.

Per row width C, row count R and output format ("rows": one scale per row;
"block128": one per row and 128-wide group) it times
  (a) separate: ops.fused_add_rmsnorm at the variant RMSNORM_REG_RULE picks
      for C, then the quantiser at its measured variant
      (ops.quantize_rows_fp8 / ops.quantize_rows_fp8_block128),
  (b) fused: ops.rmsnorm_quant_fp8,
  (c) a device copy that moves the bytes (b) has to move: it reads x and the
      residual and writes the residual and the codes, 7 C R bytes, so the
      copy is of 3.5 C R bytes,
and reports the median and min-max of each, (b) / (a), (b) / (c), and whether
(b) clears the project's routing margin over (a): median better by more than
twice the larger min-max spread.

Method of tools/bench_dense_fp8.py: variants alternate round by round; each
round times a window of back-to-back calls per variant; median (min-max)
over the rounds; three operand sets rotate call by call. The norm kernels
update x and the residual in place, so values drift from call to call; none
of the kernels' work depends on the values.

    python tools/bench_rmsnorm_quant.py [--rounds 7] [--c 5120,4096]
                                        [--r 8,64,256,2048,32768]
Writes bench_outputs/rmsnorm_quant_bench.csv (or under $BENCH_OUT)."""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from sutro_amd import ops  # noqa: E402
from sutro_amd.ops import torch_ref  # noqa: E402

CS = [5120, 4096]
RS = [8, 64, 256, 2048, 32768]
NSETS = 3
EPS = 1e-6
F8 = torch.float8_e4m3fn


def window(fn, calls):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for c in range(calls):
        fn(c % NSETS)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1000.0 / calls  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--c", type=str, default=None, metavar="C,C,..")
    ap.add_argument("--r", type=str, default=None, metavar="R,R,..")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a CPU timing says nothing here")
    cs = [int(c) for c in args.c.split(",")] if args.c else CS
    rs = [int(r) for r in args.r.split(",")] if args.r else RS
    print(f"rounds={args.rounds} operand sets={NSETS} "
          f"device={torch.cuda.get_device_name(0)}", flush=True)
    rows = ["format,C,R,calls,separate_us,separate_min_us,separate_max_us,"
            "fused_us,fused_min_us,fused_max_us,copy_us,copy_min_us,"
            "copy_max_us,fused_over_separate,fused_over_copy,fused_gbps,"
            "clears_margin"]
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    for C in cs:
        w = (1 + 0.1 * torch.randn(C, device="cuda", generator=g)).bfloat16()
        for R in rs:
            # windows of 10 ms and more
            calls = 2000 if R <= 256 else 500 if R <= 2048 else 50
            xs = [(3 * torch.randn(R, C, device="cuda", generator=g))
                  .bfloat16() for _ in range(NSETS)]
            res = [(5 * torch.randn(R, C, device="cuda", generator=g))
                   .bfloat16() for _ in range(NSETS)]
            q = torch.empty(R, torch_ref.fp8_padded_k(C), dtype=F8,
                            device="cuda")
            s = torch.empty(R, dtype=torch.float32, device="cuda")
            src = torch.empty(R * C * 7 // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)

            def sep_rows(i):
                y, _ = ops.fused_add_rmsnorm(xs[i], res[i], w, EPS)
                ops.quantize_rows_fp8(y, q, s)

            def sep_block(i):
                y, _ = ops.fused_add_rmsnorm(xs[i], res[i], w, EPS)
                ops.quantize_rows_fp8_block128(y)

            vs = [("sep_rows", sep_rows), ("sep_block128", sep_block),
                  ("fused_rows", lambda i: ops.rmsnorm_quant_fp8(
                      xs[i], res[i], w, EPS, "rows")),
                  ("fused_block128", lambda i: ops.rmsnorm_quant_fp8(
                      xs[i], res[i], w, EPS, "block128")),
                  ("copy", lambda i: dst.copy_(src))]
            times = {name: [] for name, _ in vs}
            for r in range(args.rounds + 1):  # round 0 warms up
                for name, fn in vs:
                    t = window(fn, calls if r else 3)
                    if r:
                        times[name].append(t)
            med = {n: statistics.median(t) for n, t in times.items()}
            spread = {n: max(t) - min(t) for n, t in times.items()}
            for fmt in ("rows", "block128"):
                a, b = "sep_" + fmt, "fused_" + fmt
                clears = med[a] - med[b] > 2 * max(spread[a], spread[b])
                rows.append(
                    f"{fmt},{C},{R},{calls},"
                    + ",".join(f"{f(times[n]):.2f}" for n in (a, b, "copy")
                               for f in (statistics.median, min, max))
                    + f",{med[b] / med[a]:.3f},{med[b] / med['copy']:.3f},"
                    f"{7.0 * C * R / med[b] / 1e3:.0f},{int(clears)}")
                print(f"{fmt:8s} C={C} R={R:6d}: separate {med[a]:8.2f} us "
                      f"({min(times[a]):.2f}-{max(times[a]):.2f})  fused "
                      f"{med[b]:8.2f} us ({min(times[b]):.2f}-"
                      f"{max(times[b]):.2f})  copy {med['copy']:8.2f} us "
                      f"({min(times['copy']):.2f}-{max(times['copy']):.2f})  "
                      f"fused/separate {med[b] / med[a]:.3f}  fused/copy "
                      f"{med[b] / med['copy']:.3f}  margin "
                      f"{'cleared' if clears else 'not cleared'}", flush=True)
            del xs, res, q, s, src, dst
            torch.cuda.empty_cache()

    outd = os.environ.get("BENCH_OUT", "bench_outputs")
    os.makedirs(outd, exist_ok=True)
    with open(os.path.join(outd, "rmsnorm_quant_bench.csv"), "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
