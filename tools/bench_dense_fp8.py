"""Micro-benchmark of the dense FP8 projections, per-channel W8A8
(csrc/gemm_tn_fp8_pipe.hip) and block-scaled (csrc/gemm_tn_fp8_block_pipe.hip,
dense_weight_dtype="fp8_block128"), against what the bf16 model runs for the
same projection, all in ONE process.

Per Qwen3-32B projection shape and token count M it times
  (a) the activation row quantiser (ops.quantize_rows_fp8),
  (b) the FP8 GEMM on pre-quantised operands,
  (c) the bf16 path: the library GEMM, or ops.gate_up_silu for gate_up (the
      library pair or the fused bf16 kernel, as GATE_UP_FUSED_RULE routes M),
  (d) the 128-wide group quantiser (ops.quantize_rows_fp8_block128),
  (e) the block-scaled GEMM on pre-quantised operands,
and reports TF/s of (b), (c) and (e) and the ratios (a + b) / c, (d + e) / c
and (d + e) / (a + b).

Method of tools/bench_gate_up.py: variants alternate round by round; each
round times a window of back-to-back calls per variant; median (min-max)
over the rounds. Operands are Gaussian (x ~ N(0,1), w ~ N(0,1)/sqrt(K)), real
quantised codes on the FP8 side; three operand sets rotate call by call so
no call finds its weights in the last-level cache; the TunableOp table is
loaded the way the engine loads it.

    python tools/bench_dense_fp8.py [--rounds 5] [--calls 10] [--m 64,2048]
Writes bench_outputs/dense_fp8_bench.csv (or under $BENCH_OUT)."""

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from sutro_amd import _C, ops  # noqa: E402
from sutro_amd.engine.config import EngineConfig  # noqa: E402
from sutro_amd.engine.engine import _setup_tunableop  # noqa: E402
from sutro_amd.models.registry import get_model_spec  # noqa: E402
from sutro_amd.ops import torch_ref  # noqa: E402

# (label, N, K) of Qwen3-32B at TP=1; gate_up's N is the merged 2I
SHAPES = [
    ("qkv", 10240, 5120),
    ("o", 5120, 8192),
    ("gate_up", 51200, 5120),
    ("down", 5120, 25600),
]
MS = [64, 256, 1152, 2048, 32768]
NSETS = 3
F8 = torch.float8_e4m3fn


def quantize(t):
    q = torch.empty(t.shape[0], torch_ref.fp8_padded_k(t.shape[1]), dtype=F8,
                    device=t.device)
    s = torch.empty(t.shape[0], dtype=torch.float32, device=t.device)
    ops.quantize_rows_fp8(t, q, s)
    return q, s


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--m", type=str, default=None, metavar="M,M,..")
    args = ap.parse_args()
    ms = [int(m) for m in args.m.split(",")] if args.m else MS

    _setup_tunableop(EngineConfig(spec=get_model_spec("qwen-3-32b"),
                                  device="cuda"))
    print(f"rounds={args.rounds} calls/window={args.calls} operand sets="
          f"{NSETS} device={torch.cuda.get_device_name(0)}", flush=True)
    rows = ["shape,M,N,K,quant_us,fp8_gemm_us,bf16_us,quant_min_us,"
            "quant_max_us,fp8_min_us,fp8_max_us,bf16_min_us,bf16_max_us,"
            "fp8_gemm_tflops,bf16_tflops,ratio_quant_plus_gemm_over_bf16,"
            "block_quant_us,block_gemm_us,block_quant_min_us,"
            "block_quant_max_us,block_gemm_min_us,block_gemm_max_us,"
            "block_gemm_tflops,ratio_block_over_bf16,"
            "ratio_block_over_per_channel"]
    for label, N, K in SHAPES:
        g = torch.Generator(device="cuda")
        g.manual_seed(N + K)
        ws = [(torch.randn(N, K, device="cuda", generator=g) / K ** 0.5)
              .bfloat16() for _ in range(NSETS)]
        wq = [quantize(w) for w in ws]
        wb = [torch_ref.quantize_weight_fp8_block128(w) for w in ws]
        for M in ms:
            xs = [torch.randn(M, K, device="cuda", generator=g).bfloat16()
                  for _ in range(NSETS)]
            xq = [quantize(x) for x in xs]
            xb = [ops.quantize_rows_fp8_block128(x) for x in xs]
            if label == "gate_up":
                def fp8(i):
                    _C.gemm_fp8_gate_up_silu(*xq[i], *wq[i], 1)

                def blk(i):
                    _C.gemm_fp8_block_gate_up_silu(*xb[i], *wb[i], 1)

                def bf16(i):
                    ops.gate_up_silu(xs[i], ws[i])
            else:
                def fp8(i):
                    _C.gemm_fp8_pipelined(*xq[i], *wq[i], None, 1)

                def blk(i):
                    _C.gemm_fp8_block_pipelined(*xb[i], *wb[i], None, 1)

                def bf16(i):
                    F.linear(xs[i], ws[i])

            def quant(i):
                ops.quantize_rows_fp8(xs[i], *xq[i])

            def bquant(i):
                ops.quantize_rows_fp8_block128(xs[i])

            vs = [("quant", quant), ("fp8", fp8), ("bf16", bf16),
                  ("bquant", bquant), ("blk", blk)]
            times = {name: [] for name, _ in vs}
            for r in range(args.rounds + 1):  # round 0 warms up
                for name, fn in vs:
                    t = window(fn, args.calls if r else 3)
                    if r:
                        times[name].append(t)
            med = {n: statistics.median(t) for n, t in times.items()}
            flops = 2.0 * M * N * K
            ratio = (med["quant"] + med["fp8"]) / med["bf16"]
            bratio = (med["bquant"] + med["blk"]) / med["bf16"]
            bover = (med["bquant"] + med["blk"]) / (med["quant"] + med["fp8"])
            rows.append(
                f"{label},{M},{N},{K},{med['quant']:.1f},{med['fp8']:.1f},"
                f"{med['bf16']:.1f},"
                + ",".join(f"{f(times[n]):.1f}" for n in ("quant", "fp8", "bf16")
                           for f in (min, max))
                + f",{flops / med['fp8'] / 1e6:.1f},"
                f"{flops / med['bf16'] / 1e6:.1f},{ratio:.3f},"
                f"{med['bquant']:.1f},{med['blk']:.1f},"
                + ",".join(f"{f(times[n]):.1f}" for n in ("bquant", "blk")
                           for f in (min, max))
                + f",{flops / med['blk'] / 1e6:.1f},{bratio:.3f},{bover:.3f}")
            print(f"{label:8s} M={M:6d} N={N} K={K}: quant {med['quant']:8.1f}"
                  f" us  fp8 {med['fp8']:9.1f} us ({flops / med['fp8'] / 1e6:7.1f}"
                  f" TF/s)  bf16 {med['bf16']:9.1f} us "
                  f"({flops / med['bf16'] / 1e6:7.1f} TF/s)  (a+b)/c "
                  f"{ratio:.3f}  | block: quant {med['bquant']:8.1f} us  gemm "
                  f"{med['blk']:9.1f} us ({flops / med['blk'] / 1e6:7.1f} TF/s)"
                  f"  (d+e)/c {bratio:.3f}  (d+e)/(a+b) {bover:.3f}",
                  flush=True)
            del xs, xq, xb
        del ws, wq, wb
        torch.cuda.empty_cache()

    outd = os.environ.get("BENCH_OUT", "bench_outputs")
    os.makedirs(outd, exist_ok=True)
    with open(os.path.join(outd, "dense_fp8_bench.csv"), "w") as f:
        f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
