"""Micro-benchmark of the dense-MLP gate_up + SwiGLU step: library GEMM +
silu_mul against the hand-written kernels, all in ONE process.

Variants alternate round by round; each round times a window of back-to-back
calls per variant; median (min-max) over the rounds is reported. Operands are
Gaussian (x ~ N(0,1), w ~ N(0,1)/sqrt(K)); three weight sets rotate call by
call so no call finds its weights in the last-level cache; the TunableOp
table is loaded the way the engine loads it.

    python tools/bench_gate_up.py [--rounds 5] [--calls 20] [--quick]
    python tools/bench_gate_up.py --variant-sweep [M,M,..]
Writes bench_outputs/gate_up_bench.txt (or under $BENCH_OUT).

--variant-sweep compares the fused kernel's variants on the 32B shape (same
method): the one-tile kernel ("v1"), v1 in the grouped tile order, the
persistent kernel, persistent + grouped order, and that with wide epilogue
stores, group_m in {4, 8, 16}, the wide stores on one block per tile, and
the XCD-banded order (group_m = -8) on both kernels; writes gate_up_variant_sweep.txt."""

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

# (label, M, I, K): Qwen3-32B gate_up at the decode buckets and the prefill
# wave; 8B and 14B at M=2048 for information
SHAPES = [
    ("32b", 1792, 25600, 5120),
    ("32b", 1920, 25600, 5120),
    ("32b", 2048, 25600, 5120),
    ("32b", 32768, 25600, 5120),
    ("8b", 2048, 12288, 4096),
    ("14b", 2048, 17408, 5120),
]
NSETS = 3


def variants(M):
    bm = 256 if M % 256 == 0 else 128
    return [
        ("library F.linear + silu_mul",
         lambda x, w: ops.silu_mul(F.linear(x, w))),
        (f"gemm_tn (dbuf, bm{bm}) + silu_mul",
         lambda x, w: ops.silu_mul(_C.gemm_tn(x, w, None, bm, 256, 2, 1))),
        ("pipelined plain (no silu_mul)",
         lambda x, w: _C.gemm_tn_pipelined(x, w, None, 2, 1)),
        ("pipelined plain + silu_mul",
         lambda x, w: ops.silu_mul(_C.gemm_tn_pipelined(x, w, None, 2, 1))),
        ("fused swz2 xcd1",
         lambda x, w: _C.gemm_gate_up_silu(x, w, 2, 1)),
        ("fused swz2 xcd0",
         lambda x, w: _C.gemm_gate_up_silu(x, w, 2, 0)),
        ("fused swz1 xcd1",
         lambda x, w: _C.gemm_gate_up_silu(x, w, 1, 1)),
    ]


# the M of capture G2: the routed decode buckets, the prefill waves, and the
# held-back buckets 1536 / 1664 / 1792 (for information only)
SWEEP_M = [1152, 1280, 1408, 1920, 2048, 3072, 4096, 8192, 16384, 30976,
           32768, 1536, 1664, 1792]
GROUP_MS = (4, 8, 16)


def sweep_variants():
    def fused(variant, group_m, wide, num_blocks=0):
        return lambda x, w: _C.gemm_gate_up_silu(x, w, 2, 1, variant, group_m,
                                                 num_blocks, wide)
    vs = [("v1", fused(0, 0, False))]
    vs += [(f"v1 g{g}", fused(0, g, False)) for g in GROUP_MS]
    vs += [("v1 banded g8", fused(0, -8, False))]
    vs += [("persistent", fused(1, 0, False))]
    vs += [(f"persistent g{g}", fused(1, g, False)) for g in GROUP_MS]
    vs += [(f"persistent g{g} wide", fused(1, g, True)) for g in GROUP_MS]
    # the persistent kernel's code on one block per tile: the wide stores
    # without the static tile walk
    vs += [("block per tile g8 wide", fused(1, 8, True, -1))]
    vs += [("persistent banded g8 wide", fused(1, -8, True))]
    return vs


def window(fn, xs, ws, calls):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for c in range(calls):
        fn(xs[c % NSETS], ws[c % NSETS])
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1000.0 / calls  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--quick", action="store_true",
                    help="only the M=2048 32B shape")
    ap.add_argument("--route-sweep", type=str, default=None, metavar="M,M,..",
                    help="library pair vs fused on the 32B shape at these M "
                         "(for the routing threshold)")
    ap.add_argument("--variant-sweep", type=str, default=None, nargs="?",
                    const=",".join(map(str, SWEEP_M)), metavar="M,M,..",
                    help="the fused kernel's variants on the 32B shape at "
                         "these M (default: the M of capture G2)")
    args = ap.parse_args()

    _setup_tunableop(EngineConfig(spec=get_model_spec("qwen-3-32b"),
                                  device="cuda"))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"rounds={args.rounds} calls/window={args.calls} weight sets={NSETS}"
         f" device={torch.cuda.get_device_name(0)}")
    shapes = [s for s in SHAPES if not args.quick or s[:2] == ("32b", 2048)]
    if args.route_sweep or args.variant_sweep:
        shapes = [("32b", int(m), 25600, 5120)
                  for m in (args.route_sweep or args.variant_sweep).split(",")]
    for label, M, I, K in shapes:
        g = torch.Generator(device="cuda")
        g.manual_seed(M + I)
        ws = [(torch.randn(2 * I, K, device="cuda", generator=g) / K ** 0.5)
              .bfloat16() for _ in range(NSETS)]
        xs = [torch.randn(M, K, device="cuda", generator=g).bfloat16()
              for _ in range(NSETS)]
        vs = variants(M)
        if args.route_sweep:
            vs = [vs[0], vs[4]]
        if args.variant_sweep:
            vs = sweep_variants()
        times = {name: [] for name, _ in vs}
        for r in range(args.rounds + 1):  # round 0 warms up
            for name, fn in vs:
                t = window(fn, xs, ws, args.calls if r else 3)
                if r:
                    times[name].append(t)
        flops = 2.0 * M * 2 * I * K
        emit(f"{label} gate_up M={M} N={2 * I} K={K}")
        for name, _ in vs:
            ts = times[name]
            med = statistics.median(ts)
            emit(f"  {name:34s} {med:9.1f} us ({min(ts):.1f}-{max(ts):.1f})"
                 f"  {flops / med / 1e6:7.1f} TF/s  spread "
                 f"{(max(ts) - min(ts)) / med * 100:4.1f}%")
        del ws, xs
        torch.cuda.empty_cache()

    outd = os.environ.get("BENCH_OUT", "bench_outputs")
    os.makedirs(outd, exist_ok=True)
    name = ("gate_up_route_sweep.txt" if args.route_sweep else
            "gate_up_variant_sweep.txt" if args.variant_sweep else
            "gate_up_bench.txt")
    with open(os.path.join(outd, name), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
