"""Micro-benchmark of the MoE routing glue: router logits -> (row_tok,
tile_off, counts, padpos, w), the library-op sequence of
Qwen3MoE._route_torch (moe_routing="torch", the very method the layer runs)
against ops.moe_route (moe_routing="fused", csrc/moe_route.hip), in ONE
process, eager and as a captured hipGraph replay.

Method of tools/bench_gate_up.py: the two sides alternate round by round;
each round times a window of back-to-back calls per side between device
events; median (min-max) over the rounds. Eager windows rotate three logits
sets; a graph replays on its static buffer. Logits are N(0, 2) bf16, the
router's output dtype. --count-launches counts the kernel launches per call
with the torch profiler instead of timing (a run of its own: tracing slows
the host).

    python tools/bench_moe_route.py [--rounds 7] [--calls 50] [--quick]
    python tools/bench_moe_route.py --count-launches
Writes bench_outputs/moe_route_bench.txt (or under $BENCH_OUT).
"""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from sutro_amd import ops  # noqa: E402
from sutro_amd.models.qwen3 import Qwen3MoE  # noqa: E402
from sutro_amd.models.registry import ModelSpec  # noqa: E402

# (label, E, k, T)
SHAPES = [
    ("a3b", 128, 8, 2048),
    ("a3b", 128, 8, 8192),
    ("a3b", 128, 8, 32768),
    ("gpt-oss-20b", 32, 4, 8192),
    ("mixtral", 8, 2, 4096),
]
NSETS = 3


def router_layer(E, k):
    """a layer with the shape's routing fields; the experts stay tiny, the
    routing never reads them"""
    spec = ModelSpec(name="bench-route", hidden_size=64, num_layers=1,
                     num_heads=2, num_kv_heads=1, head_dim=32,
                     intermediate_size=0, vocab_size=64, num_experts=E,
                     experts_per_token=k, moe_intermediate_size=64)
    return Qwen3MoE(spec, torch.bfloat16).to("cuda")


def window(fn, sets, calls):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for c in range(calls):
        fn(sets[c % len(sets)])
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1000.0 / calls  # us per call


def captured(fn, static):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn(static)
    return lambda _logits: graph.replay()


def launches(fn, logits):
    from torch.profiler import ProfilerActivity, profile

    fn(logits)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(logits)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events()
               if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--quick", action="store_true", help="a3b T=2048 only")
    ap.add_argument("--count-launches", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_moe_route needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"rounds={args.rounds} calls/window={args.calls} "
         f"device={torch.cuda.get_device_name(0)}")
    for label, E, k, T in SHAPES[:1] if args.quick else SHAPES:
        moe = router_layer(E, k)
        bm = 128 if T * k >= E * 256 else 64
        g = torch.Generator(device="cuda")
        g.manual_seed(T + E)
        sets = [(torch.randn(T, E, device="cuda", generator=g) * 2).bfloat16()
                for _ in range(NSETS)]
        ws_t = {"row_tok": torch.empty(T * k + E * bm, dtype=torch.int32,
                                       device="cuda")}
        ws_f = ops.moe_route_workspace(T, k, E, "cuda", bm)
        sides = [
            ("torch eager", lambda lg: moe._route_torch(lg, ws_t, bm)),
            ("fused eager", lambda lg: ops.moe_route(lg, k, 0, E, bm, ws_f)),
        ]
        if args.count_launches:
            emit(f"{label} E={E} k={k} T={T} bm={bm}  launches/call: "
                 + ", ".join(f"{name.split()[0]} {launches(fn, sets[0])}"
                             for name, fn in sides))
            continue
        static = sets[0].clone()
        sides += [(name.replace("eager", "graph"), captured(fn, static))
                  for name, fn in sides]
        times = {name: [] for name, _ in sides}
        for r in range(args.rounds + 1):  # round 0 warms up
            for name, fn in sides:
                t = window(fn, sets, args.calls if r else 5)
                if r:
                    times[name].append(t)
        emit(f"{label} E={E} k={k} T={T} bm={bm}")
        for name, _ in sides:
            ts = times[name]
            med = statistics.median(ts)
            emit(f"  {name:12s} {med:9.1f} us ({min(ts):.1f}-{max(ts):.1f})"
                 f"  spread {(max(ts) - min(ts)) / med * 100:4.1f}%")
        for mode in ("eager", "graph"):
            emit(f"  torch/fused {mode}: "
                 f"{statistics.median(times['torch ' + mode]) / statistics.median(times['fused ' + mode]):.2f}x")

    outd = os.environ.get("BENCH_OUT", "bench_outputs")
    os.makedirs(outd, exist_ok=True)
    name = ("moe_route_launches.txt" if args.count_launches
            else "moe_route_bench.txt")
    with open(os.path.join(outd, name), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
