"""Micro-benchmark of the FP8 MoE expert stage sequence at qwen-3-30b-a3b
expert shapes (E 128, h 2048, m 768, top-8), all in ONE process, by the method
of tools/bench_gate_up.py:

    block    quant(x), stage 1 (writes the quantised stage-2 input), stage 2
             (csrc/grouped_gemm_fp8_block.hip, moe_weight_dtype="fp8_block128")
    channel  quant(x), stage 1, quant(act), stage 2
             (csrc/grouped_gemm_fp8.hip, moe_weight_dtype="fp8_e4m3")

The two alternate round by round; each round times a window of back-to-back
sequences per variant; median (min-max) over the rounds is reported, and the
ratio of the medians. Operands are Gaussian (x ~ N(0,1), w ~ N(0,1)/sqrt(K));
routing is a uniform random top-8; three weight sets rotate call by call so
no call finds its weights in the last-level cache.

    python tools/bench_moe_fp8_block.py [--rounds 5] [--calls 20] [--tokens 64,2048,8192]
Writes bench_outputs/moe_fp8_block_bench.txt (or under $BENCH_OUT)."""

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from sutro_amd import ops  # noqa: E402
from sutro_amd.ops import torch_ref  # noqa: E402

E, H, M, TOPK = 128, 2048, 768, 8
NSETS = 3
F8 = torch.float8_e4m3fn


def routing(T, bm, g):
    """row_tok / tile_off / counts of a uniform random top-k routing, shaped
    as Qwen3MoE._forward_grouped shapes them"""
    idx = torch.rand(T, E, device="cuda", generator=g).topk(TOPK, dim=1)[1]
    flat_e = idx.reshape(-1)
    flat_tok = torch.arange(T, device="cuda").repeat_interleave(TOPK)
    order = torch.argsort(flat_e, stable=True)
    sorted_e = flat_e[order]
    counts = torch.bincount(flat_e, minlength=E).int()
    padded = (counts + (bm - 1)) // bm * bm
    pad_off = torch.zeros(E + 1, dtype=torch.int32, device="cuda")
    pad_off[1:] = torch.cumsum(padded, 0)
    first = torch.searchsorted(sorted_e, sorted_e, side="left")
    pos = torch.arange(T * TOPK, device="cuda") - first
    rows_max = T * TOPK + E * bm
    row_tok = torch.full((rows_max,), -1, dtype=torch.int32, device="cuda")
    row_tok[pad_off[sorted_e.long()].long() + pos] = flat_tok[order].int()
    return row_tok, pad_off // bm, counts, rows_max


def window(fn, calls):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for c in range(calls):
        fn(c % NSETS)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1000.0 / calls  # us per sequence


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--tokens", type=str, default="64,2048,8192")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"rounds={args.rounds} calls/window={args.calls} weight sets={NSETS}"
         f" device={torch.cuda.get_device_name(0)}")
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    blk, chn = [], []
    for _ in range(NSETS):
        sets = {}
        for name, (n, k) in (("gate_up", (2 * M, H)), ("down", (H, M))):
            w = (torch.randn(E, n, k, device="cuda", generator=g)
                 / k ** 0.5).bfloat16()
            pairs = [torch_ref.quantize_weight_fp8_block128(w[e])
                     for e in range(E)]
            sets[name + "_b"] = (torch.stack([q for q, _ in pairs]),
                                 torch.stack([s for _, s in pairs]))
            w_q = torch.empty(E, n, k, dtype=F8, device="cuda")
            w_s = torch.empty(E, n, dtype=torch.float32, device="cuda")
            ops.quantize_rows_fp8(w.view(E * n, k), w_q.view(E * n, k),
                                  w_s.view(-1))
            sets[name + "_c"] = (w_q, w_s)
            del w
        blk.append((sets["gate_up_b"], sets["down_b"]))
        chn.append((sets["gate_up_c"], sets["down_c"]))

    for T in (int(t) for t in args.tokens.split(",")):
        bm = 128 if T * TOPK >= E * 256 else 64  # the layer's rule
        row_tok, tile_off, counts, rows_max = routing(T, bm, g)
        max_tiles = rows_max // bm
        rows_al = (rows_max + 3) // 4 * 4
        xs = [torch.randn(T, H, device="cuda", generator=g).bfloat16()
              for _ in range(NSETS)]
        x_q = torch.empty(T, H, dtype=F8, device="cuda")
        x_sb = torch.empty(H // 128, T, device="cuda")
        x_sc = torch.empty(T, device="cuda")
        act = torch.zeros(rows_max, M, dtype=torch.bfloat16, device="cuda")
        act_q = torch.zeros(rows_max, M, dtype=torch.uint8,
                            device="cuda").view(F8)
        act_sb = torch.ones(M // 128, rows_al, device="cuda")
        act_sc = torch.ones(rows_max, device="cuda")
        out = torch.zeros(rows_max, H, dtype=torch.bfloat16, device="cuda")

        def block(i):
            (gu, gu_s), (dn, dn_s) = blk[i]
            ops.quantize_rows_fp8_block128_out(xs[i], x_q, x_sb)
            ops.grouped_gemm_fp8_block128_gate_q(
                act_q, act_sb, x_q, x_sb, gu, gu_s, row_tok, tile_off, counts,
                max_tiles, bm=bm)
            ops.grouped_gemm_fp8_block128(out, act_q, act_sb, dn, dn_s,
                                          tile_off, counts, max_tiles, bm=bm)

        def channel(i):
            (gu, gu_s), (dn, dn_s) = chn[i]
            ops.quantize_rows_fp8(xs[i], x_q, x_sc)
            ops.grouped_gemm_fp8(act, x_q, x_sc, gu, gu_s, row_tok, tile_off,
                                 counts, max_tiles, True, bm=bm)
            ops.quantize_rows_fp8(act, act_q, act_sc, row_limit=tile_off[E:],
                                  limit_mul=bm)
            ops.grouped_gemm_fp8(out, act_q, act_sc, dn, dn_s, None, tile_off,
                                 counts, max_tiles, False, bm=bm)

        vs = [("block", block), ("channel", channel)]
        times = {name: [] for name, _ in vs}
        for r in range(args.rounds + 1):  # round 0 warms up
            for name, fn in vs:
                t = window(fn, args.calls if r else 3)
                if r:
                    times[name].append(t)
        emit(f"a3b experts T={T} (rows {T * TOPK}, bm {bm})")
        med = {}
        for name, _ in vs:
            ts = times[name]
            med[name] = statistics.median(ts)
            emit(f"  {name:8s} {med[name]:9.1f} us ({min(ts):.1f}-{max(ts):.1f})"
                 f"  spread {(max(ts) - min(ts)) / med[name] * 100:4.1f}%")
        emit(f"  block / channel = {med['block'] / med['channel']:.3f}")

    outd = os.environ.get("BENCH_OUT", "bench_outputs")
    os.makedirs(outd, exist_ok=True)
    with open(os.path.join(outd, "moe_fp8_block_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
