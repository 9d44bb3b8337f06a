"""Stage-pair microbenchmark of one MoE layer's expert GEMMs on one GPU:
gather + gate/up + SwiGLU, then down, at a model's shapes, for the bf16, FP8
and MXFP4 expert storage modes in ONE process (PROFILES.md captures F1, M1).

Random top-k routing (k distinct experts per token, so segments are
near-balanced), the engine's tile rule (BM = 128 if T*k >= 256*E else 64),
weights randn / sqrt(K), activations randn * 0.5. The quantised modes time
quant_rows_fp8(x) -> stage 1 -> quant_rows_fp8(act) -> stage 2: both
activation quantisation passes are inside the time. Weight sets are rotated
call by call (--sets) so that a small-T call cannot find its weights in the
last-level cache; device events around --calls back-to-back calls, --windows
such windows per mode with the modes alternating, after --warmup calls of
each; median (min-max) ms per layer call. TF/s counts 6*T*k*h*m flops (live
rows only).

    python tools/bench_moe_stage_pair.py --shape a3b --tokens 8192 64
"""

import argparse
import json
import statistics

import torch

from sutro_amd import ops
from sutro_amd.ops import torch_ref

SHAPES = {  # h, m, E, k
    "a3b": (2048, 768, 128, 8),
    "gpt-oss": (2880, 2880, 32, 4),
}
F8 = torch.float8_e4m3fn
DEV = "cuda"


def shaping(T, E, k, BM):
    idx = torch.rand(T, E, device=DEV).topk(k, dim=1).indices
    flat_e = idx.reshape(-1)
    flat_tok = torch.arange(T, device=DEV).repeat_interleave(k)
    order = torch.argsort(flat_e, stable=True)
    sorted_e, sorted_tok = flat_e[order], flat_tok[order]
    counts = torch.bincount(sorted_e, minlength=E).to(torch.int32)
    padded = (counts + (BM - 1)) // BM * BM
    pad_off = torch.zeros(E + 1, dtype=torch.int32, device=DEV)
    pad_off[1:] = torch.cumsum(padded, 0)
    first = torch.searchsorted(sorted_e, sorted_e, side="left")
    pos = torch.arange(T * k, device=DEV) - first
    rows_max = T * k + E * BM
    row_tok = torch.full((rows_max,), -1, dtype=torch.int32, device=DEV)
    row_tok[pad_off[sorted_e.long()].long() + pos] = sorted_tok.to(torch.int32)
    return row_tok, pad_off // BM, counts, rows_max


def convert(mode, w):
    E, N, K = w.shape
    if mode == "bf16":
        return (w,)
    if mode == "mxfp4":
        return ops.quantize_weight_mxfp4(w)
    Kp = torch_ref.fp8_padded_k(K)
    w_q = torch.empty(E, N, Kp, dtype=F8, device=DEV)
    s = torch.empty(E, N, dtype=torch.float32, device=DEV)
    ops.quantize_rows_fp8(w.view(E * N, K), w_q.view(E * N, Kp), s.view(-1))
    return w_q, s


def bench_shape(name, T, args):
    h, m, E, k = SHAPES[name]
    BM = 128 if T * k >= 256 * E else 64
    row_tok, tile_off, counts, rows_max = shaping(T, E, k, BM)
    max_tiles = rows_max // BM
    x = (torch.randn(T, h, device=DEV) * 0.5).to(torch.bfloat16)
    act = torch.zeros(rows_max, m, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(rows_max, h, dtype=torch.bfloat16, device=DEV)
    hp, mp = torch_ref.fp8_padded_k(h), torch_ref.fp8_padded_k(m)
    x_q = torch.zeros(T, hp, dtype=torch.uint8, device=DEV).view(F8)
    x_s = torch.ones(T, device=DEV)
    a_q = torch.zeros(rows_max, mp, dtype=torch.uint8, device=DEV).view(F8)
    a_s = torch.ones(rows_max, device=DEV)
    lim = tile_off[E:]

    # every mode stores the SAME bf16 weights, so outputs are comparable
    weights = {mode: [] for mode in args.modes}
    for _ in range(args.sets):
        w_gu = (torch.randn(E, 2 * m, h, device=DEV) / h ** 0.5).to(
            torch.bfloat16)
        w_dn = (torch.randn(E, h, m, device=DEV) / m ** 0.5).to(torch.bfloat16)
        for mode in args.modes:
            weights[mode].append((convert(mode, w_gu), convert(mode, w_dn)))
        del w_gu, w_dn
    tick = {mode: 0 for mode in args.modes}

    def call(mode):
        gu, dn = weights[mode][tick[mode] % args.sets]
        tick[mode] += 1
        if mode == "bf16":
            ops.grouped_gemm(act, x, gu[0], row_tok, tile_off, counts,
                             max_tiles, True, bm=BM)
            ops.grouped_gemm(out, act, dn[0], None, tile_off, counts,
                             max_tiles, False, bm=BM)
            return
        gemm = (ops.grouped_gemm_mxfp4 if mode == "mxfp4"
                else ops.grouped_gemm_fp8)
        ops.quantize_rows_fp8(x, x_q, x_s)
        gemm(act, x_q, x_s, gu[0], gu[1], row_tok, tile_off, counts,
             max_tiles, True, bm=BM)
        ops.quantize_rows_fp8(act, a_q, a_s, row_limit=lim, limit_mul=BM)
        gemm(out, a_q, a_s, dn[0], dn[1], None, tile_off, counts, max_tiles,
             False, bm=BM)

    outs = {}
    for mode in args.modes:
        for _ in range(args.warmup):
            call(mode)
        tick[mode] = 0
        call(mode)
        tick[mode] = 0
        outs[mode] = out.float().clone()
    torch.cuda.synchronize()
    times = {mode: [] for mode in args.modes}
    for _ in range(args.windows):
        for mode in args.modes:
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.calls):
                call(mode)
            t1.record()
            t1.synchronize()
            times[mode].append(t0.elapsed_time(t1) / args.calls)
    flops = 6.0 * T * k * h * m
    wbytes = {"bf16": 2.0, "fp8_e4m3": 1.0, "mxfp4": 0.5 + 1 / 32}
    res = {"shape": name, "T": T, "BM": BM, "h": h, "m": m, "E": E, "k": k}
    live = row_tok >= 0
    for mode in args.modes:
        med = statistics.median(times[mode])
        res[mode] = {"ms": round(med, 4), "min": round(min(times[mode]), 4),
                     "max": round(max(times[mode]), 4),
                     "tflops": round(flops / med / 1e9, 1),
                     "weight_GBps": round(3 * E * h * m * wbytes[mode]
                                          / med / 1e6, 1)}
        if mode != args.modes[0]:
            a, b = outs[mode][live], outs[args.modes[0]][live]
            res[mode]["frob_vs_" + args.modes[0]] = round(
                ((a - b).norm() / b.norm()).item(), 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="+", default=list(SHAPES))
    ap.add_argument("--tokens", nargs="+", type=int, default=[8192, 64])
    ap.add_argument("--modes", nargs="+",
                    default=["bf16", "fp8_e4m3", "mxfp4"])
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    torch.manual_seed(0)
    for name in args.shape:
        for T in args.tokens:
            bench_shape(name, T, args)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
