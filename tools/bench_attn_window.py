"""Micro-benchmark of the MFMA decode attention kernel with and without a
sliding window, in ONE process by the method of tools/bench_attn_prefill.py:
variants alternate round by round; each round times a window of back-to-back
calls per variant between device events; round 0 warms up; median (min-max)
over the rounds is reported.

Shapes: batch 2048 decode rows at gpt-oss-20b's head layout (64 q heads, 8 kv
heads, head_dim 64), context 256 / 1024 / 4096, bf16 and e4m3 KV. Variants:

    W = 0            the default instantiation (no window, no sinks)
    W = 128          the local instantiation, window 128
    W = 128 + sinks  the same with a sink logit per head
    parent, W = 0    the same call through an extension built from the parent
                     commit (--parent-ext PATH to its _C*.so), which shows
                     what the neutral path cost; skipped without the option

Two q sets rotate call by call; the KV pages are the same on every call (at
context 4096 bf16 they are 17 GB, far past the last-level cache). The bytes
column counts q, out and the KV pages the variant has to read.

    python tools/bench_attn_window.py [--rounds 5] [--calls 10]
                                      [--parent-ext PATH] [--batch 2048]
Writes bench_outputs/attn_window_bench.txt (or under $BENCH_OUT)."""

import argparse
import importlib.machinery
import importlib.util
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from sutro_amd import ops  # noqa: E402

HQ, HK, D, BS = 64, 8, 64, 32
NSETS = 2
WINDOW = 128
CONTEXTS = (256, 1024, 4096)


def window(fn, calls):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for c in range(calls):
        fn(c % NSETS)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1000.0 / calls  # us per call


def load_parent(path):
    """The parent commit's extension under a private module name (its init
    symbol is looked up by the last component, `_C`)."""
    loader = importlib.machinery.ExtensionFileLoader("_C", path)
    spec = importlib.util.spec_from_loader("_C", loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


def inputs(batch, ctx, fp8, gen):
    # lengths spread over the last page so rows end at every offset
    lens = [ctx - (i * 7) % BS for i in range(batch)]
    pages = [(L + BS - 1) // BS for L in lens]
    nb = sum(pages)
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(1))
    bt = torch.zeros(batch, max(pages), dtype=torch.int32)
    i = 0
    for s, n in enumerate(pages):
        bt[s, :n] = perm[i:i + n].to(torch.int32)
        i += n
    shape = (nb, HK, BS, D)
    kc = torch.empty(shape, device="cuda", dtype=torch.bfloat16)
    vc = torch.empty(shape, device="cuda", dtype=torch.bfloat16)
    kc.normal_(generator=gen)
    vc.normal_(generator=gen)
    if fp8:
        kc, vc = kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)
    qs = [torch.randn(batch, HQ, D, device="cuda", generator=gen).bfloat16()
          for _ in range(NSETS)]
    ql = torch.arange(batch + 1, dtype=torch.int32, device="cuda")
    sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    es = 1 if fp8 else 2
    page_bytes = 2 * HK * BS * D * es
    qo_bytes = 2 * batch * HQ * D * 2
    full = qo_bytes + nb * page_bytes
    win_pages = sum((L + BS - 1) // BS - max(0, L - WINDOW) // BS
                    for L in lens)
    return qs, kc, vc, bt.cuda(), sl, ql, full, qo_bytes + win_pages * page_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--parent-ext", default=None,
                    help="_C*.so built from the parent commit")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    parent = load_parent(args.parent_ext) if args.parent_ext else None
    emit(f"rounds={args.rounds} calls/window={args.calls} input sets={NSETS}"
         f" device={torch.cuda.get_device_name(0)} batch={args.batch}"
         f" Hq={HQ} Hk={HK} D={D} window={WINDOW}"
         f" parent={'yes' if parent else 'no'}")
    gen = torch.Generator(device="cuda")
    scale = 1.0 / math.sqrt(D)
    sinks = torch.randn(HQ, device="cuda")
    empty = torch.empty(0, dtype=torch.int32, device="cuda")
    for fp8 in (False, True):
        for ctx in CONTEXTS:
            gen.manual_seed(ctx)
            qs, kc, vc, bt, sl, ql, b_full, b_win = inputs(
                args.batch, ctx, fp8, gen)
            n = args.batch

            def call(i, **kw):
                return ops.paged_attention(qs[i], kc, vc, bt, sl, ql, scale,
                                           num_decodes_tail=n, **kw)

            outs = [torch.empty_like(q) for q in qs]

            def call_parent(i):
                parent.paged_attention(outs[i], qs[i], kc, vc, bt, sl, ql,
                                       scale, n, empty, empty, 0)
                return outs[i]

            vs = [("W = 0", lambda i: call(i), b_full),
                  (f"W = {WINDOW}", lambda i: call(i, window=WINDOW), b_win),
                  (f"W = {WINDOW} + sinks",
                   lambda i: call(i, window=WINDOW, sinks=sinks), b_win)]
            if parent is not None:
                vs.append(("parent, W = 0", call_parent, b_full))
                assert torch.equal(call_parent(0), call(0)), "parent differs"
            # a window that covers every row is the plain call, bit for bit
            assert torch.equal(call(0, window=ctx), call(0))
            times = {name: [] for name, _, _ in vs}
            for r in range(args.rounds + 1):  # round 0 warms up
                for name, fn, _ in vs:
                    t = window(fn, args.calls if r else 2)
                    if r:
                        times[name].append(t)
            emit(f"attn_decode_mfma {'e4m3' if fp8 else 'bf16'} KV, "
                 f"context {ctx}")
            for name, _, nbytes in vs:
                ts = times[name]
                med = statistics.median(ts)
                emit(f"  {name:20s} {med:9.1f} us ({min(ts):.1f}-{max(ts):.1f})"
                     f"  {nbytes / 1e6:7.0f} MB  {nbytes / med / 1e6:6.2f} TB/s")
            del qs, kc, vc, outs
            torch.cuda.empty_cache()
    outd = os.environ.get("BENCH_OUT", "bench_outputs")
    os.makedirs(outd, exist_ok=True)
    with open(os.path.join(outd, "attn_window_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
