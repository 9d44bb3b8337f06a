"""CPU model of the work assignment of attn_prefill_pipe_kernel
(csrc/attn_prefill.hip): how a tile list built at a step of R = 32, 64 or 128
rows maps blocks and waves to (sequence, rows, causal page bound), which
block-table columns a block reads (its prefetch included), and how the V^T
staging items tile a page.

`build_tiles` is the list the engine builds; `block_plan` follows the
kernel's index arithmetic for one block; `reference_tiles` is what the
32-row reference kernel does for the same rows. tests/
test_attn_prefill_pipe_sim.py checks the two against each other.
Run: python tools/sim_attn_prefill_pipe.py"""

BS = 32
QTILE = 32
VT_PAD = 40
GRANULARITIES = (32, 64, 128)


def pipe_config(G, tile_rows):
    """(waves per block, sub-tiles per wave) or None if the kernel does not
    take the configuration (sutro_attn_prefill_pipe_supported)."""
    if tile_rows not in GRANULARITIES or G > 8:
        return None   # a wave owns one head: at most 8 waves, so G <= 8
    pairs = G * (tile_rows // QTILE)
    if pairs in (1, 2, 4, 8):
        return pairs, 1
    if pairs == 16:
        return 8, 2
    return None


def build_tiles(new_counts, tile_rows):
    """(tile_seq, tile_q0) as engine._build_forward_batch builds them."""
    ts, tq = [], []
    for s, c in enumerate(new_counts):
        for j in range(0, c, tile_rows):
            ts.append(s)
            tq.append(j)
    return ts, tq


def block_plan(G, tile_rows, s, q0_blk, qlocs, seq_lens):
    """One block of the pipelined kernel. Returns None for a pad tile, else
    dict(pages=pages the block stages, bt_reads=block-table columns it reads,
    waves=[(g, [(row_base, nq, qabs_base, nt_w), ...per sub-tile])])."""
    NW, SUBS = pipe_config(G, tile_rows)
    nq_total = qlocs[s + 1] - qlocs[s]
    L = seq_lens[s]
    ctx = L - nq_total
    rows_blk = QTILE * SUBS * (NW // G)
    assert rows_blk == tile_rows
    nq_blk = min(rows_blk, nq_total - q0_blk)
    if nq_blk <= 0:
        return None
    nt_blk = (ctx + q0_blk + nq_blk + BS - 1) // BS
    # block-table columns: page 0, then one page ahead of the prefetch,
    # clamped to the block's last page
    bt_reads = [0, min(1, nt_blk - 1)]
    for kt in range(nt_blk):
        if kt + 1 < nt_blk:
            bt_reads.append(min(kt + 2, nt_blk - 1))
    waves = []
    for w in range(NW):
        g, sub = w % G, w // G
        subs = []
        for su in range(SUBS):
            q0 = q0_blk + QTILE * (sub * SUBS + su)
            nq = min(QTILE, nq_total - q0)
            qabs_base = ctx + q0
            nt_w = (qabs_base + nq + BS - 1) // BS if nq > 0 else 0
            subs.append((qlocs[s] + q0, nq, qabs_base, nt_w))
        waves.append((g, subs))
    return dict(pages=nt_blk, bt_reads=bt_reads, waves=waves)


def reference_tiles(new_counts, qlocs, seq_lens):
    """{(seq, head-in-group-independent row_base): (nq, qabs_base, pages)}
    of the 32-row reference kernel (attn_prefill_kernel)."""
    out = {}
    ts, tq = build_tiles(new_counts, QTILE)
    for s, q0 in zip(ts, tq):
        nq_total = qlocs[s + 1] - qlocs[s]
        nq = min(QTILE, nq_total - q0)
        ctx = seq_lens[s] - nq_total
        kv_end = ctx + q0 + nq
        out[(s, qlocs[s] + q0)] = (nq, ctx + q0, (kv_end + BS - 1) // BS)
    return out


def v_stage_items(D, NT):
    """(thread, kv pair, 4-column chunk) of the V^T staging for NT threads:
    item it = (NT-1-tid) + i*NT, kvp = it % 16, c4 = it // 16."""
    items = (BS // 2) * (D // 4)
    out = []
    for tid in range(NT):
        it = NT - 1 - tid
        while it < items:
            out.append((tid, it % (BS // 2), it // (BS // 2)))
            it += NT
    return out


def v_write_banks(D, NT):
    """For every 32-lane half-wave and each of an item's 4 dword writes, the
    LDS banks hit (dword index mod 32 of vt[(c4*4+j)*VT_PAD + 2*kvp])."""
    by_thread = {}
    for tid, kvp, c4 in v_stage_items(D, NT):
        by_thread.setdefault(tid, []).append((kvp, c4))
    res = []
    for h0 in range(0, NT, 32):
        lanes = [by_thread.get(t) for t in range(h0, h0 + 32)]
        n_it = max((len(x) for x in lanes if x), default=0)
        for i in range(n_it):
            for j in range(4):
                banks = []
                for x in lanes:
                    if x and i < len(x):
                        kvp, c4 = x[i]
                        banks.append((((c4 * 4 + j) * VT_PAD + 2 * kvp) // 2) % 32)
                res.append(banks)
    return res


if __name__ == "__main__":
    new_counts = [1, 33, 128, 200]
    ctxs = [0, 40, 0, 31]
    qlocs = [0]
    for c in new_counts:
        qlocs.append(qlocs[-1] + c)
    seq_lens = [c + n for c, n in zip(ctxs, new_counts)]
    for R in GRANULARITIES:
        ts, tq = build_tiles(new_counts, R)
        staged = sum(block_plan(4, R, s, q0, qlocs, seq_lens)["pages"]
                     for s, q0 in zip(ts, tq))
        print(f"tile_rows={R}: {len(ts)} blocks per kv head, "
              f"{staged} page stagings")
