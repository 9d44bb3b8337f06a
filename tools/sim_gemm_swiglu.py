"""CPU simulation of csrc/gemm_tn_pipe.hip's index flow (sibling of
sim_gemm_tn.py): the two-base B tile (gate half + matching up half, or two
consecutive halves for the plain kernel), glds source pre-swizzle into
lane-linear LDS half-tile slots, the swizzled fragment reads, the per-wave
quadrants, the lane -> (gate, up) pairing of the SwiGLU epilogue and its
output coordinates, with clamped loads / guarded stores at the M and N edges.

The 8-phase schedule is followed in program order for one block: half-tiles
are staged into the 2 x 4 slots in the kernel's order (tail tiles clamped to
the last K-tile) and land either at issue ("eager") or only at the counted
wait that retires them ("lazy"); both extremes must give the same result,
which checks the slot bookkeeping, the vmcnt count and the tail.

sim_persistent follows the persistent SwiGLU kernel the same way: one block
over its whole tile list (grouped tile order, XCD spans), with the seam
staging that prefetches the next tile through the tail slots and the staged
loads pending across the epilogue. A seam read placed before its data lands
shows up in the lazy mode as a wrong tile.

Run: python tools/sim_gemm_swiglu.py"""

import numpy as np

WAVE = 64
LANE = np.arange(WAVE)
SLOT_B0, SLOT_A0, SLOT_B1, SLOT_A1 = 0, 1, 2, 3
LOADS_IN_FLIGHT = 6  # vmcnt(6): 3 half-tiles x 2 loads per thread


def swz(mode, byte):
    if mode == 1:
        return byte ^ (((byte >> 9) & 1) << 5)
    if mode == 2:
        return byte ^ (((byte >> 8) & 7) << 4)
    return byte


def bf16_round(a):
    """float32 array -> nearest-even bf16, returned as float32 (f2bf)."""
    u = np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def make_src(mode, row0, rows_valid):
    """Per (wave, j, lane): source row and k element offset (make_src)."""
    rows = np.empty((8, 2, WAVE), dtype=np.int64)
    koff = np.empty((8, 2, WAVE), dtype=np.int64)
    for wave in range(8):
        for j in range(2):
            b = (wave * 2 + j) * 1024 + LANE * 16
            lb = swz(mode, b)
            row = np.minimum(lb >> 7, rows_valid - 1)
            rows[wave, j] = row0 + row
            koff[wave, j] = (lb & 127) // 2
    return rows, koff


def stage_half(src, mat, kt):
    """The half-tile's LDS image ([8192] elements, lane-linear)."""
    rows, koff = src
    lds = np.empty(128 * 64)
    for wave in range(8):
        for j in range(2):
            base = ((wave * 2 + j) * 1024 + LANE * 16) // 2
            for e in range(8):
                lds[base + e] = mat[rows[wave, j], kt * 64 + koff[wave, j] + e]
    return lds


def frag(mode, lds, row0, kk):
    """[64 lanes, 8] fragment: row = row0 + lane%16, chunk = kk*4 + lane/16."""
    lb = (row0 + (LANE & 15)) * 128 + (kk * 4 + (LANE >> 4)) * 16
    b = swz(mode, lb) // 2
    return lds[b[:, None] + np.arange(8)[None, :]]


def mfma16(a_lanes, b_lanes, c_lanes):
    """c_lanes [64, 4]: lane l holds D rows (l/16)*4+r, col l%16."""
    # A[l%16][(l/16)*8+j] = a[l][j];  B[(l/16)*8+j][l%16] = b[l][j]
    A = a_lanes.reshape(4, 16, 8).transpose(1, 0, 2).reshape(16, 32)
    B = b_lanes.reshape(4, 16, 8).transpose(0, 2, 1).reshape(32, 16)
    D = A @ B
    return c_lanes + D.reshape(4, 4, 16).transpose(0, 2, 1).reshape(WAVE, 4)


def sim_block(mode, epi, x, w, M, N, K, m0, nt, lazy, out):
    I = N // 2
    nb0 = nt * 128 if epi == 2 else nt * 256
    nb1 = I + nt * 128 if epi == 2 else nt * 256 + 128
    nlim = I if epi == 2 else N
    a0v = min(128, M - m0)
    a1v = max(1, min(128, M - m0 - 128))
    b0v = min(128, nlim - nb0)
    b1v = 128 if epi == 2 else max(1, min(128, N - nb1))
    a1r = m0 + 128 if M - m0 - 128 >= 1 else m0 + a0v - 1
    b1r = nb1 if (epi == 2 or N - nb1 >= 1) else nb0 + b0v - 1
    src = {SLOT_B0: (make_src(mode, nb0, b0v), w),
           SLOT_A0: (make_src(mode, m0, a0v), x),
           SLOT_B1: (make_src(mode, b1r, b1v), w),
           SLOT_A1: (make_src(mode, a1r, a1v), x)}
    KT = K // 64
    klast = KT - 1
    lds = {}       # (P, slot) -> image
    pending = []   # issued, not landed: ((P, slot), image), 2 loads each

    def stage(P, slot, kt):
        s, mat = src[slot]
        img = stage_half(s, mat, kt)
        if lazy:
            pending.append(((P, slot), img))
        else:
            lds[(P, slot)] = img

    def wait_vmcnt(n):
        while 2 * len(pending) > n:
            key, img = pending.pop(0)
            lds[key] = img

    for slot in (SLOT_B0, SLOT_A0, SLOT_B1, SLOT_A1):
        stage(0, slot, 0)
    for slot in (SLOT_B0, SLOT_A0, SLOT_B1):
        stage(1, slot, min(1, klast))
    wait_vmcnt(LOADS_IN_FLIGHT)

    # acc[wave][a][b][i][j] -> [64, 4]
    acc = np.zeros((8, 2, 2, 4, 2, WAVE, 4))

    def mma(P, a, b):
        A = lds[(P, SLOT_A0 if a == 0 else SLOT_A1)]
        B = lds[(P, SLOT_B0 if b == 0 else SLOT_B1)]
        for wave in range(8):
            wm, wn = wave >> 2, wave & 3
            for kk in range(2):
                for i in range(4):
                    af = frag(mode, A, wm * 64 + i * 16, kk)
                    for j in range(2):
                        bf = frag(mode, B, wn * 32 + j * 16, kk)
                        acc[wave, a, b, i, j] = mfma16(af, bf,
                                                       acc[wave, a, b, i, j])

    for t in range(KT):
        P = t & 1
        kn1, kn2 = min(t + 1, klast), min(t + 2, klast)
        # the reads of a phase come before its staging; in the lazy model the
        # image read is whatever landed by the last counted wait
        a0, b0 = lds[(P, SLOT_A0)].copy(), lds[(P, SLOT_B0)].copy()
        stage(P ^ 1, SLOT_A1, kn1)                       # ph0
        b1 = lds[(P, SLOT_B1)].copy()
        stage(P, SLOT_B0, kn2)                           # ph1
        a1 = lds[(P, SLOT_A1)].copy()
        stage(P, SLOT_A0, kn2)                           # ph2
        stage(P, SLOT_B1, kn2)                           # ph3
        wait_vmcnt(LOADS_IN_FLIGHT)
        saved = dict(lds)
        lds.update({(P, SLOT_A0): a0, (P, SLOT_B0): b0, (P, SLOT_B1): b1,
                    (P, SLOT_A1): a1})
        for a in range(2):
            for b in range(2):
                mma(P, a, b)
        lds.clear()
        lds.update(saved)

    # epilogue
    drow = (LANE >> 4) * 4
    dcol = LANE & 15
    for wave in range(8):
        wm, wn = wave >> 2, wave & 3
        for a in range(2):
            for i in range(4):
                for j in range(2):
                    gm = m0 + a * 128 + wm * 64 + i * 16 + drow
                    for r in range(4):
                        ok = gm + r < M
                        if epi == 2:
                            gn = nb0 + wn * 32 + j * 16 + dcol
                            g = bf16_round(acc[wave, a, 0, i, j][:, r])
                            u = bf16_round(acc[wave, a, 1, i, j][:, r])
                            s = g / (np.float32(1) + np.exp(-g))
                            v = bf16_round(s * u)
                            out[(gm + r)[ok], gn[ok]] = v[ok]
                        else:
                            for b in range(2):
                                gn = nb0 + b * 128 + wn * 32 + j * 16 + dcol
                                k2 = ok & (gn < N)
                                out[(gm + r)[k2], gn[k2]] = bf16_round(
                                    acc[wave, a, b, i, j][:, r])[k2]


def sim(mode, epi, x, w, lazy=False, group_m=0):
    """x [M, K], w [N, K] (float arrays holding bf16 values). epi 0: returns
    bf16-rounded x @ w.T [M, N]; epi 2: SwiGLU [M, N/2]. group_m: the
    launch's tile order (tile_mn; < 0: tile_mn_banded)."""
    M, K = x.shape
    N = w.shape[0]
    out = np.full((M, N // 2 if epi == 2 else N), np.nan, dtype=np.float32)
    MT = (M + 255) // 256
    ntl = (N // 2) // 128 if epi == 2 else (N + 255) // 256
    for bid in range(MT * ntl):
        # (the XCD remap is a bijection of the block ids; only the banded
        # order depends on it)
        mt, nt = one_tile_coords(bid, MT * ntl, MT, ntl, group_m,
                                 1 if group_m < 0 else 0)
        sim_block(mode, epi, x, w, M, N, K, mt * 256, nt, lazy, out)
    return out


def tile_mn(tile, MT, NT, group_m):
    """Tile number -> (M-tile, N-tile): groups of group_m M-tiles, m fastest
    inside a group, then n; the last group takes the remainder. group_m <= 0
    or >= MT is the plain order (the kernel's tile_mn)."""
    if group_m <= 0 or group_m >= MT:
        return tile % MT, tile // MT
    per = group_m * NT
    g = tile // per
    first = g * group_m
    gsz = min(group_m, MT - first)
    local = tile - g * per
    return first + local % gsz, local // gsz


def tile_mn_banded(xl, i, nx, MT, NT, group_m):
    """The banded order (group_m < 0): label xl of nx owns MT // nx whole rows
    of M-tiles, walked in groups of -group_m, then its even share of the
    MT % nx leftover rows, m fastest (the kernel's tile_mn_banded)."""
    a = MT // nx
    b = MT - a * nx
    whole = a * NT
    if i < whole:
        mt, nt = tile_mn(i, a, NT, -group_m)
        return a * xl + mt, nt
    q, r = divmod(b * NT, nx)
    idx = (xl * (q + 1) if xl < r else r * (q + 1) + (xl - r) * q) + i - whole
    return nx * a + idx % b, idx // b


def block_coords(bid, num_blocks, MT, NT, group_m=0, xcd_swz=1):
    """(M-tile, N-tile) of every tile the persistent kernel's block `bid`
    walks, in order."""
    nx = min(8, num_blocks) if xcd_swz else 1
    xl, slot = bid % nx, bid // nx
    slots = (num_blocks - xl + nx - 1) // nx
    out = []
    for t in block_tiles(bid, num_blocks, MT * NT, xcd_swz):
        if group_m < 0:
            span0 = t - slot - len(out) * slots
            out.append(tile_mn_banded(xl, t - span0, nx, MT, NT, group_m))
        else:
            out.append(tile_mn(t, MT, NT, group_m))
    return out


def one_tile_coords(bid, tiles, MT, NT, group_m=0, xcd_swz=1):
    """(M-tile, N-tile) of block `bid` of the one-tile-per-block kernel."""
    if group_m < 0:
        assert xcd_swz, "the banded order needs the XCD remap"
        return tile_mn_banded(bid & 7, bid >> 3, 8, MT, NT, group_m)
    if xcd_swz:
        q, r = divmod(tiles, 8)
        xcd, seq = bid & 7, bid >> 3
        bid = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + seq
    return tile_mn(bid, MT, NT, group_m)


def block_tiles(bid, num_blocks, tiles, xcd_swz=1):
    """Tile numbers the persistent kernel's block `bid` walks, in order: XCD
    label xl owns one contiguous balanced span, its slots stride through it."""
    nx = min(8, num_blocks) if xcd_swz else 1
    xl, slot = bid % nx, bid // nx
    slots = (num_blocks - xl + nx - 1) // nx
    q, r = divmod(tiles, nx)
    span0 = xl * (q + 1) if xl < r else r * (q + 1) + (xl - r) * q
    span_n = q + (1 if xl < r else 0)
    return [span0 + i for i in range(slot, span_n, slots)]


def _swiglu_src(mode, x, w, M, I, m0, nb0):
    a0v = min(128, M - m0)
    a1v = max(1, min(128, M - m0 - 128))
    a1r = m0 + 128 if M - m0 - 128 >= 1 else m0 + a0v - 1
    return {SLOT_B0: (make_src(mode, nb0, 128), w),
            SLOT_A0: (make_src(mode, m0, a0v), x),
            SLOT_B1: (make_src(mode, I + nb0, 128), w),
            SLOT_A1: (make_src(mode, a1r, a1v), x)}


def sim_persistent_block(mode, x, w, M, N, K, coords, lazy, out):
    """One block of gemm_swiglu_persist_kernel over its tiles `coords`
    [(m0, nb0), ...] in program order. The prologue runs once; in a tile's
    last two K-tiles the tail slots stage the NEXT tile's K-tile 0 (all four
    halves) and K-tile 1's B0, A0, B1 (the block's last tile stages itself
    from its last K-tile and drains); the epilogue follows the tile's last
    counted wait with the next tile's loads pending across it."""
    I = N // 2
    KT = K // 64
    assert KT >= 2 and KT % 2 == 0, "persistent variant needs K % 128 == 0"
    klast = KT - 1
    if not coords:
        return
    lds = {}
    pending = []

    def stage(P, slot, src, kt):
        s, mat = src[slot]
        img = stage_half(s, mat, kt)
        if lazy:
            pending.append(((P, slot), img))
        else:
            lds[(P, slot)] = img

    def wait_vmcnt(n):
        while 2 * len(pending) > n:
            key, img = pending.pop(0)
            lds[key] = img

    cur = _swiglu_src(mode, x, w, M, I, *coords[0])
    for slot in (SLOT_B0, SLOT_A0, SLOT_B1, SLOT_A1):
        stage(0, slot, cur, 0)
    for slot in (SLOT_B0, SLOT_A0, SLOT_B1):
        stage(1, slot, cur, 1)
    wait_vmcnt(LOADS_IN_FLIGHT)

    drow = (LANE >> 4) * 4
    dcol = LANE & 15
    for it, (m0, nb0) in enumerate(coords):
        more = it + 1 < len(coords)
        nxt = _swiglu_src(mode, x, w, M, I, *coords[it + 1]) if more else cur
        kz0, kz1 = (0, 1) if more else (klast, klast)
        acc = np.zeros((8, 2, 2, 4, 2, WAVE, 4))
        for t in range(KT):
            P = t & 1
            if t < KT - 2:      # the steady loop
                plan = [(cur, t + 1)] + [(cur, t + 2)] * 3
            elif t == KT - 2:   # seam, first half
                plan = [(cur, klast)] + [(nxt, kz0)] * 3
            else:               # seam, second half
                plan = [(nxt, kz0)] + [(nxt, kz1)] * 3
            a0, b0 = lds[(P, SLOT_A0)].copy(), lds[(P, SLOT_B0)].copy()
            stage(P ^ 1, SLOT_A1, *plan[0])                  # ph0
            b1 = lds[(P, SLOT_B1)].copy()
            stage(P, SLOT_B0, *plan[1])                      # ph1
            a1 = lds[(P, SLOT_A1)].copy()
            stage(P, SLOT_A0, *plan[2])                      # ph2
            stage(P, SLOT_B1, *plan[3])                      # ph3
            wait_vmcnt(LOADS_IN_FLIGHT)
            tile = {SLOT_A0: a0, SLOT_B0: b0, SLOT_B1: b1, SLOT_A1: a1}
            for wave in range(8):
                wm, wn = wave >> 2, wave & 3
                for a, sa in ((0, SLOT_A0), (1, SLOT_A1)):
                    for b, sb in ((0, SLOT_B0), (1, SLOT_B1)):
                        for kk in range(2):
                            for i in range(4):
                                af = frag(mode, tile[sa], wm * 64 + i * 16, kk)
                                for j in range(2):
                                    bf = frag(mode, tile[sb],
                                              wn * 32 + j * 16, kk)
                                    acc[wave, a, b, i, j] = mfma16(
                                        af, bf, acc[wave, a, b, i, j])
        if not more:
            wait_vmcnt(0)
        for wave in range(8):
            wm, wn = wave >> 2, wave & 3
            for a in range(2):
                for i in range(4):
                    for j in range(2):
                        gm = m0 + a * 128 + wm * 64 + i * 16 + drow
                        gn = nb0 + wn * 32 + j * 16 + dcol
                        for r in range(4):
                            ok = gm + r < M
                            g = bf16_round(acc[wave, a, 0, i, j][:, r])
                            u = bf16_round(acc[wave, a, 1, i, j][:, r])
                            s = g / (np.float32(1) + np.exp(-g))
                            v = bf16_round(s * u)
                            assert np.isnan(out[(gm + r)[ok], gn[ok]]).all(), \
                                "an output element was stored twice"
                            out[(gm + r)[ok], gn[ok]] = v[ok]
        cur = nxt


def sim_persistent(mode, x, w, num_blocks, group_m=0, lazy=False, xcd_swz=1):
    """SwiGLU [M, N/2] as gemm_swiglu_persist_kernel computes it on a grid of
    num_blocks blocks in the grouped tile order."""
    M, K = x.shape
    N = w.shape[0]
    out = np.full((M, N // 2), np.nan, dtype=np.float32)
    MT = (M + 255) // 256
    NT = (N // 2) // 128
    for bid in range(num_blocks):
        coords = [(mt * 256, nt * 128) for mt, nt in
                  block_coords(bid, num_blocks, MT, NT, group_m, xcd_swz)]
        sim_persistent_block(mode, x, w, M, N, K, coords, lazy, out)
    return out


def reference(epi, x, w):
    y = bf16_round((x.astype(np.float64) @ w.astype(np.float64).T))
    if epi != 2:
        return y
    I = w.shape[0] // 2
    g, u = y[:, :I], y[:, I:]
    return bf16_round(g / (np.float32(1) + np.exp(-g)) * u)


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    for mode in (0, 1, 2):
        for epi, M, N, K in [(2, 130, 256, 128), (0, 300, 300, 192)]:
            x = bf16_round(rng.standard_normal((M, K)))
            w = bf16_round(rng.standard_normal((N, K)) / np.sqrt(K))
            ref = reference(epi, x, w)
            for lazy in (False, True):
                got = sim(mode, epi, x, w, lazy)
                assert np.array_equal(got, ref), (mode, epi, lazy)
        x = bf16_round(rng.standard_normal((300, 256)))
        w = bf16_round(rng.standard_normal((768, 256)) / 16)
        ref = reference(2, x, w)
        for lazy in (False, True):
            got = sim_persistent(mode, x, w, 2, 1, lazy)
            assert np.array_equal(got, ref), (mode, "persistent", lazy)
        print(f"swz mode {mode}: pipelined staging/quadrant/epilogue index "
              "flow exact OK (one-tile and persistent)")
