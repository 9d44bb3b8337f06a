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


def sim(mode, epi, x, w, lazy=False):
    """x [M, K], w [N, K] (float arrays holding bf16 values). epi 0: returns
    bf16-rounded x @ w.T [M, N]; epi 2: SwiGLU [M, N/2]."""
    M, K = x.shape
    N = w.shape[0]
    out = np.full((M, N // 2 if epi == 2 else N), np.nan, dtype=np.float32)
    MT = (M + 255) // 256
    ntl = (N // 2) // 128 if epi == 2 else (N + 255) // 256
    for bid in range(MT * ntl):
        sim_block(mode, epi, x, w, M, N, K, (bid % MT) * 256, bid // MT,
                  lazy, out)
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
        print(f"swz mode {mode}: pipelined staging/quadrant/epilogue index "
              "flow exact OK")
