"""CPU simulation of the index flow of csrc/grouped_gemm_mxfp4.hip: the
global_load_lds staging (wave-uniform LDS base + lane * 16, per-lane
pre-swizzled global source; W pieces dealt round-robin to the waves, gate/up
streams contiguous in LDS) against the read-side swizzles of gx_frag_a /
gx_frag_w, and the lane map against the block structure of
mfma_scale_f32_16x16x128_f8f6f4 as found on the hardware.

Hardware model (16x16x128, found with exact data, see the kernel header):
the low four operand dwords of the four k-groups hold the first 64 k-bytes'
worth of the tile, the high four the second. An 8-bit operand (A) therefore
has element j of k-group q at k = 64(j >> 4) + 16q + (j & 15); a 4-bit
operand (B) has only the low four dwords, which span all 128 k:
k = 32q + j. The scale byte of the lanes of k-group g scales k = 32g..32g+31.

Proves, for the three tile configurations and both stage kinds:
  1. W staging is a bijection: every 16-byte chunk of every (stream, row) of
     the tile lands in exactly one LDS slot, every slot is written once;
  2. a W fragment read (row, k-group q) returns the 16 bytes of
     k = 32q .. 32q+31 of that row — the MX block whose scale byte lane
     (row, q) loads; an A fragment read returns k = 16q .. 16q+15 and
     64+16q .. 64+16q+15 of its 128-byte row: both operands put the k the
     hardware expects into every element;
  3. the LDS reads of the main loop are bank-conflict free. Banks are 64 x 4
     bytes, bank = (addr / 4) % 64; ds_read_b128 serves the lane groups
     {0-3,12-15,20-27}, {4-11,16-19,28-31}, {32-35,44-47,52-59},
     {36-43,48-51,60-63} one LDS cycle each, so the 16 lanes of a group must
     hit 16 distinct 16-byte bank groups;
  4. the row-bit XOR of the 128-byte-row kernels (qswz) fails 3 on the
     64-byte W rows, which is why the W swizzle was re-derived.
Run: python tools/sim_grouped_gemm_mxfp4.py"""

WAVE = 64

B128_GROUPS = [
    list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
    list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
    list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64)),
]


def wswz(byte):
    return byte ^ (((0x78 >> (((byte >> 8) & 3) << 1)) & 3) << 4)


def aswz(byte):
    return byte ^ (((byte >> 8) & 7) << 4)


def hw_k8(q, j):
    """k of element j of k-group q, 8-bit operand (hardware model)."""
    return 64 * (j >> 4) + 16 * q + (j & 15)


def hw_k4(q, j):
    """k of element j of k-group q, 4-bit operand (hardware model)."""
    return 32 * q + j


def conflicts(addrs, width, groups):
    n = 0
    for g in groups:
        banks = [(addrs[l] + o) // 4 % 64 for l in g for o in range(0, width, 4)]
        n += len(banks) - len(set(banks))
    return n


def stage_w(swz, BN, NB, WAVES, n_cols):
    """LDS image as {lds_byte_of_chunk: (global_row, byte_in_row)}."""
    pieces = NB * BN // 16
    ch = (pieces + WAVES - 1) // WAVES
    lds = {}
    for wave in range(WAVES):
        for j in range(ch):
            c = j * WAVES + wave
            if c >= pieces:
                break
            for lane in range(WAVE):
                b = c * 1024 + lane * 16
                lb = swz(b)
                row = lb >> 6
                grow = row if row < BN else n_cols + row - BN
                assert b not in lds
                lds[b] = (grow, lb & 63)
    return lds


def check_w(swz, BN, WR, WC, NB, n_cols):
    WAVES = WR * WC
    WN = BN // WC
    NF = WN // 16
    lds = stage_w(swz, BN, NB, WAVES, n_cols)
    # 1. bijection onto the tile's chunks and onto the LDS slots
    want = {(r if s == 0 else n_cols + r, c * 16)
            for s in range(NB) for r in range(BN) for c in range(4)}
    assert set(lds.values()) == want and len(lds) == len(want)
    assert set(lds) == {i * 16 for i in range(NB * BN * 4)}
    bad = 0
    for s in range(NB):
        for wn in range(WC):
            for j in range(NF):
                addr = []
                for l in range(WAVE):
                    row = wn * WN + j * 16 + (l & 15)
                    q = l >> 4
                    a = s * BN * 64 + swz(row * 64 + q * 16)
                    # 2. the 16 bytes are codes hw_k4(q, 0..31) of the row
                    grow, byte = lds[a]
                    assert grow == (row if s == 0 else n_cols + row)
                    assert [2 * byte + e for e in range(32)] == [
                        hw_k4(q, e) for e in range(32)], (row, q)
                    addr.append(a)
                bad += conflicts(addr, 16, B128_GROUPS)       # 3.
    return bad


def check_a(BM, WR):
    """A tile: 128-byte rows, lane-linear staging with aswz (the fp8
    kernel's), reads of chunks q and 4 + q."""
    lds = {}
    for b in range(0, BM * 128, 16):
        lb = aswz(b)
        lds[b] = (lb >> 7, lb & 127)
    assert len(set(lds.values())) == BM * 8
    WM = BM // WR
    bad = 0
    for wm in range(WR):
        for i in range(WM // 16):
            for half in range(2):
                addr = []
                for l in range(WAVE):
                    row = wm * WM + i * 16 + (l & 15)
                    q = l >> 4
                    a = aswz(row * 128 + q * 16 + half * 64)
                    assert lds[a] == (row, hw_k8(q, 16 * half))
                    addr.append(a)
                bad += conflicts(addr, 16, B128_GROUPS)
    return bad


def check_blocks():
    """Both maps cover the K-tile once, and the scale block of an A element
    is the k-group of the B lane that holds the same k."""
    assert sorted(hw_k8(q, j) for q in range(4) for j in range(32)) == \
        list(range(128))
    assert sorted(hw_k4(q, j) for q in range(4) for j in range(32)) == \
        list(range(128))
    for q in range(4):
        for j in range(32):
            assert hw_k4(hw_k8(q, j) >> 5, hw_k8(q, j) & 31) == hw_k8(q, j)


CONFIGS = [(64, 64, 2, 2), (128, 64, 4, 2), (128, 128, 2, 4)]

if __name__ == "__main__":
    check_blocks()
    print("A map k = 64(j>>4) + 16q + (j&15), B map k = 32q + j: each covers "
          "the K-tile once OK")
    for BM, BN, WR, WC in CONFIGS:
        for NB in (1, 2):
            n_cols = 3 * BN
            assert check_w(wswz, BN, WR, WC, NB, n_cols) == 0
            assert check_w(aswz, BN, WR, WC, NB, n_cols) > 0
        assert check_a(BM, WR) == 0
        print(f"{BM}x{BN} ({WR * WC} waves): W staging bijective, fragment "
              "reads exact, ds_read_b128 of W and A "
              "conflict-free OK")
    print("qswz on 64-byte rows: conflicts, as expected")
