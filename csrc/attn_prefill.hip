// Varlen causal prefill attention over the paged KV cache, flash-style,
// on MFMA matrix cores (mfma_f32_32x32x16_bf16). head_dim 128, page size 32.
//
// Geometry: one workgroup per (q_tile of 32 tokens, kv_head); G = Hq/Hk waves
// per workgroup, one q-head per wave (the whole GQA group shares each staged
// K/V page). Swapped QK^T (scores = mfma(A=K, B=Q)) puts each q row's scores
// in a lane pair; online softmax is lane-local + one shfl_xor(32).
// PV = mfma(A=P, B=V^T) with V transposed into LDS at stage time (row pad 40
// elems keeps ds_read_b128 16B-aligned and bank-conflict-free; see guide §6
// Guideline 4) and P round-tripped through LDS to reach its A-fragment layout.
//
// Fragment layout (gfx950 v_mfma_f32_32x32x16_bf16, verified by the probe
// kernel below on hardware):
//   A[32,16]: lane l holds A[l%32][(l/32)*8 + j], j=0..7
//   B[16,32]: lane l holds B[(l/32)*8 + j][l%32]
//   C/D     : lane l holds D[(r&3) + 8*(r>>2) + 4*(l/32)][l%32], r=0..15
#include "common.h"

#define BS 32
#define QTILE 32
#define VT_PAD 40  // padded row length (elems) of the transposed V tile

typedef s16x8 bf16frag;

__device__ __forceinline__ f32x16 mfma32(bf16frag a, bf16frag b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ int d_row(int r, int hi) {
  return (r & 3) + 8 * (r >> 2) + 4 * hi;
}

// K tile XOR swizzle: a row-major [32][D] bf16 tile puts a whole 16-lane
// ds_read_b128 group on few 16B slots. byte ^= (row&mask)<<4, mask chosen so
// the swizzle stays inside the row (D=128: 15, D=64: 7).
template <int D>
__device__ __forceinline__ int k_swz(int row, int byte_in_row) {
  constexpr int mask = (D == 128) ? 15 : 7;
  return row * (2 * D) + (byte_in_row ^ ((row & mask) << 4));
}

template <int D>
struct PrefillSmem {
  u16 ktile[BS * D];        // swizzled K page
  u16 vt[D * VT_PAD];       // V^T, padded rows
  // per-wave regions follow (P tile + softmax broadcast), carved at runtime
};

#define PWAVE_ELEMS (QTILE * VT_PAD)  // P tile per wave (bf16)

// LOCAL (local attention): `window` W > 0 lets the query at position i see
// keys i - W < j <= i, so the page loop starts at the page holding row 0's
// window start; `sinks` (f32 [Hq], or null) seeds each row's softmax state
// with m = sinks[head], l = 1. Rows further down the tile start later than
// row 0, so a walked page can be fully masked for them while their state is
// still m = -1e30: a masked score's weight is set to 0, not computed as
// exp(-1e30 - m). Without the flag the kernel is the one it was before.
template <int D, bool KV8, bool LOCAL = false>
__global__ void attn_prefill_kernel(
    u16* __restrict__ out,            // [T, Hq, D]
    const u16* __restrict__ q,        // [T, Hq, D]
    const u8* __restrict__ k_cache,   // [nb, Hk, BS, D] bf16 or e4m3
    const u8* __restrict__ v_cache,
    const int* __restrict__ block_tables,  // [S, bt_stride]
    const int* __restrict__ seq_lens,      // [S]
    const int* __restrict__ qlocs,         // [S+1]
    const int* __restrict__ tile_seq,      // [n_tiles]
    const int* __restrict__ tile_q0,       // [n_tiles]
    int bt_stride, int Hq, int Hk, float scale,
    int window = 0,                        // (LOCAL)
    const float* __restrict__ sinks = nullptr) {  // [Hq] (LOCAL)
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = threadIdx.x / WAVE;      // wave id == q-head within group
  const int G = blockDim.x / WAVE;
  const int tile = blockIdx.x;
  const int kh = blockIdx.y;
  const int hq = kh * G + w;

  const int s = tile_seq[tile];
  const int q0 = tile_q0[tile];          // local row offset within new tokens
  const int row_base = qlocs[s] + q0;    // flat q row
  const int nq_total = qlocs[s + 1] - qlocs[s];
  const int nq = min(QTILE, nq_total - q0);
  const int L = seq_lens[s];
  const int ctx = L - nq_total;          // tokens already cached before chunk
  const int qabs_base = ctx + q0;        // absolute pos of tile row 0
  const int kv_end = qabs_base + nq;     // causal bound (exclusive)
  const int ntiles_kv = (kv_end + BS - 1) / BS;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  PrefillSmem<D>* sm = (PrefillSmem<D>*)smem_raw;
  u16* p_lds = (u16*)(smem_raw + sizeof(PrefillSmem<D>)) + (long)w * PWAVE_ELEMS;
  float* stat_lds = (float*)((u16*)(smem_raw + sizeof(PrefillSmem<D>)) +
                             (long)G * PWAVE_ELEMS) + w * 2 * QTILE;
  float* alpha_lds = stat_lds;           // [32]
  float* lsum_lds = stat_lds + QTILE;    // [32]

  const int my_q = lane & 31;            // q row this lane's scores belong to
  const int hi = lane >> 5;

  // ---- Q fragments (B-operand), loaded once: D/16 k-steps x 8 bf16
  bf16frag qb[D / 16];
  {
    const int qrow = row_base + (my_q < nq ? my_q : 0);
    const u16* qptr = q + ((long)qrow * Hq + hq) * D + hi * 8;
#pragma unroll
    for (int kk = 0; kk < D / 16; ++kk)
      qb[kk] = *(const s16x8*)(qptr + kk * 16);
  }

  f32x16 acc_o[D / 32];  // PV accumulator, d-blocks of 32
#pragma unroll
  for (int b = 0; b < D / 32; ++b) acc_o[b] = (f32x16)(0.f);
  float m_run = -1e30f, l_run = 0.f;
  int kt0 = 0;
  if constexpr (LOCAL) {
    if (window > 0) kt0 = max(0, qabs_base - window + 1) / BS;
    if (sinks != nullptr) {
      m_run = sinks[hq];
      l_run = 1.f;
    }
  }

  for (int kt = kt0; kt < ntiles_kv; ++kt) {
    const int blk = block_tables[(long)s * bt_stride + kt];
    const long kv_base = (((long)blk * Hk + kh) * BS) * D;  // in elements
    const int kv0 = kt * BS;
    constexpr int SLOTS = D / 8;   // 8-element chunks per row
    constexpr int ES = KV8 ? 1 : 2;

    // ---- cooperative stage: K (swizzled) and V^T into LDS, as bf16
    // (fp8 caches are dequantized here so the MFMA path is unchanged)
    {
      const int tid = threadIdx.x, nthr = blockDim.x;
      // K: 32 rows; thread moves one 8-element chunk: item = row*SLOTS + slot
      for (int it = tid; it < BS * SLOTS; it += nthr) {
        const int row = it / SLOTS, slot = it % SLOTS;
        const u8* src = k_cache + ((long)kv_base + row * D + slot * 8) * ES;
        u16x8 kx;
        if constexpr (KV8) {
          const u32x2 raw = *(const u32x2*)src;
          float f[8];
          fp8x4_to_f32(raw[0], f);
          fp8x4_to_f32(raw[1], f + 4);
#pragma unroll
          for (int j = 0; j < 8; ++j) kx[j] = f2bf(f[j]);
        } else {
          kx = *(const u16x8*)src;
        }
        *(u16x8*)((char*)sm->ktile + k_swz<D>(row, slot * 16)) = kx;
      }
      // V^T: read V[kv][d0..d0+8), write 8 u16 at vt[d][kv].
      // kv-major across consecutive threads: the 2B scatter writes of a
      // 16-lane group then span 16 banks instead of hitting one (d-stride
      // 8*PV pad rows is 0 mod 32 banks).
      for (int it = tid; it < BS * SLOTS; it += nthr) {
        const int kv = it % BS, d0 = (it / BS) * 8;
        const u8* src = v_cache + ((long)kv_base + kv * D + d0) * ES;
        u16x8 vx;
        if constexpr (KV8) {
          const u32x2 raw = *(const u32x2*)src;
          float f[8];
          fp8x4_to_f32(raw[0], f);
          fp8x4_to_f32(raw[1], f + 4);
#pragma unroll
          for (int j = 0; j < 8; ++j) vx[j] = f2bf(f[j]);
        } else {
          vx = *(const u16x8*)src;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) sm->vt[(d0 + j) * VT_PAD + kv] = vx[j];
      }
    }
    __syncthreads();

    // ---- QK^T: D1[kv][q] = sum_k K[kv][k] * Q^T[k][q]
    f32x16 d1 = (f32x16)(0.f);
#pragma unroll
    for (int kk = 0; kk < D / 16; ++kk) {
      // A = K frag: lane holds K[l%32][kk*16 + hi*8 + j]
      const int row = lane & 31;
      const int byte_in_row = (kk * 16 + hi * 8) * 2;
      bf16frag ka = *(const s16x8*)((char*)sm->ktile + k_swz<D>(row, byte_in_row));
      d1 = mfma32(ka, qb[kk], d1);
    }

    // ---- online softmax (lane owns q = my_q; rows d_row(r,hi) of this tile)
    float sc[16];
    float tmax = -1e30f;
    const int qabs = qabs_base + my_q;
    // first visible key of this row (LOCAL)
    const int klo = (LOCAL && window > 0) ? qabs - window + 1 : 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kvpos = kv0 + d_row(r, hi);
      float v = d1[r] * scale;
      if (kvpos > qabs || kvpos >= L) v = -1e30f;
      if constexpr (LOCAL)
        if (kvpos < klo) v = -1e30f;
      sc[r] = v;
      tmax = fmaxf(tmax, v);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m_run, tmax);
    const float alpha = __expf(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float p = __expf(sc[r] - m_new);
      if constexpr (LOCAL) {
        // a masked key weighs exactly 0 even where the whole page is masked
        // and m_new is still -1e30 (exp(0) = 1 otherwise)
        const int kvpos = kv0 + d_row(r, hi);
        if (kvpos > qabs || kvpos >= L || kvpos < klo) p = 0.f;
      }
      sc[r] = p;
      psum += p;
    }
    psum += __shfl_xor(psum, 32, 64);
    l_run = l_run * alpha + psum;
    m_run = m_new;

    // write P (bf16) to LDS in [q][kv] layout for the PV A-fragment reads
#pragma unroll
    for (int r = 0; r < 16; ++r)
      p_lds[my_q * VT_PAD + d_row(r, hi)] = f2bf(sc[r]);
    if (hi == 0) alpha_lds[my_q] = alpha;

    // ---- rescale O accumulator: alpha indexed by the D-layout q rows
    float al[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) al[r] = alpha_lds[d_row(r, hi)];
#pragma unroll
    for (int b = 0; b < D / 32; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc_o[b][r] *= al[r];

    // ---- PV: D2[q][d] += P[q][kv] * V^T-read B[kv][d]
    bf16frag pa[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
      pa[kk] = *(const s16x8*)(p_lds + (lane & 31) * VT_PAD + kk * 16 + hi * 8);
#pragma unroll
    for (int b = 0; b < D / 32; ++b) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        // B = V^T frag: lane holds V[kk*16 + hi*8 + j][b*32 + l%32]
        bf16frag vb = *(const s16x8*)(sm->vt + (b * 32 + (lane & 31)) * VT_PAD +
                                      kk * 16 + hi * 8);
        acc_o[b] = mfma32(pa[kk], vb, acc_o[b]);
      }
    }
    __syncthreads();  // before next tile overwrites K/V LDS
  }

  // ---- epilogue: divide by l, scatter to out
  if (hi == 0) lsum_lds[my_q] = l_run;
  // LDS write then read within the same wave; other waves own other regions
  float inv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float l = lsum_lds[d_row(r, hi)];
    inv[r] = l > 0.f ? 1.0f / l : 0.f;
  }
  const int d_col = lane & 31;
#pragma unroll
  for (int b = 0; b < D / 32; ++b) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qrow = d_row(r, hi);
      if (qrow < nq) {
        out[((long)(row_base + qrow) * Hq + hq) * D + b * 32 + d_col] =
            f2bf(acc_o[b][r] * inv[r]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Pipelined variant. Same arithmetic per (q row, head) as attn_prefill_kernel
// above (same pages in the same order, same MFMA chain, same softmax update,
// same roundings), so the two return identical bits; what differs is how the
// pages reach LDS and how the result leaves:
//  - a workgroup covers QG = NW/G consecutive 32-row sub-tiles of one
//    sequence (tile_q0 steps by 32*QG); wave w is (head w%G, sub-tile w/G).
//    Every staged page is shared by all of them. A wave stops computing after
//    its own causal bound but keeps joining the barriers.
//  - K/V LDS tiles are double-buffered: page t+1 is loaded into registers
//    before page t's MFMA/softmax work and written to the other buffer after
//    it, one barrier per page. The block-table entry is read one page further
//    ahead, clamped to the block's last page (later columns are undefined).
//  - V^T is built from (kv, kv+1) row pairs, 4-byte LDS writes: lanes of a
//    half-wave are 16 kv pairs x 2 four-column chunks, whose rows sit 16 banks
//    apart (4 rows * 20 dwords), so the 32 writes hit 32 banks.
//  - the output tile goes through the wave's P region, 32 columns at a time,
//    and is stored 16 bytes per lane.
// NW (waves per workgroup) is a template parameter so the per-thread staging
// registers are indexed statically.
// ---------------------------------------------------------------------------

// Q fragments (16 bytes per lane each) the pipelined kernel parks in LDS per
// wave instead of holding them in registers; see Q_LDS in the kernel.
constexpr bool pipe_q_in_lds(int d, int subs) { return d == 128 && subs == 2; }
constexpr int PIPE_Q_KEEP = 5;  // first sub-tile's fragments kept in registers
constexpr int pipe_q_lds_frags(int d, int subs) {
  return pipe_q_in_lds(d, subs) ? d / 16 + (d / 16 - PIPE_Q_KEEP) : 0;
}

template <int D, bool KV8, int NW, int SUBS>
__global__ __launch_bounds__(NW * 64) void attn_prefill_pipe_kernel(
    u16* __restrict__ out, const u16* __restrict__ q,
    const u8* __restrict__ k_cache, const u8* __restrict__ v_cache,
    const int* __restrict__ block_tables, const int* __restrict__ seq_lens,
    const int* __restrict__ qlocs, const int* __restrict__ tile_seq,
    const int* __restrict__ tile_q0, int bt_stride, int Hq, int Hk, int G,
    float scale) {
  constexpr int NT = NW * 64;
  constexpr int SLOTS = D / 8;               // 8-element chunks per K row
  constexpr int ES = KV8 ? 1 : 2;
  constexpr int KITEMS = BS * SLOTS;         // (row, 8-elem chunk)
  constexpr int VITEMS = (BS / 2) * (D / 4); // (kv pair, 4-elem chunk)
  constexpr int KI = (KITEMS + NT - 1) / NT;
  constexpr int VI = (VITEMS + NT - 1) / NT;
  constexpr int KW = KV8 ? 2 : 4;            // dwords per K item
  constexpr int VW = KV8 ? 1 : 2;            // dwords per V item row
  typedef u32 kraw_t __attribute__((ext_vector_type(KW)));
  typedef u32 vraw_t __attribute__((ext_vector_type(VW)));
  // head_dim 128 with two sub-tiles per wave: two Q tiles next to two
  // accumulators do not fit 256 registers, so the last sub-tile's Q fragments
  // and the first one's beyond PIPE_Q_KEEP are parked in LDS, lane-linear (a
  // lane reads back its own 16 bytes), and re-read for every page
  constexpr bool Q_LDS = pipe_q_in_lds(D, SUBS);
  constexpr int Q_FRAGS = pipe_q_lds_frags(D, SUBS);
  // LDS slot of fragment (su, kk), or -1 if it stays in qb[su][kk]
  auto q_slot = [](int su, int kk) {
    if (!Q_LDS) return -1;
    if (su == SUBS - 1) return kk;
    return kk >= PIPE_Q_KEEP ? D / 16 + kk - PIPE_Q_KEEP : -1;
  };

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int w = tid / WAVE;
  const int g = w % G;                   // q-head within the GQA group
  const int sub = w / G;                 // first of its SUBS 32-row sub-tiles
  const int rows_blk = QTILE * SUBS * (NW / G);
  const int tile = blockIdx.x;
  const int kh = blockIdx.y;
  const int hq = kh * G + g;

  const int s = tile_seq[tile];
  const int q0_blk = tile_q0[tile];
  const int nq_total = qlocs[s + 1] - qlocs[s];
  const int L = seq_lens[s];
  const int ctx = L - nq_total;
  const int nq_blk = min(rows_blk, nq_total - q0_blk);
  if (nq_blk <= 0) return;               // pad tile (block-uniform)
  // pages the block stages: up to its last row's causal bound (<= L)
  const int nt_blk = (ctx + q0_blk + nq_blk + BS - 1) / BS;

  // per sub-tile of this wave (su is always unrolled: static indexing)
  int row_base[SUBS], nq[SUBS], qabs_base[SUBS], nt_w[SUBS];
#pragma unroll
  for (int su = 0; su < SUBS; ++su) {
    const int q0 = q0_blk + QTILE * (sub * SUBS + su);
    row_base[su] = qlocs[s] + q0;
    nq[su] = min(QTILE, nq_total - q0);  // <= 0: no rows in this sub-tile
    qabs_base[su] = ctx + q0;
    nt_w[su] = nq[su] > 0 ? (qabs_base[su] + nq[su] + BS - 1) / BS : 0;
  }

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  u16* kbuf = (u16*)smem_raw;                        // [2][BS * D]
  u16* vbuf = kbuf + 2 * BS * D;                     // [2][D * VT_PAD]
  u16* p_base = vbuf + 2 * D * VT_PAD;
  u16* p_lds = p_base + (long)w * PWAVE_ELEMS;
  float* stat_lds = (float*)(p_base + (long)NW * PWAVE_ELEMS) + w * 2 * QTILE;
  float* alpha_lds = stat_lds;
  float* lsum_lds = stat_lds + QTILE;
  u16* q_lds = (u16*)((float*)(p_base + (long)NW * PWAVE_ELEMS) +
                      NW * 2 * QTILE) + (long)w * (Q_FRAGS * 64 * 8);

  const int my_q = lane & 31;
  const int hi = lane >> 5;

  kraw_t kraw[KI];
  vraw_t vraw[VI][2];
  const int vtid = NT - 1 - tid;   // V items from the top: K and V staging
                                   // land on different waves when NT allows
  auto stage_load = [&](int blk) {
    const long kv_base = (((long)blk * Hk + kh) * BS) * D;  // in elements
#pragma unroll
    for (int i = 0; i < KI; ++i) {
      const int it = tid + i * NT;
      if (KITEMS % NT == 0 || it < KITEMS) {
        const int row = it / SLOTS, slot = it % SLOTS;
        kraw[i] = *(const kraw_t*)(k_cache +
                                   ((long)kv_base + row * D + slot * 8) * ES);
      }
    }
#pragma unroll
    for (int i = 0; i < VI; ++i) {
      const int it = vtid + i * NT;
      if (VITEMS % NT == 0 || it < VITEMS) {
        const int kvp = it % (BS / 2), c4 = it / (BS / 2);
        const u8* src = v_cache + ((long)kv_base + 2 * kvp * D + c4 * 4) * ES;
        vraw[i][0] = *(const vraw_t*)src;
        vraw[i][1] = *(const vraw_t*)(src + D * ES);
      }
    }
  };
  auto stage_write = [&](int buf) {
    char* kt_lds = (char*)(kbuf + buf * (BS * D));
    u16* vt_lds = vbuf + buf * (D * VT_PAD);
#pragma unroll
    for (int i = 0; i < KI; ++i) {
      const int it = tid + i * NT;
      if (KITEMS % NT == 0 || it < KITEMS) {
        const int row = it / SLOTS, slot = it % SLOTS;
        u16x8 kx;
        if constexpr (KV8) {
          float f[8];
          fp8x4_to_f32(kraw[i][0], f);
          fp8x4_to_f32(kraw[i][1], f + 4);
#pragma unroll
          for (int j = 0; j < 8; ++j) kx[j] = f2bf(f[j]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            kx[2 * j] = (u16)(kraw[i][j] & 0xFFFFu);
            kx[2 * j + 1] = (u16)(kraw[i][j] >> 16);
          }
        }
        *(u16x8*)(kt_lds + k_swz<D>(row, slot * 16)) = kx;
      }
    }
#pragma unroll
    for (int i = 0; i < VI; ++i) {
      const int it = vtid + i * NT;
      if (VITEMS % NT == 0 || it < VITEMS) {
        const int kvp = it % (BS / 2), c4 = it / (BS / 2);
        u16 v0[4], v1[4];
        if constexpr (KV8) {
          float f0[4], f1[4];
          fp8x4_to_f32(vraw[i][0][0], f0);
          fp8x4_to_f32(vraw[i][1][0], f1);
#pragma unroll
          for (int j = 0; j < 4; ++j) { v0[j] = f2bf(f0[j]); v1[j] = f2bf(f1[j]); }
        } else {
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            v0[2 * j] = (u16)(vraw[i][0][j] & 0xFFFFu);
            v0[2 * j + 1] = (u16)(vraw[i][0][j] >> 16);
            v1[2 * j] = (u16)(vraw[i][1][j] & 0xFFFFu);
            v1[2 * j + 1] = (u16)(vraw[i][1][j] >> 16);
          }
        }
        // vt[d][kv], vt[d][kv+1] as one dword (kv even: 4-byte aligned)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          *(u32*)(vt_lds + (c4 * 4 + j) * VT_PAD + 2 * kvp) =
              (u32)v0[j] | ((u32)v1[j] << 16);
      }
    }
  };

  // ---- prologue: page 0 in flight while the Q fragments load
  const int* bt_row = block_tables + (long)s * bt_stride;
  stage_load(bt_row[0]);
  int blk_next = bt_row[min(1, nt_blk - 1)];

  bf16frag qb[SUBS][D / 16];
#pragma unroll
  for (int su = 0; su < SUBS; ++su) {
    if (nq[su] > 0) {
      const int qrow = row_base[su] + (my_q < nq[su] ? my_q : 0);
      const u16* qptr = q + ((long)qrow * Hq + hq) * D + hi * 8;
#pragma unroll
      for (int kk = 0; kk < D / 16; ++kk) {
        const s16x8 qf = *(const s16x8*)(qptr + kk * 16);
        if (q_slot(su, kk) >= 0)
          *(s16x8*)(q_lds + (q_slot(su, kk) * 64 + lane) * 8) = qf;
        else
          qb[su][kk] = qf;
      }
    }
  }
  stage_write(0);

  f32x16 acc_o[SUBS][D / 32];
  float m_run[SUBS], l_run[SUBS];
#pragma unroll
  for (int su = 0; su < SUBS; ++su) {
#pragma unroll
    for (int b = 0; b < D / 32; ++b) acc_o[su][b] = (f32x16)(0.f);
    m_run[su] = -1e30f;
    l_run[su] = 0.f;
  }

  for (int kt = 0; kt < nt_blk; ++kt) {
    // buffer kt&1 is complete; every wave is done reading the other one
    __syncthreads();
    const bool more = kt + 1 < nt_blk;
    if (more) {
      stage_load(blk_next);
      blk_next = bt_row[min(kt + 2, nt_blk - 1)];
    }

#pragma unroll
    for (int su = 0; su < SUBS; ++su) {
      if (kt < nt_w[su]) {
        const char* kt_lds = (const char*)(kbuf + (kt & 1) * (BS * D));
        const u16* vt_lds = vbuf + (kt & 1) * (D * VT_PAD);
        const int kv0 = kt * BS;

        // ---- QK^T: D1[kv][q] = sum_k K[kv][k] * Q^T[k][q]
        f32x16 d1 = (f32x16)(0.f);
#pragma unroll
        for (int kk = 0; kk < D / 16; ++kk) {
          const int row = lane & 31;
          const int byte_in_row = (kk * 16 + hi * 8) * 2;
          bf16frag ka = *(const s16x8*)(kt_lds + k_swz<D>(row, byte_in_row));
          bf16frag qf;
          if (q_slot(su, kk) >= 0)
            qf = *(const s16x8*)(q_lds + (q_slot(su, kk) * 64 + lane) * 8);
          else
            qf = qb[su][kk];
          d1 = mfma32(ka, qf, d1);
          // two K fragments in flight at most (register budget)
          if constexpr (SUBS > 1)
            if (kk & 1) __builtin_amdgcn_sched_barrier(0);
        }

        // ---- online softmax (identical to attn_prefill_kernel)
        float sc[16];
        float tmax = -1e30f;
        const int qabs = qabs_base[su] + my_q;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kvpos = kv0 + d_row(r, hi);
          float v = d1[r] * scale;
          if (kvpos > qabs || kvpos >= L) v = -1e30f;
          sc[r] = v;
          tmax = fmaxf(tmax, v);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float m_new = fmaxf(m_run[su], tmax);
        const float alpha = __expf(m_run[su] - m_new);
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = __expf(sc[r] - m_new);
          sc[r] = p;
          psum += p;
        }
        psum += __shfl_xor(psum, 32, 64);
        l_run[su] = l_run[su] * alpha + psum;
        m_run[su] = m_new;

#pragma unroll
        for (int r = 0; r < 16; ++r)
          p_lds[my_q * VT_PAD + d_row(r, hi)] = f2bf(sc[r]);
        if (hi == 0) alpha_lds[my_q] = alpha;

        float al[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) al[r] = alpha_lds[d_row(r, hi)];
#pragma unroll
        for (int b = 0; b < D / 32; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc_o[su][b][r] *= al[r];

        // ---- PV: D2[q][d] += P[q][kv] * V^T-read B[kv][d]
        bf16frag pa[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          pa[kk] = *(const s16x8*)(p_lds + (lane & 31) * VT_PAD + kk * 16 + hi * 8);
#pragma unroll
        for (int b = 0; b < D / 32; ++b) {
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            bf16frag vb = *(const s16x8*)(vt_lds + (b * 32 + (lane & 31)) * VT_PAD +
                                          kk * 16 + hi * 8);
            acc_o[su][b] = mfma32(pa[kk], vb, acc_o[su][b]);
          }
          if constexpr (SUBS > 1) __builtin_amdgcn_sched_barrier(0);
        }
      }
      // keep the sub-tiles' bodies apart: interleaved, their score and
      // fragment registers would be live together
      if constexpr (SUBS > 1) __builtin_amdgcn_sched_barrier(0);
    }

    if (more) stage_write((kt + 1) & 1);
  }

#pragma unroll
  for (int su = 0; su < SUBS; ++su) {
    if (nq[su] <= 0) continue;   // no barrier follows

    // ---- epilogue: divide by l; 32-column blocks through the wave's P region,
    // then 16-byte stores (a row's 64 bytes per 4 lanes)
    if (hi == 0) lsum_lds[my_q] = l_run[su];
    float inv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float l = lsum_lds[d_row(r, hi)];
      inv[r] = l > 0.f ? 1.0f / l : 0.f;
    }
    const int d_col = lane & 31;
#pragma unroll
    for (int b = 0; b < D / 32; ++b) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        p_lds[d_row(r, hi) * VT_PAD + d_col] = f2bf(acc_o[su][b][r] * inv[r]);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int idx = lane + 64 * i;
        const int qrow = idx >> 2, ch = idx & 3;
        const u16x8 o8 = *(const u16x8*)(p_lds + qrow * VT_PAD + ch * 8);
        if (qrow < nq[su])
          *(u16x8*)(out + ((long)(row_base[su] + qrow) * Hq + hq) * D + b * 32 +
                    ch * 8) = o8;
      }
    }
  }
}

// Configurations the pipelined kernel takes. A block has G * tile_rows / 32
// (head, sub-tile) pairs: up to 8 run one per wave; 16 run on 8 waves that
// walk two sub-tiles each (16 waves would leave 128 registers per wave, which
// head_dim 128 does not fit without scratch). NW is a template parameter, so
// only power-of-two group sizes are built.
extern "C" int sutro_attn_prefill_pipe_supported(int Hq, int Hk, int head_dim,
                                                 int tile_rows) {
  if (Hk <= 0 || Hq % Hk != 0) return 0;
  if (head_dim != 64 && head_dim != 128) return 0;
  if (tile_rows != 32 && tile_rows != 64 && tile_rows != 128) return 0;
  const int G = Hq / Hk;
  // a wave owns one head: G <= 8 waves, so that NW = min(pairs, 8) is a
  // multiple of G
  if (G > 8) return 0;
  const int pairs = G * (tile_rows / QTILE);
  return pairs == 1 || pairs == 2 || pairs == 4 || pairs == 8 || pairs == 16;
}

// variant 0: attn_prefill_kernel (32-row tiles only); 1: the pipelined kernel
// with tile lists built at a step of tile_rows. Returns 0; -1 for a
// configuration the chosen kernel does not take (nothing is launched); -2
// if the pipelined kernel's LDS size was refused or its launch failed.
extern "C" int sutro_attn_prefill_local(void*, const void*, const void*,
                                        const void*, const int*, const int*,
                                        const int*, const int*, const int*,
                                        int, int, int, int, int, int, float,
                                        int, int, int, const float*,
                                        hipStream_t);

extern "C" int sutro_attn_prefill(void* out, const void* q,
                                  const void* k_cache, const void* v_cache,
                                  const int* block_tables,
                                  const int* seq_lens, const int* qlocs,
                                  const int* tile_seq, const int* tile_q0,
                                  int n_tiles, int bt_stride, int Hq, int Hk,
                                  int head_dim, int kv_fp8, float scale,
                                  int tile_rows, int variant, hipStream_t s) {
  return sutro_attn_prefill_local(out, q, k_cache, v_cache, block_tables,
                                  seq_lens, qlocs, tile_seq, tile_q0, n_tiles,
                                  bt_stride, Hq, Hk, head_dim, kv_fp8, scale,
                                  tile_rows, variant, 0, nullptr, s);
}

// The same with local attention: window > 0 and/or sinks != null run the
// reference kernel's LOCAL instantiation whatever `variant` says (the
// pipelined kernel has neither), so tile lists must be built at 32 rows:
// -1 otherwise. window == 0 and sinks == null is sutro_attn_prefill.
extern "C" int sutro_attn_prefill_local(void* out, const void* q,
                                        const void* k_cache,
                                        const void* v_cache,
                                        const int* block_tables,
                                        const int* seq_lens, const int* qlocs,
                                        const int* tile_seq,
                                        const int* tile_q0, int n_tiles,
                                        int bt_stride, int Hq, int Hk,
                                        int head_dim, int kv_fp8, float scale,
                                        int tile_rows, int variant, int window,
                                        const float* sinks, hipStream_t s) {
  const int G = Hq / Hk;
  const bool local = window > 0 || sinks != nullptr;
  if (local) variant = 0;
  if (variant == 0) {
    if (tile_rows != QTILE) return -1;
  } else if (!sutro_attn_prefill_pipe_supported(Hq, Hk, head_dim, tile_rows)) {
    return -1;
  }
  if (n_tiles == 0) return 0;
  int rc = 0;
#define LAUNCH_PF_L(DV, KV, LOC)                                              \
  hipLaunchKernelGGL((attn_prefill_kernel<DV, KV, LOC>), dim3(n_tiles, Hk),   \
                     dim3(G * WAVE), smem, s, (u16*)out, (const u16*)q,       \
                     (const u8*)k_cache, (const u8*)v_cache, block_tables,    \
                     seq_lens, qlocs, tile_seq, tile_q0, bt_stride, Hq, Hk,   \
                     scale, window, sinks)
#define LAUNCH_PF(DV, KV)                                                     \
  do {                                                                        \
    const size_t smem = sizeof(PrefillSmem<DV>) +                             \
                        (size_t)G * PWAVE_ELEMS * sizeof(u16) +               \
                        (size_t)G * 2 * QTILE * sizeof(float);                \
    if (local) LAUNCH_PF_L(DV, KV, true);                                     \
    else       LAUNCH_PF_L(DV, KV, false);                                    \
  } while (0)
#define LAUNCH_PIPE(DV, KV, NWV, SUBSV)                                       \
  do {                                                                        \
    const size_t smem = 2 * sizeof(PrefillSmem<DV>) +                         \
                        (size_t)NWV * PWAVE_ELEMS * sizeof(u16) +             \
                        (size_t)NWV * 2 * QTILE * sizeof(float) +             \
                        (size_t)NWV * pipe_q_lds_frags(DV, SUBSV) * 64 * 16;  \
    auto kern = attn_prefill_pipe_kernel<DV, KV, NWV, SUBSV>;                 \
    if (smem > 48 * 1024 &&                                                   \
        hipFuncSetAttribute((const void*)kern,                                \
                            hipFuncAttributeMaxDynamicSharedMemorySize,       \
                            (int)smem) != hipSuccess) {                       \
      rc = -2;                                                                \
      break;                                                                  \
    }                                                                         \
    hipLaunchKernelGGL(kern, dim3(n_tiles, Hk), dim3(NWV * WAVE), smem, s,    \
                       (u16*)out, (const u16*)q, (const u8*)k_cache,          \
                       (const u8*)v_cache, block_tables, seq_lens, qlocs,     \
                       tile_seq, tile_q0, bt_stride, Hq, Hk, G, scale);       \
    if (hipGetLastError() != hipSuccess) rc = -2;                             \
  } while (0)
#define PIPE_NW(DV, KV)                                                       \
  do {                                                                        \
    switch (pairs) {                                                          \
      case 1: LAUNCH_PIPE(DV, KV, 1, 1); break;                               \
      case 2: LAUNCH_PIPE(DV, KV, 2, 1); break;                               \
      case 4: LAUNCH_PIPE(DV, KV, 4, 1); break;                               \
      case 8: LAUNCH_PIPE(DV, KV, 8, 1); break;                               \
      case 16: LAUNCH_PIPE(DV, KV, 8, 2); break;                              \
      default: break;                                                         \
    }                                                                         \
  } while (0)
  if (variant == 0) {
    if (head_dim == 128) {
      if (kv_fp8) LAUNCH_PF(128, true); else LAUNCH_PF(128, false);
    } else {
      if (kv_fp8) LAUNCH_PF(64, true); else LAUNCH_PF(64, false);
    }
  } else {
    const int pairs = G * (tile_rows / QTILE);
    if (head_dim == 128) {
      if (kv_fp8) PIPE_NW(128, true); else PIPE_NW(128, false);
    } else {
      if (kv_fp8) PIPE_NW(64, true); else PIPE_NW(64, false);
    }
  }
#undef PIPE_NW
#undef LAUNCH_PIPE
#undef LAUNCH_PF
#undef LAUNCH_PF_L
  return rc;
}

// ---------------------------------------------------------------------------
// MFMA layout probe: C[32,32] = A[32,16] @ B[16,32] using exactly the fragment
// loaders above. Run on hardware against torch.matmul to pin the layout.
// ---------------------------------------------------------------------------

__global__ void mfma32_probe_kernel(float* __restrict__ c,
                                    const u16* __restrict__ a,   // [32,16]
                                    const u16* __restrict__ b) { // [16,32]
  const int lane = threadIdx.x & (WAVE - 1);
  const int hi = lane >> 5;
  bf16frag af, bf;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    af[j] = (short)a[(lane & 31) * 16 + hi * 8 + j];
    bf[j] = (short)b[(hi * 8 + j) * 32 + (lane & 31)];
  }
  f32x16 d = (f32x16)(0.f);
  d = mfma32(af, bf, d);
#pragma unroll
  for (int r = 0; r < 16; ++r)
    c[d_row(r, hi) * 32 + (lane & 31)] = d[r];
}

extern "C" void sutro_mfma32_probe(float* c, const void* a, const void* b,
                                   hipStream_t s) {
  hipLaunchKernelGGL(mfma32_probe_kernel, dim3(1), dim3(64), 0, s, c,
                     (const u16*)a, (const u16*)b);
}
