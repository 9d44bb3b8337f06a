// Fused MoE routing for gfx950: router logits -> (w, padpos, row_tok,
// tile_off, counts), the tensors the grouped GEMMs and moe_combine consume.
// Semantics: torch_ref.moe_route (top-k on the logits compared as f32, ties to
// the lower expert index, softmax over the k selected logits, assignments laid
// out by (expert, t*k + j) in segments padded to bm).
//
// Three launches, every shape static, no atomics on global memory and none
// that decide a position, so the output bits do not depend on scheduling:
//
//   select   16 lanes own a token; its E logits sit in their registers as
//            packed keys (ordered f32 image << 32 | E-1-index) and each of
//            the k rounds is a lane-local max plus a 4-step DPP row rotation.
//            Writes idx / w, the block's per-expert tally, and -1 over
//            row_tok.
//   offsets  one block, one thread per local expert: walks the block tallies
//            in block order (per-block bases, counts), then scans the padded
//            sizes across experts into tile_off.
//   scatter  same token partition; 64 consecutive flat indices t*k + j per
//            wave, rank inside the wave from log2(E_l) ballots, per-wave
//            totals scanned through LDS in wave order.
//
// A block owns RT_TOK consecutive tokens in both select and scatter.
#include "common.h"

constexpr int RT_THREADS = 256;
constexpr int RT_TOK = 128;       // tokens per block
constexpr int RT_MAX_E = 128;
constexpr int RT_MAX_K = 8;
constexpr int RT_MAX_WC = RT_TOK * RT_MAX_K / 64;   // 64-lane chunks per block

// u32 whose unsigned order is the f32 order; -0 maps with +0 (they compare
// equal, so the tie rule decides between them)
__device__ __forceinline__ u32 f32_ordered(float f) {
  u32 u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float f32_from_ordered(u32 o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// max over the 16 lanes of a DPP row, result in all of them: rotations by
// 1, 2, 4, 8 inside the row (row_ror), no LDS
template <int CTRL>
__device__ __forceinline__ u64 row_rotate_u64(u64 v) {
  const int lo = (int)(u32)v, hi = (int)(u32)(v >> 32);
  const u32 rlo = (u32)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
  const u32 rhi = (u32)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
  return ((u64)rhi << 32) | rlo;
}

__device__ __forceinline__ u64 max_u64(u64 a, u64 b) { return a > b ? a : b; }

__device__ __forceinline__ u64 row16_max_u64(u64 v) {
  v = max_u64(v, row_rotate_u64<0x121>(v));
  v = max_u64(v, row_rotate_u64<0x122>(v));
  v = max_u64(v, row_rotate_u64<0x124>(v));
  v = max_u64(v, row_rotate_u64<0x128>(v));
  return v;
}

// EPL consecutive logits of one lane as f32: one load of up to 16 bytes (two
// for eight f32)
template <int EPL>
__device__ __forceinline__ void load_logits(const u16* p, float* v) {
  if constexpr (EPL == 8) {
    const u16x8 x = *(const u16x8*)p;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bf2f(x[j]);
  } else if constexpr (EPL == 4) {
    const u16x4 x = *(const u16x4*)p;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = bf2f(x[j]);
  } else if constexpr (EPL == 2) {
    const u16x2 x = *(const u16x2*)p;
    v[0] = bf2f(x[0]); v[1] = bf2f(x[1]);
  } else {
    v[0] = bf2f(*p);
  }
}

template <int EPL>
__device__ __forceinline__ void load_logits(const float* p, float* v) {
  if constexpr (EPL >= 4) {
#pragma unroll
    for (int q = 0; q < EPL / 4; ++q) {
      const f32x4 x = *(const f32x4*)(p + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * q + j] = x[j];
    }
  } else if constexpr (EPL == 2) {
    const f32x2 x = *(const f32x2*)p;
    v[0] = x[0]; v[1] = x[1];
  } else {
    v[0] = *p;
  }
}

// E == 16 * EPL, or E <= 16 with EPL == 1 (lanes >= E of a group hold nothing)
template <typename LT, int EPL>
__global__ void __launch_bounds__(RT_THREADS) NO_PACKED_F32
moe_route_select_kernel(
    const LT* __restrict__ logits,   // [T, E]
    int* __restrict__ idx_out,       // [T, k] selected expert (global index)
    float* __restrict__ w_out,       // [T, k] 0 where the expert is not local
    int* __restrict__ blk_hist,      // [gridDim.x, E_l]
    int* __restrict__ row_tok,       // [rows_max] <- -1
    int T, int E, int k, int base, int E_l, int rows_max) {
  __shared__ int hist[RT_MAX_E];
  const int tid = threadIdx.x;
  if (tid < RT_MAX_E) hist[tid] = 0;
  __syncthreads();

  const int grp = tid >> 4, gl = tid & 15;
  const int e0 = gl * EPL;
  for (int it = 0; it < RT_TOK / 16; ++it) {
    const int t = blockIdx.x * RT_TOK + it * 16 + grp;
    u64 key[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) key[j] = 0;   // below every live key
    if (t < T && e0 < E) {
      float v[EPL];
      load_logits<EPL>(logits + (long)t * E + e0, v);
#pragma unroll
      for (int j = 0; j < EPL; ++j)
        key[j] = ((u64)f32_ordered(v[j]) << 32) | (u32)(E - 1 - (e0 + j));
    }
    // k rounds: every lane of the group learns each winner; the owner
    // retires it (keys are distinct, so only the owner matches)
    u64 win[RT_MAX_K];
#pragma unroll
    for (int r = 0; r < RT_MAX_K; ++r) {
      win[r] = 0;
      if (r < k) {
        u64 m = key[0];
#pragma unroll
        for (int j = 1; j < EPL; ++j) m = max_u64(m, key[j]);
        m = row16_max_u64(m);
#pragma unroll
        for (int j = 0; j < EPL; ++j)
          if (key[j] == m) key[j] = 0;
        win[r] = m;
      }
    }
    // exponentials in slot order; lane j of the group keeps slot j
    const float lmax = f32_from_ordered((u32)(win[0] >> 32));
    float sum = 0.f, mine = 0.f;
    u32 my_low = 0;
#pragma unroll
    for (int r = 0; r < RT_MAX_K; ++r) {
      if (r < k) {
        const float ex = expf(f32_from_ordered((u32)(win[r] >> 32)) - lmax);
        sum += ex;
        if (r == gl) { mine = ex; my_low = (u32)win[r]; }
      }
    }
    if (t < T && gl < k) {
      const int e = E - 1 - (int)my_low;
      const int e_loc = e - base;
      const bool local = e_loc >= 0 && e_loc < E_l;
      idx_out[(long)t * k + gl] = e;
      w_out[(long)t * k + gl] = local ? mine / sum : 0.f;
      if (local) atomicAdd(&hist[e_loc], 1);   // integer tally: order-free
    }
  }
  __syncthreads();
  if (tid < E_l) blk_hist[(long)blockIdx.x * E_l + tid] = hist[tid];

  for (long i = (long)blockIdx.x * RT_THREADS + tid; i < rows_max;
       i += (long)gridDim.x * RT_THREADS)
    row_tok[i] = -1;
}

__global__ void __launch_bounds__(RT_MAX_E) moe_route_offsets_kernel(
    const int* __restrict__ blk_hist,   // [nblk, E_l]
    int* __restrict__ blk_base,         // [nblk, E_l] rows of e before block b
    int* __restrict__ counts,           // [E_l]
    int* __restrict__ tile_off,         // [E_l + 1]
    int nblk, int E_l, int bm) {
  __shared__ int wave_total[RT_MAX_E / 64];
  const int e = threadIdx.x;
  int run = 0;
  if (e < E_l) {
#pragma unroll 8
    for (int b = 0; b < nblk; ++b) {
      const int c = blk_hist[(long)b * E_l + e];
      blk_base[(long)b * E_l + e] = run;
      run += c;
    }
    counts[e] = run;
  }
  const int padded = (run + bm - 1) / bm * bm;
  int inc = padded;   // inclusive scan over the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(inc, off, 64);
    if ((e & 63) >= off) inc += o;
  }
  if ((e & 63) == 63) wave_total[e >> 6] = inc;
  __syncthreads();
  const int excl = (e >= 64 ? wave_total[0] : 0) + inc - padded;
  if (e < E_l) tile_off[e] = excl / bm;
  if (e == E_l - 1) tile_off[E_l] = (excl + padded) / bm;
}

__global__ void __launch_bounds__(RT_THREADS) moe_route_scatter_kernel(
    const int* __restrict__ idx,        // [T, k]
    const int* __restrict__ blk_base,   // [gridDim.x, E_l]
    const int* __restrict__ tile_off,   // [E_l + 1]
    int* __restrict__ row_tok,          // [rows_max]
    long* __restrict__ padpos,          // [T, k]
    int T, int k, int base, int E_l, int bm, int nbits, int rows_max) {
  // [64-lane chunk of the block's flat indices][local expert]: first the
  // chunk's count, then the padded row of its first assignment
  __shared__ int cnt[RT_MAX_WC][RT_MAX_E];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nwc = RT_TOK * k / 64;
  for (int i = tid; i < nwc * RT_MAX_E; i += RT_THREADS) (&cnt[0][0])[i] = 0;
  __syncthreads();

  const long total = (long)T * k;
  const long f0 = (long)blockIdx.x * RT_TOK * k;
  constexpr int NC = RT_MAX_WC / (RT_THREADS / 64);
  int el[NC], rk[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int wc = c * (RT_THREADS / 64) + wave;
    el[c] = -1;
    rk[c] = 0;
    if (wc < nwc) {
      const long f = f0 + wc * 64 + lane;
      int e = -1;
      if (f < total) {
        e = idx[f] - base;
        if (e < 0 || e >= E_l) e = -1;
      }
      // lanes of this wave with my expert: per bit keep the ballot or its
      // complement; lane order is the stable order
      u64 same = __ballot(e >= 0);
      for (int bit = 0; bit < nbits; ++bit) {
        const bool mine = (e >> bit) & 1;
        const u64 b = __ballot(mine);
        same &= mine ? b : ~b;
      }
      el[c] = e;
      rk[c] = __popcll(same & ((1ull << lane) - 1ull));
      if (e >= 0 && rk[c] == 0) cnt[wc][e] = __popcll(same);
    }
  }
  __syncthreads();
  if (tid < E_l) {
    int run = tile_off[tid] * bm + blk_base[(long)blockIdx.x * E_l + tid];
    for (int wc = 0; wc < nwc; ++wc) {
      const int c = cnt[wc][tid];
      cnt[wc][tid] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int wc = c * (RT_THREADS / 64) + wave;
    const long f = f0 + wc * 64 + lane;
    if (wc < nwc && f < total) {
      if (el[c] >= 0) {
        const int pos = cnt[wc][el[c]] + rk[c];
        row_tok[pos] = (int)(f / k);
        padpos[f] = pos;
      } else {
        // not local (EP): the last slot, past every padded segment
        padpos[f] = rows_max - 1;
      }
    }
  }
}

// returns 0, or -1 for a shape outside the supported set (the binding checks
// first). No error-state query here: they are rejected while a stream is
// capturing, and decode steps replay this inside hipGraphs.
extern "C" int sutro_moe_route(
    const void* logits, int logits_f32, int* idx, float* w, long* padpos,
    int* row_tok, int* tile_off, int* counts, int* blk_hist, int* blk_base,
    int T, int E, int k, int base, int E_l, int bm, hipStream_t stream) {
  const int epl = E <= 16 ? 1 : E / 16;
  if (T <= 0 || E < 1 || E > RT_MAX_E || (E > 16 && E % 16) ||
      (epl != 1 && epl != 2 && epl != 4 && epl != 8) || k < 1 ||
      k > RT_MAX_K || k > E || E_l < 1 || E_l > E || (bm != 64 && bm != 128))
    return -1;
  const int nblk = (T + RT_TOK - 1) / RT_TOK;
  const int rows_max = T * k + E_l * bm;
  int nbits = 0;
  while ((1 << nbits) < E_l) ++nbits;
#define RT_SELECT(EPL_)                                                      \
  if (logits_f32)                                                            \
    moe_route_select_kernel<float, EPL_><<<nblk, RT_THREADS, 0, stream>>>(   \
        (const float*)logits, idx, w, blk_hist, row_tok, T, E, k, base, E_l, \
        rows_max);                                                           \
  else                                                                       \
    moe_route_select_kernel<u16, EPL_><<<nblk, RT_THREADS, 0, stream>>>(     \
        (const u16*)logits, idx, w, blk_hist, row_tok, T, E, k, base, E_l,   \
        rows_max);
  if (epl == 8) { RT_SELECT(8) }
  else if (epl == 4) { RT_SELECT(4) }
  else if (epl == 2) { RT_SELECT(2) }
  else { RT_SELECT(1) }
#undef RT_SELECT
  moe_route_offsets_kernel<<<1, RT_MAX_E, 0, stream>>>(
      blk_hist, blk_base, counts, tile_off, nblk, E_l, bm);
  moe_route_scatter_kernel<<<nblk, RT_THREADS, 0, stream>>>(
      idx, blk_base, tile_off, row_tok, padpos, T, k, base, E_l, bm, nbits,
      rows_max);
  return 0;
}
