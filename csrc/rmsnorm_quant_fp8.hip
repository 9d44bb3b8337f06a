// RMSNorm (optionally residual-add) with the FP8 activation quantiser fused
// in: bf16 x (+ residual) -> e4m3 codes + f32 scales, for the dense FP8
// projections that are a block norm's only consumer. The normalised row is
// never written in bf16: it is rounded to bf16 in registers and quantised
// from there, so codes, scales and the new residual are bit-equal to
// fused_add_rmsnorm (rmsnorm without a residual) followed by quant_rows_fp8 /
// quant_rows_fp8_block128.
//
// One 256-thread block per row, grid-stride. Thread tid owns the 8-element
// chunks v = tid + i * 256, i < NCH = ceil(C / 8 / 256); NCH is a template
// parameter, so the row (f32), the weight chunks and the rounded bf16 row all
// stay in registers. The arithmetic of the norm is rmsnorm_wide_reg_kernel's,
// operation for operation (per thread i then j ascending, wave_sum_f32, the
// waves in order), and so is its frame: the next grid-stride row is loaded
// before the current one is reduced, and the LDS slots are double-buffered so
// that each reduction costs one barrier.
//
// Two output formats:
//  rows     codes [R, Kp] (Kp = C rounded up to 128, tail zeroed) + one scale
//           per row [R]. The amax is a second block reduction (wave max, one
//           LDS round).
//  block128 codes [R, C] + one scale per row and group of 128 elements,
//           K-block-major [C/128, lds]. Chunk v covers elements [8v, 8v + 8),
//           so a group is 16 consecutive lanes of one wave at one i and its
//           amax is a 16-lane shfl_xor reduction: no LDS.
#include "fp8_gemm.h"

// rmsnorm without a residual sums the squares of rows of 64, 128, 192 or 256
// elements in another order (rmsnorm_small_kernel: one wave per row, lane l
// owns the C / 64 consecutive elements from l * C / 64). The no-residual
// instantiation reproduces that order through LDS for exactly those widths.
__device__ __forceinline__ bool small_row_order(int C) {
  return C % (int)WAVE == 0 && C <= 256;
}

template <bool FUSED_ADD, int NCH, bool BLOCK128>
__global__ __launch_bounds__(256) void rmsnorm_quant_fp8_kernel(
    u8* __restrict__ out_q,        // rows: [R, Kp]; block128: [R, C]
    float* __restrict__ out_s,     // rows: [R]; block128: [C/128, lds]
    u16* __restrict__ residual,    // [R, C], updated in place (FUSED_ADD)
    const u16* __restrict__ in,    // [R, C]
    const u16* __restrict__ w,     // [C]
    float eps, int rows, int C, int Kp, long lds) {
  constexpr int NT = 256;
  constexpr int NW = NT / (int)WAVE;
  constexpr bool SMALL = !FUSED_ADD && NCH == 1;
  const int tid = threadIdx.x;
  const int vec_per_row = C / 8;
  __shared__ float red[2][NW];
  __shared__ float amx[BLOCK128 ? 1 : 2][NW];
  __shared__ float srow[SMALL ? 2 : 1][SMALL ? 256 : 1];

  u16x8 wv[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int v = tid + i * NT;
    if (v < vec_per_row) wv[i] = *(const u16x8*)(w + v * 8);
  }

  u16x8 xr[NCH], rr[NCH];
  auto load_row = [&](int row) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int v = tid + i * NT;
      if (v < vec_per_row) {
        xr[i] = *(const u16x8*)(in + (long)row * C + v * 8);
        if (FUSED_ADD) rr[i] = *(const u16x8*)(residual + (long)row * C + v * 8);
      }
    }
  };

  int row = blockIdx.x;
  if (row >= rows) return;
  load_row(row);
  for (int par = 0; row < rows; row += gridDim.x, par ^= 1) {
    float xf[NCH][8];
    float ssq = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int v = tid + i * NT;
      if (v < vec_per_row) {
        if (FUSED_ADD) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float s = bf2f(xr[i][j]) + bf2f(rr[i][j]);
            xf[i][j] = s;
            ssq += s * s;
          }
          u16x8 nr;
#pragma unroll
          for (int j = 0; j < 8; ++j) nr[j] = f2bf(xf[i][j]);
          *(u16x8*)(residual + (long)row * C + v * 8) = nr;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float f = bf2f(xr[i][j]);
            xf[i][j] = f;
            ssq += f * f;
          }
        }
      }
    }
    // next row's loads fly during the reductions and the quantise pass
    const int next = row + (int)gridDim.x;
    if (next < rows) load_row(next);

    float total = 0.f;
    if (SMALL && small_row_order(C)) {
      // every wave redoes rmsnorm_small_kernel's sum from the row in LDS
      if (tid < vec_per_row) {
#pragma unroll
        for (int j = 0; j < 8; ++j) srow[par][tid * 8 + j] = xf[0][j];
      }
      __syncthreads();
      const int lane = tid & (int)(WAVE - 1);
      const int per_lane = C / (int)WAVE;
      float s = 0.f;
      for (int j = 0; j < per_lane; ++j) {
        const float f = srow[par][lane * per_lane + j];
        s += f * f;
      }
      total = wave_sum_f32(s);
    } else {
      ssq = wave_sum_f32(ssq);
      if ((tid & (WAVE - 1)) == 0) red[par][tid / WAVE] = ssq;
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NW; ++i) total += red[par][i];
    }
    const float inv = rsqrtf(total / (float)C + eps);

    // the normalised row, rounded to bf16 as the norm kernels store it
    u16x8 y[NCH];
    float amax[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int v = tid + i * NT;
      y[i] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (v < vec_per_row) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          y[i][j] = f2bf(xf[i][j] * inv * bf2f(wv[i][j]));
      }
      amax[i] = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) amax[i] = fmaxf(amax[i], fabsf(bf2f(y[i][j])));
    }

    if (BLOCK128) {
      // C % 128 == 0: the 16 lanes of a group are all live or all past the row
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        float a = amax[i];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
        const int v = tid + i * NT;
        if (v < vec_per_row) {
          const float scale = fp8_quant_scale(a);
          if ((tid & 15) == 0) out_s[(long)(v >> 4) * lds + row] = scale;
          *(u32x2*)(out_q + (long)row * C + v * 8) = fp8_quant8(y[i], scale);
        }
      }
    } else {
      float a = amax[0];
#pragma unroll
      for (int i = 1; i < NCH; ++i) a = fmaxf(a, amax[i]);
      a = wave_max_f32(a);
      if ((tid & (WAVE - 1)) == 0) amx[par][tid / WAVE] = a;
      __syncthreads();
      a = amx[par][0];
#pragma unroll
      for (int i = 1; i < NW; ++i) a = fmaxf(a, amx[par][i]);
      const float scale = fp8_quant_scale(a);
      if (tid == 0) out_s[row] = scale;
      u8* qr = out_q + (long)row * Kp;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int v = tid + i * NT;
        if (v < vec_per_row) *(u32x2*)(qr + v * 8) = fp8_quant8(y[i], scale);
      }
      // zero tail [C, Kp): at most 15 chunks
      const int vt = vec_per_row + tid;
      if (vt < Kp / 8) *(u32x2*)(qr + vt * 8) = u32x2{0u, 0u};
    }
  }
}

// mode 0: rows (C % 8 == 0, Kp = C rounded up to 128, out_s [R]); mode 1:
// block128 (C % 128 == 0, out_s [C/128, lds], lds >= R). residual may be null
// (a block's first norm). C <= 16384. Static grid, no host sync, no
// hipGetLastError: runs inside captured decode steps.
extern "C" void sutro_rmsnorm_quant_fp8(void* out_q, float* out_s,
                                        void* residual, const void* x,
                                        const void* w, float eps, long rows,
                                        int C, int Kp, long lds, int mode,
                                        hipStream_t s) {
  const int grid = rows < 2048 ? (int)rows : 2048;
  if (grid == 0) return;
#define LAUNCH_RQ(ADD, NCHV, BLK)                                             \
  hipLaunchKernelGGL((rmsnorm_quant_fp8_kernel<ADD, NCHV, BLK>), dim3(grid),  \
                     dim3(256), 0, s, (u8*)out_q, out_s, (u16*)residual,      \
                     (const u16*)x, (const u16*)w, eps, (int)rows, C, Kp, lds)
#define LAUNCH_RQ_NCH(ADD, BLK)                                               \
  switch ((C / 8 + 255) / 256) {                                              \
    case 1: LAUNCH_RQ(ADD, 1, BLK); break;                                    \
    case 2: LAUNCH_RQ(ADD, 2, BLK); break;                                    \
    case 3: LAUNCH_RQ(ADD, 3, BLK); break;                                    \
    case 4: LAUNCH_RQ(ADD, 4, BLK); break;                                    \
    case 5: LAUNCH_RQ(ADD, 5, BLK); break;                                    \
    case 6: LAUNCH_RQ(ADD, 6, BLK); break;                                    \
    case 7: LAUNCH_RQ(ADD, 7, BLK); break;                                    \
    default: LAUNCH_RQ(ADD, 8, BLK); break;                                   \
  }
  if (residual) {
    if (mode == 1) { LAUNCH_RQ_NCH(true, true) } else { LAUNCH_RQ_NCH(true, false) }
  } else {
    if (mode == 1) { LAUNCH_RQ_NCH(false, true) } else { LAUNCH_RQ_NCH(false, false) }
  }
#undef LAUNCH_RQ_NCH
#undef LAUNCH_RQ
}
