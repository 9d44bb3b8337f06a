// Sparse logit penalties (CDNA4 / gfx950): repetition / presence / frequency
// penalties + logit_bias, applied IN PLACE to the rows that ask for them, one
// 256-thread workgroup per penalised row. No dense per-row state over the
// vocab: the row's token history (device-resident, engine/penalties.py) and
// its bias keys are folded into an open-addressing hash table in LDS, then
// each occupied table slot -- exactly one owner thread per distinct token --
// does the read-modify-write of logits[row, t].
//
// Semantics (shared with sutro_amd/ops/torch_ref.py::apply_logit_penalties):
//   a(t) = t in h[0..L)            c(t) = #{ j >= P : h[j] = t }
//   y = f32(x[t])
//   if a(t):    y = (y > 0) ? y / rep : y * rep
//   y = y - freq * f32(c(t))
//   if c(t)>0:  y = y - pres
//   if t in bias: y = y + bias[t]        (first matching entry of the row)
//   x[t] = rne(y)
// Only touched elements (a(t) or t a bias key, t < vl) are written; all other
// bits of the tensor are left alone. Every f32 op is individually rounded
// (contraction is OFF in penalise(); the divide is the correctly-rounded one),
// counts are integers and every token has one owner, so the result does not
// depend on thread order and equals the torch reference bit for bit.
//
// Table: u32 key (token id, EMPTY = ~0) claimed with atomicCAS + u32 payload:
// bits 0..13 output count (<= 8192), bit 14 seen-in-prompt, bits 22..31 the
// index of the token's first entry in the row's bias list (0x3FF = none).
// Bias keys go in first, while every count is still zero, so an atomicMin on
// the whole word orders by index alone; the history pass then only touches
// the low bits. The owner reads its bias value by index, with no search.
// Capacity is a power of two >= 2 * (max hist_len + B), picked by the host among
// 2048 / 8192 / 16384 entries (16 / 64 / 128 KiB of dynamic LDS), so typical
// few-hundred-token histories keep many workgroups per CU. The kernel clamps
// the history it inserts to cap/2 - B entries: a table can never fill, so
// linear probing always terminates whatever the device-side lengths hold.

#include <hip/hip_runtime.h>

#include "common.h"

#define PEN_THREADS 256
#define PEN_EMPTY 0xFFFFFFFFu
#define PEN_SEEN 0x00004000u
#define PEN_CNT_MASK 0x00003FFFu
#define PEN_BIAS_SHIFT 22
#define PEN_NO_BIAS 0x3FFu
#define PEN_PAY_INIT (PEN_NO_BIAS << PEN_BIAS_SHIFT)

typedef int i32x4 __attribute__((ext_vector_type(4)));

template <int LOG2>
__device__ __forceinline__ u32 pen_hash(u32 t) {
  return (t * 2654435761u) >> (32 - LOG2);
}

// claim-or-find the slot of token t (table is never more than half full)
template <int LOG2>
__device__ __forceinline__ u32 pen_insert(u32* keys, u32 t) {
  constexpr u32 MASK = (1u << LOG2) - 1u;
  u32 s = pen_hash<LOG2>(t);
  for (u32 probe = 0; probe <= MASK; ++probe) {
    const u32 prev = atomicCAS(&keys[s], PEN_EMPTY, t);
    if (prev == PEN_EMPTY || prev == t) return s;
    s = (s + 1u) & MASK;
  }
  return PEN_EMPTY;  // unreachable: load factor <= 1/2
}

template <int LOG2>
__device__ __forceinline__ void pen_hist_token(u32* keys, u32* pay, int t,
                                               int vl, bool is_output) {
  if (t < 0 || t >= vl) return;
  const u32 s = pen_insert<LOG2>(keys, (u32)t);
  if (s == PEN_EMPTY) return;
  if (is_output) atomicAdd(&pay[s], 1u);
  else atomicOr(&pay[s], PEN_SEEN);
}

__device__ __forceinline__ float pen_load(const float* p) { return *p; }
__device__ __forceinline__ float pen_load(const u16* p) { return bf2f(*p); }
__device__ __forceinline__ void pen_store(float* p, float y) { *p = y; }
__device__ __forceinline__ void pen_store(u16* p, float y) {
  const u32 u = __float_as_uint(y);
  // NaN keeps a quiet-NaN pattern; everything else rounds to nearest even
  *p = (y != y) ? (u16)0x7FC0u : (u16)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// the arithmetic of the semantics block; one rounding per operation
__device__ __forceinline__ float penalise(float y, bool seen, u32 cnt,
                                          float rep, float pres, float freq,
                                          bool has_bias, float bias) {
#pragma clang fp contract(off)
  if (seen) y = (y > 0.0f) ? (y / rep) : (y * rep);
  const float fc = freq * (float)cnt;
  y = y - fc;
  if (cnt > 0u) y = y - pres;
  if (has_bias) y = y + bias;
  return y;
}

template <typename T, int LOG2>
__global__ __launch_bounds__(PEN_THREADS) void logit_penalties_kernel(
    T* __restrict__ logits, const int* __restrict__ row_idx,
    const int* __restrict__ hist, const int* __restrict__ slot,
    const int* __restrict__ hist_len, const int* __restrict__ prompt_len,
    const float* __restrict__ rep, const float* __restrict__ pres,
    const float* __restrict__ freq, const int* __restrict__ bias_tok,
    const float* __restrict__ bias_val, int n_rows, long v_row, int vl,
    int n_slots, int lcap, int n_bias) {
  constexpr int CAP = 1 << LOG2;
  extern __shared__ u32 pen_lds[];
  u32* keys = pen_lds;
  u32* pay = pen_lds + CAP;

  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const int row = row_idx[r];
  const int sl = slot[r];
  if (row < 0 || row >= n_rows) return;  // block-uniform

  int L = hist_len[r];
  const int max_hist = CAP / 2 - n_bias;
  L = min(min(L, lcap), max_hist);
  if (sl < 0 || sl >= n_slots || L < 0) L = 0;
  const int P = max(0, min(prompt_len[r], L));

  for (int i = tid; i < CAP; i += PEN_THREADS) {
    keys[i] = PEN_EMPTY;
    pay[i] = PEN_PAY_INIT;
  }
  __syncthreads();

  const int* btok = bias_tok + (long)r * n_bias;
  const float* bval = bias_val + (long)r * n_bias;
  for (int b = tid; b < n_bias; b += PEN_THREADS) {
    const int t = btok[b];
    if (t < 0 || t >= vl) continue;
    const u32 s = pen_insert<LOG2>(keys, (u32)t);
    if (s != PEN_EMPTY) atomicMin(&pay[s], (u32)b << PEN_BIAS_SHIFT);
  }
  __syncthreads();  // counts start only after every bias index has settled

  const int* h = hist + (long)(L > 0 ? sl : 0) * lcap;
  // 16-byte loads over the aligned body, scalar tail
  const bool vec_ok = (lcap % 4 == 0) && ((((size_t)hist) & 15u) == 0);
  const int nvec = vec_ok ? (L >> 2) : 0;
  for (int i = tid; i < nvec; i += PEN_THREADS) {
    const i32x4 v = *reinterpret_cast<const i32x4*>(h + 4 * i);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      pen_hist_token<LOG2>(keys, pay, v[k], vl, 4 * i + k >= P);
  }
  for (int j = 4 * nvec + tid; j < L; j += PEN_THREADS)
    pen_hist_token<LOG2>(keys, pay, h[j], vl, j >= P);

  __syncthreads();

  const float rp = rep[r], pr = pres[r], fq = freq[r];
  T* x = logits + (long)row * v_row;
  for (int s = tid; s < CAP; s += PEN_THREADS) {
    const u32 t = keys[s];
    if (t == PEN_EMPTY) continue;
    const u32 p = pay[s];
    const u32 cnt = p & PEN_CNT_MASK;
    const bool seen = (p & PEN_SEEN) != 0u || cnt > 0u;
    const u32 bidx = p >> PEN_BIAS_SHIFT;
    const bool has_bias = bidx < (u32)n_bias;  // PEN_NO_BIAS >= 512 >= n_bias
    const float bias = has_bias ? bval[bidx] : 0.0f;
    const float y = penalise(pen_load(x + t), seen, cnt, rp, pr, fq, has_bias,
                             bias);
    pen_store(x + t, y);
  }
}

template <typename T, int LOG2>
static void pen_launch(void* logits, const int* row_idx, const int* hist,
                       const int* slot, const int* hist_len,
                       const int* prompt_len, const float* rep,
                       const float* pres, const float* freq,
                       const int* bias_tok, const float* bias_val, int m,
                       int n_rows, long v_row, int vl, int n_slots, int lcap,
                       int n_bias, hipStream_t stream) {
  constexpr size_t LDS = (size_t)(2u << LOG2) * sizeof(u32);
  auto kern = logit_penalties_kernel<T, LOG2>;
  if (LDS > 64u * 1024u) {
    // above the default dynamic-LDS limit: opt in once per instantiation
    static bool raised = false;
    if (!raised) {
      hipError_t e = hipFuncSetAttribute(
          (const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
          (int)LDS);
      if (e != hipSuccess)
        printf("logit_penalties: LDS opt-in failed: %s\n",
               hipGetErrorString(e));
      raised = true;
    }
  }
  kern<<<m, PEN_THREADS, LDS, stream>>>(
      (T*)logits, row_idx, hist, slot, hist_len, prompt_len, rep, pres, freq,
      bias_tok, bias_val, n_rows, v_row, vl, n_slots, lcap, n_bias);
  HIP_CHECK_LAUNCH();
}

template <typename T>
static void pen_dispatch(int log2_cap, void* logits, const int* row_idx,
                         const int* hist, const int* slot, const int* hist_len,
                         const int* prompt_len, const float* rep,
                         const float* pres, const float* freq,
                         const int* bias_tok, const float* bias_val, int m,
                         int n_rows, long v_row, int vl, int n_slots, int lcap,
                         int n_bias, hipStream_t stream) {
#define PEN_CASE(L2)                                                          \
  pen_launch<T, L2>(logits, row_idx, hist, slot, hist_len, prompt_len, rep,   \
                    pres, freq, bias_tok, bias_val, m, n_rows, v_row, vl,     \
                    n_slots, lcap, n_bias, stream)
  if (log2_cap <= 11) PEN_CASE(11);
  else if (log2_cap <= 13) PEN_CASE(13);
  else PEN_CASE(14);
#undef PEN_CASE
}

// log2_cap: 11, 13 or 14 (host picks the smallest table with
// 2^log2_cap >= 2 * (max hist_len + n_bias); 14 is the largest supported)
extern "C" void sutro_logit_penalties(
    void* logits, int is_f32, const int* row_idx, const int* hist,
    const int* slot, const int* hist_len, const int* prompt_len,
    const float* rep, const float* pres, const float* freq,
    const int* bias_tok, const float* bias_val, int m, int n_rows, long v_row,
    int vl, int n_slots, int lcap, int n_bias, int log2_cap,
    hipStream_t stream) {
  if (m <= 0) return;
  if (is_f32)
    pen_dispatch<float>(log2_cap, logits, row_idx, hist, slot, hist_len,
                        prompt_len, rep, pres, freq, bias_tok, bias_val, m,
                        n_rows, v_row, vl, n_slots, lcap, n_bias, stream);
  else
    pen_dispatch<u16>(log2_cap, logits, row_idx, hist, slot, hist_len,
                      prompt_len, rep, pres, freq, bias_tok, bias_val, m,
                      n_rows, v_row, vl, n_slots, lcap, n_bias, stream);
}
