// Python bindings for the sutro-amd CDNA4 kernels.
// Tensors are validated here; raw pointers + the current HIP stream go to the
// extern "C" launchers in the .hip translation units.
#include <torch/extension.h>

#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>

#include <climits>

#define CHECK_CUDA(x) TORCH_CHECK((x).is_cuda(), #x " must be a GPU tensor")
#define CHECK_CONTIG(x) TORCH_CHECK((x).is_contiguous(), #x " must be contiguous")
#define CHECK_BF16(x) \
  TORCH_CHECK((x).scalar_type() == at::kBFloat16, #x " must be bf16")

static hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

extern "C" {
void sutro_rmsnorm(void*, const void*, const void*, float, long, int,
                   hipStream_t);
void sutro_fused_add_rmsnorm(void*, void*, const void*, float, long, int, int,
                             hipStream_t);
void sutro_silu_mul(void*, const void*, long, int, hipStream_t);
void sutro_rope_and_cache(void*, void*, const void*, const long*, const long*,
                          void*, void*, const float*, int, int, int, int, int,
                          hipStream_t);
static bool is_fp8(const torch::Tensor& t) {
  return t.scalar_type() == at::kFloat8_e4m3fn;
}
void sutro_mean_pool_normalize(float*, const void*, const int*, int, int,
                               hipStream_t);
void sutro_attn_decode(void*, const void*, const void*, const void*,
                       const int*, const int*, int, int, int, int, int, int,
                       int, float, hipStream_t);
int sutro_attn_prefill(void*, const void*, const void*, const void*,
                       const int*, const int*, const int*, const int*,
                       const int*, int, int, int, int, int, int, float, int,
                       int, hipStream_t);
int sutro_attn_decode_local(void*, const void*, const void*, const void*,
                            const int*, const int*, int, int, int, int, int,
                            int, int, float, int, const float*, hipStream_t);
int sutro_attn_prefill_local(void*, const void*, const void*, const void*,
                             const int*, const int*, const int*, const int*,
                             const int*, int, int, int, int, int, int, float,
                             int, int, int, const float*, hipStream_t);
int sutro_attn_prefill_pipe_supported(int, int, int, int);
void sutro_attn_decode_shared(void*, const void*, const void*, const void*,
                              const int*, const int*, int, int, int, int,
                              float, int, int, const int*, const int*, int,
                              int, float*, float*, float*, hipStream_t);
int sutro_attn_prefix_tile_rows(int, int);
void sutro_mfma32_probe(float*, const void*, const void*, hipStream_t);
void sutro_gemm_tn_launch(void*, const void*, const void*, const void*, int,
                          int, long, int, int, int, int, hipStream_t);
int sutro_gemm_tn_pipe_launch(void*, const void*, const void*, const void*,
                              int, int, long, int, int, int, hipStream_t,
                              int variant = 0, int group_m = 0,
                              int num_blocks = 0, int wide = 0);
void sutro_mfma16_probe(float*, const void*, const void*, hipStream_t);
void sutro_hd64_stage_probe(float*, float*, void*, const void*, const void*,
                            const void*, int, float, hipStream_t);
void sutro_qkv_prep(const void*, void*, void*, void*, const long*, const long*,
                    const float*, const void*, const void*, float, int, int,
                    int, int, int, int, int, hipStream_t);
void sutro_sampler_fused(const void*, int, const float*, const float*,
                         const int*, const float*, const unsigned int*, int,
                         long, int, int, int*, float*, hipStream_t);
void sutro_grouped_gemm(void*, const void*, const void*, const int*,
                        const int*, const int*, int, int, int, long, int,
                        int, hipStream_t);
void sutro_moe_combine(void*, const void*, const long*, const float*, int,
                       int, int, hipStream_t);
void sutro_logit_penalties(void*, int, const int*, const int*, const int*,
                           const int*, const int*, const float*, const float*,
                           const float*, const int*, const float*, int, int,
                           long, int, int, int, int, int, hipStream_t);
void sutro_quant_rows_fp8(void*, float*, const void*, const int*, int, long,
                          int, int, hipStream_t);
void sutro_grouped_gemm_fp8(void*, const void*, const float*, const void*,
                            const float*, const int*, const int*, const int*,
                            int, int, int, long, int, int, hipStream_t);
void sutro_quant_weight_mxfp4(void*, void*, const void*, long, int, int,
                              hipStream_t);
void sutro_grouped_gemm_mxfp4(void*, const void*, const float*, const void*,
                              const void*, const int*, const int*, const int*,
                              int, int, int, long, int, int, hipStream_t);
void sutro_quant_rows_fp8_block128(void*, float*, const void*, long, long,
                                   long, hipStream_t);
int sutro_gemm_tn_fp8_block_pipe_launch(void*, const void*, const float*,
                                        long, const void*, const float*,
                                        const void*, int, int, long, int, int,
                                        hipStream_t);
int sutro_gemm_tn_fp8_pipe_launch(void*, const void*, const float*,
                                  const void*, const float*, const void*, int,
                                  int, long, int, int, hipStream_t);
}

void rmsnorm(torch::Tensor out, torch::Tensor x, torch::Tensor w, double eps) {
  CHECK_CUDA(x); CHECK_CONTIG(x); CHECK_BF16(x);
  const long C = x.size(-1);
  const long rows = x.numel() / C;
  TORCH_CHECK(C % 8 == 0 && C <= 16384, "unsupported row size ", C);
  sutro_rmsnorm(out.data_ptr(), x.data_ptr(), w.data_ptr(), (float)eps, rows,
                (int)C, cur_stream());
}

void fused_add_rmsnorm(torch::Tensor x, torch::Tensor residual, torch::Tensor w,
                       double eps, int64_t variant) {
  CHECK_CUDA(x); CHECK_CONTIG(x); CHECK_BF16(x); CHECK_CONTIG(residual);
  const long C = x.size(-1);
  const long rows = x.numel() / C;
  TORCH_CHECK(C % 8 == 0 && C <= 16384, "unsupported row size ", C);
  TORCH_CHECK(variant == 0 || variant == 1, "rmsnorm variant 0 or 1");
  sutro_fused_add_rmsnorm(x.data_ptr(), residual.data_ptr(), w.data_ptr(),
                          (float)eps, rows, (int)C, (int)variant,
                          cur_stream());
}

void silu_mul(torch::Tensor out, torch::Tensor x) {
  CHECK_CUDA(x); CHECK_CONTIG(x); CHECK_BF16(x);
  const long I = x.size(-1) / 2;
  const long T = x.numel() / (2 * I);
  TORCH_CHECK(I % 8 == 0, "intermediate size must be a multiple of 8");
  sutro_silu_mul(out.data_ptr(), x.data_ptr(), T, (int)I, cur_stream());
}

void rope_and_cache(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                    torch::Tensor positions, torch::Tensor slot_mapping,
                    torch::Tensor k_cache, torch::Tensor v_cache,
                    torch::Tensor cos_sin) {
  CHECK_CUDA(q); CHECK_CONTIG(q); CHECK_BF16(q);
  CHECK_CONTIG(k); CHECK_CONTIG(v); CHECK_CONTIG(k_cache);
  TORCH_CHECK(cos_sin.scalar_type() == at::kFloat, "cos_sin must be f32");
  const int T = q.size(0), Hq = q.size(1), D = q.size(2);
  const int Hk = k.size(1);
  const int bs = k_cache.size(2);
  TORCH_CHECK(D % 2 == 0 && D / 2 <= 128, "unsupported head_dim ", D);
  sutro_rope_and_cache(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                       positions.data_ptr<long>(), slot_mapping.data_ptr<long>(),
                       k_cache.data_ptr(), v_cache.data_ptr(),
                       cos_sin.data_ptr<float>(), T, Hq, Hk, D, bs,
                       cur_stream());
}

void mean_pool_normalize(torch::Tensor out, torch::Tensor hidden,
                         torch::Tensor qlocs) {
  CHECK_CUDA(hidden); CHECK_CONTIG(hidden); CHECK_BF16(hidden);
  const int S = out.size(0), H = hidden.size(-1);
  TORCH_CHECK(H % 8 == 0, "hidden size must be a multiple of 8");
  sutro_mean_pool_normalize(out.data_ptr<float>(), hidden.data_ptr(),
                            qlocs.data_ptr<int>(), S, H, cur_stream());
}

void paged_attention(torch::Tensor out, torch::Tensor q, torch::Tensor k_cache,
                     torch::Tensor v_cache, torch::Tensor block_tables,
                     torch::Tensor seq_lens, torch::Tensor qlocs, double scale,
                     int64_t num_decodes, torch::Tensor tile_seq,
                     torch::Tensor tile_q0, int64_t prefill_token_count,
                     int64_t tile_rows, int64_t prefill_variant,
                     int64_t window, c10::optional<torch::Tensor> sinks) {
  CHECK_CUDA(q); CHECK_CONTIG(q); CHECK_BF16(q); CHECK_CONTIG(k_cache);
  const int Hq = q.size(1), D = q.size(2);
  const int Hk = k_cache.size(1);
  const int bs = k_cache.size(2);
  const int S = seq_lens.size(0);
  TORCH_CHECK(D == 128 || D == 64,
              "attention kernels support head_dim 64/128 (got ", D, ")");
  TORCH_CHECK(bs == 32, "attention kernels require kv_block_size 32");
  TORCH_CHECK(Hq % Hk == 0 && Hq / Hk <= 8,
              "GQA group size must divide and be <= 8");
  // local attention: a window of `window` keys (0 = none) and/or one sink
  // logit per q head; either makes both kernels take their LOCAL route
  TORCH_CHECK(window >= 0 && window <= INT_MAX,
              "window must be >= 0 (got ", window, ")");
  const float* sinks_p = nullptr;
  if (sinks.has_value()) {
    const torch::Tensor& sk = *sinks;
    TORCH_CHECK(sk.is_cuda() && sk.device() == q.device(),
                "sinks must be on q's device");
    TORCH_CHECK(sk.scalar_type() == at::kFloat, "sinks must be f32");
    TORCH_CHECK(sk.is_contiguous(), "sinks must be contiguous");
    TORCH_CHECK(sk.numel() == Hq, "sinks must have one entry per q head (",
                Hq, "), got ", sk.numel());
    sinks_p = sk.data_ptr<float>();
  }
  const bool local = window > 0 || sinks_p != nullptr;
  const int bt_stride = block_tables.size(1);
  const int n_tiles = tile_seq.numel();
  if (n_tiles > 0 && local) {
    TORCH_CHECK(tile_rows == 32, "prefill attention with a window or sinks "
                "runs the reference kernel: build the tile lists at 32 rows "
                "(got tile_rows ", tile_rows, ")");
    const int rc = sutro_attn_prefill_local(
        out.data_ptr(), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
        block_tables.data_ptr<int>(), seq_lens.data_ptr<int>(),
        qlocs.data_ptr<int>(), tile_seq.data_ptr<int>(),
        tile_q0.data_ptr<int>(), n_tiles, bt_stride, Hq, Hk, D,
        is_fp8(k_cache) ? 1 : 0, (float)scale, (int)tile_rows, 0,
        (int)window, sinks_p, cur_stream());
    TORCH_CHECK(rc == 0, "prefill attention (window/sinks) refused Hq ", Hq,
                ", Hk ", Hk, ", head_dim ", D);
  } else if (n_tiles > 0) {
    // prefill_variant 0: the one-tile-per-block kernel (32-row tiles);
    // 1: the pipelined kernel, tile lists built at a step of tile_rows
    const int rc = sutro_attn_prefill(
        out.data_ptr(), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
        block_tables.data_ptr<int>(), seq_lens.data_ptr<int>(),
        qlocs.data_ptr<int>(), tile_seq.data_ptr<int>(),
        tile_q0.data_ptr<int>(), n_tiles, bt_stride, Hq, Hk, D,
        is_fp8(k_cache) ? 1 : 0, (float)scale, (int)tile_rows,
        (int)prefill_variant, cur_stream());
    TORCH_CHECK(rc != -2, "pipelined prefill attention: the LDS size was "
                "refused or the launch failed");
    TORCH_CHECK(rc == 0, "prefill attention variant ", prefill_variant,
                " does not take tile_rows ", tile_rows, " with Hq ", Hq,
                ", Hk ", Hk, ", head_dim ", D);
  }
  if (num_decodes > 0) {
    const long dec_off = prefill_token_count;  // decode rows are the tail
    const int seq_offset = S - (int)num_decodes;
    const u_int16_t* qp = (const u_int16_t*)q.data_ptr();
    u_int16_t* op = (u_int16_t*)out.data_ptr();
    if (local) {
      const int rc = sutro_attn_decode_local(
          op + dec_off * Hq * D, qp + dec_off * Hq * D, k_cache.data_ptr(),
          v_cache.data_ptr(), block_tables.data_ptr<int>(),
          seq_lens.data_ptr<int>(), bt_stride, (int)num_decodes, Hq, Hk, D,
          is_fp8(k_cache) ? 1 : 0, seq_offset, (float)scale, (int)window,
          sinks_p, cur_stream());
      TORCH_CHECK(rc == 0, "decode attention with a window or sinks needs "
                  "the MFMA kernel, but SUTRO_DECODE_VALU routes this call "
                  "to the VALU kernel, which has neither");
      return;
    }
    sutro_attn_decode(op + dec_off * Hq * D, qp + dec_off * Hq * D,
                      k_cache.data_ptr(), v_cache.data_ptr(),
                      block_tables.data_ptr<int>(), seq_lens.data_ptr<int>(),
                      bt_stride, (int)num_decodes, Hq, Hk, D,
                      is_fp8(k_cache) ? 1 : 0, seq_offset, (float)scale,
                      cur_stream());
  }
}

// decode-only paged attention with shared-prefix tiles (attn_decode_prefix.hip)
void paged_attention_decode_shared(
    torch::Tensor out, torch::Tensor q, torch::Tensor k_cache,
    torch::Tensor v_cache, torch::Tensor block_tables, torch::Tensor seq_lens,
    double scale, torch::Tensor row_prefix_pages, torch::Tensor tile_rows,
    torch::Tensor part_o, torch::Tensor part_m, torch::Tensor part_l) {
  CHECK_CUDA(q); CHECK_CONTIG(q); CHECK_BF16(q); CHECK_CONTIG(k_cache);
  CHECK_CONTIG(out); CHECK_CONTIG(v_cache); CHECK_CONTIG(block_tables);
  CHECK_CONTIG(row_prefix_pages); CHECK_CONTIG(tile_rows);
  CHECK_CONTIG(part_o); CHECK_CONTIG(part_m); CHECK_CONTIG(part_l);
  const int n = q.size(0), Hq = q.size(1), D = q.size(2);
  const int Hk = k_cache.size(1);
  TORCH_CHECK(D == 128 || D == 64,
              "shared-prefix decode supports head_dim 64/128 (got ", D, ")");
  TORCH_CHECK(k_cache.size(2) == 32, "attention kernels require kv_block_size 32");
  TORCH_CHECK(Hq % Hk == 0 && Hq / Hk <= 8,
              "GQA group size must divide and be <= 8");
  TORCH_CHECK(block_tables.scalar_type() == at::kInt &&
              seq_lens.scalar_type() == at::kInt &&
              row_prefix_pages.scalar_type() == at::kInt &&
              tile_rows.scalar_type() == at::kInt, "index tensors must be int32");
  TORCH_CHECK(block_tables.size(0) >= n && seq_lens.numel() >= n &&
              row_prefix_pages.numel() >= n, "per-row tensors shorter than q");
  TORCH_CHECK(tile_rows.dim() == 2 &&
              tile_rows.size(1) == sutro_attn_prefix_tile_rows(Hq, Hk),
              "tile_rows must be [NT, ", sutro_attn_prefix_tile_rows(Hq, Hk), "]");
  TORCH_CHECK(part_o.scalar_type() == at::kFloat &&
              part_m.scalar_type() == at::kFloat &&
              part_l.scalar_type() == at::kFloat, "partial buffers must be f32");
  TORCH_CHECK(part_o.numel() >= (int64_t)n * Hq * D &&
              part_m.numel() >= (int64_t)n * Hq &&
              part_l.numel() >= (int64_t)n * Hq, "partial buffers too small");
  sutro_attn_decode_shared(
      out.data_ptr(), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
      block_tables.data_ptr<int>(), seq_lens.data_ptr<int>(),
      (int)block_tables.size(1), n, Hq, Hk, (float)scale,
      is_fp8(k_cache) ? 1 : 0, D, row_prefix_pages.data_ptr<int>(),
      tile_rows.data_ptr<int>(), (int)tile_rows.size(0),
      (int)tile_rows.size(1), part_o.data_ptr<float>(),
      part_m.data_ptr<float>(), part_l.data_ptr<float>(), cur_stream());
}

int64_t prefix_tile_rows(int64_t Hq, int64_t Hk) {
  return sutro_attn_prefix_tile_rows((int)Hq, (int)Hk);
}

void qkv_prep(torch::Tensor qkv, torch::Tensor q_out, torch::Tensor k_cache,
              torch::Tensor v_cache, torch::Tensor positions,
              torch::Tensor slot_mapping, torch::Tensor cos_sin,
              c10::optional<torch::Tensor> q_norm_w,
              c10::optional<torch::Tensor> k_norm_w, double eps) {
  CHECK_CUDA(qkv); CHECK_CONTIG(qkv); CHECK_BF16(qkv);
  CHECK_CONTIG(q_out); CHECK_CONTIG(k_cache); CHECK_CONTIG(v_cache);
  const int T = qkv.size(0);
  const int Hq = q_out.size(1), D = q_out.size(2);
  const int Hk = k_cache.size(1);
  const int bs = k_cache.size(2);
  const int row_stride = qkv.size(1);
  TORCH_CHECK(row_stride == Hq * D + 2 * Hk * D, "qkv width mismatch");
  const void* qw = q_norm_w ? q_norm_w->data_ptr() : nullptr;
  const void* kw = k_norm_w ? k_norm_w->data_ptr() : nullptr;
  sutro_qkv_prep(qkv.data_ptr(), q_out.data_ptr(), k_cache.data_ptr(),
                 v_cache.data_ptr(), positions.data_ptr<long>(),
                 slot_mapping.data_ptr<long>(), cos_sin.data_ptr<float>(), qw,
                 kw, (float)eps, T, Hq, Hk, D, bs, row_stride,
                 is_fp8(k_cache) ? 1 : 0, cur_stream());
}

// out[M,N] = x[M,K] @ w[N,K]^T (+ res), bf16 in/out, fp32 accumulate.
// bm/bn pick the macro-tile; M%bm==0 and K%64==0 required (caller falls back
// to torch.mm otherwise). res, when given, is added to the output (fused
// residual epilogue).
torch::Tensor gemm_tn(torch::Tensor x, torch::Tensor w,
                      c10::optional<torch::Tensor> res, long bm, long bn,
                      long swz, long xcd_swz) {
  CHECK_CUDA(x); CHECK_BF16(x); CHECK_CUDA(w); CHECK_BF16(w);
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous(), "contiguous required");
  const long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "K mismatch");
  TORCH_CHECK(M % bm == 0 && K % 64 == 0, "shape not tile-divisible");
  auto out = torch::empty({M, N}, x.options());
  const void* rp = nullptr;
  if (res.has_value()) {
    CHECK_CUDA(*res); CHECK_BF16(*res);
    TORCH_CHECK(res->is_contiguous() && res->size(0) == M && res->size(1) == N,
                "res shape");
    rp = res->data_ptr();
  }
  sutro_gemm_tn_launch(out.data_ptr(), x.data_ptr(), w.data_ptr(), rp, (int)M,
                       (int)N, K, (int)bm, (int)bn, (int)swz, (int)xcd_swz,
                       cur_stream());
  return out;
}

// gemm_tn on the 8-phase pipelined kernel (csrc/gemm_tn_pipe.hip): 256x256
// tile, any M >= 1 and N >= 1 (edges clamped on load, guarded on store),
// K%64==0. Bit-identical to gemm_tn at the same swz / xcd_swz.
torch::Tensor gemm_tn_pipelined(torch::Tensor x, torch::Tensor w,
                                c10::optional<torch::Tensor> res, long swz,
                                long xcd_swz) {
  CHECK_CUDA(x); CHECK_BF16(x); CHECK_CUDA(w); CHECK_BF16(w);
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2, "x and w must be 2-d");
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous(), "contiguous required");
  const long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "K mismatch");
  TORCH_CHECK(M >= 1 && N >= 1 && K >= 64 && K % 64 == 0,
              "shape not tile-divisible");
  TORCH_CHECK(M < (1L << 31) && N < (1L << 31), "M/N too large");
  TORCH_CHECK(swz >= 0 && swz <= 2, "swz must be 0, 1 or 2");
  auto out = torch::empty({M, N}, x.options());
  const void* rp = nullptr;
  if (res.has_value()) {
    CHECK_CUDA(*res); CHECK_BF16(*res);
    TORCH_CHECK(res->is_contiguous() && res->dim() == 2 &&
                res->size(0) == M && res->size(1) == N, "res shape");
    rp = res->data_ptr();
  }
  const int e = sutro_gemm_tn_pipe_launch(
      out.data_ptr(), x.data_ptr(), w.data_ptr(), rp, (int)M, (int)N, K,
      rp ? 1 : 0, (int)swz, (int)xcd_swz, cur_stream());
  TORCH_CHECK(e == 0, "gemm_tn_pipelined launch setup failed: ", e);
  return out;
}

// out[M,I] = silu(x @ w[:I]^T) * (x @ w[I:]^T) on the merged gate_up weight
// w [2I, K] (gate rows first), fused into the pipelined GEMM's epilogue.
// Both products are rounded to bf16 before the activation, so the result
// equals gemm_tn_pipelined followed by silu_mul bit for bit.
// variant 0: one tile per block; 1: the persistent kernel (K % 128 == 0) on
// num_blocks blocks (0 = one per CU, -1 = one per tile), wide = dwordx4
// epilogue stores.
// group_m > 0 numbers the tiles in groups of that many M-tiles, group_m < 0
// gives each XCD a band of M-tiles walked in groups of -group_m (both
// variants). Every combination returns the same bits; the defaults are the
// one-tile kernel in its plain order.
torch::Tensor gemm_gate_up_silu(torch::Tensor x, torch::Tensor w, long swz,
                                long xcd_swz, long variant, long group_m,
                                long num_blocks, bool wide) {
  CHECK_CUDA(x); CHECK_BF16(x); CHECK_CUDA(w); CHECK_BF16(w);
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2, "x and w must be 2-d");
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous(), "contiguous required");
  const long M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "K mismatch");
  TORCH_CHECK(M >= 1 && K >= 64 && K % 64 == 0, "shape not tile-divisible");
  TORCH_CHECK(N >= 256 && N % 256 == 0,
              "gate_up rows must be 2*I with I % 128 == 0");
  TORCH_CHECK(M < (1L << 31) && N < (1L << 31), "M/N too large");
  TORCH_CHECK(swz >= 0 && swz <= 2, "swz must be 0, 1 or 2");
  TORCH_CHECK(variant == 0 || variant == 1,
              "variant must be 0 (one tile per block) or 1 (persistent)");
  TORCH_CHECK(group_m > -(1L << 24) && group_m < (1L << 24),
              "group_m out of range");
  TORCH_CHECK(group_m >= 0 || xcd_swz != 0,
              "the banded tile order (group_m < 0) needs xcd_swz");
  TORCH_CHECK(num_blocks >= -1 && num_blocks <= (1L << 20),
              "num_blocks out of range");
  TORCH_CHECK(((M + 255) / 256) * (N / 256) < (1L << 31), "too many tiles");
  if (variant == 1) {
    TORCH_CHECK(K % 128 == 0 && K <= (1L << 23),
                "the persistent gate_up kernel needs K % 128 == 0 (got K = ",
                K, "); use variant 0");
  } else {
    TORCH_CHECK(num_blocks == 0 && !wide,
                "num_blocks / wide apply to the persistent variant only");
  }
  auto out = torch::empty({M, N / 2}, x.options());
  const int e = sutro_gemm_tn_pipe_launch(
      out.data_ptr(), x.data_ptr(), w.data_ptr(), nullptr, (int)M, (int)N, K,
      2, (int)swz, (int)xcd_swz, cur_stream(), (int)variant, (int)group_m,
      (int)num_blocks, wide ? 1 : 0);
  TORCH_CHECK(e == 0, "gemm_gate_up_silu launch setup failed: ", e);
  return out;
}

// shared operand checks of the two FP8 dense GEMM bindings
static void check_fp8_gemm_args(const torch::Tensor& a_q,
                                const torch::Tensor& a_scale,
                                const torch::Tensor& w_q,
                                const torch::Tensor& w_scale) {
  CHECK_CUDA(a_q); CHECK_CONTIG(a_q); CHECK_CUDA(w_q); CHECK_CONTIG(w_q);
  TORCH_CHECK(is_fp8(a_q) && is_fp8(w_q), "a_q, w_q must be float8_e4m3fn");
  CHECK_CUDA(a_scale); CHECK_CONTIG(a_scale);
  CHECK_CUDA(w_scale); CHECK_CONTIG(w_scale);
  TORCH_CHECK(a_scale.scalar_type() == at::kFloat
              && w_scale.scalar_type() == at::kFloat, "scales must be f32");
  TORCH_CHECK(a_q.dim() == 2 && w_q.dim() == 2, "a_q and w_q must be 2-d");
  const long M = a_q.size(0), Kp = a_q.size(1), N = w_q.size(0);
  TORCH_CHECK(w_q.size(1) == Kp, "Kp mismatch");
  TORCH_CHECK(M >= 1 && Kp >= 128 && Kp % 128 == 0,
              "needs M >= 1 and Kp a positive multiple of 128 (Kp=", Kp, ")");
  // the kernel rounds M and N up to the 256 tile in int
  TORCH_CHECK(M <= (1L << 31) - 256 && N <= (1L << 31) - 256,
              "M/N too large");
  TORCH_CHECK(a_scale.numel() == M, "a_scale must be [M]");
  TORCH_CHECK(w_scale.numel() == N, "w_scale must be [N]");
}

// out[M,N] bf16 = (a_q[M,Kp] @ w_q[N,Kp]^T) * a_scale[m] * w_scale[n]
// (+ res, added in f32 before the one rounding) on the 8-phase pipelined
// block-scaled MFMA kernel (csrc/gemm_tn_fp8_pipe.hip). Any M >= 1,
// N % 64 == 0, Kp % 128 == 0.
torch::Tensor gemm_fp8_pipelined(torch::Tensor a_q, torch::Tensor a_scale,
                                 torch::Tensor w_q, torch::Tensor w_scale,
                                 c10::optional<torch::Tensor> res,
                                 long xcd_swz) {
  check_fp8_gemm_args(a_q, a_scale, w_q, w_scale);
  const long M = a_q.size(0), Kp = a_q.size(1), N = w_q.size(0);
  TORCH_CHECK(N >= 64 && N % 64 == 0, "N must be a multiple of 64 (N=", N, ")");
  auto out = torch::empty({M, N}, a_q.options().dtype(at::kBFloat16));
  const void* rp = nullptr;
  if (res.has_value()) {
    CHECK_CUDA(*res); CHECK_BF16(*res);
    TORCH_CHECK(res->is_contiguous() && res->dim() == 2 &&
                res->size(0) == M && res->size(1) == N, "res shape");
    rp = res->data_ptr();
  }
  const int e = sutro_gemm_tn_fp8_pipe_launch(
      out.data_ptr(), a_q.data_ptr(), a_scale.data_ptr<float>(),
      w_q.data_ptr(), w_scale.data_ptr<float>(), rp, (int)M, (int)N, Kp,
      rp ? 1 : 0, (int)xcd_swz, cur_stream());
  TORCH_CHECK(e == 0, "gemm_fp8_pipelined launch setup failed: ", e);
  return out;
}

// out[M,I] = silu(g) * u, g / u the scaled products with the gate / up rows
// of the merged w_q [2I, Kp]; f32 SwiGLU with one rounding (the grouped FP8
// kernel's epilogue). I % 128 == 0.
torch::Tensor gemm_fp8_gate_up_silu(torch::Tensor a_q, torch::Tensor a_scale,
                                    torch::Tensor w_q, torch::Tensor w_scale,
                                    long xcd_swz) {
  check_fp8_gemm_args(a_q, a_scale, w_q, w_scale);
  const long M = a_q.size(0), Kp = a_q.size(1), N = w_q.size(0);
  TORCH_CHECK(N >= 256 && N % 256 == 0,
              "gate_up rows must be 2*I with I % 128 == 0");
  auto out = torch::empty({M, N / 2}, a_q.options().dtype(at::kBFloat16));
  const int e = sutro_gemm_tn_fp8_pipe_launch(
      out.data_ptr(), a_q.data_ptr(), a_scale.data_ptr<float>(),
      w_q.data_ptr(), w_scale.data_ptr<float>(), nullptr, (int)M, (int)N, Kp,
      2, (int)xcd_swz, cur_stream());
  TORCH_CHECK(e == 0, "gemm_fp8_gate_up_silu launch setup failed: ", e);
  return out;
}

// bf16 [R, K] -> (e4m3 codes [R, K], f32 scales [K/128, R]): one scale per
// row and group of 128 K elements, K-block-major
// (csrc/gemm_tn_fp8_block_pipe.hip). K % 128 == 0.
std::vector<torch::Tensor> quant_rows_fp8_block128(torch::Tensor x) {
  CHECK_CUDA(x); CHECK_CONTIG(x); CHECK_BF16(x);
  TORCH_CHECK(x.dim() == 2, "x must be 2-d");
  const long R = x.size(0), K = x.size(1);
  TORCH_CHECK(K >= 128 && K % 128 == 0,
              "K must be a positive multiple of 128 (K=", K, ")");
  auto q = torch::empty({R, K}, x.options().dtype(at::kFloat8_e4m3fn));
  auto s = torch::empty({K / 128, R}, x.options().dtype(at::kFloat));
  sutro_quant_rows_fp8_block128(q.data_ptr(), s.data_ptr<float>(),
                                x.data_ptr(), R, K, R, cur_stream());
  return {q, s};
}

// shared operand checks of the two block-scaled FP8 dense GEMM bindings:
// a_q [M, K] e4m3 + a_s [K/128, M] f32 (rows may be strided), w_q [N, K]
// e4m3 + w_s [N/128, K/128] f32
static void check_fp8_block_gemm_args(const torch::Tensor& a_q,
                                      const torch::Tensor& a_s,
                                      const torch::Tensor& w_q,
                                      const torch::Tensor& w_s) {
  CHECK_CUDA(a_q); CHECK_CONTIG(a_q); CHECK_CUDA(w_q); CHECK_CONTIG(w_q);
  TORCH_CHECK(is_fp8(a_q) && is_fp8(w_q), "a_q, w_q must be float8_e4m3fn");
  CHECK_CUDA(a_s); CHECK_CUDA(w_s); CHECK_CONTIG(w_s);
  TORCH_CHECK(a_s.scalar_type() == at::kFloat
              && w_s.scalar_type() == at::kFloat, "scales must be f32");
  TORCH_CHECK(a_q.dim() == 2 && w_q.dim() == 2 && a_s.dim() == 2
              && w_s.dim() == 2, "a_q, a_s, w_q and w_s must be 2-d");
  const long M = a_q.size(0), K = a_q.size(1), N = w_q.size(0);
  TORCH_CHECK(w_q.size(1) == K, "K mismatch");
  TORCH_CHECK(M >= 1 && K >= 128 && K % 128 == 0,
              "needs M >= 1 and K a positive multiple of 128 (K=", K, ")");
  TORCH_CHECK(N >= 128 && N % 128 == 0,
              "N must be a positive multiple of 128 (N=", N, ")");
  // the kernel rounds M and N up to the 256 tile in int
  TORCH_CHECK(M <= (1L << 31) - 256 && N <= (1L << 31) - 256,
              "M/N too large");
  TORCH_CHECK(a_s.size(0) == K / 128 && a_s.size(1) == M,
              "a_s must be [K/128, M]");
  // (a dimension of size 1 carries no meaningful stride)
  TORCH_CHECK((M == 1 || a_s.stride(1) == 1)
              && (K == 128 || a_s.stride(0) >= M), "a_s rows must be dense");
  TORCH_CHECK(w_s.size(0) == N / 128 && w_s.size(1) == K / 128,
              "w_s must be [N/128, K/128]");
}

// out[M,N] bf16 = sum_kb (a_q[:, kb] @ w_q[:, kb]^T) * a_s[kb, m]
// * w_s[n/128, kb] (+ res, added in f32 before the one rounding) on the
// 8-phase pipelined kernel with the scales folded in per K-tile
// (csrc/gemm_tn_fp8_block_pipe.hip). Any M >= 1, N % 128 == 0, K % 128 == 0.
torch::Tensor gemm_fp8_block_pipelined(torch::Tensor a_q, torch::Tensor a_s,
                                       torch::Tensor w_q, torch::Tensor w_s,
                                       c10::optional<torch::Tensor> res,
                                       long xcd_swz) {
  check_fp8_block_gemm_args(a_q, a_s, w_q, w_s);
  const long M = a_q.size(0), K = a_q.size(1), N = w_q.size(0);
  auto out = torch::empty({M, N}, a_q.options().dtype(at::kBFloat16));
  const void* rp = nullptr;
  if (res.has_value()) {
    CHECK_CUDA(*res); CHECK_BF16(*res);
    TORCH_CHECK(res->is_contiguous() && res->dim() == 2 &&
                res->size(0) == M && res->size(1) == N, "res shape");
    rp = res->data_ptr();
  }
  const int e = sutro_gemm_tn_fp8_block_pipe_launch(
      out.data_ptr(), a_q.data_ptr(), a_s.data_ptr<float>(),
      K == 128 ? M : a_s.stride(0), w_q.data_ptr(), w_s.data_ptr<float>(), rp,
      (int)M, (int)N, K, rp ? 1 : 0, (int)xcd_swz, cur_stream());
  TORCH_CHECK(e == 0, "gemm_fp8_block_pipelined launch setup failed: ", e);
  return out;
}

// out[M,I] = silu(g) * u, g / u the block-scaled products with the gate / up
// rows of the merged w_q [2I, K]; f32 SwiGLU with one rounding. I % 128 == 0.
torch::Tensor gemm_fp8_block_gate_up_silu(torch::Tensor a_q,
                                          torch::Tensor a_s,
                                          torch::Tensor w_q,
                                          torch::Tensor w_s, long xcd_swz) {
  check_fp8_block_gemm_args(a_q, a_s, w_q, w_s);
  const long M = a_q.size(0), K = a_q.size(1), N = w_q.size(0);
  TORCH_CHECK(N >= 256 && N % 256 == 0,
              "gate_up rows must be 2*I with I % 128 == 0");
  auto out = torch::empty({M, N / 2}, a_q.options().dtype(at::kBFloat16));
  const int e = sutro_gemm_tn_fp8_block_pipe_launch(
      out.data_ptr(), a_q.data_ptr(), a_s.data_ptr<float>(),
      K == 128 ? M : a_s.stride(0), w_q.data_ptr(), w_s.data_ptr<float>(),
      nullptr, (int)M, (int)N, K, 2, (int)xcd_swz, cur_stream());
  TORCH_CHECK(e == 0, "gemm_fp8_block_gate_up_silu launch setup failed: ", e);
  return out;
}

torch::Tensor mfma32_probe(torch::Tensor a, torch::Tensor b) {
  CHECK_CUDA(a); CHECK_BF16(a);
  auto c = torch::zeros({32, 32}, a.options().dtype(at::kFloat));
  sutro_mfma32_probe(c.data_ptr<float>(), a.data_ptr(), b.data_ptr(),
                     cur_stream());
  return c;
}

std::vector<torch::Tensor> hd64_stage_probe(torch::Tensor q, torch::Tensor k,
                                             torch::Tensor v, long L,
                                             double scale) {
  CHECK_CUDA(q); CHECK_BF16(q);
  auto fopt = q.options().dtype(at::kFloat);
  auto vt = torch::zeros({64 * 40}, fopt);
  auto p = torch::zeros({16 * 40}, fopt);
  auto out = torch::zeros({1, 64}, q.options());
  sutro_hd64_stage_probe(vt.data_ptr<float>(), p.data_ptr<float>(),
                         out.data_ptr(), q.data_ptr(), k.data_ptr(),
                         v.data_ptr(), (int)L, (float)scale, cur_stream());
  return {vt, p, out};
}

torch::Tensor mfma16_probe(torch::Tensor a, torch::Tensor b) {
  CHECK_CUDA(a); CHECK_BF16(a);
  auto c = torch::zeros({16, 16}, a.options().dtype(at::kFloat));
  sutro_mfma16_probe(c.data_ptr<float>(), a.data_ptr(), b.data_ptr(),
                     cur_stream());
  return c;
}

void grouped_gemm(torch::Tensor out, torch::Tensor a, torch::Tensor w,
                  c10::optional<torch::Tensor> row_tok, torch::Tensor tile_off,
                  torch::Tensor counts, long max_tiles, bool gate_silu,
                  long bm) {
  TORCH_CHECK(bm == 64 || bm == 128, "bm must be 64 or 128");
  CHECK_CUDA(a); CHECK_CONTIG(a); CHECK_BF16(a);
  CHECK_CUDA(w); CHECK_CONTIG(w); CHECK_BF16(w);
  CHECK_CONTIG(out); CHECK_BF16(out);
  const long E = w.size(0), N = w.size(1), K = w.size(2);
  const long n_cols = gate_silu ? N / 2 : N;
  TORCH_CHECK(K % 64 == 0 && n_cols % 64 == 0,
              "grouped_gemm needs K, n_cols multiples of 64 (K=", K,
              ", n_cols=", n_cols, ")");
  TORCH_CHECK(a.size(1) == K, "A K mismatch");
  TORCH_CHECK(out.size(1) == n_cols, "out width mismatch");
  TORCH_CHECK(tile_off.scalar_type() == at::kInt
              && counts.scalar_type() == at::kInt, "tile_off/counts int32");
  TORCH_CHECK(tile_off.numel() == E + 1 && counts.numel() == E, "seg sizes");
  const int* rt = nullptr;
  if (row_tok.has_value()) {
    TORCH_CHECK(row_tok->scalar_type() == at::kInt, "row_tok int32");
    rt = row_tok->data_ptr<int>();
  }
  sutro_grouped_gemm(out.data_ptr(), a.data_ptr(), w.data_ptr(), rt,
                     tile_off.data_ptr<int>(), counts.data_ptr<int>(), (int)E,
                     (int)max_tiles, (int)n_cols, K, gate_silu ? 1 : 0,
                     (int)bm, cur_stream());
}

// bf16 [R, K] -> e4m3 [R, Kp] + f32 scale [R] (Kp = K rounded up to 128, zero
// tail). row_limit (int32 device scalar) * limit_mul bounds the rows written.
void quant_rows_fp8(torch::Tensor x, torch::Tensor out_q,
                    torch::Tensor out_scale,
                    c10::optional<torch::Tensor> row_limit, long limit_mul) {
  CHECK_CUDA(x); CHECK_CONTIG(x); CHECK_BF16(x);
  CHECK_CUDA(out_q); CHECK_CONTIG(out_q);
  CHECK_CUDA(out_scale); CHECK_CONTIG(out_scale);
  TORCH_CHECK(x.dim() == 2 && out_q.dim() == 2, "x, out_q must be 2-D");
  TORCH_CHECK(is_fp8(out_q), "out_q must be float8_e4m3fn");
  TORCH_CHECK(out_scale.scalar_type() == at::kFloat, "out_scale must be f32");
  const long R = x.size(0), K = x.size(1), Kp = out_q.size(1);
  TORCH_CHECK(K % 8 == 0 && K > 0, "K must be a positive multiple of 8");
  TORCH_CHECK(Kp == (K + 127) / 128 * 128, "out_q width must be K rounded "
              "up to 128 (K=", K, ", Kp=", Kp, ")");
  TORCH_CHECK(Kp < (1L << 31), "row too wide");
  TORCH_CHECK(out_q.size(0) >= R && out_scale.numel() >= R,
              "out_q/out_scale hold fewer rows than x");
  const int* lim = nullptr;
  if (row_limit.has_value()) {
    CHECK_CUDA(*row_limit);
    TORCH_CHECK(row_limit->scalar_type() == at::kInt
                && row_limit->numel() >= 1, "row_limit int32 scalar");
    lim = row_limit->data_ptr<int>();
  }
  sutro_quant_rows_fp8(out_q.data_ptr(), out_scale.data_ptr<float>(),
                       x.data_ptr(), lim, (int)limit_mul, R, (int)K, (int)Kp,
                       cur_stream());
}

void grouped_gemm_fp8(torch::Tensor out, torch::Tensor a_q,
                      torch::Tensor a_scale, torch::Tensor w_q,
                      torch::Tensor w_scale,
                      c10::optional<torch::Tensor> row_tok,
                      torch::Tensor tile_off, torch::Tensor counts,
                      long max_tiles, bool gate_silu, long bm) {
  TORCH_CHECK(bm == 64 || bm == 128, "bm must be 64 or 128");
  CHECK_CUDA(a_q); CHECK_CONTIG(a_q); CHECK_CUDA(w_q); CHECK_CONTIG(w_q);
  TORCH_CHECK(is_fp8(a_q) && is_fp8(w_q), "a_q, w_q must be float8_e4m3fn");
  CHECK_CUDA(a_scale); CHECK_CONTIG(a_scale);
  CHECK_CUDA(w_scale); CHECK_CONTIG(w_scale);
  TORCH_CHECK(a_scale.scalar_type() == at::kFloat
              && w_scale.scalar_type() == at::kFloat, "scales must be f32");
  CHECK_CUDA(out); CHECK_CONTIG(out); CHECK_BF16(out);
  TORCH_CHECK(w_q.dim() == 3 && a_q.dim() == 2 && out.dim() == 2, "ranks");
  const long E = w_q.size(0), N = w_q.size(1), Kp = w_q.size(2);
  const long n_cols = gate_silu ? N / 2 : N;
  TORCH_CHECK(Kp % 128 == 0 && Kp > 0 && n_cols % 64 == 0 && n_cols > 0,
              "grouped_gemm_fp8 needs Kp a multiple of 128 and n_cols of 64 "
              "(Kp=", Kp, ", n_cols=", n_cols, ")");
  TORCH_CHECK(a_q.size(1) == Kp, "A Kp mismatch");
  TORCH_CHECK(out.size(1) == n_cols, "out width mismatch");
  TORCH_CHECK(max_tiles >= 0 && out.size(0) >= max_tiles * bm,
              "out holds fewer rows than max_tiles * bm");
  TORCH_CHECK(w_scale.numel() == E * N, "w_scale must be [E, N]");
  TORCH_CHECK(tile_off.scalar_type() == at::kInt
              && counts.scalar_type() == at::kInt, "tile_off/counts int32");
  TORCH_CHECK(tile_off.numel() == E + 1 && counts.numel() == E, "seg sizes");
  const int* rt = nullptr;
  if (row_tok.has_value()) {
    TORCH_CHECK(row_tok->scalar_type() == at::kInt, "row_tok int32");
    TORCH_CHECK(row_tok->numel() >= max_tiles * bm, "row_tok too short");
    rt = row_tok->data_ptr<int>();
  } else {
    TORCH_CHECK(a_q.size(0) >= max_tiles * bm,
                "a_q holds fewer rows than max_tiles * bm");
  }
  TORCH_CHECK(!gate_silu || rt, "the gate/up stage gathers through row_tok");
  TORCH_CHECK(a_scale.numel() >= a_q.size(0), "a_scale shorter than a_q");
  sutro_grouped_gemm_fp8(out.data_ptr(), a_q.data_ptr(),
                         a_scale.data_ptr<float>(), w_q.data_ptr(),
                         w_scale.data_ptr<float>(), rt,
                         tile_off.data_ptr<int>(), counts.data_ptr<int>(),
                         (int)E, (int)max_tiles, (int)n_cols, Kp,
                         gate_silu ? 1 : 0, (int)bm, cur_stream());
}

// bf16 [R, K] -> MXFP4: e2m1 codes u8 [R, Kp/2] (two per byte, low nibble
// first) + e8m0 block scales u8 [R, Kp/32]; Kp = K rounded up to 128.
void quant_weight_mxfp4(torch::Tensor x, torch::Tensor out_q,
                        torch::Tensor out_scale) {
  CHECK_CUDA(x); CHECK_CONTIG(x); CHECK_BF16(x);
  CHECK_CUDA(out_q); CHECK_CONTIG(out_q);
  CHECK_CUDA(out_scale); CHECK_CONTIG(out_scale);
  TORCH_CHECK(x.dim() == 2 && out_q.dim() == 2 && out_scale.dim() == 2,
              "x, out_q, out_scale must be 2-D");
  TORCH_CHECK(out_q.scalar_type() == at::kByte
              && out_scale.scalar_type() == at::kByte,
              "out_q, out_scale must be uint8");
  const long R = x.size(0), K = x.size(1);
  TORCH_CHECK(K % 8 == 0 && K > 0, "K must be a positive multiple of 8");
  const long Kp = (K + 127) / 128 * 128;
  TORCH_CHECK(Kp < (1L << 31), "row too wide");
  TORCH_CHECK(out_q.size(1) == Kp / 2 && out_scale.size(1) == Kp / 32,
              "out_q / out_scale widths must be Kp/2 and Kp/32 with Kp = K "
              "rounded up to 128 (K=", K, ", Kp=", Kp, ")");
  TORCH_CHECK(out_q.size(0) == R && out_scale.size(0) == R,
              "out_q/out_scale rows differ from x");
  sutro_quant_weight_mxfp4(out_q.data_ptr(), out_scale.data_ptr(),
                           x.data_ptr(), R, (int)K, (int)Kp, cur_stream());
}

void grouped_gemm_mxfp4(torch::Tensor out, torch::Tensor a_q,
                        torch::Tensor a_scale, torch::Tensor w_q,
                        torch::Tensor w_scale,
                        c10::optional<torch::Tensor> row_tok,
                        torch::Tensor tile_off, torch::Tensor counts,
                        long max_tiles, bool gate_silu, long bm) {
  TORCH_CHECK(bm == 64 || bm == 128, "bm must be 64 or 128");
  CHECK_CUDA(a_q); CHECK_CONTIG(a_q); CHECK_CUDA(w_q); CHECK_CONTIG(w_q);
  TORCH_CHECK(is_fp8(a_q), "a_q must be float8_e4m3fn");
  CHECK_CUDA(a_scale); CHECK_CONTIG(a_scale);
  CHECK_CUDA(w_scale); CHECK_CONTIG(w_scale);
  TORCH_CHECK(a_scale.scalar_type() == at::kFloat, "a_scale must be f32");
  TORCH_CHECK(w_q.scalar_type() == at::kByte
              && w_scale.scalar_type() == at::kByte,
              "w_q (e2m1 pairs) and w_scale (e8m0) must be uint8");
  CHECK_CUDA(out); CHECK_CONTIG(out); CHECK_BF16(out);
  TORCH_CHECK(w_q.dim() == 3 && w_scale.dim() == 3 && a_q.dim() == 2
              && out.dim() == 2, "ranks");
  const long E = w_q.size(0), N = w_q.size(1), Kp = w_q.size(2) * 2;
  const long n_cols = gate_silu ? N / 2 : N;
  TORCH_CHECK(Kp % 128 == 0 && Kp > 0 && n_cols % 64 == 0 && n_cols > 0,
              "grouped_gemm_mxfp4 needs Kp a multiple of 128 and n_cols of 64 "
              "(Kp=", Kp, ", n_cols=", n_cols, ")");
  TORCH_CHECK(!gate_silu || N == 2 * n_cols, "gate/up needs an even N");
  TORCH_CHECK(a_q.size(1) == Kp, "A Kp mismatch");
  TORCH_CHECK(out.size(1) == n_cols, "out width mismatch");
  TORCH_CHECK(max_tiles >= 0 && out.size(0) >= max_tiles * bm,
              "out holds fewer rows than max_tiles * bm");
  TORCH_CHECK(w_scale.size(0) == E && w_scale.size(1) == N
              && w_scale.size(2) == Kp / 32, "w_scale must be [E, N, Kp/32]");
  TORCH_CHECK(tile_off.scalar_type() == at::kInt
              && counts.scalar_type() == at::kInt, "tile_off/counts int32");
  TORCH_CHECK(tile_off.numel() == E + 1 && counts.numel() == E, "seg sizes");
  const int* rt = nullptr;
  if (row_tok.has_value()) {
    TORCH_CHECK(row_tok->scalar_type() == at::kInt, "row_tok int32");
    TORCH_CHECK(row_tok->numel() >= max_tiles * bm, "row_tok too short");
    rt = row_tok->data_ptr<int>();
  } else {
    TORCH_CHECK(a_q.size(0) >= max_tiles * bm,
                "a_q holds fewer rows than max_tiles * bm");
  }
  TORCH_CHECK(!gate_silu || rt, "the gate/up stage gathers through row_tok");
  TORCH_CHECK(a_scale.numel() >= a_q.size(0), "a_scale shorter than a_q");
  sutro_grouped_gemm_mxfp4(out.data_ptr(), a_q.data_ptr(),
                           a_scale.data_ptr<float>(), w_q.data_ptr(),
                           w_scale.data_ptr(), rt,
                           tile_off.data_ptr<int>(), counts.data_ptr<int>(),
                           (int)E, (int)max_tiles, (int)n_cols, Kp,
                           gate_silu ? 1 : 0, (int)bm, cur_stream());
}

void moe_combine(torch::Tensor out, torch::Tensor rows, torch::Tensor padpos,
                 torch::Tensor w) {
  CHECK_CUDA(rows); CHECK_CONTIG(rows); CHECK_BF16(rows);
  CHECK_CONTIG(out); CHECK_BF16(out);
  const long T = out.size(0), h = out.size(1), k = padpos.size(1);
  TORCH_CHECK(h % 8 == 0, "h must be a multiple of 8");
  TORCH_CHECK(padpos.scalar_type() == at::kLong, "padpos must be int64");
  TORCH_CHECK(w.scalar_type() == at::kFloat, "w must be f32");
  TORCH_CHECK(padpos.is_contiguous() && w.is_contiguous(), "contig");
  sutro_moe_combine(out.data_ptr(), rows.data_ptr(),
                    padpos.data_ptr<long>(), w.data_ptr<float>(), (int)T,
                    (int)h, (int)k, cur_stream());
}

void sampler_fused(torch::Tensor logits, torch::Tensor temps,
                   torch::Tensor topps, torch::Tensor topks, torch::Tensor us,
                   c10::optional<torch::Tensor> mask, long vl,
                   torch::Tensor out_tok, torch::Tensor out_lp) {
  CHECK_CUDA(logits); CHECK_CONTIG(logits);
  const bool f32 = logits.scalar_type() == at::kFloat;
  TORCH_CHECK(f32 || logits.scalar_type() == at::kBFloat16,
              "logits must be bf16 or f32");
  const long n = logits.size(0), v_row = logits.size(1);
  TORCH_CHECK(vl <= v_row, "vocab_limit exceeds logits row");
  TORCH_CHECK(temps.numel() >= n && topps.numel() >= n && topks.numel() >= n
              && us.numel() >= n, "param tensors too small");
  TORCH_CHECK(topks.scalar_type() == at::kInt, "topks must be int32");
  const unsigned int* mptr = nullptr;
  int w_words = 0;
  if (mask.has_value()) {
    auto& mt = mask.value();
    CHECK_CUDA(mt); CHECK_CONTIG(mt);
    TORCH_CHECK(mt.scalar_type() == at::kInt, "mask must be int32 packed");
    TORCH_CHECK(mt.size(0) == n, "mask rows mismatch");
    w_words = (int)mt.size(1);
    TORCH_CHECK((long)w_words * 32 >= vl, "mask too narrow for vocab_limit");
    mptr = (const unsigned int*)mt.data_ptr();
  }
  sutro_sampler_fused(logits.data_ptr(), f32 ? 1 : 0,
                      temps.data_ptr<float>(), topps.data_ptr<float>(),
                      topks.data_ptr<int>(), us.data_ptr<float>(), mptr,
                      (int)n, v_row, (int)vl, w_words,
                      out_tok.data_ptr<int>(), out_lp.data_ptr<float>(),
                      cur_stream());
}

// In-place sparse penalties on the rows listed in row_idx (unique rows; one
// workgroup each). max_hist_len is the host's upper bound on hist_len and
// sizes the LDS table; the kernel clamps device-side lengths to what the
// chosen table holds, so a stale bound can drop history but never overflow.
void logit_penalties(torch::Tensor logits, torch::Tensor row_idx,
                     torch::Tensor hist, torch::Tensor slot,
                     torch::Tensor hist_len, torch::Tensor prompt_len,
                     torch::Tensor rep, torch::Tensor pres, torch::Tensor freq,
                     c10::optional<torch::Tensor> bias_tok,
                     c10::optional<torch::Tensor> bias_val, long vl,
                     long max_hist_len) {
  CHECK_CUDA(logits); CHECK_CONTIG(logits);
  const bool f32 = logits.scalar_type() == at::kFloat;
  TORCH_CHECK(f32 || logits.scalar_type() == at::kBFloat16,
              "logits must be bf16 or f32");
  TORCH_CHECK(logits.dim() == 2, "logits must be [n, V]");
  const long n = logits.size(0), v_row = logits.size(1);
  TORCH_CHECK(vl >= 0 && vl <= v_row, "vocab_limit exceeds logits row");
  TORCH_CHECK(v_row < (1L << 31) && n < (1L << 31), "logits too large");
  const long m = row_idx.numel();
  if (m == 0) return;
  auto chk_i32 = [&](const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous()
                && t.scalar_type() == at::kInt && t.numel() == m,
                name, " must be a contiguous int32 GPU tensor of ", m);
  };
  auto chk_f32 = [&](const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.is_contiguous()
                && t.scalar_type() == at::kFloat && t.numel() == m,
                name, " must be a contiguous f32 GPU tensor of ", m);
  };
  chk_i32(row_idx, "row_idx"); chk_i32(slot, "slot");
  chk_i32(hist_len, "hist_len"); chk_i32(prompt_len, "prompt_len");
  chk_f32(rep, "rep"); chk_f32(pres, "pres"); chk_f32(freq, "freq");
  CHECK_CUDA(hist); CHECK_CONTIG(hist);
  TORCH_CHECK(hist.scalar_type() == at::kInt && hist.dim() == 2,
              "hist must be int32 [S, Lcap]");
  const long n_slots = hist.size(0), lcap = hist.size(1);
  TORCH_CHECK(lcap < (1L << 31) && n_slots < (1L << 31), "hist too large");
  long n_bias = 0;
  const int* btp = nullptr;
  const float* bvp = nullptr;
  TORCH_CHECK(bias_tok.has_value() == bias_val.has_value(),
              "bias_tok and bias_val go together");
  if (bias_tok.has_value() && bias_tok->numel() > 0) {
    auto& bt = bias_tok.value();
    auto& bv = bias_val.value();
    CHECK_CUDA(bt); CHECK_CONTIG(bt); CHECK_CUDA(bv); CHECK_CONTIG(bv);
    TORCH_CHECK(bt.scalar_type() == at::kInt && bv.scalar_type() == at::kFloat,
                "bias_tok int32 / bias_val f32");
    TORCH_CHECK(bt.dim() == 2 && bt.size(0) == m && bv.dim() == 2
                && bv.size(0) == m && bv.size(1) == bt.size(1),
                "bias_tok/bias_val must be [m, B]");
    n_bias = bt.size(1);
    TORCH_CHECK(n_bias <= 512, "at most 512 bias entries per row");
    btp = bt.data_ptr<int>();
    bvp = bv.data_ptr<float>();
  }
  TORCH_CHECK(max_hist_len >= 0 && max_hist_len + n_bias <= 8192,
              "hist_len + bias entries above 8192: use the torch reference");
  const long need = 2 * (max_hist_len + n_bias);
  const int log2_cap = need <= 2048 ? 11 : (need <= 8192 ? 13 : 14);
  sutro_logit_penalties(logits.data_ptr(), f32 ? 1 : 0,
                        row_idx.data_ptr<int>(), hist.data_ptr<int>(),
                        slot.data_ptr<int>(), hist_len.data_ptr<int>(),
                        prompt_len.data_ptr<int>(), rep.data_ptr<float>(),
                        pres.data_ptr<float>(), freq.data_ptr<float>(), btp,
                        bvp, (int)m, (int)n, v_row, (int)vl, (int)n_slots,
                        (int)lcap, (int)n_bias, log2_cap, cur_stream());
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm", &rmsnorm, "RMSNorm (bf16, CDNA4)");
  m.def("fused_add_rmsnorm", &fused_add_rmsnorm, "residual+=x; x=rmsnorm",
        py::arg("x"), py::arg("residual"), py::arg("w"), py::arg("eps"),
        py::arg("variant") = 0);
  m.def("silu_mul", &silu_mul, "fused SwiGLU");
  m.def("rope_and_cache", &rope_and_cache, "RoPE + paged KV write");
  m.def("qkv_prep", &qkv_prep, "fused qk-norm + RoPE + KV write + q gather");
  m.def("mean_pool_normalize", &mean_pool_normalize, "varlen mean pool + L2");
  m.def("paged_attention", &paged_attention, "paged prefill+decode attention",
        py::arg("out"), py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("block_tables"), py::arg("seq_lens"), py::arg("qlocs"),
        py::arg("scale"), py::arg("num_decodes"), py::arg("tile_seq"),
        py::arg("tile_q0"), py::arg("prefill_token_count"),
        py::arg("tile_rows") = 32, py::arg("prefill_variant") = 0,
        py::arg("window") = 0, py::arg("sinks") = py::none());
  m.def("attn_prefill_pipe_supported",
        [](int64_t hq, int64_t hk, int64_t d, int64_t rows) {
          return sutro_attn_prefill_pipe_supported((int)hq, (int)hk, (int)d,
                                                   (int)rows) != 0;
        },
        "whether the pipelined prefill kernel takes (Hq, Hk, D, tile_rows)");
  m.def("paged_attention_decode_shared", &paged_attention_decode_shared,
        "decode attention, shared-prefix tiles + per-row continuation");
  m.def("prefix_tile_rows", &prefix_tile_rows,
        "rows per shared-prefix tile for a (Hq, Hk) head layout");
  m.def("mfma32_probe", &mfma32_probe, "MFMA fragment-layout probe");
  m.def("mfma16_probe", &mfma16_probe, "16x16 MFMA fragment-layout probe");
  m.def("hd64_stage_probe", &hd64_stage_probe, "D=64 decode stage dump probe");
  m.def("moe_combine", &moe_combine, "fused MoE weighted gather-combine");
  m.def("grouped_gemm", &grouped_gemm,
        "dropless MoE grouped GEMM (padded segments, static grid)");
  m.def("quant_rows_fp8", &quant_rows_fp8,
        "bf16 rows -> e4m3 codes + f32 per-row scale (K padded to 128)");
  m.def("grouped_gemm_fp8", &grouped_gemm_fp8,
        "dropless MoE grouped GEMM, e4m3 operands on the block-scaled MFMA");
  m.def("quant_weight_mxfp4", &quant_weight_mxfp4,
        "bf16 rows -> e2m1 code pairs + e8m0 scale per 32 (K padded to 128)");
  m.def("grouped_gemm_mxfp4", &grouped_gemm_mxfp4,
        "dropless MoE grouped GEMM, e4m3 x MXFP4 on the block-scaled MFMA");
  m.def("sampler_fused", &sampler_fused,
        "fused mask+temp+topk/topp+sample+logprob (radix descent, no sort)");
  m.def("logit_penalties", &logit_penalties,
        "sparse repetition/presence/frequency penalties + logit_bias "
        "(LDS hash of the row history, in place)");
  m.def("gemm_tn", &gemm_tn, "bf16 TN GEMM (MFMA, glds dbuf)",
        py::arg("x"), py::arg("w"), py::arg("res") = c10::nullopt,
        py::arg("bm") = 256, py::arg("bn") = 256, py::arg("swz") = 2,
        py::arg("xcd_swz") = 0);
  m.def("gemm_tn_pipelined", &gemm_tn_pipelined,
        "bf16 TN GEMM (MFMA, 8-phase glds pipeline, any M/N)",
        py::arg("x"), py::arg("w"), py::arg("res") = c10::nullopt,
        py::arg("swz") = 2, py::arg("xcd_swz") = 1);
  m.def("gemm_gate_up_silu", &gemm_gate_up_silu,
        "SwiGLU fused into the pipelined gate_up GEMM",
        py::arg("x"), py::arg("w"), py::arg("swz") = 2,
        py::arg("xcd_swz") = 1, py::arg("variant") = 0,
        py::arg("group_m") = 0, py::arg("num_blocks") = 0,
        py::arg("wide") = false);
  m.def("gemm_fp8_pipelined", &gemm_fp8_pipelined,
        "e4m3 W8A8 TN GEMM (block-scaled MFMA, 8-phase glds pipeline)",
        py::arg("a_q"), py::arg("a_scale"), py::arg("w_q"),
        py::arg("w_scale"), py::arg("res") = c10::nullopt,
        py::arg("xcd_swz") = 1);
  m.def("gemm_fp8_gate_up_silu", &gemm_fp8_gate_up_silu,
        "SwiGLU fused into the pipelined e4m3 gate_up GEMM",
        py::arg("a_q"), py::arg("a_scale"), py::arg("w_q"),
        py::arg("w_scale"), py::arg("xcd_swz") = 1);
  m.def("quant_rows_fp8_block128", &quant_rows_fp8_block128,
        "bf16 rows -> e4m3 codes + f32 scales per group of 128 K elements",
        py::arg("x"));
  m.def("gemm_fp8_block_pipelined", &gemm_fp8_block_pipelined,
        "e4m3 TN GEMM with 128x128 weight and 1x128 activation scales",
        py::arg("a_q"), py::arg("a_s"), py::arg("w_q"), py::arg("w_s"),
        py::arg("res") = c10::nullopt, py::arg("xcd_swz") = 1);
  m.def("gemm_fp8_block_gate_up_silu", &gemm_fp8_block_gate_up_silu,
        "SwiGLU fused into the block-scaled e4m3 gate_up GEMM",
        py::arg("a_q"), py::arg("a_s"), py::arg("w_q"), py::arg("w_s"),
        py::arg("xcd_swz") = 1);
}
