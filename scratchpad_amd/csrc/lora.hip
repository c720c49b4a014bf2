// LoRA toppings: per-row adapter products of a batch whose rows name different adapters.
//
// Call sites they serve: the topping layers over the four Llama projections (nn/toppings/topping_layer.py:
// ColumnParallelLinearWithTopping 41-70, MergedColumnParallelLinearWithTopping 73-160, QKVParallelLinearWithToppings
// 163-296, RowParallelLinearWithTopping 299-348).  The reference hands the arithmetic to an external package
// (triteia.python.ops.ldmm) that is not part of its tree; its other branches run one masked torch product per adapter
// of the batch.  Here it is two launches per projection (three for qkv), whatever the number of adapters:
//
//   sp_lora_shrink:  tmp[t, :R]           = scale * (x[t, :K] . A[idx[t]])        A[slot]: [K, R],    R = S r
//   sp_lora_expand:  y[t, s n + c]       += tmp[t, s r : (s+1) r] . B[idx[t]][:, s n + c]     B[slot]: [r, S n]
//
// Both buffers keep the reference's layout (memory/topping_pool.py:88-124): the contiguous dimension is R resp. S n,
// and that is the dimension the lanes run along, in 16-byte vectors.
//
// Shrink: a workgroup (256 threads) owns kShrinkRows consecutive rows.  Thread (g, c) takes vector column c (8 of the
// R columns) of the 8-row k-chunks g, g + G, ... (G = 256 / (R / 8) thread groups): per chunk 8 vectors of A and ONE
// 16-byte vector of x per row.  A maximal run of rows with the same adapter shares the A loads.  The G partial sums of
// an output are added through LDS in ascending g.  A[slot] is at most a few hundred KB and lives in L2; the launch is
// latency-bound and there is no LDS pipeline.
//
// Expand: a workgroup owns kExpandRows consecutive rows and 256 vectors (2048 columns) of the S n output columns.  The
// S r values of a row's tmp go through LDS (broadcast reads); per output one fp32 FMA chain over j ascending, then
// y = round(y + chain): one read-modify-write of y in the activation dtype.
//
// BATCH INVARIANCE: the bits a row receives depend on that row's x, y, index and adapter only.  A row's chain of
// operations is the same whichever rows share its workgroup or its run: the k-chunks of a thread, the order inside a
// chunk and the order over g are functions of (K, R) alone, those of expand of r alone, and every product is an
// explicit fmaf.
//
// Safety: an index < 0 or >= num_slots skips the row (nothing of it is read or written); no address is formed from an
// index before that check; slot, row and column offsets are 64-bit.
#include "sp_common.h"

namespace sp {

constexpr int kLoraThreads = 256;
constexpr int kShrinkRows = 4;
constexpr int kExpandRows = 4;
constexpr int kLoraMaxR = 192;

struct ShrinkArgs {
  float* tmp;
  const char* x;
  const char* a;
  const int32_t* idx;
  int T, K, R, num_slots;
  int64_t x_stride, a_slot_stride, tmp_stride;   // elements
  float scale;
};

// slot of every row of the block into LDS: -1 for a row past T or an index outside [0, num_slots)
template <int ROWS>
__device__ __forceinline__ void load_slots(int* s_slot, const int32_t* idx, int64_t row0, int T, int num_slots) {
  if (threadIdx.x < ROWS) {
    const int64_t row = row0 + threadIdx.x;
    int s = -1;
    if (row < T) {
      s = idx[row];
      if (s < 0 || s >= num_slots) s = -1;
    }
    s_slot[threadIdx.x] = s;
  }
}

template <typename Tag>
__global__ __launch_bounds__(kLoraThreads) void lora_shrink_kernel(ShrinkArgs p) {
  __shared__ float red[kShrinkRows][kLoraThreads * 8];
  __shared__ int s_slot[kShrinkRows];
  const int tid = threadIdx.x;
  const int V = p.R >> 3, G = kLoraThreads / V;        // vector columns of A, thread groups along k
  const int g = tid / V, c = tid - g * V;
  const int NC = p.K >> 3;                             // 8-row chunks of k
  const int Gact = min(G, NC);                         // groups that own at least one chunk
  const int64_t row0 = (int64_t)blockIdx.x * kShrinkRows;
  load_slots<kShrinkRows>(s_slot, p.idx, row0, p.T, p.num_slots);
  __syncthreads();
  int a0 = 0;
  while (a0 < kShrinkRows) {
    const int slot = s_slot[a0];
    if (slot < 0) {
      ++a0;
      continue;
    }
    int a1 = a0 + 1;                                   // rows a0 .. a1-1 of the block: one adapter, A streamed once
    while (a1 < kShrinkRows && s_slot[a1] == slot) ++a1;
    if (g < Gact) {
      float acc[kShrinkRows][8];
#pragma unroll
      for (int rr = 0; rr < kShrinkRows; ++rr)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[rr][e] = 0.f;
      const char* ap = p.a + ((int64_t)slot * p.a_slot_stride + (int64_t)c * 8) * 2;
      for (int ch = g; ch < NC; ch += G) {
        u32x4 av[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) av[j] = ld16(ap + ((int64_t)ch * 8 + j) * p.R * 2);
#pragma unroll
        for (int rr = 0; rr < kShrinkRows; ++rr) {
          if (rr >= a0 && rr < a1) {
            float xf[8];
            unpack16<Tag>(ld16(p.x + ((row0 + rr) * p.x_stride + (int64_t)ch * 8) * 2), xf);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              float af[8];
              unpack16<Tag>(av[j], af);
#pragma unroll
              for (int e = 0; e < 8; ++e) acc[rr][e] = __fmaf_rn(xf[j], af[e], acc[rr][e]);
            }
          }
        }
      }
#pragma unroll
      for (int rr = 0; rr < kShrinkRows; ++rr) {
        if (rr >= a0 && rr < a1) {
#pragma unroll
          for (int e = 0; e < 8; ++e) red[rr][g * p.R + c * 8 + e] = acc[rr][e];
        }
      }
    }
    __syncthreads();
    for (int o = tid; o < (a1 - a0) * p.R; o += kLoraThreads) {
      const int rr = a0 + o / p.R, col = o % p.R;
      float s = 0.f;
      for (int gg = 0; gg < Gact; ++gg) s = __fadd_rn(s, red[rr][gg * p.R + col]);
      p.tmp[(row0 + rr) * p.tmp_stride + col] = __fmul_rn(s, p.scale);
    }
    __syncthreads();
    a0 = a1;
  }
}

struct ExpandArgs {
  char* y;
  const float* tmp;
  const char* b;
  const int32_t* idx;
  int T, r, n, S, num_slots;
  int64_t y_stride, tmp_stride, b_slot_stride;   // elements
};

template <typename Tag>
__global__ __launch_bounds__(kLoraThreads) void lora_expand_kernel(ExpandArgs p) {
  __shared__ float s_tmp[kExpandRows][kLoraMaxR];
  __shared__ int s_slot[kExpandRows];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kExpandRows;
  const int R = p.S * p.r;
  load_slots<kExpandRows>(s_slot, p.idx, row0, p.T, p.num_slots);
  __syncthreads();
  for (int i = tid; i < kExpandRows * R; i += kLoraThreads) {
    const int rr = i / R, cc = i - rr * R;
    if (s_slot[rr] >= 0) s_tmp[rr][cc] = p.tmp[(row0 + rr) * p.tmp_stride + cc];
  }
  __syncthreads();
  const int nvec = p.n >> 3;
  const int v = blockIdx.y * kLoraThreads + tid;       // vector of the S n columns: slice v / nvec, columns 8 v ..
  if (v >= p.S * nvec) return;
  const int tbase = (v / nvec) * p.r;
  const int64_t col = (int64_t)v * 8, brow = (int64_t)p.S * p.n;
  int a0 = 0;
  while (a0 < kExpandRows) {
    const int slot = s_slot[a0];
    if (slot < 0) {
      ++a0;
      continue;
    }
    int a1 = a0 + 1;
    while (a1 < kExpandRows && s_slot[a1] == slot) ++a1;
    float acc[kExpandRows][8];
#pragma unroll
    for (int rr = 0; rr < kExpandRows; ++rr)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[rr][e] = 0.f;
    const char* bp = p.b + ((int64_t)slot * p.b_slot_stride + col) * 2;
    for (int j0 = 0; j0 < p.r; j0 += 8) {
      u32x4 bv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) bv[j] = ld16(bp + (int64_t)(j0 + j) * brow * 2);
#pragma unroll
      for (int rr = 0; rr < kExpandRows; ++rr) {
        if (rr >= a0 && rr < a1) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float bf[8];
            unpack16<Tag>(bv[j], bf);
            const float t = s_tmp[rr][tbase + j0 + j];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[rr][e] = __fmaf_rn(t, bf[e], acc[rr][e]);
          }
        }
      }
    }
#pragma unroll
    for (int rr = 0; rr < kExpandRows; ++rr) {
      if (rr >= a0 && rr < a1) {
        char* yp = p.y + ((row0 + rr) * p.y_stride + col) * 2;
        float yf[8];
        unpack16<Tag>(ld16(yp), yf);
#pragma unroll
        for (int e = 0; e < 8; ++e) yf[e] = __fadd_rn(yf[e], acc[rr][e]);
        st16(yp, pack16<Tag>(yf));
      }
    }
    a0 = a1;
  }
}

}  // namespace sp

extern "C" int sp_lora_shrink(float* tmp, const void* x, const void* a, const int32_t* indices, int64_t num_tokens,
                              int K, int R, int num_slots, int64_t x_stride, int64_t a_slot_stride,
                              int64_t tmp_stride, float scale, int dtype, void* stream) {
  SP_CHECK_ARG(num_tokens >= 0 && K >= 0 && R >= 0 && num_slots >= 0);
  if (num_tokens == 0) return SP_OK;
  SP_CHECK_ARG(tmp && x && a && indices);
  SP_CHECK_ARG(num_tokens <= INT32_MAX);
  if (dtype != SP_BF16 && dtype != SP_F16) return SP_ERR_UNSUPPORTED;
  if (K == 0 || K % 8 != 0 || R == 0 || R % 8 != 0 || R > sp::kLoraMaxR) return SP_ERR_UNSUPPORTED;
  SP_CHECK_ARG(x_stride >= K && tmp_stride >= R && a_slot_stride >= (int64_t)K * R);
  SP_CHECK_ARG(x_stride % 8 == 0 && a_slot_stride % 8 == 0);
  SP_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)a & 15) == 0 && ((uintptr_t)tmp & 3) == 0);
  sp::ShrinkArgs p{tmp, (const char*)x, (const char*)a, indices, (int)num_tokens, K, R, num_slots,
                   x_stride, a_slot_stride, tmp_stride, scale};
  const dim3 grid((unsigned)((num_tokens + sp::kShrinkRows - 1) / sp::kShrinkRows));
  if (dtype == SP_BF16) sp::lora_shrink_kernel<sp::bf16_tag><<<grid, sp::kLoraThreads, 0, (hipStream_t)stream>>>(p);
  else sp::lora_shrink_kernel<sp::f16_tag><<<grid, sp::kLoraThreads, 0, (hipStream_t)stream>>>(p);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_lora_expand(void* y, const float* tmp, const void* b, const int32_t* indices, int64_t num_tokens,
                              int r, int n, int num_slices, int num_slots, int64_t y_stride, int64_t tmp_stride,
                              int64_t b_slot_stride, int dtype, void* stream) {
  SP_CHECK_ARG(num_tokens >= 0 && r >= 0 && n >= 0 && num_slices >= 0 && num_slots >= 0);
  if (num_tokens == 0) return SP_OK;
  SP_CHECK_ARG(y && tmp && b && indices);
  SP_CHECK_ARG(num_tokens <= INT32_MAX);
  if (dtype != SP_BF16 && dtype != SP_F16) return SP_ERR_UNSUPPORTED;
  if (r != 8 && r != 16 && r != 32 && r != 64) return SP_ERR_UNSUPPORTED;
  if (num_slices == 0 || (int64_t)num_slices * r > sp::kLoraMaxR || n == 0 || n % 8 != 0) return SP_ERR_UNSUPPORTED;
  const int64_t width = (int64_t)num_slices * n;
  SP_CHECK_ARG(width <= INT32_MAX);
  SP_CHECK_ARG(y_stride >= width && tmp_stride >= (int64_t)num_slices * r && b_slot_stride >= (int64_t)r * width);
  SP_CHECK_ARG(y_stride % 8 == 0 && b_slot_stride % 8 == 0);
  SP_CHECK_ARG(((uintptr_t)y & 15) == 0 && ((uintptr_t)b & 15) == 0 && ((uintptr_t)tmp & 3) == 0);
  sp::ExpandArgs p{(char*)y, tmp, (const char*)b, indices, (int)num_tokens, r, n, num_slices, num_slots,
                   y_stride, tmp_stride, b_slot_stride};
  const int64_t col_blocks = (width / 8 + sp::kLoraThreads - 1) / sp::kLoraThreads;
  SP_CHECK_ARG(col_blocks <= 65535);
  const dim3 grid((unsigned)((num_tokens + sp::kExpandRows - 1) / sp::kExpandRows), (unsigned)col_blocks);
  if (dtype == SP_BF16) sp::lora_expand_kernel<sp::bf16_tag><<<grid, sp::kLoraThreads, 0, (hipStream_t)stream>>>(p);
  else sp::lora_expand_kernel<sp::f16_tag><<<grid, sp::kLoraThreads, 0, (hipStream_t)stream>>>(p);
  SP_LAUNCH_CHECK();
  return SP_OK;
}
