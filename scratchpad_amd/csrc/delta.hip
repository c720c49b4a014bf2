// Delta toppings: the per-row product with a 4-bit, 2:4-sparse full-model delta (W_finetuned - W_base) of the row's
// adapter slot, added in place to the base projection's output.
//
// Call sites they serve: the DeltaW= half of every ldmm(...) call of the topping layers
// (nn/toppings/topping_layer.py) over the buffers of memory/topping_pool.py:126-172.  The reference hands the arithmetic
// to triteia (not part of its tree) over Marlin-ordered buffers; the layout here is this project's own
// (include/scratchpad_hip.h states it): per slot and output row n, byte g of `codes` is the group of dense columns
// 4 g .. 4 g + 3 (low nibble: the code at p0, high nibble: the code at p1 > p0), nibble g of `meta` is p0 | p1 << 2,
// and the dense value is scales[n] * (code - 8).  The lanes of a row read contiguous bytes.
//
//   sp_delta_group  the stable counting sort of the rows t with 0 <= indices[t] < slots by slot: slot_offsets[slots + 1],
//                   sorted_rows[T]: the shared sort (group_sort.hip)
//   sp_delta_mm     y[t, n] = round(y[t, n] + scale_s[n] * sum_k x[t, k] * q_s[n, k])  for every sorted row t of slot s
//
// The product is the grouped form of the weight-streaming core of stream_gemm.h with group = slot (geometry, block
// search, park and sum, batch invariance and the safety rules are stated there) and the weight operand unpacked in
// registers.  What is its own:
//   * a workgroup owns 32 consecutive sorted rows of ONE slot x 16 rows of that slot's delta;
//   * the reduction is cut into super-steps of 256 dense columns, which the 8 waves take round-robin.  In a super-step
//     lane (r16, q) loads 16 B of codes and 8 B of meta of delta row n0 + r16 - the 64 dense columns 256 ss + 64 q ..
//     + 63 - and spends them over 8 v_mfma_f32_16x16x32: k-slot (q, i) of MFMA j carries dense column
//     256 ss + 64 q + 8 j + i, so the activation operand of MFMA j is the 16 B at that column of the lane's row (two
//     16-row sub-blocks: one unpacked fragment feeds 2 MFMAs).  A tail super-step (K % 256 != 0) has lanes whose 64
//     columns lie past K: they load nothing and feed zeros on both sides.  No LDS on the way in;
//   * unpacking is VALU: a code byte becomes two 16-bit floats through the exponent trick (0x6400 | c is 1024 + c in
//     fp16, 0x4300 | c is 128 + c in bf16; subtracting 1032 resp. 136 leaves the integer c - 8 exactly), and the pair is
//     shifted to the 16-bit positions p0 and p1 of the group's four;
//   * the epilogue: the sum is multiplied by the row's scale, added to y and rounded once.  Every (t, n) has one writer.
// The sparse MFMA (v_smfmac_f32_16x16x64) is not used: see DESIGN.md 4.6c.
//
// BATCH INVARIANCE: the bits a row receives depend on that row's x and y, its slot's packed delta and (N, K) only.  The
// super-steps of a wave, the 8 MFMAs inside one and the order over the waves are functions of K alone (stream_gemm.h).
#include "delta_unpack.h"
#include "stream_gemm.h"

namespace sp {

constexpr int kDeltaMaxTokens = 16384;

struct DeltaArgs {
  char* y;                        // [T, >= N] in dtype, updated in place
  const char* x;                  // [T, >= K] in dtype
  const char* codes;              // [slots][N, K / 4] bytes
  const char* meta;               // [slots][N, K / 8] bytes
  const char* scales;             // [slots][N] in dtype
  const int32_t* offsets;
  const int32_t* sorted_rows;
  int T, S, N, K;
  int64_t x_stride, y_stride, codes_slot_stride, meta_slot_stride, scales_slot_stride;   // elements (bytes for the packed two)
};

template <typename Tag>
__global__ __launch_bounds__(kStreamWaves * 64) void delta_mm_kernel(DeltaArgs p) {
  typedef Elem<Tag> E_;
  __shared__ float red[kStreamWaves][kStreamMB][16 * 17];
  __shared__ int s_row[kStreamBM];
  __shared__ int s_loc[3];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (wave == 0) find_row_block<kStreamBM>(p.offsets, p.S, p.T, s_loc);
  __syncthreads();
  const int slot = s_loc[0];
  if (slot < 0) return;
  const int row0 = s_loc[1], row_end = s_loc[2];
  block_rows<kStreamBM>(s_row, p.sorted_rows, row0, row_end, p.T);
  __syncthreads();
  const int r16 = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.y * 16;
  const int64_t n = n0 + r16;                               // N % 16 == 0: in range
  const char* cp = p.codes + (int64_t)slot * p.codes_slot_stride + n * (p.K / 4) + 16 * q;
  const char* mp = p.meta + (int64_t)slot * p.meta_slot_stride + n * (p.K / 8) + 8 * q;
  const char* xp[kStreamMB];
  bool valid[kStreamMB];
#pragma unroll
  for (int sb = 0; sb < kStreamMB; ++sb) {
    const int row = s_row[16 * sb + r16];
    valid[sb] = row >= 0;
    xp[sb] = p.x + ((int64_t)max(row, 0) * p.x_stride + 64 * q) * 2;
  }
  const int chunks = p.K / 64;                              // 64 dense columns each
  const int steps = (chunks + 3) / 4;
  f32x4 acc[kStreamMB];
#pragma unroll
  for (int sb = 0; sb < kStreamMB; ++sb) acc[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int ss = wave; ss < steps; ss += kStreamWaves) {
    const bool live = 4 * ss + q < chunks;                  // this lane's 64 columns lie below K
    u32x4 c = {0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u};     // code 8: the value 0
    u32x2 m = {0x44444444u, 0x44444444u};                               // p0 = 0, p1 = 1
    if (live) {
      c = ld16(cp + (int64_t)ss * 64);
      m = *(const u32x2*)(mp + (int64_t)ss * 32);
    }
    u32x4 xf[8][kStreamMB];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int sb = 0; sb < kStreamMB; ++sb)
        xf[j][sb] = (live && valid[sb]) ? ld16(xp[sb] + (int64_t)ss * 512 + 16 * j) : zero;
    const uint32_t cw[4] = {c[0], c[1], c[2], c[3]};
    const uint32_t mw[2] = {m[0], m[1]};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const u32x4 a = delta_expand<Tag>(cw[j >> 1] >> (16 * (j & 1)), mw[j >> 2] >> (8 * (j & 3)));
#pragma unroll
      for (int sb = 0; sb < kStreamMB; ++sb) acc[sb] = mfma_16x16x32<Tag>(a, xf[j][sb], acc[sb]);
    }
  }
  // acc[sb][r] = partial of (row 16 sb + r16 of the block, delta row n0 + 4 q + r)
  park_tile<kStreamMB>(red, wave, r16, q, acc);
  __syncthreads();
  for (int idx = tid; idx < kStreamBM * 16; idx += kStreamWaves * 64) {
    const int mrow = idx >> 4, col = idx & 15;
    const int row = s_row[mrow];
    if (row < 0) continue;
    // (y's index is formed ahead of the sum so that the scale and y loads are both in flight during it)
    const int64_t yi = (int64_t)row * p.y_stride + n0 + col;
    const float s = sum_tile<kStreamMB>(red, mrow >> 4, col, mrow & 15);
    const float sc = E_::load(p.scales, (int64_t)slot * p.scales_slot_stride + n0 + col);
    E_::store(p.y, yi, __fadd_rn(E_::load(p.y, yi), __fmul_rn(sc, s)));
  }
}

}  // namespace sp

static int delta_shape_status(int64_t num_tokens, int num_slots) {
  if (num_slots == 0 || num_slots > sp::kMaxGroups || num_tokens > sp::kDeltaMaxTokens) return SP_ERR_UNSUPPORTED;
  return SP_OK;
}

extern "C" int sp_delta_group(int32_t* slot_offsets, int32_t* sorted_rows, const int32_t* indices, int64_t num_tokens,
                              int num_slots, void* stream) {
  SP_CHECK_ARG(num_tokens >= 0 && num_slots >= 0);
  SP_CHECK_ARG(slot_offsets && sorted_rows && indices);
  if (const int st = delta_shape_status(num_tokens, num_slots)) return st;
  // (num_tokens == 0 still launches: slot_offsets has to read all zero for whoever looks at it)
  sp::launch_group_sort(slot_offsets, sorted_rows, indices, (int)num_tokens, num_slots, (hipStream_t)stream);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_delta_mm(void* y, const void* x, const void* codes, const void* meta, const void* scales,
                           const int32_t* slot_offsets, const int32_t* sorted_rows, int64_t num_tokens, int num_slots,
                           int N, int K, int64_t x_stride, int64_t y_stride, int64_t codes_slot_stride,
                           int64_t meta_slot_stride, int64_t scales_slot_stride, int dtype, void* stream) {
  SP_CHECK_ARG(num_tokens >= 0 && num_slots >= 0 && N >= 0 && K >= 0);
  SP_CHECK_ARG(y && x && codes && meta && scales && slot_offsets && sorted_rows);
  if (num_tokens == 0) return SP_OK;
  if (dtype != SP_BF16 && dtype != SP_F16) return SP_ERR_UNSUPPORTED;
  if (const int st = delta_shape_status(num_tokens, num_slots)) return st;
  if (K == 0 || K % 64 != 0 || N == 0 || N % 16 != 0 || N / 16 > 65535) return SP_ERR_UNSUPPORTED;
  SP_CHECK_ARG(x_stride >= K && y_stride >= N && scales_slot_stride >= N);
  SP_CHECK_ARG(codes_slot_stride >= (int64_t)N * (K / 4) && meta_slot_stride >= (int64_t)N * (K / 8));
  SP_CHECK_ARG(x_stride % 8 == 0 && codes_slot_stride % 16 == 0 && meta_slot_stride % 8 == 0);
  SP_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)codes & 15) == 0 && ((uintptr_t)meta & 7) == 0);
  SP_CHECK_ARG(((uintptr_t)y & 1) == 0 && ((uintptr_t)scales & 1) == 0);
  const int T = (int)num_tokens;
  sp::DeltaArgs p{(char*)y, (const char*)x, (const char*)codes, (const char*)meta, (const char*)scales, slot_offsets,
                  sorted_rows, T, num_slots, N, K, x_stride, y_stride, codes_slot_stride, meta_slot_stride,
                  scales_slot_stride};
  const dim3 grid((unsigned)((T + sp::kStreamBM - 1) / sp::kStreamBM + num_slots), (unsigned)(N / 16));
  SP_DISPATCH_16BIT(dtype, (sp::delta_mm_kernel<Tag><<<grid, sp::kStreamWaves * 64, 0, (hipStream_t)stream>>>(p)));
  SP_LAUNCH_CHECK();
  return SP_OK;
}
