// Sampling penalties and grammar vocab masks for gfx950: what the reference runs between the logits processor and
// the sampler (SamplingBatchInfo.apply_logits_bias, sampling/sampling_batch_info.py:324-344, fed by
// sampling/penaltylib/penalizers/{frequency_penalty,presence_penalty,min_new_tokens}.py and by the grammar back-ends'
// apply_vocab_mask: constrained/triton_ops/bitmask_ops.py for xgrammar, outlines_backend.py:82-83 for outlines).
//
// The reference keeps one dense fp32 [bs, vocab] tensor per penalizer and subtracts each from the logits in a pass
// of its own.  A request's penalties only touch the tokens that request has emitted, so the state here is, per
// REQUEST (row = req_pool_idx, the row of req_to_token), the list of its distinct output tokens with their counts:
//
//   entries    [pool_rows, capacity, 2] int32   (token, count), the first n_distinct[row] are live, tokens distinct
//   n_distinct [pool_rows]              int32
//   out_len    [pool_rows]              int32   tokens emitted so far (min_new_tokens)
//
// sp_penalty_apply, per live entry (t, c) of the row, in this order (the reference iterates a Python set of penalizer
// classes, so its order of the two subtractions is not fixed; here it is):
//   x = logits[r, t];  x -= c * frequency[r];  x -= presence[r];  x = x > 0 ? x / repetition[r] : x * repetition[r]
// and then, while out_len < min_new_tokens[r], logits[r, s] = -inf for the row's stop ids s.  Entries are distinct, so
// no two lanes touch one column; the stop ids are written after a workgroup barrier behind the entry pass.
//
// Traffic (derived from the layout, not measured): a step reads bs x n_distinct x 8 B of entries and reads + writes
// bs x n_distinct x 4 B of logits, 16 B per live entry, where the dense form moves bs x vocab x 4 B three times per
// pass (read logits, read penalty, write logits) for each penalizer.  At bs 256, vocab 128 256, 1 024 distinct tokens
// per row: 4 MB against 394 MB per dense pass.  sp_vocab_mask_apply is the one dense pass: it reads the mask and
// writes only the forbidden columns.
//
// Plain C++ with vector loads / stores and one LDS word; no atomics are needed (one workgroup owns a row).
#include "sp_common.h"

namespace sp {

constexpr int kPenThreads = 256;

__global__ __launch_bounds__(kPenThreads) void penalty_reset_kernel(int32_t* __restrict__ n_distinct,
                                                                    int32_t* __restrict__ out_len,
                                                                    const void* __restrict__ rows, int idx64,
                                                                    int num_rows, int pool_rows) {
  const int i = blockIdx.x * kPenThreads + threadIdx.x;
  if (i >= num_rows) return;
  const int64_t row = load_idx(rows, i, idx64);
  if (row < 0 || row >= pool_rows) return;
  n_distinct[row] = 0;
  out_len[row] = 0;
}

// One workgroup per batch row.  The rows of a batch are distinct requests, so a pool row has one writer.
__global__ __launch_bounds__(kPenThreads) void penalty_cumulate_kernel(
    int32_t* __restrict__ entries, int32_t* __restrict__ n_distinct, int32_t* __restrict__ out_len,
    int32_t* __restrict__ error, const void* __restrict__ req_pool_indices, int idx64,
    const int64_t* __restrict__ token_ids, int pool_rows, int capacity, int vocab) {
  __shared__ int s_found;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t tok = token_ids[b];
  const int64_t row = load_idx(req_pool_indices, b, idx64);
  if (tok < 0 || tok >= vocab || row < 0 || row >= pool_rows) return;      // padding row, unresolved placeholder
  int32_t* __restrict__ list = entries + row * (int64_t)capacity * 2;
  const int n = min(max(n_distinct[row], 0), capacity);
  if (tid == 0) s_found = -1;
  __syncthreads();
  for (int i = tid; i < n; i += kPenThreads)
    if (list[2 * i] == (int32_t)tok) s_found = i;       // tokens are distinct: at most one lane writes
  __syncthreads();
  if (tid != 0) return;
  const int at = s_found;
  if (at >= 0) {
    list[2 * at + 1] += 1;
  } else if (n < capacity) {
    list[2 * n] = (int32_t)tok;
    list[2 * n + 1] = 1;
    n_distinct[row] = n + 1;
  } else {
    *error = 1;       // sticky: a row cannot fill up while capacity = the pool's max_context_len; the host raises on it
    return;
  }
  out_len[row] += 1;
}

__global__ __launch_bounds__(kPenThreads) void penalty_apply_kernel(
    float* __restrict__ logits, int64_t row_stride, const int32_t* __restrict__ entries,
    const int32_t* __restrict__ n_distinct, const int32_t* __restrict__ out_len,
    const void* __restrict__ req_pool_indices, int idx64, const float* __restrict__ frequency,
    const float* __restrict__ presence, const float* __restrict__ repetition,
    const int32_t* __restrict__ min_new_tokens, const int32_t* __restrict__ stop_token_ids, int max_stops,
    int pool_rows, int capacity, int vocab) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const float f = frequency[b], p = presence[b], rep = repetition[b];
  const int min_new = min_new_tokens ? min_new_tokens[b] : 0;
  if (f == 0.f && p == 0.f && rep == 1.f && min_new <= 0) return;
  const int64_t row = load_idx(req_pool_indices, b, idx64);
  if (row < 0 || row >= pool_rows) return;
  float* __restrict__ x = logits + (int64_t)b * row_stride;
  if (f != 0.f || p != 0.f || rep != 1.f) {
    const int32_t* __restrict__ list = entries + row * (int64_t)capacity * 2;
    const int n = min(max(n_distinct[row], 0), capacity);
    for (int i = tid; i < n; i += kPenThreads) {
      const int2 e = *(const int2*)(list + 2 * i);
      if (e.x < 0 || e.x >= vocab) continue;
      float v = x[e.x];
      v -= (float)e.y * f;
      v -= p;
      v = v > 0.f ? v / rep : v * rep;
      x[e.x] = v;
    }
  }
  if (min_new <= 0 || stop_token_ids == nullptr || out_len[row] >= min_new) return;
  __syncthreads();      // a stop id may also be an entry: its -inf lands behind the entry pass (the branch is uniform)
  for (int s = tid; s < max_stops; s += kPenThreads) {
    const int t = stop_token_ids[(int64_t)b * max_stops + s];
    if (t >= 0 && t < vocab) x[t] = -INFINITY;
  }
}

constexpr int kMaskCols = 4 * kPenThreads;      // columns per workgroup

// kind 0: packed int32 words, bit j of word i = token 32 i + j, 1 = allowed; kind 1: one byte per token, non-zero =
// forbidden.  `limit` = the columns the mask speaks about.  Only forbidden columns are written.
template <int KIND>
__global__ __launch_bounds__(kPenThreads) void vocab_mask_apply_kernel(float* __restrict__ logits, int64_t row_stride,
                                                                       const void* __restrict__ mask,
                                                                       int64_t mask_stride, int limit) {
  const int b = blockIdx.y;
  float* __restrict__ x = logits + (int64_t)b * row_stride;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int col = blockIdx.x * kMaskCols + k * kPenThreads + threadIdx.x;
    if (col >= limit) return;
    bool forbidden;
    if (KIND == 0) {
      const uint32_t w = ((const uint32_t*)mask)[(int64_t)b * mask_stride + (col >> 5)];
      forbidden = ((w >> (col & 31)) & 1u) == 0u;
    } else {
      forbidden = ((const uint8_t*)mask)[(int64_t)b * mask_stride + col] != 0;
    }
    if (forbidden) x[col] = -INFINITY;
  }
}

}  // namespace sp

extern "C" int sp_penalty_reset(int32_t* n_distinct, int32_t* out_len, const void* pool_row_indices, int idx64,
                                int num_rows, int pool_rows, void* stream) {
  SP_CHECK_ARG(num_rows >= 0 && pool_rows >= 0);
  if (num_rows == 0) return SP_OK;
  SP_CHECK_ARG(n_distinct && out_len && pool_row_indices);
  sp::penalty_reset_kernel<<<dim3((num_rows + sp::kPenThreads - 1) / sp::kPenThreads), sp::kPenThreads, 0,
                             (hipStream_t)stream>>>(n_distinct, out_len, pool_row_indices, idx64, num_rows, pool_rows);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_penalty_cumulate(int32_t* entries, int32_t* n_distinct, int32_t* out_len, int32_t* error,
                                   const void* req_pool_indices, int idx64, const int64_t* token_ids, int num_rows,
                                   int pool_rows, int capacity, int vocab, void* stream) {
  SP_CHECK_ARG(num_rows >= 0 && pool_rows >= 0 && capacity >= 0 && vocab >= 0);
  if (num_rows == 0) return SP_OK;
  SP_CHECK_ARG(entries && n_distinct && out_len && error && req_pool_indices && token_ids);
  sp::penalty_cumulate_kernel<<<dim3(num_rows), sp::kPenThreads, 0, (hipStream_t)stream>>>(
      entries, n_distinct, out_len, error, req_pool_indices, idx64, token_ids, pool_rows, capacity, vocab);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_penalty_apply(float* logits, int64_t row_stride, const int32_t* entries, const int32_t* n_distinct,
                                const int32_t* out_len, const void* req_pool_indices, int idx64,
                                const float* frequency_penalties, const float* presence_penalties,
                                const float* repetition_penalties, const int32_t* min_new_tokens,
                                const int32_t* stop_token_ids, int max_stops, int num_rows, int pool_rows,
                                int capacity, int vocab, void* stream) {
  SP_CHECK_ARG(num_rows >= 0 && pool_rows >= 0 && capacity >= 0 && vocab >= 0 && max_stops >= 0);
  if (num_rows == 0) return SP_OK;
  SP_CHECK_ARG(logits && entries && n_distinct && out_len && req_pool_indices && frequency_penalties &&
               presence_penalties && repetition_penalties && row_stride >= vocab);
  SP_CHECK_ARG(max_stops == 0 || (stop_token_ids && min_new_tokens));
  sp::penalty_apply_kernel<<<dim3(num_rows), sp::kPenThreads, 0, (hipStream_t)stream>>>(
      logits, row_stride, entries, n_distinct, out_len, req_pool_indices, idx64, frequency_penalties,
      presence_penalties, repetition_penalties, min_new_tokens, max_stops ? stop_token_ids : nullptr, max_stops,
      pool_rows, capacity, vocab);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_vocab_mask_apply(float* logits, int64_t row_stride, const void* mask, int64_t mask_stride,
                                   int mask_width, int mask_kind, int num_rows, int vocab, void* stream) {
  SP_CHECK_ARG(num_rows >= 0 && vocab >= 0 && mask_width >= 0 && (mask_kind == 0 || mask_kind == 1));
  // xgrammar's rule (bitmask_ops.py:104-108): a bitmask wider than ceil(vocab / 32) words is refused; a narrower one
  // speaks about its own 32 w columns only.  The bool form has one element per column.
  if (mask_kind == 0) SP_CHECK_ARG(mask_width <= (vocab + 31) / 32);
  else SP_CHECK_ARG(mask_width == vocab);
  if (num_rows == 0) return SP_OK;
  SP_CHECK_ARG(logits && mask && row_stride >= vocab && mask_stride >= mask_width);
  const int limit = mask_kind == 0 ? (vocab < 32 * mask_width ? vocab : 32 * mask_width) : vocab;
  if (limit == 0) return SP_OK;
  SP_CHECK_ARG(num_rows <= 65535);
  const dim3 grid((limit + sp::kMaskCols - 1) / sp::kMaskCols, num_rows);
  if (mask_kind == 0)
    sp::vocab_mask_apply_kernel<0><<<grid, sp::kPenThreads, 0, (hipStream_t)stream>>>(logits, row_stride, mask,
                                                                                      mask_stride, limit);
  else
    sp::vocab_mask_apply_kernel<1><<<grid, sp::kPenThreads, 0, (hipStream_t)stream>>>(logits, row_stride, mask,
                                                                                      mask_stride, limit);
  SP_LAUNCH_CHECK();
  return SP_OK;
}
