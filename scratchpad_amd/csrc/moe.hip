// Mixture of experts (Llama-MoE): device routing and the grouped expert MLP.
//
// Call site they serve: LlamaMoE.forward (nn/models/llama/llama_moe.py:98-120).  The reference loops over the experts
// with torch.where and boolean indexing: a host synchronisation and a data-dependent shape in every layer, which a
// HIP-graph replay cannot contain.  Here every grid depends on (T, K, E) and the widths alone and the grouping is read
// from device memory:
//
//   sp_moe_route    ids[t, :K] = the K largest of logits[t, :E] (ties: lower index; NaN counts as largest),
//                   w[t, :K] = round(softmax over those K), then the stable counting sort of the T K (token, k) pairs
//                   by expert: expert_offsets[E + 1], sorted_pos[T K]                        (two launches)
//   sp_moe_gate_up  h[p, :I]   = round(silu(round(x[t] . Wg[e]^T)) * round(x[t] . Wu[e]^T))   p a sorted position
//   sp_moe_down     tmp[t K + k, :H] = round(round(h[p] . W2[e]^T) * w[t, k])
//   sp_moe_combine  out[t] = tmp rows of token t added in ascending expert index, rounded after every addition
//
// Route.  One wave per token: lane e holds logit e (E <= 64), K rounds of a wave-wide arg-max over a total order
// (not taken, NaN, value, lower index).  The softmax of the K selected values runs in fp64 (exp, sum in k order,
// divide) and is rounded to fp32 and then to the activation dtype (two roundings, the reference's): K <= 8 exponentials
// per token are free, and an fp64 host statement reproduces the result bit for bit.  The sort is the shared one
// (group_sort.hip).  T <= 16384 (sp_moe_max_tokens): above it the single workgroup's chunks grow past what a prefill
// chunk needs, and the entry refuses.
//
// The two GEMMs are one kernel (moe_gemm_kernel), the grouped form of the weight-streaming core of stream_gemm.h with
// group = expert (geometry, block search, batch invariance and the safety rules are stated there).  What is its own:
//   * a workgroup owns 32 consecutive sorted positions of ONE expert x 16 rows of that expert's weight (gate_up: 8
//     gate rows and the 8 matching up rows, as epilogue 1 of the skinny kernel); one W fragment feeds 2 MFMAs;
//   * the activations are gathered through sorted_pos for gate_up and read directly for down;
//   * the epilogues: SiLU-mul, and (down) the routing weight times the rounded sum, scattered to the pair's row.
// Why BM = 32 and not more: at decode an expert has a handful of rows and a second sub-block costs one idle MFMA per
// k-step, far below the weight stream; at a prefill chunk the row blocks of one expert re-read its weights out of L2 /
// the Infinity Cache.  A compute-bound LDS-tiled form for long prefills is left for a later change.
//
// BATCH INVARIANCE: the bits of an output row depend on that row's input, its expert's weights and (for down) its
// routing weight only (stream_gemm.h).
#include "stream_gemm.h"

namespace sp {

constexpr int kMoeMaxTopK = 8;
constexpr int kMoeMaxTokens = 16384;
constexpr int kMoeUnroll = 8;

// ------------------------------------------------------------------------------------------------ route
// is candidate a (index, value, is-NaN) ahead of b?  An index >= 64 marks a lane that cannot be chosen.
__device__ __forceinline__ bool moe_ahead(int ai, float av, int an, int bi, float bv, int bn) {
  const bool aok = ai < 64, bok = bi < 64;
  if (aok != bok) return aok;
  if (aok) {
    if (an != bn) return an != 0;
    if (!an && av != bv) return av > bv;
  }
  return ai < bi;
}

template <typename Tag>
__global__ __launch_bounds__(256) void moe_topk_kernel(int32_t* ids, float* wts, const void* logits, int T, int E,
                                                       int K, int64_t stride) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;                                     // wave-uniform
  bool ok = lane < E;
  const float v = ok ? Elem<Tag>::load(logits, t * stride + lane) : 0.f;
  const int isnan_ = v != v;
  float mine = 0.f;
  int myid = 0;
  for (int j = 0; j < K; ++j) {
    int bi = ok ? lane : 64 + lane, bn = isnan_;
    float bv = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int oi = __shfl_xor(bi, off, 64), on = __shfl_xor(bn, off, 64);
      const float ov = __shfl_xor(bv, off, 64);
      if (moe_ahead(oi, ov, on, bi, bv, bn)) bi = oi, bv = ov, bn = on;
    }
    // K <= E: at least one lane below E is still free, so bi < E
    if (lane == j) mine = bv, myid = bi;
    if (lane == bi) ok = false;
  }
  const double top = (double)__shfl(mine, 0, 64);         // the first selected is the largest
  const double ex = lane < K ? exp((double)mine - top) : 0.0;
  double sum = 0.0;
  for (int j = 0; j < K; ++j) sum += __shfl(ex, j, 64);
  if (lane < K) {
    // two roundings, as the reference's softmax(dtype=float).to(x.dtype): fp64 -> fp32, then fp32 -> dtype.  The empty
    // asm keeps the fp32 value apart: without it the compiler merges the two conversions into ONE fp64 -> fp16
    // rounding, which differs from the statement wherever the fp32 value lands on a 16-bit rounding boundary
    float w32 = (float)(ex / sum);
    asm volatile("" : "+v"(w32));
    ids[t * K + lane] = min(max(myid, 0), E - 1);
    wts[t * K + lane] = Elem<Tag>::round(w32);
  }
}

// ------------------------------------------------------------------------------------------------ grouped GEMM
struct MoeGemmArgs {
  const char* a;                  // GATE_UP: x [T, K]; down: h [T topk, K] by sorted position
  const char* w;                  // [E, rows, K], rows = 2 N (gate | up) resp. N
  void* out;                      // GATE_UP: h [T topk, N] by sorted position; down: tmp [T topk, N] by pair
  const int32_t* offsets;
  const int32_t* sorted_pos;
  const float* topk_w;            // down only
  int NP, topk, E, N, K;          // NP = T topk pairs, N output columns, K reduction length
  int64_t a_stride, out_stride, w_expert_stride;   // elements
};

template <typename Tag, bool GATE_UP>
__global__ __launch_bounds__(kStreamWaves * 64) void moe_gemm_kernel(MoeGemmArgs p) {
  typedef Elem<Tag> E_;
  __shared__ float red[kStreamWaves][kStreamMB][16 * 17];
  __shared__ int s_pair[kStreamBM];
  __shared__ float s_scale[kStreamBM];
  __shared__ int s_loc[3];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (wave == 0) find_row_block<kStreamBM>(p.offsets, p.E, p.NP, s_loc);
  __syncthreads();
  const int e = s_loc[0];
  if (e < 0) return;
  const int row0 = s_loc[1], row_end = s_loc[2];
  const int mine = block_rows<kStreamBM>(s_pair, p.sorted_pos, row0, row_end, p.NP);
  if (tid < kStreamBM) s_scale[tid] = (!GATE_UP && mine >= 0) ? p.topk_w[mine] : 0.f;
  __syncthreads();
  const int r16 = lane & 15, q = lane >> 4;
  const int n0 = GATE_UP ? blockIdx.y * 8 : blockIdx.y * 16;
  const int n = GATE_UP ? (r16 < 8 ? 0 : p.N) + n0 + (r16 & 7) : n0 + r16;      // N % 8 (16) == 0: in range
  const char* const wp[1] = {p.w + ((int64_t)e * p.w_expert_stride + (int64_t)n * p.K + 8 * q) * 2};
  const char* xp[kStreamMB];
  int valid[kStreamMB];
#pragma unroll
  for (int sb = 0; sb < kStreamMB; ++sb) {
    const int pair = s_pair[16 * sb + r16];
    valid[sb] = pair >= 0;
    const int64_t arow = GATE_UP ? (int64_t)(max(pair, 0) / p.topk) : (int64_t)row0 + 16 * sb + r16;
    xp[sb] = p.a + (arow * p.a_stride + 8 * q) * 2;
  }
  f32x4 acc[kStreamMB];
#pragma unroll
  for (int sb = 0; sb < kStreamMB; ++sb) acc[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
  stream_ksteps<Tag, 1, kStreamMB, kMoeUnroll, false>(acc, wp, xp, valid, wave, p.K / 32);
  // acc[sb][r] = partial of (row 16 sb + r16 of the block, tile column 4 q + r)
  park_tile<kStreamMB>(red, wave, r16, q, acc);
  __syncthreads();
  if constexpr (GATE_UP) {
    // tile columns 0-7 are the gate sums, 8-15 the up sums of output columns n0 .. n0 + 7
    for (int idx = tid; idx < kStreamBM * 8; idx += kStreamWaves * 64) {
      const int m = idx >> 3, c = idx & 7;
      if (s_pair[m] < 0) continue;
      const float g = sum_tile<kStreamMB>(red, m >> 4, c, m & 15), u = sum_tile<kStreamMB>(red, m >> 4, c + 8, m & 15);
      E_::store(p.out, ((int64_t)row0 + m) * p.out_stride + n0 + c,
                __fmul_rn(E_::round(silu_ref(E_::round(g))), E_::round(u)));
    }
  } else {
    for (int idx = tid; idx < kStreamBM * 16; idx += kStreamWaves * 64) {
      const int m = idx >> 4, c = idx & 15;
      const int pair = s_pair[m];
      if (pair < 0) continue;
      const float s = sum_tile<kStreamMB>(red, m >> 4, c, m & 15);
      E_::store(p.out, (int64_t)pair * p.out_stride + n0 + c, __fmul_rn(E_::round(s), s_scale[m]));
    }
  }
}

// ------------------------------------------------------------------------------------------------ combine
template <typename Tag>
__global__ __launch_bounds__(256) void moe_combine_kernel(char* out, const char* tmp, const int32_t* ids, int K, int E,
                                                          int H, int64_t tmp_stride, int64_t out_stride) {
  __shared__ int s_key[kMoeMaxTopK];
  const int64_t t = blockIdx.x;
  if (threadIdx.x < K) {
    const int id = ids[t * K + threadIdx.x];
    s_key[threadIdx.x] = (unsigned)id < (unsigned)E ? id * kMoeMaxTopK + (int)threadIdx.x : -1;
  }
  __syncthreads();
  const int64_t col = ((int64_t)blockIdx.y * 256 + threadIdx.x) * 8;
  if (col >= H) return;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  int last = -1;                                          // ascending (expert, k): k = key & 7
  for (int step = 0; step < K; ++step) {
    int best = INT32_MAX;
    for (int j = 0; j < K; ++j) {
      const int key = s_key[j];
      if (key > last && key < best) best = key;
    }
    if (best == INT32_MAX) break;
    last = best;
    float f[8];
    unpack16<Tag>(ld16(tmp + ((t * K + (best & (kMoeMaxTopK - 1))) * tmp_stride + col) * 2), f);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = Elem<Tag>::round(__fadd_rn(acc[i], f[i]));
  }
  st16(out + (t * out_stride + col) * 2, pack16<Tag>(acc));
}

}  // namespace sp

extern "C" int sp_moe_block_rows(void) { return sp::kStreamBM; }
extern "C" int sp_moe_max_tokens(void) { return sp::kMoeMaxTokens; }

static int moe_shape_status(int64_t num_tokens, int num_experts, int top_k) {
  if (num_experts == 0 || num_experts > sp::kMaxGroups || top_k == 0 || top_k > sp::kMoeMaxTopK ||
      top_k > num_experts || num_tokens > sp::kMoeMaxTokens)
    return SP_ERR_UNSUPPORTED;
  return SP_OK;
}

extern "C" int sp_moe_route(int32_t* topk_ids, float* topk_weights, int32_t* expert_offsets, int32_t* sorted_pos,
                            const void* router_logits, int64_t num_tokens, int num_experts, int top_k,
                            int64_t logits_stride, int dtype, void* stream) {
  SP_CHECK_ARG(num_tokens >= 0 && num_experts >= 0 && top_k >= 0);
  if (num_tokens == 0) return SP_OK;
  SP_CHECK_ARG(topk_ids && topk_weights && expert_offsets && sorted_pos && router_logits);
  if (dtype != SP_F32 && dtype != SP_F16 && dtype != SP_BF16) return SP_ERR_UNSUPPORTED;
  if (const int st = moe_shape_status(num_tokens, num_experts, top_k)) return st;
  SP_CHECK_ARG(logits_stride >= num_experts);
  const int T = (int)num_tokens;
  const dim3 grid((unsigned)((T + 3) / 4));
  SP_DISPATCH_DTYPE(dtype, (sp::moe_topk_kernel<Tag><<<grid, 256, 0, (hipStream_t)stream>>>(
                               topk_ids, topk_weights, router_logits, T, num_experts, top_k, logits_stride)));
  SP_LAUNCH_CHECK();
  sp::launch_group_sort(expert_offsets, sorted_pos, topk_ids, T * top_k, num_experts, (hipStream_t)stream);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

// the checks the two GEMM entries share; `red` = reduction length, `cols` = output columns
static int moe_gemm_status(int64_t num_tokens, int num_experts, int top_k, int red, int cols, int dtype) {
  if (dtype != SP_BF16 && dtype != SP_F16) return SP_ERR_UNSUPPORTED;
  if (const int st = moe_shape_status(num_tokens, num_experts, top_k)) return st;
  if (red == 0 || red % 32 != 0 || cols == 0 || cols % 32 != 0) return SP_ERR_UNSUPPORTED;
  return SP_OK;
}

extern "C" int sp_moe_gate_up(void* h, const void* x, const void* w13, const int32_t* expert_offsets,
                              const int32_t* sorted_pos, int64_t num_tokens, int top_k, int num_experts, int hidden,
                              int inter, int64_t x_stride, int64_t h_stride, int64_t w_expert_stride, int dtype,
                              void* stream) {
  SP_CHECK_ARG(num_tokens >= 0 && top_k >= 0 && num_experts >= 0 && hidden >= 0 && inter >= 0);
  if (num_tokens == 0) return SP_OK;
  SP_CHECK_ARG(h && x && w13 && expert_offsets && sorted_pos);
  if (const int st = moe_gemm_status(num_tokens, num_experts, top_k, hidden, inter, dtype)) return st;
  SP_CHECK_ARG(x_stride >= hidden && h_stride >= inter && w_expert_stride >= (int64_t)2 * inter * hidden);
  SP_CHECK_ARG(x_stride % 8 == 0 && w_expert_stride % 8 == 0);
  SP_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)w13 & 15) == 0);
  SP_CHECK_ARG(inter / 8 <= 65535);
  const int NP = (int)num_tokens * top_k;
  sp::MoeGemmArgs p{(const char*)x, (const char*)w13, h, expert_offsets, sorted_pos, nullptr, NP, top_k,
                    num_experts, inter, hidden, x_stride, h_stride, w_expert_stride};
  const dim3 grid((unsigned)((NP + sp::kStreamBM - 1) / sp::kStreamBM + num_experts), (unsigned)(inter / 8));
  SP_DISPATCH_16BIT(dtype, (sp::moe_gemm_kernel<Tag, true><<<grid, sp::kStreamWaves * 64, 0, (hipStream_t)stream>>>(p)));
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_moe_down(void* tmp, const void* h, const void* w2, const float* topk_weights,
                           const int32_t* expert_offsets, const int32_t* sorted_pos, int64_t num_tokens, int top_k,
                           int num_experts, int hidden, int inter, int64_t h_stride, int64_t tmp_stride,
                           int64_t w_expert_stride, int dtype, void* stream) {
  SP_CHECK_ARG(num_tokens >= 0 && top_k >= 0 && num_experts >= 0 && hidden >= 0 && inter >= 0);
  if (num_tokens == 0) return SP_OK;
  SP_CHECK_ARG(tmp && h && w2 && topk_weights && expert_offsets && sorted_pos);
  if (const int st = moe_gemm_status(num_tokens, num_experts, top_k, inter, hidden, dtype)) return st;
  SP_CHECK_ARG(h_stride >= inter && tmp_stride >= hidden && w_expert_stride >= (int64_t)inter * hidden);
  SP_CHECK_ARG(h_stride % 8 == 0 && w_expert_stride % 8 == 0);
  SP_CHECK_ARG(((uintptr_t)h & 15) == 0 && ((uintptr_t)w2 & 15) == 0);
  SP_CHECK_ARG(hidden / 16 <= 65535);
  const int NP = (int)num_tokens * top_k;
  sp::MoeGemmArgs p{(const char*)h, (const char*)w2, tmp, expert_offsets, sorted_pos, topk_weights, NP, top_k,
                    num_experts, hidden, inter, h_stride, tmp_stride, w_expert_stride};
  const dim3 grid((unsigned)((NP + sp::kStreamBM - 1) / sp::kStreamBM + num_experts), (unsigned)(hidden / 16));
  SP_DISPATCH_16BIT(dtype, (sp::moe_gemm_kernel<Tag, false><<<grid, sp::kStreamWaves * 64, 0, (hipStream_t)stream>>>(p)));
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_moe_combine(void* out, const void* tmp, const int32_t* topk_ids, int64_t num_tokens, int top_k,
                              int num_experts, int hidden, int64_t tmp_stride, int64_t out_stride, int dtype,
                              void* stream) {
  SP_CHECK_ARG(num_tokens >= 0 && top_k >= 0 && num_experts >= 0 && hidden >= 0);
  if (num_tokens == 0) return SP_OK;
  SP_CHECK_ARG(out && tmp && topk_ids);
  if (dtype != SP_BF16 && dtype != SP_F16) return SP_ERR_UNSUPPORTED;
  if (const int st = moe_shape_status(num_tokens, num_experts, top_k)) return st;
  if (hidden == 0 || hidden % 32 != 0) return SP_ERR_UNSUPPORTED;
  SP_CHECK_ARG(tmp_stride >= hidden && out_stride >= hidden && tmp_stride % 8 == 0 && out_stride % 8 == 0);
  SP_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)tmp & 15) == 0);
  const int64_t col_blocks = ((int64_t)hidden / 8 + 255) / 256;
  SP_CHECK_ARG(col_blocks <= 65535);
  const dim3 grid((unsigned)num_tokens, (unsigned)col_blocks);
  SP_DISPATCH_16BIT(dtype, (sp::moe_combine_kernel<Tag><<<grid, 256, 0, (hipStream_t)stream>>>(
                               (char*)out, (const char*)tmp, topk_ids, top_k, num_experts, hidden, tmp_stride,
                               out_stride)));
  SP_LAUNCH_CHECK();
  return SP_OK;
}
