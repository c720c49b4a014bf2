// Llama-Quant-MoE: the grouped expert MLP over 4-bit, 2:4-sparse experts, folded onto a dense base MLP's output.
//
// Call sites they serve: LlamaQuantisedMoE.forward (nn/models/llama/llama_quant_moe.py:204-257) and the naive variant
// (llama_naive_quant_moe.py:140-163).  The reference hands the products to triteia (not part of its tree) over
// Marlin-ordered buffers; the experts here are stored in this project's own packed layout, delta.py's
// (include/scratchpad_hip.h states it), stacked over the experts.  Routing and the sort are sp_moe_route's, unchanged.
//
//   sp_qmoe_gate_up  h[p, n]     = rnd(rnd(silu(rnd(sg[n] G))) * rnd(su[n] U))     p a sorted position of pair t K + k
//                    G = sum_k x[t, k] q_e[n, k], U the same sum over row I + n; the scale is multiplied once, in fp32
//   sp_qmoe_down     tmp[pair, n] = rnd(rnd(s[n] sum_k h[p, k] q_e[n, k]) * w[t, k])
//   sp_qmoe_combine  acc = +0; acc = rnd(acc + tmp[t K + j]) over the K pairs of token t in the chosen order;
//                    out[t] = rnd(acc + base[t])      order 0: ascending expert index, ties by k; order 1: j = 0 .. K-1
// (rnd = round to fp32, then to the activation dtype).
//
// The two products are ONE kernel (qmoe_gemm_kernel).  Its operand path is delta_mm_kernel's (delta.hip): super-steps of
// 256 dense columns dealt round-robin to the 8 waves; per super-step lane (r16, q) loads 16 B of codes and 8 B of meta
// of its weight row and spends them over 8 v_mfma_f32_16x16x32, MFMA j carrying dense columns 256 ss + 64 q + 8 j + i;
// lanes of a tail super-step whose 64 columns lie past K feed zeros on both sides; nothing goes through LDS on the way
// in.  Its block search, row table, gather, park and wave-order sum are moe_gemm_kernel's (moe.hip) by the same
// definitions of stream_gemm.h with group = expert.  What is its own:
//   * a workgroup owns 32 consecutive sorted positions of ONE expert x kQmoeNW 16-row weight tiles (gate_up: a tile is
//     8 gate rows and the 8 matching up rows), so one activation fragment feeds 2 kQmoeNW MFMAs.  kQmoeNW changes which
//     workgroup computes an element, never the element's reduction order;
//   * the epilogues: the row's scale in fp32 behind the sum, then SiLU-mul resp. the routing weight.
// Reduction order: sp_delta_mm's by definition, so sp_qmoe_down with K = 1, ascending ids and weights 1.0 equals
// sp_delta_mm on a zeroed y bit for bit (tests/test_gpu_quant_moe.py holds it).
//
// BATCH INVARIANCE: a token's bits depend on its input, its routing, the packed experts and (H, I) only.
// Safety: stream_gemm.h's rules.  Every (row, n) has one writer; no atomics, no zero-fill launch.
#include "delta_unpack.h"
#include "stream_gemm.h"

namespace sp {

#ifndef SP_QMOE_NW
#define SP_QMOE_NW 1
#endif
constexpr int kQmoeNW = SP_QMOE_NW;          // 16-row weight tiles of a workgroup: 1 or 2
// (the widths are multiples of 64, so 4 would divide too: that build computed wrong values in its first tile on an
// MI355X, cause not found - DESIGN.md 4.6d - and is refused here until it is)
static_assert(kQmoeNW == 1 || kQmoeNW == 2, "1 or 2 weight tiles per workgroup are built");
constexpr int kQmoeTiles = kQmoeNW * kStreamMB;
constexpr int kQmoeMaxTopK = 8;
constexpr int kQmoeMaxTokens = 16384;

struct QmoeGemmArgs {
  const char* a;                  // GATE_UP: x [T, K]; down: h [T topk, K] by sorted position
  const char* codes;              // [E][rows, K / 4] bytes, rows = 2 N (gate | up) resp. N
  const char* meta;               // [E][rows, K / 8] bytes
  const char* scales;             // [E][rows] in dtype
  void* out;                      // GATE_UP: h [T topk, N] by sorted position; down: tmp [T topk, N] by pair
  const int32_t* offsets;
  const int32_t* sorted_pos;
  const float* topk_w;            // down only
  int NP, topk, E, N, K;          // NP = T topk pairs, N output columns, K reduction length
  int64_t a_stride, out_stride, codes_expert_stride, meta_expert_stride, scales_expert_stride;   // elements / bytes
};

template <typename Tag, bool GATE_UP>
__global__ __launch_bounds__(kStreamWaves * 64) void qmoe_gemm_kernel(QmoeGemmArgs p) {
  typedef Elem<Tag> E_;
  __shared__ float red[kStreamWaves][kQmoeTiles][16 * 17];
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
  constexpr int kTileCols = GATE_UP ? 8 : 16;               // output columns of one weight tile
  const int nb = blockIdx.y * (kQmoeNW * kTileCols);        // N % 64 == 0: every tile is in range
  const char* cp[kQmoeNW];
  const char* mp[kQmoeNW];
#pragma unroll
  for (int nw = 0; nw < kQmoeNW; ++nw) {
    const int n0 = nb + nw * kTileCols;
    const int64_t n = GATE_UP ? (r16 < 8 ? 0 : p.N) + n0 + (r16 & 7) : n0 + r16;
    cp[nw] = p.codes + (int64_t)e * p.codes_expert_stride + n * (p.K / 4) + 16 * q;
    mp[nw] = p.meta + (int64_t)e * p.meta_expert_stride + n * (p.K / 8) + 8 * q;
  }
  const char* xp[kStreamMB];
  bool valid[kStreamMB];
#pragma unroll
  for (int sb = 0; sb < kStreamMB; ++sb) {
    const int pair = s_pair[16 * sb + r16];
    valid[sb] = pair >= 0;
    const int64_t arow = GATE_UP ? (int64_t)(max(pair, 0) / p.topk) : (int64_t)row0 + 16 * sb + r16;
    xp[sb] = p.a + (arow * p.a_stride + 64 * q) * 2;
  }
  const int chunks = p.K / 64;                              // 64 dense columns each
  const int steps = (chunks + 3) / 4;
  f32x4 acc[kQmoeTiles];
#pragma unroll
  for (int t = 0; t < kQmoeTiles; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int ss = wave; ss < steps; ss += kStreamWaves) {
    const bool live = 4 * ss + q < chunks;                  // this lane's 64 columns lie below K
    u32x4 c[kQmoeNW];
    u32x2 m[kQmoeNW];
#pragma unroll
    for (int nw = 0; nw < kQmoeNW; ++nw) {
      c[nw] = u32x4{0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u};     // code 8: the value 0
      m[nw] = u32x2{0x44444444u, 0x44444444u};                               // p0 = 0, p1 = 1
      if (live) {
        c[nw] = ld16(cp[nw] + (int64_t)ss * 64);
        m[nw] = *(const u32x2*)(mp[nw] + (int64_t)ss * 32);
      }
    }
    u32x4 xf[8][kStreamMB];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int sb = 0; sb < kStreamMB; ++sb)
        xf[j][sb] = (live && valid[sb]) ? ld16(xp[sb] + (int64_t)ss * 512 + 16 * j) : zero;
#pragma unroll
    for (int nw = 0; nw < kQmoeNW; ++nw) {
      const uint32_t cw[4] = {c[nw][0], c[nw][1], c[nw][2], c[nw][3]};
      const uint32_t mw[2] = {m[nw][0], m[nw][1]};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const u32x4 a = delta_expand<Tag>(cw[j >> 1] >> (16 * (j & 1)), mw[j >> 2] >> (8 * (j & 3)));
#pragma unroll
        for (int sb = 0; sb < kStreamMB; ++sb)
          acc[nw * kStreamMB + sb] = mfma_16x16x32<Tag>(a, xf[j][sb], acc[nw * kStreamMB + sb]);
      }
    }
  }
  // acc[nw MB + sb][r] = partial of (row 16 sb + r16 of the block, row 4 q + r of weight tile nw)
  park_tile<kQmoeTiles>(red, wave, r16, q, acc);
  __syncthreads();
  const int64_t sbase = (int64_t)e * p.scales_expert_stride;
  if constexpr (GATE_UP) {
    // tile rows 0-7 are the gate sums, 8-15 the up sums of output columns n0 .. n0 + 7
    for (int idx = tid; idx < kQmoeNW * kStreamBM * 8; idx += kStreamWaves * 64) {
      const int nw = idx / (kStreamBM * 8), m = (idx >> 3) & (kStreamBM - 1), c = idx & 7;
      if (s_pair[m] < 0) continue;
      const int n = nb + nw * 8 + c;
      const int t = nw * kStreamMB + (m >> 4);
      const float g = sum_tile<kQmoeTiles>(red, t, c, m & 15), u = sum_tile<kQmoeTiles>(red, t, c + 8, m & 15);
      const float sg = E_::load(p.scales, sbase + n), su = E_::load(p.scales, sbase + p.N + n);
      E_::store(p.out, ((int64_t)row0 + m) * p.out_stride + n,
                __fmul_rn(E_::round(silu_ref(E_::round(__fmul_rn(sg, g)))), E_::round(__fmul_rn(su, u))));
    }
  } else {
    for (int idx = tid; idx < kQmoeNW * kStreamBM * 16; idx += kStreamWaves * 64) {
      const int nw = idx / (kStreamBM * 16), m = (idx >> 4) & (kStreamBM - 1), c = idx & 15;
      const int pair = s_pair[m];
      if (pair < 0) continue;
      const int n = nb + nw * 16 + c;
      const float s = sum_tile<kQmoeTiles>(red, nw * kStreamMB + (m >> 4), c, m & 15);
      const float sc = E_::load(p.scales, sbase + n);
      E_::store(p.out, (int64_t)pair * p.out_stride + n, __fmul_rn(E_::round(__fmul_rn(sc, s)), s_scale[m]));
    }
  }
}

// ------------------------------------------------------------------------------------------------ combine
template <typename Tag>
__global__ __launch_bounds__(256) void qmoe_combine_kernel(char* out, const char* tmp, const char* base,
                                                           const int32_t* ids, int K, int E, int H, int order,
                                                           int64_t tmp_stride, int64_t base_stride,
                                                           int64_t out_stride) {
  __shared__ int s_key[kQmoeMaxTopK];
  const int64_t t = blockIdx.x;
  if (threadIdx.x < K) {
    const int id = ids[t * K + threadIdx.x];
    // order 0: (expert, k) ascending; order 1: k ascending.  k = key & 7 in both
    s_key[threadIdx.x] = (unsigned)id < (unsigned)E ? (order == 0 ? id : 0) * kQmoeMaxTopK + (int)threadIdx.x : -1;
  }
  __syncthreads();
  const int64_t col = ((int64_t)blockIdx.y * 256 + threadIdx.x) * 8;
  if (col >= H) return;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  int last = -1;
  for (int step = 0; step < K; ++step) {
    int best = INT32_MAX;
    for (int j = 0; j < K; ++j) {
      const int key = s_key[j];
      if (key > last && key < best) best = key;
    }
    if (best == INT32_MAX) break;
    last = best;
    float f[8];
    unpack16<Tag>(ld16(tmp + ((t * K + (best & (kQmoeMaxTopK - 1))) * tmp_stride + col) * 2), f);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = Elem<Tag>::round(__fadd_rn(acc[i], f[i]));
  }
  float b[8];
  unpack16<Tag>(ld16(base + (t * base_stride + col) * 2), b);       // read before the store: out may alias base
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = __fadd_rn(acc[i], b[i]);
  st16(out + (t * out_stride + col) * 2, pack16<Tag>(acc));
}

}  // namespace sp

extern "C" int sp_qmoe_weight_tiles(void) { return sp::kQmoeNW; }

static int qmoe_shape_status(int64_t num_tokens, int num_experts, int top_k, int hidden, int inter, int dtype) {
  if (dtype != SP_BF16 && dtype != SP_F16) return SP_ERR_UNSUPPORTED;
  if (num_experts == 0 || num_experts > sp::kMaxGroups || top_k == 0 || top_k > sp::kQmoeMaxTopK ||
      top_k > num_experts || num_tokens > sp::kQmoeMaxTokens)
    return SP_ERR_UNSUPPORTED;
  if (hidden == 0 || hidden % 64 != 0 || inter == 0 || inter % 64 != 0) return SP_ERR_UNSUPPORTED;
  return SP_OK;
}

extern "C" int sp_qmoe_gate_up(void* h, const void* x, const void* codes, const void* meta, const void* scales,
                               const int32_t* expert_offsets, const int32_t* sorted_pos, int64_t num_tokens, int top_k,
                               int num_experts, int hidden, int inter, int64_t x_stride, int64_t h_stride,
                               int64_t codes_expert_stride, int64_t meta_expert_stride, int64_t scales_expert_stride,
                               int dtype, void* stream) {
  SP_CHECK_ARG(num_tokens >= 0 && top_k >= 0 && num_experts >= 0 && hidden >= 0 && inter >= 0);
  SP_CHECK_ARG(h && x && codes && meta && scales && expert_offsets && sorted_pos);
  if (num_tokens == 0) return SP_OK;
  if (const int st = qmoe_shape_status(num_tokens, num_experts, top_k, hidden, inter, dtype)) return st;
  const int64_t rows = (int64_t)2 * inter;
  SP_CHECK_ARG(x_stride >= hidden && h_stride >= inter && scales_expert_stride >= rows);
  SP_CHECK_ARG(codes_expert_stride >= rows * (hidden / 4) && meta_expert_stride >= rows * (hidden / 8));
  SP_CHECK_ARG(x_stride % 8 == 0 && h_stride % 8 == 0 && codes_expert_stride % 16 == 0 && meta_expert_stride % 8 == 0);
  SP_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)h & 15) == 0 && ((uintptr_t)codes & 15) == 0 &&
               ((uintptr_t)meta & 7) == 0 && ((uintptr_t)scales & 1) == 0);
  SP_CHECK_ARG(inter / (8 * sp::kQmoeNW) <= 65535);
  const int NP = (int)num_tokens * top_k;
  sp::QmoeGemmArgs p{(const char*)x, (const char*)codes, (const char*)meta, (const char*)scales, h, expert_offsets,
                     sorted_pos, nullptr, NP, top_k, num_experts, inter, hidden, x_stride, h_stride,
                     codes_expert_stride, meta_expert_stride, scales_expert_stride};
  const dim3 grid((unsigned)((NP + sp::kStreamBM - 1) / sp::kStreamBM + num_experts),
                  (unsigned)(inter / (8 * sp::kQmoeNW)));
  SP_DISPATCH_16BIT(dtype, (sp::qmoe_gemm_kernel<Tag, true><<<grid, sp::kStreamWaves * 64, 0, (hipStream_t)stream>>>(p)));
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_qmoe_down(void* tmp, const void* h, const void* codes, const void* meta, const void* scales,
                            const float* topk_weights, const int32_t* expert_offsets, const int32_t* sorted_pos,
                            int64_t num_tokens, int top_k, int num_experts, int hidden, int inter, int64_t h_stride,
                            int64_t tmp_stride, int64_t codes_expert_stride, int64_t meta_expert_stride,
                            int64_t scales_expert_stride, int dtype, void* stream) {
  SP_CHECK_ARG(num_tokens >= 0 && top_k >= 0 && num_experts >= 0 && hidden >= 0 && inter >= 0);
  SP_CHECK_ARG(tmp && h && codes && meta && scales && topk_weights && expert_offsets && sorted_pos);
  if (num_tokens == 0) return SP_OK;
  if (const int st = qmoe_shape_status(num_tokens, num_experts, top_k, hidden, inter, dtype)) return st;
  SP_CHECK_ARG(h_stride >= inter && tmp_stride >= hidden && scales_expert_stride >= hidden);
  SP_CHECK_ARG(codes_expert_stride >= (int64_t)hidden * (inter / 4) && meta_expert_stride >= (int64_t)hidden * (inter / 8));
  SP_CHECK_ARG(h_stride % 8 == 0 && tmp_stride % 8 == 0 && codes_expert_stride % 16 == 0 && meta_expert_stride % 8 == 0);
  SP_CHECK_ARG(((uintptr_t)h & 15) == 0 && ((uintptr_t)tmp & 15) == 0 && ((uintptr_t)codes & 15) == 0 &&
               ((uintptr_t)meta & 7) == 0 && ((uintptr_t)scales & 1) == 0);
  SP_CHECK_ARG(hidden / (16 * sp::kQmoeNW) <= 65535);
  const int NP = (int)num_tokens * top_k;
  sp::QmoeGemmArgs p{(const char*)h, (const char*)codes, (const char*)meta, (const char*)scales, tmp, expert_offsets,
                     sorted_pos, topk_weights, NP, top_k, num_experts, hidden, inter, h_stride, tmp_stride,
                     codes_expert_stride, meta_expert_stride, scales_expert_stride};
  const dim3 grid((unsigned)((NP + sp::kStreamBM - 1) / sp::kStreamBM + num_experts),
                  (unsigned)(hidden / (16 * sp::kQmoeNW)));
  SP_DISPATCH_16BIT(dtype, (sp::qmoe_gemm_kernel<Tag, false><<<grid, sp::kStreamWaves * 64, 0, (hipStream_t)stream>>>(p)));
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_qmoe_combine(void* out, const void* tmp, const void* base, const int32_t* topk_ids,
                               int64_t num_tokens, int top_k, int num_experts, int hidden, int64_t tmp_stride,
                               int64_t base_stride, int64_t out_stride, int order, int dtype, void* stream) {
  SP_CHECK_ARG(num_tokens >= 0 && top_k >= 0 && num_experts >= 0 && hidden >= 0);
  SP_CHECK_ARG(out && tmp && base && topk_ids);
  if (num_tokens == 0) return SP_OK;
  if (const int st = qmoe_shape_status(num_tokens, num_experts, top_k, hidden, 64, dtype)) return st;
  if (order != 0 && order != 1) return SP_ERR_UNSUPPORTED;
  SP_CHECK_ARG(tmp_stride >= hidden && base_stride >= hidden && out_stride >= hidden);
  SP_CHECK_ARG(tmp_stride % 8 == 0 && base_stride % 8 == 0 && out_stride % 8 == 0);
  SP_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)tmp & 15) == 0 && ((uintptr_t)base & 15) == 0);
  const int64_t col_blocks = ((int64_t)hidden / 8 + 255) / 256;
  SP_CHECK_ARG(col_blocks <= 65535);
  const dim3 grid((unsigned)num_tokens, (unsigned)col_blocks);
  SP_DISPATCH_16BIT(dtype, (sp::qmoe_combine_kernel<Tag><<<grid, 256, 0, (hipStream_t)stream>>>(
                               (char*)out, (const char*)tmp, (const char*)base, topk_ids, top_k, num_experts, hidden,
                               order, tmp_stride, base_stride, out_stride)));
  SP_LAUNCH_CHECK();
  return SP_OK;
}
