// The weight-streaming GEMM core that gemm_skinny.hip, moe.hip (moe_gemm_kernel) and delta.hip (delta_mm_kernel) share.
//
// Geometry.  A workgroup is 8 waves and owns one 16-row tile of the weight matrix (the A operand of
// v_mfma_f32_16x16x32: 16 output columns) x one or more 16-row sub-blocks of activations (the B operand).  The 8 waves
// take the k-steps (32 elements of the reduction) round-robin, so at any moment the workgroup reads 512 contiguous
// bytes of each of its 16 weight rows.  Per k-step a lane loads 16 B of W and 16 B of each activation sub-block straight
// into the operand registers; UNROLL k-steps of loads are in flight per wave before the first MFMA consumes one.  Each
// wave parks its 16x16 partial tiles in red[wave][sub-block][16 * 17], and after one barrier the tiles are summed in
// ascending wave order, every addition rounded on its own; the kernel's epilogue rounds the sum once.
//
// Why nothing goes through LDS on the way in: at these row counts the product is a pure stream of the weight matrix (2
// flop per weight byte per row, HBM-bound); every weight byte is read once by one lane, so an LDS hop is pure overhead,
// and the activations of a workgroup (<= 32 x K) are re-read out of L2.
//
// Grouped form (MoE: group = expert; delta: group = adapter slot).  The rows are sorted by group (group_sort.hip: ONE
// workgroup, thread i counts the groups of the i-th contiguous chunk of keys into its own LDS column, a flat prefix
// over [group][thread] gives every (group, thread) its first entry, and the thread writes its chunk in order - no
// atomic, the order is a function of the keys alone).  grid.x = ceil(rows / BM) + groups row blocks, an upper bound
// computed on the host; wave 0 finds the (group, first row) of block blockIdx.x from the offsets with one wave prefix
// sum (find_row_block) and the workgroup exits if there is none, so a group without rows costs no weight traffic.
//
// BATCH INVARIANCE.  The k-steps of a wave, their order and the order over the waves are functions of the reduction
// length alone; a row's position inside its block only selects the lane column of the MFMA, and rows that are absent
// feed zeros into columns of their own.  So the bits of an output row depend on that row's input and its group's
// weights only, and the three kernels agree bit for bit on equal operands (tests/test_gpu_stream_gemm.py).
//
// Safety rules.  Offsets read from device memory are clamped to [0, total] before they are used; every sorted entry is
// checked against [0, total) before an address is formed from it (block_rows: anything else becomes -1 and is never
// loaded or stored); rows past a group's end are never touched; byte offsets are 64-bit.
//
// Limits.  kMaxGroups = 64: find_row_block is ONE wave's prefix sum, and the sort's [group][thread] table is 64 x 128
// ints = 32 KB of LDS.  kSortThreads = 128 and the 32-row block (kStreamMB = 2 sub-blocks) are the kernels' shape.
#pragma once
#include "sp_common.h"

namespace sp {

constexpr int kStreamWaves = 8;
constexpr int kStreamMB = 2;                 // 16-row activation sub-blocks of a grouped workgroup
constexpr int kStreamBM = 16 * kStreamMB;    // rows of a grouped workgroup
constexpr int kMaxGroups = 64;
constexpr int kSortThreads = 128;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <typename Tag>
__device__ __forceinline__ f32x4 mfma_16x16x32(const u32x4& a, const u32x4& b, const f32x4& c);
template <>
__device__ __forceinline__ f32x4 mfma_16x16x32<bf16_tag>(const u32x4& a, const u32x4& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0,
                                                 0);
}
template <>
__device__ __forceinline__ f32x4 mfma_16x16x32<f16_tag>(const u32x4& a, const u32x4& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ u32x4 ld16_nt(const void* p) { return __builtin_nontemporal_load((const u32x4*)p); }

// stable counting sort of keys[0 .. n) by group (group_sort.hip): offsets[groups + 1], sorted[n]; keys outside
// [0, groups) are left out and offsets[groups] counts the rest.  groups <= kMaxGroups.  The caller checks the launch
void launch_group_sort(int32_t* offsets, int32_t* sorted, const int32_t* keys, int n, int groups, hipStream_t stream);

// Called by wave 0: s_loc = {group, first row, end of the group's rows} of row block blockIdx.x, or {-1} if there is
// none.  offsets[groups + 1] is clamped to [0, total]; groups <= 64.  The caller's __syncthreads() publishes s_loc
template <int BM>
__device__ __forceinline__ void find_row_block(const int32_t* offsets, int groups, int total, int* s_loc) {
  const int lane = threadIdx.x & 63, blk = blockIdx.x;
  int b = 0, en = 0, nb = 0;
  if (lane < groups) {
    b = min(max(offsets[lane], 0), total);
    en = min(max(offsets[lane + 1], b), total);
    nb = (en - b + BM - 1) / BM;
  }
  int incl = nb;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  const unsigned long long m = __ballot(lane < groups && blk < incl);
  if (m == 0) {
    if (lane == 0) s_loc[0] = -1;
  } else if (lane == __ffsll((long long)m) - 1) {         // the first such group has rows
    s_loc[0] = lane;
    s_loc[1] = b + (blk - (incl - nb)) * BM;
    s_loc[2] = en;
  }
}

// Threads 0 .. BM - 1: s_row[tid] = sorted[row0 + tid], or -1 past the group's end or outside [0, total).  Returns what
// the thread wrote (-1 for the other threads); the caller's __syncthreads() publishes s_row
template <int BM>
__device__ __forceinline__ int block_rows(int* s_row, const int32_t* sorted, int row0, int row_end, int total) {
  const int tid = threadIdx.x;
  int row = -1;
  if (tid < BM) {
    if (row0 + tid < row_end) {
      row = sorted[row0 + tid];
      if ((unsigned)row >= (unsigned)total) row = -1;
    }
    s_row[tid] = row;
  }
  return row;
}

// The dense k-step loop of a wave: acc[nw * NX + nx] += W fragment nw . x fragment nx over k-steps wave, wave + 8, ...
// below `ksteps`, in ascending order.  wp / xp point at the lane's 16 B of k-step 0; x fragments with xvalid false are
// zeros and are never loaded (xvalid is 0 / 1).  All loads of a group of UNROLL k-steps are issued before its MFMAs; the tail takes one
// k-step at a time.  NT: non-temporal weight loads
template <typename Tag, int NW, int NX, int UNROLL, bool NT>
__device__ __forceinline__ void stream_ksteps(f32x4 (&acc)[NW * NX], const char* const (&wp)[NW],
                                              const char* const (&xp)[NX], const int (&xvalid)[NX], int wave,
                                              int ksteps) {
  const u32x4 zero = {0u, 0u, 0u, 0u};
  int ks = wave;
  for (; ks + (UNROLL - 1) * kStreamWaves < ksteps; ks += UNROLL * kStreamWaves) {
    u32x4 wf[UNROLL][NW], xf[UNROLL][NX];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t off = (int64_t)(ks + u * kStreamWaves) * 64;
#pragma unroll
      for (int nw = 0; nw < NW; ++nw) wf[u][nw] = NT ? ld16_nt(wp[nw] + off) : ld16(wp[nw] + off);
#pragma unroll
      for (int nx = 0; nx < NX; ++nx) xf[u][nx] = xvalid[nx] ? ld16(xp[nx] + off) : zero;
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
#pragma unroll
      for (int nw = 0; nw < NW; ++nw)
#pragma unroll
        for (int nx = 0; nx < NX; ++nx)
          acc[nw * NX + nx] = mfma_16x16x32<Tag>(wf[u][nw], xf[u][nx], acc[nw * NX + nx]);
  }
  for (; ks < ksteps; ks += kStreamWaves) {
    const int64_t off = (int64_t)ks * 64;
    u32x4 xf[NX];
#pragma unroll
    for (int nx = 0; nx < NX; ++nx) xf[nx] = xvalid[nx] ? ld16(xp[nx] + off) : zero;
#pragma unroll
    for (int nw = 0; nw < NW; ++nw) {
      const u32x4 wf = NT ? ld16_nt(wp[nw] + off) : ld16(wp[nw] + off);
#pragma unroll
      for (int nx = 0; nx < NX; ++nx) acc[nw * NX + nx] = mfma_16x16x32<Tag>(wf, xf[nx], acc[nw * NX + nx]);
    }
  }
}

// acc[t][r] = partial of (lane column r16 = lane & 15, tile row 4 q + r, q = lane >> 4) of tile t: park it for the sum
// over the waves
template <int NTILE>
__device__ __forceinline__ void park_tile(float (*red)[NTILE][16 * 17], int wave, int r16, int q,
                                          const f32x4 (&acc)[NTILE]) {
#pragma unroll
  for (int t = 0; t < NTILE; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][t][(4 * q + r) * 17 + r16] = acc[t][r];
}

// The sum over the waves of element (tile row `col`, lane column `row`) of tile t, in ascending wave order from +0,
// every addition rounded on its own.  ONE form for the three kernels: starting from red[0] instead (delta.hip's earlier
// form) differs only where a partial is -0.f, which an MFMA chain from a +0 accumulator cannot produce under
// round-to-nearest (x + -x and +0 + -0 are +0); profiles/stream_gemm_refactor.txt holds the A/B
template <int NTILE>
__device__ __forceinline__ float sum_tile(float (*red)[NTILE][16 * 17], int t, int col, int row) {
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < kStreamWaves; ++w) s = __fadd_rn(s, red[w][t][col * 17 + row]);
  return s;
}

}  // namespace sp
