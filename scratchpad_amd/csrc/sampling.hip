// Sampler kernels for gfx950: greedy argmax, temperature softmax, and top-k / top-p / min-p
// filtering + sampling without a sort.
//
// Replaces nn/layers/sampler.py:63-75 (argmax / div_ + softmax), 195-232 (the torch top-k/top-p/
// min-p sampler and top_p_normalize_probs_torch) and the flashinfer entry points wrapped by
// nn/kernels/sampling.py (top_k_renorm_probs 19-50, top_p_renorm_probs 64-97,
// top_k_top_p_sampling_from_probs 209-292, min_p_sampling_from_probs 319-373).
//
// The reference sorts every row (128k floats) and takes an fp32 cumulative sum.  Here one
// workgroup owns a row and finds the cut of the (p desc, id asc) ranking by a 3-level radix
// descent over the fp32 bit pattern (11+11+10 bits): per level an LDS histogram of count, mass
// and minimum per digit, a scan from the top digit down, and the first digit whose smallest
// member is dropped is refined further.  Mass is carried as integers, fx(p) = floor(p * 2^48),
// so LDS atomics commute and the result does not depend on arrival order: all TP ranks draw the
// same token from the same probabilities (what sampler.py:146-157 asks of the kernels).
// The row (513 KB at vocab 128256) stays in the XCD's L2 between passes; HBM sees it once.
//
// tests/test_gpu_sampling.py and tests/test_gpu_sampling_rows.py hold the kernels to the CPU statement
// of the same definition, exactly (ids, keep counts), the latter on every row of tie-heavy batches.
#include "sp_common.h"

namespace sp {

constexpr int kSampThreads = 1024;
constexpr int kSampWaves = kSampThreads / 64;
constexpr int kBins = 2048;
constexpr double kFxOne = 281474976710656.0;  // 2^48

__device__ __forceinline__ uint32_t prob_bits(float p) { return p > 0.f ? as_u32(p) : 0u; }  // NaN, -x -> 0
__device__ __forceinline__ uint64_t fx_of_bits(uint32_t b) { return (uint64_t)((double)as_f32(b) * kFxOne); }

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d) {
  const uint32_t lo = __shfl_up((uint32_t)v, d, 64), hi = __shfl_up((uint32_t)(v >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int d) {
  const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}

struct SelectArgs {
  const float* probs;
  int64_t row_stride;
  const int32_t* top_ks;  // nullable: no rank limit
  const float* top_ps;    // nullable: no mass limit
  const float* min_ps;    // nullable: no floor
  const float* uniform;   // SAMPLE mode
  int vocab;
  int64_t* out_ids;       // SAMPLE mode
  float* renorm;          // RENORM mode
  int64_t renorm_stride;
  int32_t* keep_count;    // nullable
};

struct SelectShared {
  uint32_t cnt[kBins];
  uint64_t mass[kBins];
  uint32_t mn[kBins];
  uint32_t wave_cnt[kSampWaves];
  uint64_t wave_mass[kSampWaves];
  int sel;
  uint32_t sel_cnt;
  uint32_t base_cnt;   // tokens ranked above the current digit range
  uint64_t base_mass;  // their mass
  uint64_t grand_mass;
  uint32_t red_u32[kSampWaves];
  uint32_t seg_ties[kSampWaves];
  uint64_t seg_mass[kSampWaves];
};

// The cut, as every thread sees it after select_cut(): a token with pattern b is kept iff
//   b > pivot, or b == pivot and it is among the first `ties_kept` such tokens in id order.
struct Cut {
  uint32_t pivot;
  uint32_t ties_kept;
  uint32_t above;   // number of tokens with b > pivot
  uint64_t total;   // kept mass
};

__device__ Cut select_cut(const SelectArgs& a, const float* __restrict__ row, SelectShared& sh, int b) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int vocab = a.vocab;
  const int64_t top_k = a.top_ks ? (int64_t)max(a.top_ks[b], 0) : (int64_t)1 << 40;
  const uint64_t top_p_fx = a.top_ps ? (uint64_t)((double)a.top_ps[b] * kFxOne) : ~(uint64_t)0;

  // p_max (only needed for the min-p floor)
  float thr = 0.f;
  if (a.min_ps) {
    uint32_t mx = 0;
    for (int i = tid; i < vocab; i += kSampThreads) mx = max(mx, prob_bits(row[i]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
    if (lane == 0) sh.red_u32[wave] = mx;
    __syncthreads();
    mx = 0;
#pragma unroll
    for (int w = 0; w < kSampWaves; ++w) mx = max(mx, sh.red_u32[w]);
    thr = as_f32(mx) * a.min_ps[b];
  }
  if (tid == 0) { sh.base_cnt = 0; sh.base_mass = 0; }

  uint32_t prefix = 0;   // digits fixed so far
  bool keep_all = false;
#pragma unroll 1
  for (int level = 0; level < 3; ++level) {
    const int shift = level == 0 ? 21 : (level == 1 ? 10 : 0);
    const int width = level == 2 ? 10 : 11;
    const uint32_t mask = (1u << width) - 1;
    for (int i = tid; i < kBins; i += kSampThreads) { sh.cnt[i] = 0; sh.mass[i] = 0; sh.mn[i] = 0xffffffffu; }
    if (tid == 0) sh.sel = -1;
    __syncthreads();
    for (int i = tid; i < vocab; i += kSampThreads) {
      const uint32_t bits = prob_bits(row[i]);
      if (level == 0 || (bits >> (shift + width)) == prefix) {
        const uint32_t d = (bits >> shift) & mask;
        atomicAdd(&sh.cnt[d], 1u);
        atomicAdd((unsigned long long*)&sh.mass[d], (unsigned long long)fx_of_bits(bits));
        atomicMin(&sh.mn[d], bits);
      }
    }
    __syncthreads();
    // scan digits from the top: thread t owns digits (2047-2t, 2046-2t)
    const int d0 = kBins - 1 - 2 * tid, d1 = d0 - 1;
    const uint32_t c0 = sh.cnt[d0], c1 = sh.cnt[d1];
    const uint64_t m0 = sh.mass[d0], m1 = sh.mass[d1];
    uint32_t ci = c0 + c1;
    uint64_t mi = m0 + m1;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t cu = __shfl_up(ci, off, 64);
      const uint64_t mu = shfl_up_u64(mi, off);
      if (lane >= off) { ci += cu; mi += mu; }
    }
    if (lane == 63) { sh.wave_cnt[wave] = ci; sh.wave_mass[wave] = mi; }
    __syncthreads();
    uint32_t c_above = sh.base_cnt + ci - (c0 + c1);
    uint64_t m_above = sh.base_mass + mi - (m0 + m1);
    for (int w = 0; w < wave; ++w) { c_above += sh.wave_cnt[w]; m_above += sh.wave_mass[w]; }
    // does the smallest member of the digit fall outside the kept prefix?
    auto fails = [&](uint32_t c, uint64_t m, uint32_t mn, uint32_t ca, uint64_t ma) -> bool {
      if (c == 0) return false;
      return (int64_t)ca + (int64_t)c > top_k || ma + m - fx_of_bits(mn) > top_p_fx || as_f32(mn) < thr;
    };
    const bool f0 = fails(c0, m0, sh.mn[d0], c_above, m_above);
    const bool f1 = fails(c1, m1, sh.mn[d1], c_above + c0, m_above + m0);
    if (f0) atomicMax(&sh.sel, d0);
    else if (f1) atomicMax(&sh.sel, d1);
    if (level == 0 && tid == kSampThreads - 1) sh.grand_mass = m_above + m0 + m1;
    __syncthreads();
    const int sel = sh.sel;
    if (sel < 0) { keep_all = true; break; }   // only possible at level 0 (see header)
    __syncthreads();
    if (sel == d0) { sh.base_cnt = c_above; sh.base_mass = m_above; sh.sel_cnt = c0; }
    if (sel == d1) { sh.base_cnt = c_above + c0; sh.base_mass = m_above + m0; sh.sel_cnt = c1; }
    prefix = (prefix << width) | (uint32_t)sel;
    __syncthreads();
  }

  Cut cut;
  if (keep_all) {
    cut.pivot = 0;
    cut.ties_kept = 0xffffffffu;
    cut.above = 0;            // not used when everything is kept
    cut.total = sh.grand_mass;
    return cut;
  }
  const uint32_t m = sh.sel_cnt, above = sh.base_cnt;
  const uint64_t mass_above = sh.base_mass, w = fx_of_bits(prefix);
  uint64_t t = m;
  t = min(t, (uint64_t)max((int64_t)0, top_k - (int64_t)above));
  if (mass_above > top_p_fx) t = 0;
  else if (w > 0) t = min(t, (top_p_fx - mass_above) / w + 1);
  if (as_f32(prefix) < thr) t = 0;
  cut.pivot = prefix;
  cut.ties_kept = (uint32_t)t;
  cut.above = above;
  cut.total = mass_above + t * w;
  return cut;
}

// Per-wave id segments: mass of tokens above the pivot and number of pivot ties in each.
__device__ __forceinline__ int seg_len(int vocab) { return (((vocab + kSampWaves - 1) / kSampWaves) + 63) & ~63; }

__device__ void segment_totals(const float* __restrict__ row, int vocab, const Cut& cut, SelectShared& sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = seg_len(vocab), lo = wave * seg, hi = min(lo + seg, vocab);
  uint64_t msum = 0;
  uint32_t ties = 0;
  for (int i = lo + lane; i < hi; i += 64) {
    const uint32_t bits = prob_bits(row[i]);
    if (bits > cut.pivot) msum += fx_of_bits(bits);
    ties += bits == cut.pivot;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    msum += shfl_xor_u64(msum, off);
    ties += __shfl_xor(ties, off, 64);
  }
  if (lane == 0) { sh.seg_mass[wave] = msum; sh.seg_ties[wave] = ties; }
  __syncthreads();
}

template <bool SAMPLE>
__global__ __launch_bounds__(kSampThreads) void select_kernel(SelectArgs a) {
  __shared__ SelectShared sh;
  const int b = blockIdx.x;
  const float* __restrict__ row = a.probs + (int64_t)b * a.row_stride;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Cut cut = select_cut(a, row, sh, b);
  const uint64_t wpiv = fx_of_bits(cut.pivot);
  if (a.keep_count && threadIdx.x == 0) {
    // tokens kept; under keep-all every token counts (zeros included, they carry no mass)
    a.keep_count[b] = cut.ties_kept == 0xffffffffu ? a.vocab : (int32_t)(cut.above + cut.ties_kept);
  }
  segment_totals(row, a.vocab, cut, sh);
  const int seg = seg_len(a.vocab);

  if (SAMPLE) {
    if (cut.total == 0) {               // degenerate row (all zero / NaN): token 0, like an empty draw
      if (threadIdx.x == 0) a.out_ids[b] = 0;
      return;
    }
    uint64_t r = (uint64_t)((double)a.uniform[b] * (double)cut.total);
    r = min(r, cut.total - 1);
    // which segment holds r
    uint64_t run = 0;
    uint32_t ties_before = 0;
    int target = -1;
    for (int w = 0; w < kSampWaves; ++w) {
      const uint32_t tk = (uint32_t)min((uint64_t)sh.seg_ties[w],
                                        (uint64_t)(cut.ties_kept > ties_before ? cut.ties_kept - ties_before : 0));
      const uint64_t wm = sh.seg_mass[w] + (uint64_t)tk * wpiv;
      if (run + wm > r) { target = w; break; }
      run += wm;
      ties_before += sh.seg_ties[w];
    }
    if (wave != target) return;        // target >= 0 because r < total
    const int lo = wave * seg, hi = min(lo + seg, a.vocab);
    for (int base = lo; base < hi; base += 64) {
      const int i = base + lane;
      const uint32_t bits = i < hi ? prob_bits(row[i]) : 0u;
      const bool tie = i < hi && bits == cut.pivot;
      const uint64_t tmask = __ballot(tie);
      const uint32_t rank = ties_before + __popcll(tmask & ((1ull << lane) - 1));
      uint64_t wt = 0;
      if (i < hi) {
        if (bits > cut.pivot) wt = fx_of_bits(bits);
        else if (tie && rank < cut.ties_kept) wt = wpiv;
      }
      uint64_t inc = wt;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint64_t u = shfl_up_u64(inc, off);
        if (lane >= off) inc += u;
      }
      const uint64_t hit = __ballot(run + inc > r);
      if (hit) {
        if (lane == 0) a.out_ids[b] = base + (__ffsll((unsigned long long)hit) - 1);
        return;
      }
      run += ((uint64_t)__shfl((uint32_t)(inc >> 32), 63, 64) << 32) | __shfl((uint32_t)inc, 63, 64);
      ties_before += __popcll(tmask);
    }
  } else {
    float* __restrict__ out = a.renorm + (int64_t)b * a.renorm_stride;
    const float denom = (float)((double)cut.total / kFxOne);
    uint32_t ties_before = 0;
    for (int w = 0; w < wave; ++w) ties_before += sh.seg_ties[w];
    const int lo = wave * seg, hi = min(lo + seg, a.vocab);
    for (int base = lo; base < hi; base += 64) {
      const int i = base + lane;
      const float p = i < hi ? row[i] : 0.f;
      const uint32_t bits = prob_bits(p);
      const bool tie = i < hi && bits == cut.pivot;
      const uint64_t tmask = __ballot(tie);
      const uint32_t rank = ties_before + __popcll(tmask & ((1ull << lane) - 1));
      const bool keep = bits > cut.pivot || (tie && rank < cut.ties_kept);
      // as_f32(bits), not p: a kept bad entry (NaN, negative: they rank as zero) renormalises to 0
      if (i < hi) out[i] = (keep && cut.total) ? as_f32(bits) / denom : 0.f;
      ties_before += __popcll(tmask);
    }
  }
}

// per-thread scan of a row for (maximum, first index): 16-byte loads (8 x 16-bit or 4 x fp32 values) when
// the row allows it - a 2-byte load per lane leaves the memory pipeline at a quarter of its rate
template <typename Tag>
__device__ __forceinline__ void thread_argmax(const void* __restrict__ logits, int64_t base, int cols, int tid,
                                              float& best, int& idx) {
  constexpr int V = Elem<Tag>::kVec;
  best = -INFINITY;
  idx = 0x7fffffff;
  const char* row = (const char*)logits + base * Elem<Tag>::kBytes;
  int done = 0;
  if ((((uintptr_t)row) & 15) == 0) {
    const int nvec = cols / V;
    for (int i = tid; i < nvec; i += kSampThreads) {
      float f[V];
      unpack16<Tag>(ld16(row + (int64_t)i * 16), f);
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (f[e] > best || idx == 0x7fffffff) { best = f[e]; idx = i * V + e; }   // ids ascend per thread
    }
    done = nvec * V;
  }
  for (int i = done + tid; i < cols; i += kSampThreads) {
    const float v = Elem<Tag>::load(logits, base + i);
    if (v > best || idx == 0x7fffffff || (v == best && i < idx)) { best = v; idx = i; }
  }
}

// ---- greedy argmax (sampler.py:63-65): first maximal index, NaN-free input assumed -----------
template <typename Tag>
__global__ __launch_bounds__(kSampThreads) void argmax_kernel(const void* __restrict__ logits, int64_t row_stride,
                                                              int vocab, int64_t* __restrict__ out) {
  __shared__ float s_val[kSampWaves];
  __shared__ int s_idx[kSampWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = (int64_t)b * row_stride;
  float best;
  int idx;
  thread_argmax<Tag>(logits, base, vocab, tid, best, idx);
  auto better = [](float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); };
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(idx, off, 64);
    if (better(ov, oi, best, idx)) { best = ov; idx = oi; }
  }
  if (lane == 0) { s_val[wave] = best; s_idx[wave] = idx; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kSampWaves; ++w)
      if (better(s_val[w], s_idx[w], best, idx)) { best = s_val[w]; idx = s_idx[w]; }
    out[b] = idx == 0x7fffffff ? 0 : idx;
  }
}

// ---- vocab-parallel greedy: every rank reduces its own vocab shard to one (value, global index)
// pair per row, the pairs ([bs, 2] words per rank instead of [bs, vocab / tp] logits) are
// all-gathered, and the merge picks the maximum with the lowest global index - the token
// torch.argmax would return on the gathered row (logits_processor.py:362-369 + sampler.py:63-65).
template <typename Tag>
__global__ __launch_bounds__(kSampThreads) void argmax_shard_kernel(const void* __restrict__ logits,
                                                                    int64_t row_stride, int cols,
                                                                    int index_offset,
                                                                    int32_t* __restrict__ pairs) {
  __shared__ float s_val[kSampWaves];
  __shared__ int s_idx[kSampWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = (int64_t)b * row_stride;
  float best;
  int idx;
  thread_argmax<Tag>(logits, base, cols, tid, best, idx);
  auto better = [](float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); };
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(idx, off, 64);
    if (better(ov, oi, best, idx)) { best = ov; idx = oi; }
  }
  if (lane == 0) { s_val[wave] = best; s_idx[wave] = idx; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kSampWaves; ++w)
      if (better(s_val[w], s_idx[w], best, idx)) { best = s_val[w]; idx = s_idx[w]; }
    // an empty shard (cols == 0: every column of this rank is vocabulary padding) never wins
    pairs[2 * b] = (int32_t)as_u32(idx == 0x7fffffff ? -INFINITY : best);
    pairs[2 * b + 1] = idx == 0x7fffffff ? 0x7fffffff : idx + index_offset;
  }
}

// pairs: [shards][bs][2]; one thread per row
__global__ __launch_bounds__(256) void argmax_merge_kernel(const int32_t* __restrict__ pairs, int shards,
                                                           int bs, int64_t* __restrict__ out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= bs) return;
  float best = -INFINITY;
  int idx = 0x7fffffff;
  for (int r = 0; r < shards; ++r) {
    const float v = as_f32((uint32_t)pairs[((int64_t)r * bs + b) * 2]);
    const int i = pairs[((int64_t)r * bs + b) * 2 + 1];
    if (v > best || (v == best && i < idx) || idx == 0x7fffffff) { best = v; idx = i; }
  }
  out[b] = idx == 0x7fffffff ? 0 : idx;
}

// ---- probs = softmax(logits / T) in place, fp32 (sampler.py:71-73) ---------------------------
__global__ __launch_bounds__(kSampThreads) void softmax_temperature_kernel(float* __restrict__ x, int64_t row_stride,
                                                                          const float* __restrict__ temps, int vocab) {
  __shared__ float s_red[kSampWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* __restrict__ row = x + (int64_t)b * row_stride;
  const float t = temps ? temps[b] : 1.f;
  float mx = -INFINITY;
  for (int i = tid; i < vocab; i += kSampThreads) mx = fmaxf(mx, row[i] / t);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  if (lane == 0) s_red[wave] = mx;
  __syncthreads();
  mx = s_red[0];
#pragma unroll
  for (int w = 1; w < kSampWaves; ++w) mx = fmaxf(mx, s_red[w]);
  __syncthreads();
  float sum = 0.f;
  for (int i = tid; i < vocab; i += kSampThreads) sum += expf(row[i] / t - mx);
  sum = wave_sum(sum);
  if (lane == 0) s_red[wave] = sum;
  __syncthreads();
  sum = 0.f;
#pragma unroll
  for (int w = 0; w < kSampWaves; ++w) sum += s_red[w];
  const float inv = 1.f / sum;
  for (int i = tid; i < vocab; i += kSampThreads) row[i] = expf(row[i] / t - mx) * inv;
}

// ---- log-probabilities of a few tokens per row (sp_logprobs) ---------------------------------
// Replaces nn/layers/sampler.py:66-67, 116-141, 234-263 and nn/layers/logits_processor.py:378-460: a log_softmax (or
// renormalise + log + clamp) over [rows, vocab], a topk over the result and gathers out of it, for a few dozen numbers
// per row.  Two launches, no [rows, vocab] intermediate:
//   partial: workgroup (row, split) streams its slice of the row ONCE with 16-byte loads and keeps, per lane, the
//            running (max, sum-exp) of a logit row or the integer mass floor(p * 2^48) of a probability row, and per
//            WAVE the slice's best `top_k` entries as a sorted list held one entry per lane: a candidate above the
//            list's last entry is inserted with one ballot and one lane shift, everything else costs one compare.
//            Entries are ranked by the 64-bit key (value bits made monotone, ~token id): value descending, id
//            ascending, all keys distinct - so the result does not depend on how the row was cut.
//   merge:   one workgroup per row folds the splits' statistics and lists, finds the top-p cut of a probability row
//            whose mass exceeds its top_p with select_cut() above (the row is then re-read from L2, as the sampler
//            does), and writes the asked values only.
constexpr int kLogprobMaxTopK = 32;      // = SP_LOGPROBS_MAX_TOP_K
constexpr int kLogprobMaxSplits = 32;
constexpr int kLogprobMinSlice = 4096;   // one 16-byte load per thread
constexpr int kLogprobGroups = 256;      // workgroups wanted per launch: one per compute unit
constexpr float kLogprobFloor = -3.402823466e+38f;   // finfo(float32).min

inline int logprob_splits(int num_rows, int vocab) {
  int s = kLogprobGroups / (num_rows > 0 ? num_rows : 1);
  if (s > vocab / kLogprobMinSlice) s = vocab / kLogprobMinSlice;
  if (s > kLogprobMaxSplits) s = kLogprobMaxSplits;
  return s > 1 ? s : 1;
}
inline int logprob_slice(int vocab, int splits) { return (((vocab + splits - 1) / splits) + 3) & ~3; }

struct LogprobStat {   // of one (row, split)
  float mx, sum;       // kind 0: running maximum and sum of exp(x - mx)
  uint64_t mass;       // kind 1: sum of floor(p * 2^48)
};

struct LogprobArgs {
  const float* rows;
  int64_t row_stride;
  int kind, vocab, splits, slice, max_top_k;
  const float* top_ps;
  const int64_t* chosen_ids;
  const int32_t* top_ks;
  const int32_t* ids_offsets;
  const int64_t* ids_flat;
  float* out_chosen;
  float* out_top_vals;
  int32_t* out_top_ids;
  float* out_ids_vals;
  LogprobStat* stats;   // [num_rows, splits]
  uint64_t* keys;       // [num_rows, splits, max_top_k]
};

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
  return ((uint64_t)hi << 32) | lo;
}
// larger key = ranked earlier: value descending (-0 counts as +0), then token id ascending; never 0
__device__ __forceinline__ uint64_t rank_key(float v, int id) {
  uint32_t u = as_u32(v + 0.f);
  u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
  return ((uint64_t)u << 32) | (0xffffffffu - (uint32_t)id);
}
__device__ __forceinline__ float key_value(uint64_t k) {
  uint32_t u = (uint32_t)(k >> 32);
  u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;
  return as_f32(u);
}
__device__ __forceinline__ int key_id(uint64_t k) { return (int)(0xffffffffu - (uint32_t)k); }

// The wave's list: lane l holds its l-th best key so far (0 = none yet), `thr` = the entry of lane k - 1.  Offers one
// candidate per lane (0 = none).  Wave-uniform control flow: call with all 64 lanes.
__device__ __forceinline__ void topk_offer(uint64_t& mine, uint64_t& thr, uint64_t c, int k, int lane) {
  uint64_t m = __ballot(c > thr);
  while (m) {
    const int src = __ffsll((unsigned long long)m) - 1;
    m &= m - 1;
    const uint64_t cand = shfl_u64(c, src);
    if (cand <= thr) continue;                     // the list has moved on since the ballot
    const int pos = __popcll(__ballot(mine > cand));   // sorted: the lanes above the candidate are a prefix
    const uint64_t up = shfl_up_u64(mine, 1);
    if (lane > pos) mine = up;
    else if (lane == pos) mine = cand;
    thr = shfl_u64(mine, k - 1);
  }
}

// (mx, sum) <- (mx, sum) + (omx, osum); a side that has seen nothing finite is (-inf, 0)
__device__ __forceinline__ void lse_merge(float& mx, float& sum, float omx, float osum) {
  const float nm = fmaxf(mx, omx);
  if (nm > -INFINITY) {
    sum = sum * expf(mx - nm) + osum * expf(omx - nm);
    mx = nm;
  }
}

struct LogprobLane {
  float mx = -INFINITY, sum = 0.f;
  uint64_t mass = 0;
};

__device__ __forceinline__ void logprob_stat4(LogprobLane& st, int kind, const float* f, int n) {
  if (kind == 0) {
    float nm = st.mx;
    for (int e = 0; e < n; ++e) nm = fmaxf(nm, f[e]);
    if (nm > -INFINITY) {
      float s = st.sum * expf(st.mx - nm);
      for (int e = 0; e < n; ++e) s += expf(f[e] - nm);
      st.sum = s;
      st.mx = nm;
    }
  } else {
    for (int e = 0; e < n; ++e) st.mass += fx_of_bits(prob_bits(f[e]));
  }
}

// fold the 64 lanes' statistics; every lane returns the total
__device__ __forceinline__ void logprob_wave_fold(LogprobLane& st) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lse_merge(st.mx, st.sum, __shfl_xor(st.mx, off, 64), __shfl_xor(st.sum, off, 64));
    st.mass += shfl_xor_u64(st.mass, off);
  }
}

__global__ __launch_bounds__(kSampThreads) void logprob_partial_kernel(LogprobArgs a) {
  __shared__ uint64_t s_keys[kSampWaves][kLogprobMaxTopK];
  __shared__ LogprobStat s_stat[kSampWaves];
  const int b = blockIdx.x, split = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lo = min(split * a.slice, a.vocab), hi = min(lo + a.slice, a.vocab), n = hi - lo;
  const float* __restrict__ p = a.rows + (int64_t)b * a.row_stride + lo;
  const int K = a.max_top_k;
  LogprobLane st;
  uint64_t mine = 0, thr = 0;

  // [0, head): up to the first 16-byte boundary; then nvec vectors; then [tail0, n)
  const int head = min(n, (int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2));
  const int nvec = (n - head) >> 2, tail0 = head + 4 * nvec;
  const int iters = (nvec + kSampThreads - 1) / kSampThreads;
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    const int i = it * kSampThreads + tid;
    const bool ok = i < nvec;
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    if (ok) {
      unpack16<f32_tag>(ld16(p + head + 4 * i), f);
      logprob_stat4(st, a.kind, f, 4);
    }
    if (K > 0) {
      const int id0 = lo + head + 4 * i;
#pragma unroll
      for (int e = 0; e < 4; ++e) topk_offer(mine, thr, ok ? rank_key(f[e], id0 + e) : 0, K, lane);
    }
  }
  if (wave == 0) {   // the at most 3 + 3 elements beside the vectors: lanes 0..2 and 8..10
    int i = -1;
    if (lane < head) i = lane;
    else if (lane >= 8 && tail0 + (lane - 8) < n) i = tail0 + (lane - 8);
    float x = 0.f;
    if (i >= 0) {
      x = p[i];
      logprob_stat4(st, a.kind, &x, 1);
    }
    if (K > 0) topk_offer(mine, thr, i >= 0 ? rank_key(x, lo + i) : 0, K, lane);
  }

  logprob_wave_fold(st);
  if (lane == 0) s_stat[wave] = LogprobStat{st.mx, st.sum, st.mass};
  if (lane < K) s_keys[wave][lane] = mine;
  __syncthreads();
  if (wave != 0) return;
  LogprobLane all;
  if (lane < kSampWaves) { all.mx = s_stat[lane].mx; all.sum = s_stat[lane].sum; all.mass = s_stat[lane].mass; }
  logprob_wave_fold(all);
  const int64_t slot = (int64_t)b * a.splits + split;
  if (lane == 0) a.stats[slot] = LogprobStat{all.mx, all.sum, all.mass};
  if (K > 0) {
    for (int w = 1; w < kSampWaves; ++w) topk_offer(mine, thr, lane < K ? s_keys[w][lane] : 0, K, lane);
    if (lane < K) a.keys[slot * K + lane] = mine;
  }
}

__global__ __launch_bounds__(kSampThreads) void logprob_merge_kernel(LogprobArgs a) {
  __shared__ SelectShared sh;
  __shared__ uint64_t s_top[kLogprobMaxTopK];
  __shared__ LogprobStat s_all;
  __shared__ int s_pick, s_pick_t;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* __restrict__ row = a.rows + (int64_t)b * a.row_stride;
  const int K = a.max_top_k;

  if (wave == 0) {
    LogprobLane all;
    if (lane < a.splits) {
      const LogprobStat s = a.stats[(int64_t)b * a.splits + lane];
      all.mx = s.mx; all.sum = s.sum; all.mass = s.mass;
    }
    logprob_wave_fold(all);
    if (lane == 0) s_all = LogprobStat{all.mx, all.sum, all.mass};
    if (K > 0) {
      uint64_t mine = 0, thr = 0;
      for (int s = 0; s < a.splits; ++s)
        topk_offer(mine, thr, lane < K ? a.keys[((int64_t)b * a.splits + s) * K + lane] : 0, K, lane);
      if (lane < K) s_top[lane] = mine;
    }
  }
  __syncthreads();

  // kind 0: log_softmax(row)[t] = x - lse.  kind 1: log(p / kept mass) under the cut, kLogprobFloor where dropped
  const double lse = (double)s_all.mx + log((double)s_all.sum);
  Cut cut{0u, 0xffffffffu, 0u, s_all.mass};
  uint32_t pivot_count = 0;
  if (a.kind == 1 && a.top_ps) {
    const uint64_t top_p_fx = (uint64_t)((double)a.top_ps[b] * kFxOne);
    if (s_all.mass > top_p_fx) {   // else no token has more than top_p ranked above it: all are kept
      SelectArgs sa{a.rows, a.row_stride, nullptr, a.top_ps, nullptr, nullptr, a.vocab, nullptr, nullptr, 0, nullptr};
      cut = select_cut(sa, row, sh, b);
      pivot_count = sh.sel_cnt;
      __syncthreads();
    }
  }
  const bool keep_all = cut.ties_kept == 0xffffffffu;
  const double log_total = cut.total ? log((double)cut.total / kFxOne) : 0.0;

  const int k_row = K > 0 ? (a.top_ks ? min(max(a.top_ks[b], 0), K) : K) : 0;
  const int ids_lo = a.ids_offsets ? a.ids_offsets[b] : 0;
  const int n_ids = a.ids_offsets ? max(a.ids_offsets[b + 1] - ids_lo, 0) : 0;
  const int n_chosen = a.chosen_ids ? 1 : 0;
  const int nq = n_chosen + k_row + n_ids;
#pragma unroll 1
  for (int base = 0; base < nq; base += kSampThreads) {
    const int q = base + tid;
    float* dst = nullptr;
    int64_t t = -1;
    float x = 0.f;
    if (q < nq) {
      if (q < n_chosen) {
        dst = a.out_chosen + b;
        t = a.chosen_ids[b];
      } else if (q < n_chosen + k_row) {
        const int j = q - n_chosen;
        const uint64_t key = s_top[j];
        if (key) {               // fewer than k_row tokens in the vocabulary: the rest is not written
          dst = a.out_top_vals + (int64_t)b * K + j;
          t = key_id(key);
          a.out_top_ids[(int64_t)b * K + j] = (int32_t)t;
        }
      } else {
        const int j = q - n_chosen - k_row;
        dst = a.out_ids_vals + ids_lo + j;
        t = a.ids_flat[ids_lo + j];
      }
    }
    const bool in_range = dst && t >= 0 && t < a.vocab;
    if (in_range) x = row[t];
    float result = kLogprobFloor;   // an id outside the vocabulary, a dropped or massless token
    bool pending = false;           // a token on the pivot of which only the first ties_kept are kept
    if (in_range) {
      if (a.kind == 0) {
        result = (float)((double)x - lse);
      } else {
        const uint32_t bits = prob_bits(x);
        bool kept = bits && cut.total && (keep_all || bits > cut.pivot);
        if (bits && cut.total && !keep_all && bits == cut.pivot) {
          if (cut.ties_kept >= pivot_count) kept = true;
          else if (cut.ties_kept > 0) pending = true;
        }
        if (kept) result = (float)(log((double)as_f32(bits)) - log_total);
      }
    }
    // pending tokens, one at a time: rank among the pivot's ties = ties with a lower id
    while (true) {
      if (tid == 0) s_pick = 0x7fffffff;
      __syncthreads();
      if (pending) atomicMin(&s_pick, tid);
      __syncthreads();
      const int pick = s_pick;
      if (pick == 0x7fffffff) break;
      if (tid == pick) s_pick_t = (int)t;
      __syncthreads();
      const int upto = s_pick_t;
      uint32_t before = 0;
      for (int i = tid; i < upto; i += kSampThreads) before += prob_bits(row[i]) == cut.pivot;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off, 64);
      if (lane == 0) sh.red_u32[wave] = before;
      __syncthreads();
      if (tid == pick) {
        before = 0;
        for (int w = 0; w < kSampWaves; ++w) before += sh.red_u32[w];
        if (before < cut.ties_kept) result = (float)(log((double)as_f32(cut.pivot)) - log_total);
        pending = false;
      }
      __syncthreads();
    }
    if (dst) *dst = result;
  }
}

}  // namespace sp

extern "C" int sp_argmax(const void* logits, int64_t row_stride, int batch_size, int vocab, int64_t* out_ids,
                         int dtype, void* stream) {
  SP_CHECK_ARG(batch_size >= 0 && vocab > 0);
  if (batch_size == 0) return SP_OK;
  SP_CHECK_ARG(logits && out_ids && row_stride >= vocab);
  SP_DISPATCH_DTYPE(dtype, (sp::argmax_kernel<Tag><<<dim3(batch_size), sp::kSampThreads, 0, (hipStream_t)stream>>>(
                               logits, row_stride, vocab, out_ids)));
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_argmax_shard(const void* logits, int64_t row_stride, int batch_size, int cols, int index_offset,
                               int32_t* out_pairs, int dtype, void* stream) {
  SP_CHECK_ARG(batch_size >= 0 && cols >= 0 && index_offset >= 0);
  if (batch_size == 0) return SP_OK;
  SP_CHECK_ARG(logits && out_pairs && row_stride >= cols);
  SP_DISPATCH_DTYPE(dtype, (sp::argmax_shard_kernel<Tag><<<dim3(batch_size), sp::kSampThreads, 0,
                                                          (hipStream_t)stream>>>(logits, row_stride, cols,
                                                                                 index_offset, out_pairs)));
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_argmax_merge(const int32_t* pairs, int num_shards, int batch_size, int64_t* out_ids,
                               void* stream) {
  SP_CHECK_ARG(batch_size >= 0 && num_shards > 0);
  if (batch_size == 0) return SP_OK;
  SP_CHECK_ARG(pairs && out_ids);
  sp::argmax_merge_kernel<<<dim3((batch_size + 255) / 256), 256, 0, (hipStream_t)stream>>>(pairs, num_shards,
                                                                                            batch_size, out_ids);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_softmax_temperature(float* logits, int64_t row_stride, const float* temperatures, int batch_size,
                                      int vocab, void* stream) {
  SP_CHECK_ARG(batch_size >= 0 && vocab > 0);
  if (batch_size == 0) return SP_OK;
  SP_CHECK_ARG(logits && row_stride >= vocab);
  sp::softmax_temperature_kernel<<<dim3(batch_size), sp::kSampThreads, 0, (hipStream_t)stream>>>(
      logits, row_stride, temperatures, vocab);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_top_k_top_p_min_p_sample(const float* probs, int64_t row_stride, const int32_t* top_ks,
                                           const float* top_ps, const float* min_ps, const float* uniform,
                                           int batch_size, int vocab, int64_t* out_ids, int32_t* keep_count,
                                           void* stream) {
  SP_CHECK_ARG(batch_size >= 0 && vocab > 0);
  if (batch_size == 0) return SP_OK;
  SP_CHECK_ARG(probs && uniform && out_ids && row_stride >= vocab);
  sp::SelectArgs a{probs, row_stride, top_ks, top_ps, min_ps, uniform, vocab, out_ids, nullptr, 0, keep_count};
  sp::select_kernel<true><<<dim3(batch_size), sp::kSampThreads, 0, (hipStream_t)stream>>>(a);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_top_k_top_p_min_p_renorm(const float* probs, int64_t row_stride, const int32_t* top_ks,
                                           const float* top_ps, const float* min_ps, int batch_size, int vocab,
                                           float* out, int64_t out_stride, int32_t* keep_count, void* stream) {
  SP_CHECK_ARG(batch_size >= 0 && vocab > 0);
  if (batch_size == 0) return SP_OK;
  SP_CHECK_ARG(probs && out && row_stride >= vocab && out_stride >= vocab);
  sp::SelectArgs a{probs, row_stride, top_ks, top_ps, min_ps, nullptr, vocab, nullptr, out, out_stride, keep_count};
  sp::select_kernel<false><<<dim3(batch_size), sp::kSampThreads, 0, (hipStream_t)stream>>>(a);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" size_t sp_logprobs_workspace_bytes(int num_rows, int vocab, int max_top_k) {
  if (num_rows <= 0 || vocab <= 0 || max_top_k < 0 || max_top_k > sp::kLogprobMaxTopK) return 0;
  const size_t slots = (size_t)num_rows * sp::logprob_splits(num_rows, vocab);
  return slots * (sizeof(sp::LogprobStat) + sizeof(uint64_t) * (size_t)max_top_k);
}

extern "C" int sp_logprobs(const float* rows, int64_t row_stride, int kind, const float* top_ps,
                           const int64_t* chosen_ids, const int32_t* top_ks, int max_top_k,
                           const int32_t* ids_offsets, const int64_t* ids_flat, int num_rows, int vocab,
                           float* out_chosen, float* out_top_vals, int32_t* out_top_ids, float* out_ids_vals,
                           void* workspace, size_t workspace_bytes, void* stream) {
  SP_CHECK_ARG(num_rows >= 0 && vocab > 0 && (kind == 0 || kind == 1));
  SP_CHECK_ARG(max_top_k >= 0 && max_top_k <= sp::kLogprobMaxTopK);
  if (num_rows == 0) return SP_OK;
  SP_CHECK_ARG(rows && workspace && row_stride >= vocab);
  SP_CHECK_ARG(!chosen_ids || out_chosen);
  SP_CHECK_ARG(max_top_k == 0 || (out_top_vals && out_top_ids));
  SP_CHECK_ARG((ids_offsets == nullptr) == (ids_flat == nullptr) && (!ids_offsets || out_ids_vals));
  if (workspace_bytes < sp_logprobs_workspace_bytes(num_rows, vocab, max_top_k)) return SP_ERR_WORKSPACE;
  const int splits = sp::logprob_splits(num_rows, vocab);
  sp::LogprobStat* stats = (sp::LogprobStat*)workspace;
  sp::LogprobArgs a{rows, row_stride, kind, vocab, splits, sp::logprob_slice(vocab, splits), max_top_k,
                    kind == 1 ? top_ps : nullptr, chosen_ids, top_ks, ids_offsets, ids_flat,
                    out_chosen, out_top_vals, out_top_ids, out_ids_vals,
                    stats, (uint64_t*)(stats + (size_t)num_rows * splits)};
  sp::logprob_partial_kernel<<<dim3(num_rows, splits), sp::kSampThreads, 0, (hipStream_t)stream>>>(a);
  SP_LAUNCH_CHECK();
  sp::logprob_merge_kernel<<<dim3(num_rows), sp::kSampThreads, 0, (hipStream_t)stream>>>(a);
  SP_LAUNCH_CHECK();
  return SP_OK;
}
