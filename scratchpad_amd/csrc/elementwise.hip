// HBM-bound row kernels of the hot path: RMSNorm (+fused add), SiLU-mul, xIELU, rotary (+fused KV
// store), KV store, req_to_token scatter, positions.  All vectorised to 16 B per lane
// (cdna_hip_programming.md Guideline 13); each has a scalar twin for odd shapes / alignments.
//
// Rounding points follow the reference's torch path (forward_native) so that 16-bit results
// are bit-comparable with torch's tensor arithmetic: see the per-kernel comments.
#include "sp_common.h"

// The rounding points below must survive to the ISA.  With the default -ffp-contract=fast hipcc
// rewrites `round16(a*b) - round16(c*d)` on fp16 data into v_fma_f16 (one rounding fewer than
// torch's tensor arithmetic), and a source pragma does not stop the backend: this translation
// unit is compiled with -ffp-contract=off (scratchpad_amd/build.py PER_FILE_FLAGS).
#pragma clang fp contract(off)

namespace sp {

static constexpr int kBlock = 256;

// The order of this sum and of wave_sum (sp_common.h) - six butterfly steps, then the four waves added in turn - is
// what the error bound of the embedding-pool tests counts on (`sum_depth` in the tests' error model: 6 + 4 additions
// behind a lane's own): change them together.
__device__ __forceinline__ float block_sum(float v, float* smem) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) smem[wave] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < kBlock / 64; ++i) t += smem[i];
  __syncthreads();
  return t;
}

// ------------------------------------------------------------------------------------ RMSNorm
// nn/layers/layernorm.py:34-51.  y = round(xf * rsqrt(mean(xf^2)+eps)) * w  (second product
// rounded again: torch multiplies two `dtype` tensors).  Fused: xf = x + residual in fp32,
// residual <- round(xf), and the UNROUNDED xf is normalised.
//
// The row routine, shared by the norm kernels and embedding_pool_kernel (which must give the norm kernels' bits):
// rmsnorm_load_vec / row_elem read a row (and add the residual), rmsnorm_rs reduces the lanes' partial sums of
// squares to 1 / sqrt(mean + eps), rmsnorm_elem holds the two rounding points of an output element.

// x[i] (+ residual[i] in fp32): the value the norm is taken of
template <typename Tag, bool FUSED>
__device__ __forceinline__ float row_elem(const void* x, const void* residual, int64_t xi, int64_t ri) {
  typedef Elem<Tag> E;
  float v = E::load(x, xi);
  if (FUSED) v = __fadd_rn(v, E::load(residual, ri));
  return v;
}

// 16-byte path: lane t keeps vectors t, t + kBlock, ... of the row in `cache` (fp32) and returns the sum of their
// squares, added in element order.  WRITE_RES: residual <- round(x + residual), as sp_fused_add_rmsnorm does.
template <typename Tag, bool FUSED, bool WRITE_RES, int MAXIT>
__device__ __forceinline__ float rmsnorm_load_vec(const char* xrow, char* rrow, int nvec,
                                                  float (&cache)[MAXIT][Elem<Tag>::kVec]) {
  constexpr int V = Elem<Tag>::kVec;
  float ss = 0.f;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int v = threadIdx.x + it * kBlock;
    if (v < nvec) {
      unpack16<Tag>(ld16(xrow + (int64_t)v * 16), cache[it]);
      if (FUSED) {
        float r[V];
        unpack16<Tag>(ld16(rrow + (int64_t)v * 16), r);
#pragma unroll
        for (int e = 0; e < V; ++e) cache[it][e] = __fadd_rn(cache[it][e], r[e]);
        if (WRITE_RES) st16(rrow + (int64_t)v * 16, pack16<Tag>(cache[it]));
      }
#pragma unroll
      for (int e = 0; e < V; ++e) ss += cache[it][e] * cache[it][e];
    }
  }
  return ss;
}

__device__ __forceinline__ float rmsnorm_rs(float ss, float* smem, int hidden, float eps) {
  const float mean = block_sum(ss, smem) / (float)hidden;
  return 1.0f / sqrtf(mean + eps);
}

// one output element, before the store rounds it
template <typename Tag>
__device__ __forceinline__ float rmsnorm_elem(float v, float rs, float w) {
  return __fmul_rn(Elem<Tag>::round(__fmul_rn(v, rs)), w);
}

template <typename Tag, bool FUSED, int MAXIT>
__global__ __launch_bounds__(kBlock) void rmsnorm_vec_kernel(void* out,  // may alias x_io (fused)
                                                              void* x_io, void* residual,
                                                              const void* __restrict__ weight,
                                                              int hidden, int64_t x_stride,
                                                              int64_t r_stride, int64_t o_stride,
                                                              float eps) {
  typedef Elem<Tag> E;
  constexpr int V = E::kVec;
  __shared__ float smem[kBlock / 64];
  const int64_t row = blockIdx.x;
  const char* xrow = (const char*)x_io + row * x_stride * E::kBytes;
  char* rrow = FUSED ? (char*)residual + row * r_stride * E::kBytes : nullptr;
  char* orow = (char*)out + row * o_stride * E::kBytes;
  const int nvec = hidden / V;
  float cache[MAXIT][V];
  const float ss = rmsnorm_load_vec<Tag, FUSED, true, MAXIT>(xrow, rrow, nvec, cache);
  const float rs = rmsnorm_rs(ss, smem, hidden, eps);
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int v = threadIdx.x + it * kBlock;
    if (v < nvec) {
      float w[V], y[V];
      unpack16<Tag>(ld16((const char*)weight + (int64_t)v * 16), w);
#pragma unroll
      for (int e = 0; e < V; ++e) y[e] = rmsnorm_elem<Tag>(cache[it][e], rs, w[e]);
      st16(orow + (int64_t)v * 16, pack16<Tag>(y));
    }
  }
}

// any hidden / stride / alignment; two passes over the row (second pass re-reads)
template <typename Tag, bool FUSED>
__global__ __launch_bounds__(kBlock) void rmsnorm_scalar_kernel(void* out,  // may alias x_io
                                                                 void* x_io, void* residual,
                                                                 const void* __restrict__ weight,
                                                                 int hidden, int64_t x_stride,
                                                                 int64_t r_stride,
                                                                 int64_t o_stride, float eps) {
  typedef Elem<Tag> E;
  __shared__ float smem[kBlock / 64];
  const int64_t row = blockIdx.x;
  float ss = 0.f;
  for (int i = threadIdx.x; i < hidden; i += kBlock) {
    // pass two recomputes the fp32 sum from x and the OLD residual, so nothing is written yet
    const float v = row_elem<Tag, FUSED>(x_io, residual, row * x_stride + i, row * r_stride + i);
    ss += v * v;
  }
  const float rs = rmsnorm_rs(ss, smem, hidden, eps);
  for (int i = threadIdx.x; i < hidden; i += kBlock) {
    const float v = row_elem<Tag, FUSED>(x_io, residual, row * x_stride + i, row * r_stride + i);
    if (FUSED) E::store(residual, row * r_stride + i, v);
    E::store(out, row * o_stride + i, rmsnorm_elem<Tag>(v, rs, E::load(weight, i)));
  }
}

// ------------------------------------------------------------------------------ SiLU-and-mul
// nn/layers/activation.py:22-24: F.silu(a) * b with both factors in `dtype` (silu rounded
// before the product, as torch does).
__device__ __forceinline__ float silu_f32(float a) { return silu_ref(a); }   // sp_common.h

template <typename Tag>
__global__ __launch_bounds__(kBlock) void silu_mul_vec_kernel(void* __restrict__ out,
                                                               const void* __restrict__ x,
                                                               int64_t num_tokens, int d,
                                                               int64_t x_stride,
                                                               int64_t o_stride) {
  typedef Elem<Tag> E;
  constexpr int V = E::kVec;
  const int vec_per_row = d / V;
  const int64_t total = num_tokens * vec_per_row;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kBlock) {
    const int64_t t = i / vec_per_row;
    const int v = (int)(i - t * vec_per_row);
    const char* row = (const char*)x + t * x_stride * E::kBytes;
    float a[V], b[V], y[V];
    unpack16<Tag>(ld16(row + (int64_t)v * 16), a);
    unpack16<Tag>(ld16(row + ((int64_t)d * E::kBytes) + (int64_t)v * 16), b);
#pragma unroll
    for (int e = 0; e < V; ++e) y[e] = __fmul_rn(E::round(silu_f32(a[e])), b[e]);
    st16((char*)out + t * o_stride * E::kBytes + (int64_t)v * 16, pack16<Tag>(y));
  }
}

template <typename Tag>
__global__ __launch_bounds__(kBlock) void silu_mul_scalar_kernel(void* __restrict__ out,
                                                                  const void* __restrict__ x,
                                                                  int64_t num_tokens, int d,
                                                                  int64_t x_stride,
                                                                  int64_t o_stride) {
  typedef Elem<Tag> E;
  const int64_t total = num_tokens * d;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kBlock) {
    const int64_t t = i / d;
    const int j = (int)(i - t * d);
    const float a = E::load(x, t * x_stride + j), b = E::load(x, t * x_stride + d + j);
    E::store(out, t * o_stride + j, __fmul_rn(E::round(silu_f32(a)), b));
  }
}

// -------------------------------------------------------------------------------------- xIELU
// nn/layers/activation.py:53-60 (xielu_ref, sp_common.h): fp32 from the stored input, one rounding.  A streaming
// kernel: T*d read, T*d written.  A row is cut into d / V + 2 items (V = elements per 16 bytes).  Where the row's x and
// out addresses share their offset within 16 bytes: item 0 is the scalar head up to the first 16-byte boundary, items
// 1 .. nvec one 16-byte vector each, item nvec + 1 the scalar tail.  Otherwise (differently misaligned rows) item j is
// elements [j V, j V + V) one by one.  Every element is read and written by the same lane, so out may alias x.
template <typename Tag>
__global__ __launch_bounds__(kBlock) void xielu_kernel(void* out, const void* x, const void* alpha_p_raw,
                                                        const void* alpha_n_raw, float beta, float eps,
                                                        int64_t num_tokens, int d, int64_t x_stride,
                                                        int64_t o_stride) {
  typedef Elem<Tag> E;
  constexpr int V = E::kVec;
  const XieluCoef c = xielu_coef<Tag>(alpha_p_raw, alpha_n_raw, beta, eps);
  const int items = d / V + 2;
  const int64_t total = num_tokens * items;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kBlock) {
    const int64_t t = i / items;
    const int j = (int)(i - t * items);
    const char* xrow = (const char*)x + t * x_stride * E::kBytes;
    char* orow = (char*)out + t * o_stride * E::kBytes;
    const int mis = (int)((uintptr_t)xrow & 15);
    int lo, hi;
    bool vec = false;
    if (mis == (int)((uintptr_t)orow & 15) && mis % E::kBytes == 0) {
      const int head = min(d, ((16 - mis) & 15) / E::kBytes);
      const int nvec = (d - head) / V;
      if (j == 0) {
        lo = 0, hi = head;
      } else if (j <= nvec) {
        lo = head + (j - 1) * V, hi = lo + V, vec = true;
      } else if (j == nvec + 1) {
        lo = head + nvec * V, hi = d;
      } else {
        lo = hi = 0;
      }
    } else {
      lo = min(d, j * V), hi = min(d, lo + V);
    }
    if (vec) {
      float a[V], y[V];
      unpack16<Tag>(ld16(xrow + (int64_t)lo * E::kBytes), a);
#pragma unroll
      for (int e = 0; e < V; ++e) y[e] = xielu_ref(a[e], c);
      st16(orow + (int64_t)lo * E::kBytes, pack16<Tag>(y));
    } else {
      for (int e = lo; e < hi; ++e) E::store(orow, e, xielu_ref(E::load(xrow, e), c));
    }
  }
}

// ------------------------------------------------------------------- rotary (+ fused KV store)
// nn/layers/rotary_embedding.py:23-49: o1 = x1*cos - x2*sin, o2 = x2*cos + x1*sin with every
// product and the sum rounded to `dtype` (torch tensor arithmetic).  One workgroup per token.
struct RotaryArgs {
  const int64_t* positions;
  void* q;
  void* k;
  const void* v;
  const void* cache;
  void* k_buffer;
  void* v_buffer;
  const int64_t* loc;
  int64_t q_stride, k_stride, v_stride, kv_buffer_stride;
  int Hq, Hkv, head_size, rot, is_neox;
};

template <typename Tag>
__device__ __forceinline__ void rotate_pair(float x1, float x2, float c, float s, float& o1,
                                            float& o2) {
  typedef Elem<Tag> E;
  o1 = E::round(__fsub_rn(E::round(__fmul_rn(x1, c)), E::round(__fmul_rn(x2, s))));
  o2 = E::round(__fadd_rn(E::round(__fmul_rn(x2, c)), E::round(__fmul_rn(x1, s))));
}

template <typename Tag, int V>  // V = Elem::kVec (16-byte path) or 1 (scalar path)
__global__ __launch_bounds__(kBlock) void rotary_kernel(RotaryArgs a) {
  typedef Elem<Tag> E;
  const int64_t t = blockIdx.x;
  const int64_t pos = a.positions[t];
  const int half = a.rot / 2;
  const char* cos_row = (const char*)a.cache + pos * a.rot * E::kBytes;
  const char* sin_row = cos_row + (int64_t)half * E::kBytes;
  const bool store = a.k_buffer != nullptr;
  const int64_t slot = store ? a.loc[t] : 0;
  char* kdst = store ? (char*)a.k_buffer + slot * a.kv_buffer_stride * E::kBytes : nullptr;
  const int nheads = a.Hq + a.Hkv;

  if (a.is_neox) {
    // unit = (head, vector j of the first half); partner vector sits `half` elements later
    const int vec_per_head = half / V;
    for (int u = threadIdx.x; u < nheads * vec_per_head; u += kBlock) {
      const int h = u / vec_per_head, j = u - h * vec_per_head;
      const bool is_k = h >= a.Hq;
      const int hh = is_k ? h - a.Hq : h;
      char* base = is_k ? (char*)a.k + (t * a.k_stride + (int64_t)hh * a.head_size) * E::kBytes
                        : (char*)a.q + (t * a.q_stride + (int64_t)hh * a.head_size) * E::kBytes;
      float x1[V], x2[V], c[V], s[V], o1[V], o2[V];
      if constexpr (V > 1) {
        unpack16<Tag>(ld16(base + (int64_t)j * 16), x1);
        unpack16<Tag>(ld16(base + ((int64_t)half * E::kBytes) + (int64_t)j * 16), x2);
        unpack16<Tag>(ld16(cos_row + (int64_t)j * 16), c);
        unpack16<Tag>(ld16(sin_row + (int64_t)j * 16), s);
      } else {
        x1[0] = E::load(base, j);
        x2[0] = E::load(base, half + j);
        c[0] = E::load(cos_row, j);
        s[0] = E::load(sin_row, j);
      }
#pragma unroll
      for (int e = 0; e < V; ++e) rotate_pair<Tag>(x1[e], x2[e], c[e], s[e], o1[e], o2[e]);
      if constexpr (V > 1) {
        const u32x4 p1 = pack16<Tag>(o1), p2 = pack16<Tag>(o2);
        st16(base + (int64_t)j * 16, p1);
        st16(base + ((int64_t)half * E::kBytes) + (int64_t)j * 16, p2);
        if (store && is_k) {
          char* d = kdst + (int64_t)hh * a.head_size * E::kBytes;
          st16(d + (int64_t)j * 16, p1);
          st16(d + ((int64_t)half * E::kBytes) + (int64_t)j * 16, p2);
        }
      } else {
        E::store(base, j, o1[0]);
        E::store(base, half + j, o2[0]);
        if (store && is_k) {
          char* d = kdst + (int64_t)hh * a.head_size * E::kBytes;
          E::store(d, j, o1[0]);
          E::store(d, half + j, o2[0]);
        }
      }
    }
  } else {
    // GPT-J interleaved: pairs (2i, 2i+1); unit = V elements = V/2 pairs (scalar: one pair)
    constexpr int W = V > 1 ? V : 2;
    const int vec_per_head = a.rot / W;
    for (int u = threadIdx.x; u < nheads * vec_per_head; u += kBlock) {
      const int h = u / vec_per_head, j = u - h * vec_per_head;
      const bool is_k = h >= a.Hq;
      const int hh = is_k ? h - a.Hq : h;
      char* base = is_k ? (char*)a.k + (t * a.k_stride + (int64_t)hh * a.head_size) * E::kBytes
                        : (char*)a.q + (t * a.q_stride + (int64_t)hh * a.head_size) * E::kBytes;
      float x[W], o[W];
      if constexpr (V > 1) {
        unpack16<Tag>(ld16(base + (int64_t)j * 16), x);
      } else {
        x[0] = E::load(base, 2 * j);
        x[1] = E::load(base, 2 * j + 1);
      }
#pragma unroll
      for (int e = 0; e < W / 2; ++e) {
        const int ci = j * (W / 2) + e;
        rotate_pair<Tag>(x[2 * e], x[2 * e + 1], E::load(cos_row, ci), E::load(sin_row, ci),
                         o[2 * e], o[2 * e + 1]);
      }
      char* d = (store && is_k) ? kdst + (int64_t)hh * a.head_size * E::kBytes : nullptr;
      if constexpr (V > 1) {
        const u32x4 p = pack16<Tag>(o);
        st16(base + (int64_t)j * 16, p);
        if (d) st16(d + (int64_t)j * 16, p);
      } else {
        E::store(base, 2 * j, o[0]);
        E::store(base, 2 * j + 1, o[1]);
        if (d) {
          E::store(d, 2 * j, o[0]);
          E::store(d, 2 * j + 1, o[1]);
        }
      }
    }
  }
  if (!store) return;
  // pass-through tail of k (rotary_dim < head_size) and the v rows go to the pool unchanged
  const int tail = a.head_size - a.rot;
  if (tail > 0) {
    const int per_head = tail / V;
    for (int u = threadIdx.x; u < a.Hkv * per_head; u += kBlock) {
      const int h = u / per_head, j = u - h * per_head;
      const char* src = (const char*)a.k + (t * a.k_stride + (int64_t)h * a.head_size + a.rot) * E::kBytes;
      char* d = kdst + ((int64_t)h * a.head_size + a.rot) * E::kBytes;
      if constexpr (V > 1) st16(d + (int64_t)j * 16, ld16(src + (int64_t)j * 16));
      else E::store(d, j, E::load(src, j));
    }
  }
  {
    char* vdst = (char*)a.v_buffer + slot * a.kv_buffer_stride * E::kBytes;
    const char* vsrc = (const char*)a.v + t * a.v_stride * E::kBytes;
    const int n = a.Hkv * a.head_size / V;
    for (int u = threadIdx.x; u < n; u += kBlock) {
      if constexpr (V > 1) st16(vdst + (int64_t)u * 16, ld16(vsrc + (int64_t)u * 16));
      else E::store(vdst, u, E::load(vsrc, u));
    }
  }
}

// ------------------------------------------------- per-head RMSNorm + rotary (+ fused KV store)
// nn/models/qwen/qwen3.py:114-123 (_apply_qk_norm) followed by rotary_emb and set_kv_buffer, in one launch whose
// bits are those of rmsnorm_vec_kernel on the [T*H, D] rows of q and of k followed by rotary_kernel.
//
// One workgroup per token, L = D / (2 * kVec) lanes per head: lane j of a head holds its 16-byte vectors j (A) and
// j + L (B = A's neox partner at rotary_dim = D).  rmsnorm_vec_kernel at hidden = D has lane v sum the squares of
// vector v in element order and folds the lanes with xor offsets 32 ... 1 (wave_sum), then adds three zero waves
// (block_sum): every add above offset L is an add of exact zeros, the xor-L step is A's partial + B's partial - taken
// here inside the lane - and the steps below it are the same butterfly over the head's L lanes.  The sum, the mean
// and rs are therefore the same fp32 numbers; the two products of the norm and the rotation's products and sums keep
// their rounding points (E::round where the three-launch form stores and reloads a `dtype` value).
// Norm weights and the cos/sin values depend on the lane's place in its head only: they are loaded once, in front
// of the loop over the heads this lane group takes.
struct QkNormArgs {
  RotaryArgs r;
  const void* q_weight;
  const void* k_weight;
  float eps;
};

static constexpr int kQkNormMaxBlock = 512;

template <typename Tag, int L>
__global__ __launch_bounds__(kQkNormMaxBlock) void qk_norm_rotary_kernel(QkNormArgs p) {
  typedef Elem<Tag> E;
  constexpr int V = E::kVec;
  const RotaryArgs& a = p.r;
  const int64_t t = blockIdx.x;
  const int64_t pos = a.positions[t];
  const int half = a.rot / 2;
  const char* cos_row = (const char*)a.cache + pos * a.rot * E::kBytes;
  const char* sin_row = cos_row + (int64_t)half * E::kBytes;
  const bool store = a.k_buffer != nullptr;
  const int64_t slot = store ? a.loc[t] : 0;
  char* kdst = store ? (char*)a.k_buffer + slot * a.kv_buffer_stride * E::kBytes : nullptr;
  const int nheads = a.Hq + a.Hkv;
  const int j = threadIdx.x & (L - 1), g = threadIdx.x / L, G = blockDim.x / L;
  const bool full = a.rot == a.head_size;          // else rot = D / 2 (the host admits nothing else)
  const bool lo = j < L / 2;                        // neox at rot = D / 2: A is x1 (lo) or x2 of its pair
  const bool rot_b = full;                          // GPT-J: is vector B inside rotary_dim (A always is)

  // c / s: neox - the cos / sin vector this lane's pair uses; GPT-J - [0, V/2) for vector A, [V/2, V) for vector B
  float c[V], s[V];
  if (a.is_neox) {
    const int jj = full ? j : (j & (L / 2 - 1));
    unpack16<Tag>(ld16(cos_row + (int64_t)jj * 16), c);
    unpack16<Tag>(ld16(sin_row + (int64_t)jj * 16), s);
  } else {
#pragma unroll
    for (int e = 0; e < V / 2; ++e) {
      c[e] = E::load(cos_row, j * (V / 2) + e);
      s[e] = E::load(sin_row, j * (V / 2) + e);
      c[V / 2 + e] = rot_b ? E::load(cos_row, (j + L) * (V / 2) + e) : 0.f;
      s[V / 2 + e] = rot_b ? E::load(sin_row, (j + L) * (V / 2) + e) : 0.f;
    }
  }
  u32x4 wqa = {}, wqb = {}, wka = {}, wkb = {};
  if (a.Hq > 0) {
    wqa = ld16((const char*)p.q_weight + (int64_t)j * 16);
    wqb = ld16((const char*)p.q_weight + (int64_t)(j + L) * 16);
  }
  if (a.Hkv > 0) {
    wka = ld16((const char*)p.k_weight + (int64_t)j * 16);
    wkb = ld16((const char*)p.k_weight + (int64_t)(j + L) * 16);
  }

  for (int h = g; h < nheads; h += G) {
    const bool is_k = h >= a.Hq;
    const int hh = is_k ? h - a.Hq : h;
    char* base = is_k ? (char*)a.k + (t * a.k_stride + (int64_t)hh * a.head_size) * E::kBytes
                      : (char*)a.q + (t * a.q_stride + (int64_t)hh * a.head_size) * E::kBytes;
    float xa[V], xb[V], wa[V], wb[V];
    unpack16<Tag>(ld16(base + (int64_t)j * 16), xa);
    unpack16<Tag>(ld16(base + (int64_t)(j + L) * 16), xb);
    unpack16<Tag>(is_k ? wka : wqa, wa);
    unpack16<Tag>(is_k ? wkb : wqb, wb);
    // rmsnorm_vec_kernel's partial sums of vectors j and j + L, then its reduction tree (see above)
    float ss = 0.f, sb = 0.f;
#pragma unroll
    for (int e = 0; e < V; ++e) ss += xa[e] * xa[e];
#pragma unroll
    for (int e = 0; e < V; ++e) sb += xb[e] * xb[e];
    ss += sb;
#pragma unroll
    for (int off = L / 2; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    const float mean = ss / (float)a.head_size;
    const float rs = 1.0f / sqrtf(mean + p.eps);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      xa[e] = E::round(__fmul_rn(E::round(__fmul_rn(xa[e], rs)), wa[e]));
      xb[e] = E::round(__fmul_rn(E::round(__fmul_rn(xb[e], rs)), wb[e]));
    }
    float oa[V], ob[V];
    if (a.is_neox) {
      if (full) {
#pragma unroll
        for (int e = 0; e < V; ++e) rotate_pair<Tag>(xa[e], xb[e], c[e], s[e], oa[e], ob[e]);
      } else {
        // pairs (vector i, vector i + L/2) of the first half of the head: the partner is lane j ^ (L/2)'s vector A
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float other = __shfl_xor(xa[e], L / 2, 64);
          float o1, o2;
          rotate_pair<Tag>(lo ? xa[e] : other, lo ? other : xa[e], c[e], s[e], o1, o2);
          oa[e] = lo ? o1 : o2;
          ob[e] = xb[e];
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < V / 2; ++e) {
        rotate_pair<Tag>(xa[2 * e], xa[2 * e + 1], c[e], s[e], oa[2 * e], oa[2 * e + 1]);
        float o1, o2;
        rotate_pair<Tag>(xb[2 * e], xb[2 * e + 1], c[V / 2 + e], s[V / 2 + e], o1, o2);
        ob[2 * e] = rot_b ? o1 : xb[2 * e];
        ob[2 * e + 1] = rot_b ? o2 : xb[2 * e + 1];
      }
    }
    const u32x4 pa = pack16<Tag>(oa), pb = pack16<Tag>(ob);
    st16(base + (int64_t)j * 16, pa);
    st16(base + (int64_t)(j + L) * 16, pb);
    if (store && is_k) {
      char* d = kdst + (int64_t)hh * a.head_size * E::kBytes;
      st16(d + (int64_t)j * 16, pa);
      st16(d + (int64_t)(j + L) * 16, pb);
    }
  }
  if (!store) return;
  char* vdst = (char*)a.v_buffer + slot * a.kv_buffer_stride * E::kBytes;
  const char* vsrc = (const char*)a.v + t * a.v_stride * E::kBytes;
  const int n = a.Hkv * a.head_size / V;
  for (int u = threadIdx.x; u < n; u += blockDim.x) st16(vdst + (int64_t)u * 16, ld16(vsrc + (int64_t)u * 16));
}

// ----------------------------------------------------------------------------------- KV store
// memory/pool.py:414-424: buffer[loc[t]] = cache[t].  Rows are Hkv*D contiguous elements.
template <int BYTES>  // 16 (vector) or the element size (scalar)
__global__ __launch_bounds__(kBlock) void kv_store_kernel(char* __restrict__ kbuf,
                                                           char* __restrict__ vbuf,
                                                           const int64_t* __restrict__ loc,
                                                           const char* __restrict__ k,
                                                           const char* __restrict__ v,
                                                           int64_t num_tokens, int k_row_bytes,
                                                           int v_row_bytes, int64_t k_stride_b,
                                                           int64_t v_stride_b, int64_t kb_stride_b,
                                                           int64_t vb_stride_b) {
  const int ku = k_row_bytes / BYTES, vu = v_row_bytes / BYTES;
  const int per_tok = ku + vu;
  const int64_t total = num_tokens * per_tok;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kBlock) {
    const int64_t t = i / per_tok;
    int u = (int)(i - t * per_tok);
    const int64_t slot = loc[t];
    const char* src;
    char* dst;
    if (u < ku) {
      src = k + t * k_stride_b + (int64_t)u * BYTES;
      dst = kbuf + slot * kb_stride_b + (int64_t)u * BYTES;
    } else {
      u -= ku;
      src = v + t * v_stride_b + (int64_t)u * BYTES;
      dst = vbuf + slot * vb_stride_b + (int64_t)u * BYTES;
    }
    if constexpr (BYTES == 16) *(u32x4*)dst = *(const u32x4*)src;
    else if constexpr (BYTES == 4) *(uint32_t*)dst = *(const uint32_t*)src;
    else *(uint16_t*)dst = *(const uint16_t*)src;
  }
}

// e5m2 pool: one thread converts 8 consecutive elements of a K or V row and stores 8 bytes
template <typename Tag>
__global__ __launch_bounds__(kBlock) void kv_store_fp8_kernel(char* __restrict__ kbuf, char* __restrict__ vbuf,
                                                               const int64_t* __restrict__ loc,
                                                               const void* __restrict__ k,
                                                               const void* __restrict__ v, int64_t num_tokens,
                                                               int row_elems, int64_t k_stride, int64_t v_stride,
                                                               int64_t kb_stride, int64_t vb_stride,
                                                               float k_scale, float v_scale) {
  typedef Elem<Tag> E;
  const int units = row_elems / 8;                     // per row
  const int64_t total = num_tokens * units * 2;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    const int64_t t = i / (2 * units);
    int u = (int)(i - t * 2 * units);
    const bool is_v = u >= units;
    if (is_v) u -= units;
    const int64_t slot = loc[t];
    const void* src = is_v ? v : k;
    const int64_t sbase = t * (is_v ? v_stride : k_stride) + (int64_t)u * 8;
    // the reference's two steps and two roundings (memory/pool.py:401-412): cache_k.div_(k_scale) in
    // the activation dtype (an fp32 division rounded back to that dtype), then .to(float8_e5m2)
    const float scale = is_v ? v_scale : k_scale;
    u32x2 out;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      uint32_t word = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        word |= f32_to_e5m2_bits(E::round(E::load(src, sbase + 4 * w + e) / scale)) << (8 * e);
      out[w] = word;
    }
    char* dst = (is_v ? vbuf + slot * vb_stride : kbuf + slot * kb_stride) + (int64_t)u * 8;
    *(u32x2*)dst = out;
  }
}

// --------------------------------------------------------------- req_to_token write / positions
__device__ __forceinline__ int64_t block_prefix_i64(const int64_t* a32or64, const int32_t* a32,
                                                    int n, int64_t* smem) {
  int64_t s = 0;
  for (int i = threadIdx.x; i < n; i += kBlock) s += a32 ? (int64_t)a32[i] : a32or64[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = s;
  __syncthreads();
  int64_t t = 0;
#pragma unroll
  for (int i = 0; i < kBlock / 64; ++i) t += smem[i];
  return t;
}

// scheduler/schedule_batch.py:1546-1580
__global__ __launch_bounds__(kBlock) void write_req_to_token_kernel(
    int32_t* __restrict__ table, int64_t row_stride, const int64_t* __restrict__ req_pool_indices,
    const int64_t* __restrict__ pre_lens, const int64_t* __restrict__ seq_lens,
    const int64_t* __restrict__ extend_lens, const int64_t* __restrict__ out_cache_loc) {
  __shared__ int64_t smem[kBlock / 64];
  const int b = blockIdx.x;
  const int64_t start = block_prefix_i64(extend_lens, nullptr, b, smem);
  const int64_t pre = pre_lens[b], n = seq_lens[b] - pre;
  int32_t* row = table + req_pool_indices[b] * row_stride + pre;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) row[i] = (int32_t)out_cache_loc[start + i];
}

// model_executor/forward_info.py:423-449
__global__ __launch_bounds__(kBlock) void compute_position_kernel(
    int64_t* __restrict__ positions, int32_t* __restrict__ extend_start_loc,
    const int32_t* __restrict__ prefix_lens, const int32_t* __restrict__ extend_lens) {
  __shared__ int64_t smem[kBlock / 64];
  const int b = blockIdx.x;
  const int64_t start = block_prefix_i64(nullptr, extend_lens, b, smem);
  const int64_t pre = prefix_lens[b];
  const int n = extend_lens[b];
  for (int i = threadIdx.x; i < n; i += kBlock) positions[start + i] = pre + i;
  if (threadIdx.x == 0) extend_start_loc[b] = (int32_t)start;
}

// model_executor/forward_info.py:469-471
__global__ void clamp_position_kernel(int64_t* __restrict__ positions,
                                      const void* __restrict__ seq_lens, int idx64, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const int64_t v = load_idx(seq_lens, i, idx64) - 1;
    positions[i] = v < 0 ? 0 : v;
  }
}

// ------------------------------------------------------------- embedding: pool + norm + L2
// nn/layers/pooler.py:38-50 behind the final norm of the decoder (nn/models/llama/llama.py:268): one workgroup per
// sequence takes the LAST row of that sequence, gives it the bits sp_fused_add_rmsnorm / sp_rmsnorm would (the row
// routine above, the same path choice and summation order) and divides it by its 2-norm at F.normalize's rounding
// points: the norm accumulated in fp32 and rounded to `dtype`, clamped below at 1e-12 as `dtype` holds it (0 in
// fp16), each quotient taken in fp32 and rounded once.  x and residual are read only.
// The sum of squares of the L2 step: lane t adds elements [c V, c V + V) of chunks c = t, t + kBlock, ... in
// ascending order, block_sum folds the lanes - an order fixed by `hidden` alone, the same on both paths, and the one
// the error bound of its tests assumes (`sum_depth`: V ceil(ceil(hidden / V) / kBlock) + 10 additions).
struct EmbedArgs {
  void* out;
  const void* x;
  const void* residual;
  const void* weight;
  const void* lens;
  int64_t o_stride, x_stride, r_stride, num_tokens;
  int hidden, idx64, normalize, out_vec;
  float eps;
};

// row of x this workgroup pools, or -1: a sequence without tokens, or lengths that leave [0, num_tokens)
__device__ __forceinline__ int64_t embedding_row(const EmbedArgs& a, int64_t* smem) {
  const int i = blockIdx.x;
  const int64_t end = block_prefix_i64(a.idx64 ? (const int64_t*)a.lens : nullptr,
                                       a.idx64 ? nullptr : (const int32_t*)a.lens, i + 1, smem);
  const int64_t row = end - 1;
  return (load_idx(a.lens, i, a.idx64) > 0 && row >= 0 && row < a.num_tokens) ? row : -1;
}

template <typename Tag>
__device__ __forceinline__ void embedding_zero_row(const EmbedArgs& a) {
  for (int i = threadIdx.x; i < a.hidden; i += kBlock)
    Elem<Tag>::store(a.out, (int64_t)blockIdx.x * a.o_stride + i, 0.f);
}

// max(round(sqrt(sum n^2)), round(1e-12)); a NaN norm stays NaN, as torch.clamp_min leaves it
template <typename Tag>
__device__ __forceinline__ float l2_denominator(float ss, float* smem) {
  typedef Elem<Tag> E;
  const float norm = E::round(__fsqrt_rn(block_sum(ss, smem)));
  const float lo = E::round(1e-12f);
  return norm < lo ? lo : norm;
}

template <typename Tag, bool FUSED, int MAXIT>
__global__ __launch_bounds__(kBlock) void embedding_pool_vec_kernel(EmbedArgs a) {
  typedef Elem<Tag> E;
  constexpr int V = E::kVec;
  __shared__ float smem[kBlock / 64];
  __shared__ int64_t ismem[kBlock / 64];
  const int64_t row = embedding_row(a, ismem);
  if (row < 0) {                                   // the same for every lane of the workgroup
    embedding_zero_row<Tag>(a);
    return;
  }
  const char* xrow = (const char*)a.x + row * a.x_stride * E::kBytes;
  char* rrow = FUSED ? (char*)a.residual + row * a.r_stride * E::kBytes : nullptr;   // read only (WRITE_RES off)
  const int nvec = a.hidden / V;
  float cache[MAXIT][V];
  const float ss = rmsnorm_load_vec<Tag, FUSED, false, MAXIT>(xrow, rrow, nvec, cache);
  float ss2 = 0.f;
  if (a.weight) {                                  // uniform
    const float rs = rmsnorm_rs(ss, smem, a.hidden, a.eps);
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int v = threadIdx.x + it * kBlock;
      if (v < nvec) {
        float w[V];
        unpack16<Tag>(ld16((const char*)a.weight + (int64_t)v * 16), w);
#pragma unroll
        for (int e = 0; e < V; ++e) cache[it][e] = E::round(rmsnorm_elem<Tag>(cache[it][e], rs, w[e]));
      }
    }
  }
  if (a.normalize) {
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      if (threadIdx.x + it * kBlock < nvec) {
#pragma unroll
        for (int e = 0; e < V; ++e) ss2 += cache[it][e] * cache[it][e];
      }
    }
    const float denom = l2_denominator<Tag>(ss2, smem);
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      if (threadIdx.x + it * kBlock < nvec) {
#pragma unroll
        for (int e = 0; e < V; ++e) cache[it][e] = __fdiv_rn(cache[it][e], denom);
      }
    }
  }
  const int64_t obase = (int64_t)blockIdx.x * a.o_stride;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int v = threadIdx.x + it * kBlock;
    if (v < nvec) {
      if (a.out_vec) {
        st16((char*)a.out + (obase + (int64_t)v * V) * E::kBytes, pack16<Tag>(cache[it]));
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) E::store(a.out, obase + (int64_t)v * V + e, cache[it][e]);
      }
    }
  }
}

// any hidden / stride / alignment: the norm step in rmsnorm_scalar_kernel's two passes and order; the row is parked in
// `out` (every lane re-reads only what it wrote itself) while its sum of squares is reduced
template <typename Tag, bool FUSED>
__global__ __launch_bounds__(kBlock) void embedding_pool_scalar_kernel(EmbedArgs a) {
  typedef Elem<Tag> E;
  constexpr int V = E::kVec;
  __shared__ float smem[kBlock / 64];
  __shared__ int64_t ismem[kBlock / 64];
  const int64_t row = embedding_row(a, ismem);
  if (row < 0) {
    embedding_zero_row<Tag>(a);
    return;
  }
  const int64_t xb = row * a.x_stride, rb = row * a.r_stride, ob = (int64_t)blockIdx.x * a.o_stride;
  float rs = 0.f;
  if (a.weight) {
    float ss = 0.f;
    for (int i = threadIdx.x; i < a.hidden; i += kBlock) {
      const float v = row_elem<Tag, FUSED>(a.x, a.residual, xb + i, rb + i);
      ss += v * v;
    }
    rs = rmsnorm_rs(ss, smem, a.hidden, a.eps);
  }
  float ss2 = 0.f;
  for (int c = threadIdx.x; (int64_t)c * V < a.hidden; c += kBlock) {
    const int hi = min(a.hidden, (c + 1) * V);
    for (int i = c * V; i < hi; ++i) {
      float n = row_elem<Tag, FUSED>(a.x, a.residual, xb + i, rb + i);
      if (a.weight) n = rmsnorm_elem<Tag>(n, rs, E::load(a.weight, i));
      n = E::round(n);
      E::store(a.out, ob + i, n);
      ss2 += n * n;
    }
  }
  if (!a.normalize) return;
  const float denom = l2_denominator<Tag>(ss2, smem);
  for (int c = threadIdx.x; (int64_t)c * V < a.hidden; c += kBlock) {
    const int hi = min(a.hidden, (c + 1) * V);
    for (int i = c * V; i < hi; ++i) E::store(a.out, ob + i, __fdiv_rn(E::load(a.out, ob + i), denom));
  }
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace sp

using namespace sp;

extern "C" int sp_abi_version(void) { return SP_ABI_VERSION; }

extern "C" const char* sp_status_string(int status) {
  switch (status) {
    case SP_OK: return "ok";
    case SP_ERR_INVALID_ARG: return "invalid argument";
    case SP_ERR_UNSUPPORTED: return "unsupported shape/dtype";
    case SP_ERR_WORKSPACE: return "workspace too small";
    case SP_ERR_LAUNCH: return "kernel launch failed";
    default: return "unknown status";
  }
}

template <typename Tag, bool FUSED>
static int launch_rmsnorm(void* out, void* x, void* residual, const void* weight, int64_t T,
                          int hidden, int64_t xs, int64_t rs, int64_t os, float eps,
                          hipStream_t st) {
  typedef Elem<Tag> E;
  constexpr int V = E::kVec;
  constexpr int MAXIT = (E::kBytes == 4) ? 8 : 4;
  const bool vec = hidden % V == 0 && xs % V == 0 && os % V == 0 && (!FUSED || rs % V == 0) &&
                   aligned16(out) && aligned16(x) && aligned16(weight) &&
                   (!FUSED || aligned16(residual)) && hidden / V <= kBlock * MAXIT;
  if (vec)
    rmsnorm_vec_kernel<Tag, FUSED, MAXIT><<<dim3((unsigned)T), kBlock, 0, st>>>(
        out, x, residual, weight, hidden, xs, rs, os, eps);
  else
    rmsnorm_scalar_kernel<Tag, FUSED><<<dim3((unsigned)T), kBlock, 0, st>>>(
        out, x, residual, weight, hidden, xs, rs, os, eps);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_rmsnorm(void* out, const void* x, const void* weight, int64_t num_tokens,
                          int hidden, int64_t x_stride, int64_t out_stride, float eps, int dtype,
                          void* stream) {
  SP_CHECK_ARG(num_tokens >= 0 && hidden > 0);
  if (num_tokens == 0) return SP_OK;
  SP_CHECK_ARG(out && x && weight);
  SP_DISPATCH_DTYPE(dtype, return (launch_rmsnorm<Tag, false>(out, (void*)x, nullptr, weight,
                                                               num_tokens, hidden, x_stride, 0,
                                                               out_stride, eps,
                                                               (hipStream_t)stream)));
}

extern "C" int sp_fused_add_rmsnorm(void* x, void* residual, const void* weight,
                                    int64_t num_tokens, int hidden, int64_t x_stride,
                                    int64_t res_stride, float eps, int dtype, void* stream) {
  SP_CHECK_ARG(num_tokens >= 0 && hidden > 0);
  if (num_tokens == 0) return SP_OK;
  SP_CHECK_ARG(x && residual && weight);
  SP_DISPATCH_DTYPE(dtype, return (launch_rmsnorm<Tag, true>(x, x, residual, weight, num_tokens,
                                                              hidden, x_stride, res_stride,
                                                              x_stride, eps,
                                                              (hipStream_t)stream)));
}

template <typename Tag>
static int launch_embedding_pool(EmbedArgs a, int num_seqs, hipStream_t st) {
  typedef Elem<Tag> E;
  constexpr int V = E::kVec;
  constexpr int MAXIT = (E::kBytes == 4) ? 8 : 4;
  const bool fused = a.residual != nullptr;
  // launch_rmsnorm's rule on x, residual and weight, so that the sums of squares run in the order the norm entries
  // use on the same inputs.  launch_rmsnorm also asks its `out` for 16 bytes: for sp_fused_add_rmsnorm that is x
  // again; sp_rmsnorm's separate out has no counterpart here, so the match with sp_rmsnorm holds for a call of it
  // whose out allows the 16-byte path (see the header).  This entry's own out only picks how rows are stored.
  const bool vec = a.hidden % V == 0 && a.x_stride % V == 0 && aligned16(a.x) && (!a.weight || aligned16(a.weight)) &&
                   (!fused || (a.r_stride % V == 0 && aligned16(a.residual))) && a.hidden / V <= kBlock * MAXIT;
  a.out_vec = a.o_stride % V == 0 && aligned16(a.out);
  const dim3 grid((unsigned)num_seqs);
  if (vec) {
    if (fused) embedding_pool_vec_kernel<Tag, true, MAXIT><<<grid, kBlock, 0, st>>>(a);
    else embedding_pool_vec_kernel<Tag, false, MAXIT><<<grid, kBlock, 0, st>>>(a);
  } else {
    if (fused) embedding_pool_scalar_kernel<Tag, true><<<grid, kBlock, 0, st>>>(a);
    else embedding_pool_scalar_kernel<Tag, false><<<grid, kBlock, 0, st>>>(a);
  }
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_embedding_pool(void* out, int64_t out_stride, const void* x, int64_t x_stride,
                                 const void* residual, int64_t res_stride, const void* weight, float eps,
                                 const void* extend_seq_lens, int idx64, int num_seqs, int64_t num_tokens,
                                 int hidden, int normalize, int dtype, void* stream) {
  SP_CHECK_ARG(num_seqs >= 0 && num_tokens >= 0 && hidden > 0);
  SP_CHECK_ARG(out && x && extend_seq_lens);
  SP_CHECK_ARG(out_stride >= hidden && x_stride >= hidden);
  if (residual) SP_CHECK_ARG(weight && res_stride >= hidden);
  if (weight) SP_CHECK_ARG(eps > 0.f);
  if (dtype != SP_F32 && dtype != SP_F16 && dtype != SP_BF16) return SP_ERR_UNSUPPORTED;
  if (num_seqs == 0) return SP_OK;
  EmbedArgs a;
  a.out = out; a.x = x; a.residual = residual; a.weight = weight; a.lens = extend_seq_lens;
  a.o_stride = out_stride; a.x_stride = x_stride; a.r_stride = residual ? res_stride : 0;
  a.num_tokens = num_tokens; a.hidden = hidden; a.idx64 = idx64 ? 1 : 0; a.normalize = normalize ? 1 : 0;
  a.out_vec = 0; a.eps = eps;
  SP_DISPATCH_DTYPE(dtype, return (launch_embedding_pool<Tag>(a, num_seqs, (hipStream_t)stream)));
}

template <typename Tag>
static int launch_silu(void* out, const void* x, int64_t T, int d, int64_t xs, int64_t os,
                       hipStream_t st) {
  typedef Elem<Tag> E;
  constexpr int V = E::kVec;
  const bool vec = d % V == 0 && xs % V == 0 && os % V == 0 && aligned16(out) && aligned16(x);
  const int64_t work = vec ? T * (d / V) : T * (int64_t)d;
  int64_t blocks = (work + kBlock - 1) / kBlock;
  if (blocks > 256 * 16) blocks = 256 * 16;
  if (vec) silu_mul_vec_kernel<Tag><<<dim3((unsigned)blocks), kBlock, 0, st>>>(out, x, T, d, xs, os);
  else silu_mul_scalar_kernel<Tag><<<dim3((unsigned)blocks), kBlock, 0, st>>>(out, x, T, d, xs, os);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_silu_and_mul(void* out, const void* x, int64_t num_tokens, int d,
                               int64_t x_stride, int64_t out_stride, int dtype, void* stream) {
  SP_CHECK_ARG(num_tokens >= 0 && d > 0);
  if (num_tokens == 0) return SP_OK;
  SP_CHECK_ARG(out && x);
  SP_DISPATCH_DTYPE(dtype, return (launch_silu<Tag>(out, x, num_tokens, d, x_stride, out_stride,
                                                     (hipStream_t)stream)));
}

template <typename Tag>
static int launch_xielu(void* out, const void* x, const void* ap, const void* an, float beta, float eps, int64_t T,
                        int d, int64_t xs, int64_t os, hipStream_t st) {
  const int64_t work = T * (d / Elem<Tag>::kVec + 2);
  int64_t blocks = (work + kBlock - 1) / kBlock;
  if (blocks > 256 * 16) blocks = 256 * 16;
  xielu_kernel<Tag><<<dim3((unsigned)blocks), kBlock, 0, st>>>(out, x, ap, an, beta, eps, T, d, xs, os);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

// device (or managed) memory: the two activation parameters and the activations are read by the kernel, never here
static bool on_device(const void* p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();      // an unknown address is an answer, not a launch failure
    return false;
  }
  return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

extern "C" int sp_xielu(void* out, const void* x, const void* alpha_p_raw, const void* alpha_n_raw, float beta,
                        float eps, int64_t num_tokens, int d, int64_t x_stride, int64_t out_stride, int dtype,
                        void* stream) {
  SP_CHECK_ARG(num_tokens >= 0 && d > 0);
  if (num_tokens == 0) return SP_OK;
  SP_CHECK_ARG(out && x && alpha_p_raw && alpha_n_raw);
  SP_CHECK_ARG(x_stride >= d && out_stride >= d);
  if (dtype != SP_F32 && dtype != SP_F16 && dtype != SP_BF16) return SP_ERR_UNSUPPORTED;
  SP_CHECK_ARG(on_device(out) && on_device(x) && on_device(alpha_p_raw) && on_device(alpha_n_raw));
  SP_DISPATCH_DTYPE(dtype, return (launch_xielu<Tag>(out, x, alpha_p_raw, alpha_n_raw, beta, eps, num_tokens, d,
                                                      x_stride, out_stride, (hipStream_t)stream)));
}

template <typename Tag>
static int launch_rotary(const RotaryArgs& a, int64_t T, hipStream_t st) {
  typedef Elem<Tag> E;
  constexpr int V = E::kVec;
  const bool store = a.k_buffer != nullptr;
  bool vec = a.head_size % V == 0 && a.q_stride % V == 0 && a.k_stride % V == 0 &&
             aligned16(a.q) && aligned16(a.k) && aligned16(a.cache) &&
             (a.is_neox ? (a.rot / 2) % V == 0 : a.rot % V == 0);
  if (store)
    vec = vec && a.v_stride % V == 0 && a.kv_buffer_stride % V == 0 && aligned16(a.v) &&
          aligned16(a.k_buffer) && aligned16(a.v_buffer) && (a.head_size - a.rot) % V == 0;
  if (vec) rotary_kernel<Tag, V><<<dim3((unsigned)T), kBlock, 0, st>>>(a);
  else rotary_kernel<Tag, 1><<<dim3((unsigned)T), kBlock, 0, st>>>(a);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_rotary_embedding(const int64_t* positions, void* q, void* k,
                                   const void* cos_sin_cache, int64_t num_tokens, int num_q_heads,
                                   int num_kv_heads, int head_size, int rotary_dim,
                                   int64_t q_stride, int64_t k_stride, int is_neox, const void* v,
                                   int64_t v_stride, void* k_buffer, void* v_buffer,
                                   const int64_t* out_cache_loc, int64_t kv_buffer_stride,
                                   int dtype, void* stream) {
  SP_CHECK_ARG(positions && q && k && cos_sin_cache && num_tokens >= 0);
  SP_CHECK_ARG(num_q_heads >= 0 && num_kv_heads >= 0 && head_size > 0);
  SP_CHECK_ARG(rotary_dim > 0 && rotary_dim <= head_size && rotary_dim % 2 == 0);
  const bool store = k_buffer != nullptr || v_buffer != nullptr;
  if (store) SP_CHECK_ARG(k_buffer && v_buffer && v && out_cache_loc && kv_buffer_stride > 0);
  if (num_tokens == 0) return SP_OK;
  RotaryArgs a;
  a.positions = positions; a.q = q; a.k = k; a.v = v; a.cache = cos_sin_cache;
  a.k_buffer = store ? k_buffer : nullptr; a.v_buffer = store ? v_buffer : nullptr;
  a.loc = out_cache_loc; a.q_stride = q_stride; a.k_stride = k_stride; a.v_stride = v_stride;
  a.kv_buffer_stride = kv_buffer_stride; a.Hq = num_q_heads; a.Hkv = num_kv_heads;
  a.head_size = head_size; a.rot = rotary_dim; a.is_neox = is_neox ? 1 : 0;
  SP_DISPATCH_DTYPE(dtype, return (launch_rotary<Tag>(a, num_tokens, (hipStream_t)stream)));
}

template <typename Tag>
static int launch_qk_norm_rotary(const QkNormArgs& p, int64_t T, hipStream_t st) {
  typedef Elem<Tag> E;
  constexpr int V = E::kVec;
  const RotaryArgs& a = p.r;
  const int D = a.head_size;
  // the lane layout reproduces rmsnorm_vec_kernel's reduction for a power-of-two number of 16-byte vectors per head
  if (D != 64 && D != 128 && D != 256) return SP_ERR_UNSUPPORTED;
  if (a.rot != D && a.rot * 2 != D) return SP_ERR_UNSUPPORTED;
  bool vec = a.q_stride % V == 0 && a.k_stride % V == 0 && aligned16(a.q) && aligned16(a.k) &&
             aligned16(a.cache) && aligned16(p.q_weight) && aligned16(p.k_weight);
  if (a.k_buffer)
    vec = vec && a.v_stride % V == 0 && a.kv_buffer_stride % V == 0 && aligned16(a.v) &&
          aligned16(a.k_buffer) && aligned16(a.v_buffer);
  if (!vec) return SP_ERR_UNSUPPORTED;
  const int L = D / (2 * V);
  int threads = ((a.Hq + a.Hkv) * L + 63) / 64 * 64;
  threads = threads < 64 ? 64 : (threads > kQkNormMaxBlock ? kQkNormMaxBlock : threads);
#define SP_QKN_LAUNCH(LL) qk_norm_rotary_kernel<Tag, LL><<<dim3((unsigned)T), threads, 0, st>>>(p)
  switch (L) {
    case 4: SP_QKN_LAUNCH(4); break;
    case 8: SP_QKN_LAUNCH(8); break;
    case 16: SP_QKN_LAUNCH(16); break;
    case 32: SP_QKN_LAUNCH(32); break;
    default: return SP_ERR_UNSUPPORTED;
  }
#undef SP_QKN_LAUNCH
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_qk_norm_rotary(const int64_t* positions, void* q, void* k, const void* q_norm_weight,
                                 const void* k_norm_weight, float eps, const void* cos_sin_cache,
                                 int64_t num_tokens, int num_q_heads, int num_kv_heads, int head_size,
                                 int rotary_dim, int64_t q_stride, int64_t k_stride, int is_neox,
                                 const void* v, int64_t v_stride, void* k_buffer, void* v_buffer,
                                 const int64_t* out_cache_loc, int64_t kv_buffer_stride, int dtype,
                                 void* stream) {
  SP_CHECK_ARG(positions && q && k && q_norm_weight && k_norm_weight && cos_sin_cache && num_tokens >= 0);
  SP_CHECK_ARG(num_q_heads >= 0 && num_kv_heads >= 0 && head_size > 0);
  SP_CHECK_ARG(rotary_dim > 0 && rotary_dim <= head_size && rotary_dim % 2 == 0);
  const bool store = k_buffer != nullptr || v_buffer != nullptr;
  if (store) SP_CHECK_ARG(k_buffer && v_buffer && v && out_cache_loc && kv_buffer_stride > 0);
  if (dtype != SP_F32 && dtype != SP_F16 && dtype != SP_BF16) return SP_ERR_UNSUPPORTED;
  QkNormArgs p;
  RotaryArgs& a = p.r;
  a.positions = positions; a.q = q; a.k = k; a.v = v; a.cache = cos_sin_cache;
  a.k_buffer = store ? k_buffer : nullptr; a.v_buffer = store ? v_buffer : nullptr;
  a.loc = out_cache_loc; a.q_stride = q_stride; a.k_stride = k_stride; a.v_stride = v_stride;
  a.kv_buffer_stride = kv_buffer_stride; a.Hq = num_q_heads; a.Hkv = num_kv_heads;
  a.head_size = head_size; a.rot = rotary_dim; a.is_neox = is_neox ? 1 : 0;
  p.q_weight = q_norm_weight; p.k_weight = k_norm_weight; p.eps = eps;
  if (num_tokens == 0) return SP_OK;
  SP_DISPATCH_DTYPE(dtype, return (launch_qk_norm_rotary<Tag>(p, num_tokens, (hipStream_t)stream)));
}

extern "C" int sp_kv_store(void* k_buffer, void* v_buffer, const int64_t* loc, const void* k,
                           const void* v, int64_t num_tokens, int num_kv_heads, int head_dim,
                           int v_head_dim, int64_t k_stride, int64_t v_stride,
                           int64_t k_buffer_stride, int64_t v_buffer_stride, int dtype,
                           void* stream) {
  SP_CHECK_ARG(k_buffer && v_buffer && loc && k && v && num_tokens >= 0);
  SP_CHECK_ARG(num_kv_heads > 0 && head_dim > 0 && v_head_dim > 0);
  if (dtype != SP_F32 && dtype != SP_F16 && dtype != SP_BF16) return SP_ERR_UNSUPPORTED;
  if (num_tokens == 0) return SP_OK;
  const int eb = dtype == SP_F32 ? 4 : 2;
  const int krow = num_kv_heads * head_dim * eb, vrow = num_kv_heads * v_head_dim * eb;
  const int64_t ks = k_stride * eb, vs = v_stride * eb, kbs = k_buffer_stride * eb,
                vbs = v_buffer_stride * eb;
  const bool vec = krow % 16 == 0 && vrow % 16 == 0 && ks % 16 == 0 && vs % 16 == 0 &&
                   kbs % 16 == 0 && vbs % 16 == 0 && aligned16(k_buffer) && aligned16(v_buffer) &&
                   aligned16(k) && aligned16(v);
  const int unit = vec ? 16 : eb;
  const int64_t work = num_tokens * ((krow + vrow) / unit);
  int64_t blocks = (work + kBlock - 1) / kBlock;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipStream_t st = (hipStream_t)stream;
#define SP_KV_LAUNCH(B)                                                                        \
  kv_store_kernel<B><<<dim3((unsigned)blocks), kBlock, 0, st>>>(                              \
      (char*)k_buffer, (char*)v_buffer, loc, (const char*)k, (const char*)v, num_tokens, krow, \
      vrow, ks, vs, kbs, vbs)
  if (vec) SP_KV_LAUNCH(16);
  else if (eb == 4) SP_KV_LAUNCH(4);
  else SP_KV_LAUNCH(2);
#undef SP_KV_LAUNCH
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_kv_store_fp8(void* k_buffer, void* v_buffer, const int64_t* loc, const void* k,
                               const void* v, int64_t num_tokens, int num_kv_heads, int head_dim,
                               int64_t k_stride, int64_t v_stride, int64_t k_buffer_stride,
                               int64_t v_buffer_stride, float k_scale, float v_scale, int src_dtype,
                               void* stream) {
  SP_CHECK_ARG(k_buffer && v_buffer && loc && k && v && num_tokens >= 0);
  SP_CHECK_ARG(num_kv_heads > 0 && head_dim > 0 && k_scale > 0.f && v_scale > 0.f);
  if (num_tokens == 0) return SP_OK;
  const int row = num_kv_heads * head_dim;
  if (row % 8 || k_buffer_stride % 8 || v_buffer_stride % 8 || ((uintptr_t)k_buffer & 7) ||
      ((uintptr_t)v_buffer & 7))
    return SP_ERR_UNSUPPORTED;
  const int64_t work = num_tokens * (row / 8) * 2;
  int64_t blocks = (work + kBlock - 1) / kBlock;
  if (blocks > 256 * 16) blocks = 256 * 16;
  SP_DISPATCH_DTYPE(src_dtype, (kv_store_fp8_kernel<Tag><<<dim3((unsigned)blocks), kBlock, 0, (hipStream_t)stream>>>(
                                   (char*)k_buffer, (char*)v_buffer, loc, k, v, num_tokens, row, k_stride, v_stride,
                                   k_buffer_stride, v_buffer_stride, k_scale, v_scale)));
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_write_req_to_token(int32_t* req_to_token, int64_t row_stride,
                                     const int64_t* req_pool_indices, const int64_t* pre_lens,
                                     const int64_t* seq_lens, const int64_t* extend_lens,
                                     const int64_t* out_cache_loc, int batch_size, void* stream) {
  SP_CHECK_ARG(req_to_token && req_pool_indices && pre_lens && seq_lens && extend_lens &&
               out_cache_loc && batch_size >= 0 && row_stride > 0);
  if (batch_size == 0) return SP_OK;
  write_req_to_token_kernel<<<dim3(batch_size), kBlock, 0, (hipStream_t)stream>>>(
      req_to_token, row_stride, req_pool_indices, pre_lens, seq_lens, extend_lens, out_cache_loc);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_compute_position(int64_t* positions, int32_t* extend_start_loc,
                                   const int32_t* extend_prefix_lens,
                                   const int32_t* extend_seq_lens, int batch_size, void* stream) {
  SP_CHECK_ARG(positions && extend_start_loc && extend_prefix_lens && extend_seq_lens &&
               batch_size >= 0);
  if (batch_size == 0) return SP_OK;
  compute_position_kernel<<<dim3(batch_size), kBlock, 0, (hipStream_t)stream>>>(
      positions, extend_start_loc, extend_prefix_lens, extend_seq_lens);
  SP_LAUNCH_CHECK();
  return SP_OK;
}

extern "C" int sp_clamp_position(int64_t* positions, const void* seq_lens, int idx64,
                                 int batch_size, void* stream) {
  SP_CHECK_ARG(positions && seq_lens && batch_size >= 0);
  if (batch_size == 0) return SP_OK;
  clamp_position_kernel<<<dim3((batch_size + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      positions, seq_lens, idx64, batch_size);
  SP_LAUNCH_CHECK();
  return SP_OK;
}
