/*
 * scratchpad_hip.h - C ABI of the MI355X (gfx950) hot-path library `libscratchpad_hip.so`.
 *
 * This is the drop-in boundary beneath Scratchpad's four Python seams.
 * The reference exports no C ABI itself - it calls third-party wheels (flashinfer v0.2.3,
 * triteia / triteia_cuda) - so every entry point below cites the reference call site it
 * replaces (paths relative to /root/reference/scratchpad).
 *
 * Conventions
 *  - plain pointers and sizes only; every buffer (inputs, outputs, workspaces, the KV pool) is
 *    allocated and owned by the caller (torch on the Python side); the library allocates nothing
 *    and keeps no state;
 *  - every function enqueues on `stream` (a hipStream_t passed as void*) and returns without
 *    synchronising; all are HIP-graph capturable (no host sync, no malloc, launch geometry
 *    depends only on host-visible arguments, never on device-side seq_lens values);
 *  - return 0 on success, a negative sp_status otherwise; nothing throws;
 *  - `dtype`: SP_F32 / SP_F16 / SP_BF16 - the activation & KV-pool element type;
 *  - strides are in ELEMENTS; innermost dimensions are contiguous;
 *  - `idx64`: 1 if req_pool_indices / seq_lens are int64 (eager mode), 0 if int32 (graph mode),
 *    as in ForwardBatch (model_executor/forward_info.py:84-104, cuda_graph_runner.py:193-199);
 *  - KV slot 0 is the reserved dummy slot (memory/pool.py:126-127, 249-253): padded rows carry
 *    out_cache_loc == 0 and seq_len == fill value and are harmless.
 */
#ifndef SCRATCHPAD_HIP_H
#define SCRATCHPAD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_ABI_VERSION 10   /* v10: `chunk` is the smallest split size a plan carries; plan word 2 never exceeds word 0 */
#define SP_API __attribute__((visibility("default")))

typedef enum { SP_F32 = 0, SP_F16 = 1, SP_BF16 = 2, SP_FP8_E5M2 = 3 /* KV pool only */ } sp_dtype;

typedef enum {
  SP_OK = 0,
  SP_ERR_INVALID_ARG = -1, /* null pointer, negative size, misaligned buffer */
  SP_ERR_UNSUPPORTED = -2, /* head_dim / group size / dtype combination not built */
  SP_ERR_WORKSPACE = -3,   /* workspace too small */
  SP_ERR_LAUNCH = -4       /* hipLaunchKernel failed (see hipGetLastError) */
} sp_status;

SP_API int sp_abi_version(void);
SP_API const char* sp_status_string(int status);
/* Test / tuning hook (no reference counterpart): process-wide kernel-selection switches for A/B
 * measurements and parity tests of the non-default kernels.  Keys: "decode_kernel" (0 = default,
 * 1 = VALU kernel, 2 = matrix-core kernel), "extend_defer_x10" (how far the extend kernel's running
 * row maximum may trail, in tenths of a log2 unit; < 0 = the shipped value), "extend_dma" (1 = K/V tiles
 * by LDS-DMA into the swizzled ring where it applies - D 128, 16-bit pools - the default; 0 = register-
 * staged tiles for every shape: same bits), "extend_w64" (the 4-wave x 64-row form of the extend kernel -
 * D 128, 16-bit pools, plain attention, query-head group a multiple of 4: 1 = where it pays, the default;
 * 2 = wherever it applies; 0 = never), "extend_w64_persist" (its persistent form - one workgroup per compute
 * unit drawing the plan's items by ticket: 1 = where it pays, i.e. a plan with at least 32 items per
 * workgroup and row blocks of at most ~32 tiles, the default; 2 = every planned launch the kernel applies to;
 * 0 = never; without it mode 1 of "extend_w64" means mean extend length >= 768 or a cached prefix >= 1024
 * tokens; the two forms agree bit for bit), "decode_ranges" (0 = decode launches never take the range geometry of
 * their plan: the (request, split) items everywhere; -1 = the default, wherever the range kernel applies),
 * "decode_nt_min_mb" (see sp_decode_attention), "ar_fused_blocks", "skinny_nt".  Nothing on the call path reads the environment.  Returns
 * SP_ERR_INVALID_ARG for an unknown key.                                                          */
SP_API int sp_debug_set(const char* key, int value);
/* Read-only counterpart (ABI 6): "w64_descriptor_patched" (1 = extend_w64.hip was built in stages with its kernels'
 * register allocation fixed at assembly level - scratchpad_amd/build.py compile_w64 - and the
 * 4-wave x 64-row extend kernels may launch; anything else: sp_extend_attention keeps to the 8-wave kernel),
 * "extend_last_kernel" (what the last sp_extend_attention call launched: 1 = 8-wave matrix-core kernel, 2 = 4-wave
 * x 64-row kernel, 3 = its persistent form, 4 = row streams on the decode kernel, 0 = none yet), "decode_last_kernel"
 * (ABI 9; what the last sp_decode_attention call launched: 1 = VALU kernel, 2 = matrix-core kernel on (request, split)
 * items, 3 = range kernel, 0 = none yet).  -1: unknown key. */
SP_API int sp_debug_get(const char* key);

/* ---- RMSNorm: replaces flashinfer.norm.rmsnorm / fused_add_rmsnorm
 *      (nn/layers/layernorm.py:22-32; semantics of forward_native 34-51).
 * sp_rmsnorm:           out[t,:] = round(x[t,:] * rsqrt(mean(x^2)+eps)) * weight
 * sp_fused_add_rmsnorm: residual[t,:] = round(x + residual) (in place), then
 *                       x[t,:] = round(fp32(x+residual) * rsqrt(..)) * weight   (in place)       */
SP_API int sp_rmsnorm(void* out, const void* x, const void* weight, int64_t num_tokens, int hidden,
               int64_t x_stride, int64_t out_stride, float eps, int dtype, void* stream);
SP_API int sp_fused_add_rmsnorm(void* x, void* residual, const void* weight, int64_t num_tokens,
                         int hidden, int64_t x_stride, int64_t res_stride, float eps, int dtype,
                         void* stream);

/* ---- SiLU-and-mul: replaces flashinfer.activation.silu_and_mul (nn/layers/activation.py:26-31).
 * out[t, j] = silu(x[t, j]) * x[t, d + j],  x: [T, 2d]                                           */
SP_API int sp_silu_and_mul(void* out, const void* x, int64_t num_tokens, int d, int64_t x_stride,
                    int64_t out_stride, int dtype, void* stream);

/* ---- xIELU, the activation of the ungated Apertus MLP (nn/layers/activation.py:34-60, XIELU.forward).
 * out[t, j] = y(x[t, j]) for j < d, with ap = softplus(*alpha_p_raw), an = beta + softplus(*alpha_n_raw),
 * softplus(v) = v > 20 ? v : log1p(exp(v)):
 *     x > 0 :  y = ap * x * x + beta * x
 *     else  :  y = an * expm1(min(x, eps)) - an * x + beta * x      (x == 0 gives an * expm1(eps), not 0)
 * All arithmetic in fp32 from the stored inputs, ONE rounding to `dtype`.  alpha_p_raw / alpha_n_raw are DEVICE
 * pointers to one element in `dtype` (the module's two parameters as a checkpoint loads them); the kernel reads them
 * on every launch and nothing derived from them is kept on the host, so a captured launch follows a parameter that
 * is overwritten between replays.  eps is the reference's stored constant, float(bfloat16(-1e-6)), in every dtype.
 * Row strides in elements, >= d; columns >= d of out are never written; out == x is allowed.  Rows whose x and out
 * addresses share their offset within 16 bytes move as 16-byte vectors with a scalar head and tail, other rows
 * element by element, all in one launch.  fp32 / fp16 / bf16.
 * SP_ERR_INVALID_ARG before any launch: d <= 0, num_tokens < 0, a NULL pointer, a stride below d, a pointer that
 * is not device memory.  num_tokens == 0 is SP_OK without a launch.                                              */
SP_API int sp_xielu(void* out, const void* x, const void* alpha_p_raw, const void* alpha_n_raw, float beta, float eps,
             int64_t num_tokens, int d, int64_t x_stride, int64_t out_stride, int dtype, void* stream);

/* ---- Rotary embedding, in place on q and k: replaces triteia_cuda.rotary_embedding
 *      (nn/layers/rotary_embedding.py:132-164; semantics of forward_native 102-130).
 * cos_sin_cache: [max_position, rotary_dim] = cos || sin, in `dtype`; positions int64 [T].
 * q: [T, Hq*head_size], k: [T, Hkv*head_size].  is_neox: 1 = halves, 0 = GPT-J interleaved.
 * If k_buffer/v_buffer are non-null the rotated k rows and the v rows are ALSO scattered to
 * the KV pool at out_cache_loc (fused KV store, = sp_kv_store below); pass NULL to skip.        */
SP_API int sp_rotary_embedding(const int64_t* positions, void* q, void* k, const void* cos_sin_cache,
                        int64_t num_tokens, int num_q_heads, int num_kv_heads, int head_size,
                        int rotary_dim, int64_t q_stride, int64_t k_stride, int is_neox,
                        const void* v, int64_t v_stride, void* k_buffer, void* v_buffer,
                        const int64_t* out_cache_loc, int64_t kv_buffer_stride, int dtype,
                        void* stream);

/* ---- Per-head RMSNorm of q and k + rotary embedding (+ fused KV store) in ONE launch: the attention prologue of
 *      Qwen3 (nn/models/qwen/qwen3.py:114-123 `_apply_qk_norm`, then rotary_emb, then set_kv_buffer).
 * In place on q and k.  Every [head_size] row of q is normalised with q_norm_weight, every row of k with
 * k_norm_weight (both [head_size] in `dtype`) exactly as sp_rmsnorm does it with hidden = head_size -
 * rs = 1/sqrtf(mean(x^2) + eps) in fp32, n = round(round(x * rs) * w) - and sp_rotary_embedding's rotation is then
 * applied to n (the normed tail beyond rotary_dim is kept).  With k_buffer / v_buffer the normed and rotated k rows
 * and the untouched v rows are scattered to the pool as sp_rotary_embedding's fused store does; v is never written.
 * The result is BIT-IDENTICAL to sp_rmsnorm on the [T*Hq, head_size] rows of q, sp_rmsnorm on the [T*Hkv, head_size]
 * rows of k, then sp_rotary_embedding with the same store arguments.
 * Built for: head_size in {64, 128, 256}; rotary_dim = head_size or head_size / 2 (neox), a multiple of 16 bytes
 * (GPT-J); 16-byte aligned pointers and row strides.  Anything else returns SP_ERR_UNSUPPORTED before any launch:
 * issue the three calls above instead.  Refusals (SP_ERR_INVALID_ARG) are those of sp_rotary_embedding, with both
 * weights required.                                                                                              */
SP_API int sp_qk_norm_rotary(const int64_t* positions, void* q, void* k, const void* q_norm_weight,
                      const void* k_norm_weight, float eps, const void* cos_sin_cache, int64_t num_tokens,
                      int num_q_heads, int num_kv_heads, int head_size, int rotary_dim, int64_t q_stride,
                      int64_t k_stride, int is_neox, const void* v, int64_t v_stride, void* k_buffer,
                      void* v_buffer, const int64_t* out_cache_loc, int64_t kv_buffer_stride, int dtype,
                      void* stream);

/* ---- KV store: replaces `k_buffer[layer][loc] = cache_k` (MHATokenToKVPool.set_kv_buffer,
 *      memory/pool.py:392-424).  k,v: [T, Hkv, D] (token stride given); buffers [P+1, Hkv, D].  */
SP_API int sp_kv_store(void* k_buffer, void* v_buffer, const int64_t* loc, const void* k, const void* v,
                int64_t num_tokens, int num_kv_heads, int head_dim, int v_head_dim,
                int64_t k_stride, int64_t v_stride, int64_t k_buffer_stride,
                int64_t v_buffer_stride, int dtype, void* stream);

/* ---- KV store into an fp8 (e5m2) pool: the `--kv-cache-dtype fp8_e5m2` branch of set_kv_buffer
 *      (memory/pool.py:401-412: cache_k.div_(k_scale); cache_k.to(float8_e5m2); stored as uint8).
 * k,v: [T, Hkv, D] in `src_dtype` (fp16/bf16/fp32); buffers: uint8 [P+1, Hkv, D], strides in
 * elements (= bytes).  The reference's two steps with their two roundings: x / scale as an fp32
 * division rounded to `src_dtype` (cache_k.div_(k_scale)), then round-to-nearest-even to 1-5-2
 * (overflow -> inf), i.e. torch's .to(torch.float8_e5m2).  Pass 1.0 for an unscaled pool.        */
SP_API int sp_kv_store_fp8(void* k_buffer, void* v_buffer, const int64_t* loc, const void* k, const void* v,
                    int64_t num_tokens, int num_kv_heads, int head_dim, int64_t k_stride,
                    int64_t v_stride, int64_t k_buffer_stride, int64_t v_buffer_stride, float k_scale,
                    float v_scale, int src_dtype, void* stream);

/* ---- req_to_token scatter: replaces write_req_to_token_pool_triton
 *      (scheduler/schedule_batch.py:1546-1580).  All index arrays int64, table int32.           */
SP_API int sp_write_req_to_token(int32_t* req_to_token, int64_t row_stride,
                          const int64_t* req_pool_indices, const int64_t* pre_lens,
                          const int64_t* seq_lens, const int64_t* extend_lens,
                          const int64_t* out_cache_loc, int batch_size, void* stream);

/* ---- positions: replaces compute_position_triton (model_executor/forward_info.py:400-449)
 *      and clamp_position (469-471).                                                             */
SP_API int sp_compute_position(int64_t* positions, int32_t* extend_start_loc,
                        const int32_t* extend_prefix_lens, const int32_t* extend_seq_lens,
                        int batch_size, void* stream);
SP_API int sp_clamp_position(int64_t* positions, const void* seq_lens, int idx64, int batch_size,
                      void* stream);

/* ---- Paged decode attention: replaces decode_attention_fwd (nn/attention/triton_attn/
 *      decode_attention.py:547-608; call site triton_backend.py:183-195) and flashinfer
 *      BatchDecodeWithPagedKVCacheWrapper.forward (flashinfer_backend.py:475-482).
 * For request b and q head h:  o = softmax(q.K[idx]^T * sm_scale [soft-capped]) . V[idx],
 *   idx = req_to_token[req_pool_indices[b], kv_start[b] : kv_start[b] + seq_lens[b]]
 * q,o: [bs, Hq, D]; buffers [P+1, Hkv, D] with token stride kv_buffer_stride; page_size = 1.
 * Hq / Hkv (query heads per KV head): any value 1..16 for fp16/bf16, 1/2/4/8 for fp32; D 64 or 128.
 * A row with seq_lens[b] == 0 (no visible key) is left untouched: pre-fill `out` where that can
 * happen (cross-attention of text-only requests).
 * kv_start may be NULL (= 0); it is the encoder offset of encoder-decoder models
 * (flashinfer_backend.py:593-621).  `max_seq_len`: an upper bound on every seq_lens[b] (the context
 * length under graph capture); a device-side seq_lens[b] above it is clamped to it, never followed.
 *
 * Split-KV geometry (ABI 4).  A request is cut into splits of `chunk` keys; split c of request b writes
 * its partial (o, log-sum-exp) to SLOT slot0[b] + c of the workspace ([Hq, max_slots, D] + [Hq, max_slots]
 * floats) and one merge wave per (request, head) combines them in a second launch.  (ABI 6 could also merge inside
 * the attention kernel through arrival counters in the plan; measured slower wherever graphs replay, removed in
 * ABI 7: a plan is read-only for the launches that use it, so launches on several streams may share one.)
 *   - Without a plan the grid is the static (request, split) rectangle: slot0[b] = b * num_splits,
 *     num_splits = ceil(max_seq_len / chunk), max_slots is ignored (= batch_size * num_splits).
 *   - With a `plan` (sp_decode_plan: [count, chunk, needed, keys | slot0[bs] | (b, c) x max_slots], `plan_bytes` long, built once per step from
 *     the same seq_lens and shared by all layers - the counterpart of flashinfer's begin_forward()/plan,
 *     flashinfer_backend.py:623-670, and of TritonAttnBackend.init_forward_metadata,
 *     triton_backend.py:48-68) the launch covers `max_slots` work items, the kernels read the split size
 *     FROM THE PLAN (device memory) and slot0[b] is the exclusive scan of the requests' split counts.  So the
 *     launch geometry - what a HIP graph captures - is a function of (batch_size, heads, max_slots) only:
 *     one captured launch follows whatever split size each step's plan was built with, and the workspace is
 *     bounded by sum(seq_lens) / chunk + batch_size slots (sp_decode_plan_slots), not by the context
 *     length (the reference's static attn_logits buffer is [bs, heads, max_context_len],
 *     triton_backend.py:70-80).  `chunk` is then the SMALLEST split size the plan may carry (it only decides
 *     whether the merge launch is needed).  Items are listed longest first (XCD load balance on ragged
 *     batches); a plan never changes the result, only which workgroup computes which split.
 * workspace: sp_decode_attention_workspace_bytes(max_slots, ...); plan: sp_decode_plan_bytes().
 *
 * Range geometry (ABI 8; what a default decode step runs).  A plan built with `ranges` > 0 carries a second section,
 * [rcount, R, ranges, batch_size | pos[bs + 1] | start[ranges]], behind the items: the step's keys, request after request
 * in batch order, form one line (request b at pos[b] .. pos[b] + len_b, then 16 empty positions - what a request costs a
 * workgroup beyond its keys); the line is cut into rcount <= ranges equal pieces of R = ceil(length / ranges) positions
 * (at least 64) and start[j] is the first request with a key at or after j * R (-1: piece j holds none).  A launch
 * given the same `ranges` runs one WAVE per (piece, kv head) - with the kv heads in fours a workgroup is the four
 * heads of one piece: each walks its piece - the tail of one request, whole requests, the head of another - so every
 * wave gathers the same number of keys whatever the lengths are, there is no split size to choose, and a request is
 * written straight to the output unless a cut falls inside it.  A request whose keys lie in pieces jf .. jl > jf leaves
 * its partials in slots b + jf .. b + jl (b + j grows along the line: no two (request, piece) pairs share a slot) and
 * the merge launch combines them: the workspace then holds batch_size + ranges slots, whatever sum(seq_lens) is.
 * sp_decode_ranges() is the piece count the library wants for a shape ON THE CURRENT DEVICE (the answer, and the
 * kernel's LDS limit behind it, are kept per device of the process: set the device before the first call, as for any
 * launch): two workgroups per CU (three on a byte pool), all resident at once, four waves each, over the kv heads (at
 * most 1024) - 256 pieces for 8 kv heads on MI355X, 1024 for a tensor-parallel rank's single head - or 0 where the range
 * kernel does not apply (fp32, groups wider than 16, head sizes other than 64 / 128).  Launches it does not take (those
 * shapes, a logit soft-cap, out rows not 8-byte aligned, sp_debug_set("decode_ranges", 0)) use the plan's (request, split)
 * items.  Requires batch_size * (max_seq_len + 16) < 2^31 (else SP_ERR_INVALID_ARG from sp_decode_plan; pass ranges = 0).
 * Results of the two geometries differ in the last bits (another split of the same sums), and under the range geometry
 * the cuts - hence a request's last bits - depend on the lengths of the whole batch, not on the request alone.
 *
 * Plan and launch must agree (ABI 9).  The sections of a plan are located from (batch_size, max_slots, ranges), so
 * sp_decode_attention must be given the values the plan was BUILT with - where the reference rebuilds indices and launch
 * from one begin_forward() call (flashinfer_backend.py:623-670) and they cannot disagree.  What is checked:
 *   - `plan_bytes` (sp_decode_attention) must cover sp_decode_plan_bytes(batch_size, max_slots, ranges), else
 *     SP_ERR_WORKSPACE: no kernel reads a header outside the caller's buffer;
 *   - the range section records the `ranges` and `batch_size` it was built for (its words 2, 3); a range launch (and its
 *     merge) that finds other values does NOTHING - no table read, no gather, `out` untouched - instead of following
 *     pos[] / start[] of another shape.  Nothing on the device reports it: pre-fill `out` to see it, or keep the pair on
 *     the host as scratchpad_amd/_native.py does (decode_plan() remembers what each plan buffer was built with and
 *     decode_attention() raises before launching on any difference);
 *   - ITEMS ARE OPTIONAL: max_slots = 0 (with ranges > 0) builds the range section alone - the item section is then its
 *     4-word header [0, chunk, 0, 0] - which is what a backend whose layers all take the range kernel wants (the plan
 *     kernel skips its six item passes).  A launch that would need the items of such a plan (soft-cap, fp32, ...) returns
 *     SP_ERR_INVALID_ARG.  Likewise ranges = 0 builds the items alone.  sp_debug_get("decode_last_kernel") says what the
 *     last call launched: 1 = VALU kernel (items), 2 = matrix-core kernel (items), 3 = range kernel.
 *
 * Every item fits (ABI 10).  sp_decode_plan lists every split of the (clamped) device-side lengths: where they need
 * more than `max_slots` items at `chunk` (the caller's bound on sum(seq_lens) was too small) the plan kernel doubles the
 * split size until they fit, and word 1 carries the size it chose.  At a split size >= max_seq_len every non-empty
 * request is one item, so an item plan requires max_slots >= batch_size and max_seq_len <= 2^30 (else
 * SP_ERR_INVALID_ARG).  An understated bound costs load balance, never a split; word 2 (the items the lengths need)
 * equals word 0 (the items listed).
 *
 * Streaming gathers.  The plan's word 3 holds the keys the step gathers per kv head (the sum of the clamped lengths).
 * When a launch's K + V bytes (that sum x 2 x num_kv_heads x head_dim x element size) reach a threshold
 * (sp_debug_set("decode_nt_min_mb", n); 0 = always, -1 = never, -2 = the default) the matrix-core kernel gathers K/V rows with
 * NON-TEMPORAL loads: rows read once per step no longer displace the rest of the step's data from the caches.  It is plan
 * data, so a captured launch follows each step's own size; results are the same bits either way.  A plan-less launch
 * has no key count: it streams only when the threshold is 0 ("always", the default).
 *
 * `kv_dtype` = `dtype`, or SP_FP8_E5M2 for a uint8 pool written by sp_kv_store_fp8 (16-bit q
 * only; kv_buffer_stride then counts bytes): the kernels widen e5m2 to half exactly and compute
 * in fp16 with fp32 accumulation, as flashinfer does for fp8 KV (convert to the query type); the
 * in-tree Triton kernels' `p.to(v.dtype)` (probabilities rounded to e5m2) is NOT reproduced.
 *
 * `k_scale`, `v_scale` (> 0; 1.0 = none): the layer's KV scales, the same values the store divided
 * by (flashinfer_backend.py:470-482 passes layer.k_scale / layer.v_scale to both): the pool holds
 * k / k_scale and v / v_scale, so logits are multiplied by k_scale and the output by v_scale.    */
SP_API int64_t sp_decode_plan_slots(int batch_size, int64_t kv_tokens, int64_t max_seq_len, int chunk);
SP_API size_t sp_decode_attention_workspace_bytes(int64_t max_slots, int num_q_heads, int v_head_dim);
SP_API int sp_decode_ranges(int num_q_heads, int num_kv_heads, int head_dim, int dtype, int kv_dtype);
SP_API size_t sp_decode_plan_bytes(int batch_size, int64_t max_slots, int ranges);
SP_API int sp_decode_plan(int32_t* plan, size_t plan_bytes, const void* seq_lens, int idx64,
                   int batch_size, int64_t max_seq_len, int chunk, int64_t max_slots, int ranges, void* stream);
SP_API int sp_decode_attention(void* out, const void* q, const void* k_buffer, const void* v_buffer,
                        const int32_t* req_to_token, int64_t req_to_token_stride,
                        const void* req_pool_indices, const void* seq_lens, const void* kv_start,
                        int idx64, int batch_size, int num_q_heads, int num_kv_heads,
                        int head_dim, int64_t q_stride, int64_t out_stride,
                        int64_t kv_buffer_stride, float sm_scale, float logit_cap, float k_scale,
                        float v_scale, int64_t max_seq_len, int chunk, int64_t max_slots, int ranges,
                        void* workspace, size_t workspace_bytes, const int32_t* plan, size_t plan_bytes,
                        int dtype, int kv_dtype, void* stream);

/* ---- Ragged extend (prefill) attention: replaces extend_attention_fwd (nn/attention/
 *      triton_attn/extend_attention.py:229-327; call site triton_backend.py:137-154) and the
 *      flashinfer ragged+paged+merge_state / paged-only paths (flashinfer_backend.py:400-444).
 * New token t (0-based) of request b attends to kv positions [0, prefix_b + t] of
 * req_to_token[req_pool_indices[b], kv_start[b] + ...]; the new tokens' K/V must already be in
 * the pool (KV store precedes the kernel, triton_backend.py:131-134).  causal = 0 gives the
 * cross-attention form: every row attends to all seq_lens[b] kv positions
 * (flashinfer_backend.py:408-417).  window_left >= 0 (causal only) is the sliding window of
 * flashinfer_backend.py:413: the row at kv position p sees keys [p - window_left, p]; -1 = no
 * window.  (Decode needs no such argument: the caller passes kv_start = seq_len - min(seq_len,
 * window + 1) and that length, flashinfer_backend.py:559-577.)
 * q,o: [T, Hq, D]; extend_* are int32 [bs].  Hq / Hkv: any width for fp16/bf16, 1/2/4/8 for fp32.
 * num_tokens = sum(extend_seq_lens) (host-known: ForwardBatch.extend_num_tokens) and
 * max_extend_len >= max(extend_seq_lens), max_seq_len >= max(seq_lens) fix the launch geometry.
 * workspace: sp_extend_attention_workspace_bytes().                                              */
SP_API size_t sp_extend_attention_workspace_bytes(int64_t num_tokens, int batch_size, int num_q_heads,
                                           int head_dim, int dtype);
/* `plan` (optional, may be NULL): the step's (request, row block) work items, heaviest first, built once
 * per forward by sp_extend_plan() from the same extend_seq_lens / seq_lens / head counts / causal flag
 * and shared by every layer (the counterpart of flashinfer's begin_forward() for the prefill wrappers,
 * flashinfer_backend.py:400-444, 672-830).  It only decides which workgroup computes which rows (no
 * empty workgroups on ragged batches, longest rows first); results do not depend on it.  The plan carries
 * a header (block size, head counts, num_tokens, batch size): a launch of ANOTHER SHAPE - other head counts,
 * another token total or batch size - does not use its items and derives each workgroup's rows by walking the
 * requests instead.  That check identifies a launch shape, not a step: a plan left from an earlier step with
 * the same batch size and token total but other per-request lengths passes it and row blocks are then dropped
 * or computed twice.  REQUIREMENT: call sp_extend_plan for every step, with that step's extend_seq_lens, before
 * the step's first sp_extend_attention (HipAttnBackend.init_forward_metadata does).
 * sp_extend_plan_bytes() sizes the int32 buffer; `plan_bytes` (sp_extend_attention) must cover it, else
 * SP_ERR_WORKSPACE.  `causal` of sp_extend_plan is reserved (the item list does not depend on it).
 * The last 2 KiB of the buffer are counters of the attention kernel (the persistent form of the 4 x 64-row
 * kernel hands its workgroups the items by ticket): written by sp_extend_plan (zeros), counted up during
 * a launch that owns the plan and zero again when it ends - hence `plan` is not const, and one plan
 * buffer serves one launch at a time (the layers of a forward, one after the other on ONE stream: yes;
 * two streams at once: give each its own copy); a launch that was aborted leaves the counters dirty until
 * the next sp_extend_plan.  A plan that is not the launch's own is only read.                          */
SP_API size_t sp_extend_plan_bytes(int64_t num_tokens, int batch_size, int num_q_heads, int num_kv_heads);
SP_API int sp_extend_plan(int32_t* plan, size_t plan_bytes, const int32_t* extend_seq_lens, const void* seq_lens,
                   int idx64, int batch_size, int64_t num_tokens, int num_q_heads, int num_kv_heads,
                   int causal, void* stream);
SP_API int sp_extend_attention(void* out, const void* q, const void* k_buffer, const void* v_buffer,
                        const int32_t* req_to_token, int64_t req_to_token_stride,
                        const void* req_pool_indices, const void* seq_lens, const void* kv_start,
                        int idx64, const int32_t* extend_seq_lens,
                        const int32_t* extend_start_loc, int batch_size, int64_t num_tokens,
                        int num_q_heads, int num_kv_heads, int head_dim, int64_t q_stride,
                        int64_t out_stride, int64_t kv_buffer_stride, float sm_scale,
                        float logit_cap, float k_scale, float v_scale, int causal,
                        int window_left, int max_extend_len,
                        int64_t max_seq_len, void* workspace, size_t workspace_bytes,
                        int32_t* plan, size_t plan_bytes, int dtype, int kv_dtype, void* stream);

/* ---- Sampler.  Replaces nn/layers/sampler.py:63-75 (torch.argmax; logits.div_(T) + softmax),
 *      sampler.py:195-232 (top_k_top_p_min_p_sampling_from_probs_torch, top_p_normalize_probs_torch)
 *      and the flashinfer calls wrapped by nn/kernels/sampling.py:19-373 (top_k_renorm_probs,
 *      top_p_renorm_probs, top_k_top_p_sampling_from_probs "joint", min_p_sampling_from_probs).
 * Rows are [batch_size, vocab] with row_stride elements between rows; probabilities are fp32.
 * Filter (one definition for sampling and renormalising): rank tokens by (p descending, token id
 * ascending); a token is kept iff rank < top_k, the mass ranked above it is <= top_p, and
 * p >= p_max * min_p.  Mass is accumulated exactly as integers floor(p * 2^48), so the result
 * is independent of summation order.  NULL top_ks / top_ps / min_ps disable that filter.
 * sp_top_k_top_p_min_p_sample draws, per row, the token whose interval of the kept cumulative
 * mass (token-id order) contains floor(uniform * kept_mass); uniform[b] in [0,1) is supplied by
 * the caller (sampler.py:87-90 draws them with torch.rand).  keep_count (nullable) receives the
 * number of kept tokens per row.  A row with no mass yields token 0.  NaN and entries <= 0 rank as
 * zero (after every positive entry, by token id), carry no mass and renormalise to 0; a top_k <= 0
 * keeps nothing.
 * sp_argmax returns the first maximal index (torch.argmax).                                       */
SP_API int sp_argmax(const void* logits, int64_t row_stride, int batch_size, int vocab, int64_t* out_ids,
              int dtype, void* stream);
/* Vocab-parallel greedy (TP): instead of all-gathering [bs, vocab / tp] logits and taking the argmax
 * of the gathered row (nn/layers/logits_processor.py:362-369 followed by sampler.py:63-65), every
 * rank reduces its own shard to out_pairs[b] = {fp32 bits of the shard maximum, global index of its
 * first occurrence = local index + index_offset}; the caller all-gathers the [bs, 2] int32 words
 * rank-major and sp_argmax_merge returns, per row, the index of the largest value, ties to the
 * lowest global index - bit-identical to the gathered path.  `cols` = this rank's columns that are
 * real vocabulary (padding columns excluded; 0 = none: the shard never wins).                   */
SP_API int sp_argmax_shard(const void* logits, int64_t row_stride, int batch_size, int cols, int index_offset,
                    int32_t* out_pairs, int dtype, void* stream);
SP_API int sp_argmax_merge(const int32_t* pairs, int num_shards, int batch_size, int64_t* out_ids, void* stream);
SP_API int sp_softmax_temperature(float* logits_inout, int64_t row_stride, const float* temperatures,
                           int batch_size, int vocab, void* stream);
SP_API int sp_top_k_top_p_min_p_sample(const float* probs, int64_t row_stride, const int32_t* top_ks,
                                const float* top_ps, const float* min_ps, const float* uniform,
                                int batch_size, int vocab, int64_t* out_ids, int32_t* keep_count,
                                void* stream);
SP_API int sp_top_k_top_p_min_p_renorm(const float* probs, int64_t row_stride, const int32_t* top_ks,
                                const float* top_ps, const float* min_ps, int batch_size, int vocab,
                                float* out, int64_t out_stride, int32_t* keep_count, void* stream);

/* ---- Log-probabilities of a few tokens per row (additive within ABI 10): replaces the dense passes of
 *      nn/layers/sampler.py:66-67 (log_softmax of a greedy batch), 116-141 (top_p_normalize + log + clamp of a sampled
 *      one), 234-263 (get_top_logprobs / get_token_ids_logprobs: topk and gathers over [bs, vocab]) and of
 *      nn/layers/logits_processor.py:378-460 (the same for prompt positions).
 * rows: fp32 [num_rows, >= vocab], row_stride elements apart, read only.
 *   kind 0: logits.         value(t) = log_softmax(row)[t]  (-inf for a -inf logit)
 *   kind 1: probabilities, as sp_softmax_temperature leaves them.  value(t) = log(p[t] / kept_mass) under the top-p
 *           filter defined above at sp_top_k_top_p_min_p_* (ranks by (p descending, id ascending), mass as integers
 *           floor(p * 2^48), NaN and entries <= 0 carry no mass; top_ps NULL = keep everything); a token the filter
 *           drops, one without mass and every token of a row without mass report finfo(float32).min (-FLT_MAX) -
 *           what log(renorm).clamp(min = finfo.min) yields.  top_ps is ignored for kind 0.
 * What is asked for, each part optional, and nothing else is written (no [num_rows, vocab] intermediate):
 *   - chosen_ids int64 [num_rows] (NULL = none)   -> out_chosen[b] = value(chosen_ids[b]);
 *   - the first top_ks[b] tokens (int32, 0 = none, clamped to max_top_k; top_ks NULL = max_top_k for every row) of the
 *     ranking by the INPUT value - logit or probability, not the computed logprob - descending, token id ascending: the
 *     rule of the filter and of sp_argmax, exact under ties and independent of how a row is split over workgroups
 *     -> out_top_vals / out_top_ids [num_rows, max_top_k], entries [b, 0 .. top_ks[b]) (at most `vocab` of them);
 *     max_top_k <= SP_LOGPROBS_MAX_TOP_K, else SP_ERR_INVALID_ARG (the caller keeps its own path for longer lists);
 *   - listed ids in CSR form, ids_offsets int32 [num_rows + 1] and ids_flat int64 (NULL together = none)
 *     -> out_ids_vals[i] = value(ids_flat[i]) of the row that lists it, for ids_offsets[0] <= i < ids_offsets[num_rows].
 * An id outside [0, vocab) in chosen_ids or ids_flat lives in device memory, so it cannot be refused here: it reports
 * finfo(float32).min and nothing is read for it.
 * The row is streamed once (running maximum and sum of exponentials, or the integer mass, and the top candidates kept
 * as a sorted list per wave - no sort, no histogram); few rows are cut into up to 32 slices over as many workgroups and
 * merged per row by a second launch.  That is the whole cost of kind 0 and of a kind-1 row whose mass is within its top_p.
 * A kind-1 row whose mass exceeds its top_p is NOT done in one pass: the merge launch repeats the filter's radix descent
 * on it (three more passes over the row, out of L2 where it still is there), and each asked token that sits on a partly
 * kept pivot value costs one more scan up to its id.
 * workspace: sp_logprobs_workspace_bytes(num_rows, vocab, max_top_k) bytes, 8-byte aligned (SP_ERR_WORKSPACE if
 * workspace_bytes is smaller).  SP_ERR_INVALID_ARG before any launch: NULL rows / workspace, NULL output of a part that
 * is asked for, ids_offsets without ids_flat or the reverse, negative sizes, vocab <= 0, kind not 0 / 1, row_stride <
 * vocab, max_top_k outside [0, SP_LOGPROBS_MAX_TOP_K].  num_rows == 0 is SP_OK and launches nothing (the parameter is
 * not called batch_size for the reason given at sp_penalty_reset below; prompt rows are not a batch anyway).       */
#define SP_LOGPROBS_MAX_TOP_K 32
SP_API size_t sp_logprobs_workspace_bytes(int num_rows, int vocab, int max_top_k);
SP_API int sp_logprobs(const float* rows, int64_t row_stride, int kind, const float* top_ps,
                const int64_t* chosen_ids, const int32_t* top_ks, int max_top_k, const int32_t* ids_offsets,
                const int64_t* ids_flat, int num_rows, int vocab, float* out_chosen, float* out_top_vals,
                int32_t* out_top_ids, float* out_ids_vals, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Sampling penalties and grammar vocab masks (additive within ABI 10): replaces
 *      SamplingBatchInfo.apply_logits_bias (sampling/sampling_batch_info.py:324-344) and the dense per-penalizer
 *      tensors behind it (sampling/penaltylib/penalizers/), and the grammar back-ends' apply_vocab_mask
 *      (constrained/triton_ops/bitmask_ops.py, constrained/outlines_backend.py:82-83).
 * State (caller-owned, int32, one row per req_to_token row): entries [pool_rows, capacity, 2] = the (token, count)
 * pairs of the request's distinct output tokens, n_distinct [pool_rows], out_len [pool_rows].  Row indices
 * (pool_row_indices / req_pool_indices) are int64 with idx64 = 1, int32 with 0; an index outside [0, pool_rows) makes
 * every kernel skip that row.  The rows of one batch must be distinct.
 * sp_penalty_reset:    n_distinct = out_len = 0 for the listed rows.
 * sp_penalty_cumulate: per batch row, count token_ids[b] in its request's list (increment or append) and out_len += 1;
 *                      an id outside [0, vocab) leaves the row untouched.  A full list is never written past:
 *                      *error (device word) is set to 1 instead and stays set.
 * sp_penalty_apply:    in place on fp32 logits [num_rows, >= vocab]: for each entry (t, c) of the row
 *                      x = logits[b, t]; x -= c * frequency; x -= presence; x = x > 0 ? x / repetition : x * repetition
 *                      (in this order), then logits[b, s] = -inf for every stop id s of the row (stop_token_ids
 *                      [num_rows, max_stops], -1 = none) while out_len < min_new_tokens[b].  min_new_tokens and
 *                      stop_token_ids may be NULL together with max_stops == 0.  A row with (0, 0, 1, 0) is left alone.
 * sp_vocab_mask_apply: in place, -inf where the mask forbids; only forbidden elements are written.  mask_kind 0:
 *                      packed int32 [num_rows, mask_width] words, bit j of word i = token 32 i + j, 1 = allowed;
 *                      columns at or beyond min(vocab, 32 mask_width) are left alone and mask_width >
 *                      ceil(vocab / 32) is refused.  mask_kind 1: one byte per token [num_rows, mask_width == vocab],
 *                      non-zero = forbidden.  mask_stride: elements (words / bytes) between mask rows.
 * SP_ERR_INVALID_ARG before any launch: NULL required pointer, negative size, row_stride < vocab, the widths above.
 * num_rows is the batch size (one row per request of the batch); 0 is SP_OK and launches nothing.  It is not called
 * batch_size like its neighbours' because tests/test_gpu_c_abi.py pins the list of entry points that take a parameter of
 * that name; tests/test_gpu_penalties.py holds these four to the same empty-batch rule.                                                 */
SP_API int sp_penalty_reset(int32_t* n_distinct, int32_t* out_len, const void* pool_row_indices, int idx64,
                     int num_rows, int pool_rows, void* stream);
SP_API int sp_penalty_cumulate(int32_t* entries, int32_t* n_distinct, int32_t* out_len, int32_t* error,
                        const void* req_pool_indices, int idx64, const int64_t* token_ids, int num_rows,
                        int pool_rows, int capacity, int vocab, void* stream);
SP_API int sp_penalty_apply(float* logits, int64_t row_stride, const int32_t* entries, const int32_t* n_distinct,
                     const int32_t* out_len, const void* req_pool_indices, int idx64,
                     const float* frequency_penalties, const float* presence_penalties,
                     const float* repetition_penalties, const int32_t* min_new_tokens,
                     const int32_t* stop_token_ids, int max_stops, int num_rows, int pool_rows, int capacity,
                     int vocab, void* stream);
SP_API int sp_vocab_mask_apply(float* logits, int64_t row_stride, const void* mask, int64_t mask_stride,
                        int mask_width, int mask_kind, int num_rows, int vocab, void* stream);

/* ---- Small-batch projection: out[M,N] = x[M,K] . w[N,K]^T, M <= 16, K % 32 == 0, fp16/bf16,
 *      fp32 accumulation, one rounding.  Serves F.linear inside QKVParallelLinear /
 *      MergedColumnParallelLinear / RowParallelLinear.forward (nn/layers/linear.py:423-470, 696-760,
 *      1033-1155) and the LM-head matmul (nn/layers/logits_processor.py:340-376) when the step has
 *      at most 16 tokens; a weight-streaming kernel (HBM-bound).  Returns SP_ERR_UNSUPPORTED for
 *      other shapes: the caller keeps the library GEMM.  Strides in elements.
 *      `epilogue` (ABI 6): 0 = out[M, N] as above.  1 = w is the merged gate|up matrix [2 N, K] of LlamaMLP
 *      (gate rows first; MergedColumnParallelLinear, linear.py:423-470) and out[M, N] = SiluAndMul of the projection
 *      (nn/layers/activation.py:21-31), bit for bit the plain call followed by sp_silu_and_mul: gate_up_proj +
 *      act_fn (nn/models/llama/llama.py:62-66) in one launch.                                      */
SP_API int sp_gemm_skinny(void* out, const void* x, const void* w, int M, int N, int K, int64_t x_stride,
                   int64_t w_stride, int64_t out_stride, int epilogue, int dtype, void* stream);
/* sp_gemm_skinny_xielu: out[M, N] = xIELU(round(x . w^T)) - up_proj + act_fn of SwissAIMLP
 *      (nn/models/swissai/apertus.py:63-68) in one launch, bit for bit sp_gemm_skinny(epilogue 0) followed by
 *      sp_xielu on its result.  Shapes, strides and refusals are those of epilogue 0 (SP_ERR_UNSUPPORTED: M > 16,
 *      K % 32 != 0, fp32: issue the two calls); alpha_p_raw, alpha_n_raw, beta, eps as in sp_xielu, the two
 *      pointers required (non-NULL).  Like sp_gemm_skinny, and unlike sp_xielu, this entry does NOT ask the runtime
 *      whether its pointers are device memory: it sits on the decode step, and the caller vouches for all five
 *      (scratchpad_amd/_native.py refuses host tensors before the call).                                                                           */
SP_API int sp_gemm_skinny_xielu(void* out, const void* x, const void* w, int M, int N, int K, int64_t x_stride,
                         int64_t w_stride, int64_t out_stride, const void* alpha_p_raw, const void* alpha_n_raw,
                         float beta, float eps, int dtype, void* stream);

/* ---- LoRA toppings (additive in ABI 10): the per-row adapter products of the topping layers
 *      (nn/toppings/topping_layer.py:41-348), which the reference hands to triteia.python.ops.ldmm or runs as one
 *      masked torch product per adapter of the batch.  indices: int32 [num_tokens], the adapter slot of every row
 *      (ToppingsManager.prepare_topping_batch); a row whose index is < 0 (the reference's -1: base model only) or
 *      >= num_slots is SKIPPED: nothing of it is read or written, and no address is formed from its index.
 *      Buffers keep the reference's layout (memory/topping_pool.py:88-124): a[slot] is [K, R] with R contiguous,
 *      b[slot] is [r, num_slices * n] with the columns contiguous; slot strides in elements.
 * sp_lora_shrink:  tmp[t, :R] = scale * (x[t, :K] . a[idx[t]])   fp32 [num_tokens, R], NOT rounded to `dtype`;
 *      R = (stacked slices) * r: 3 r for qkv_proj, 2 r for gate_up_proj.  scale = lora_alpha / r.
 * sp_lora_expand:  y[t, s n + c] += tmp[t, s r : (s+1) r] . b[idx[t]][:, s n + c]  for s < num_slices, c < n;
 *      y and tmp are passed already offset to the first column they touch.  y is read and written in `dtype`; per
 *      output ONE fp32 chain over j ascending, y = round(y + chain).  Columns >= num_slices * n of y are never touched.
 * Batch invariance: the bits a row receives depend on that row's x, y, index and adapter only - not on num_tokens,
 *      the row's position or its neighbours (the summation order is a function of (K, R, r) alone).
 * SP_ERR_UNSUPPORTED: dtype other than fp16 / bf16; K or n not a positive multiple of 8; R not a positive multiple
 *      of 8 or above 192; r not in {8, 16, 32, 64}; num_slices * r above 192.
 * SP_ERR_INVALID_ARG before any launch: a negative size, a NULL pointer, x_stride < K, tmp_stride < R (resp.
 *      num_slices * r), a_slot_stride < K * R, y_stride < num_slices * n, b_slot_stride < r * num_slices * n,
 *      x / a / y / b not 16-byte aligned or x_stride / y_stride / a slot stride not a multiple of 8 (16-byte vectors),
 *      tmp not 4-byte aligned.  num_tokens == 0 is SP_OK without a launch.  Like sp_gemm_skinny these entries sit on
 *      the decode step and do not ask the runtime whether their pointers are device memory.                        */
SP_API int sp_lora_shrink(float* tmp, const void* x, const void* a, const int32_t* indices, int64_t num_tokens,
                   int K, int R, int num_slots, int64_t x_stride, int64_t a_slot_stride, int64_t tmp_stride,
                   float scale, int dtype, void* stream);
SP_API int sp_lora_expand(void* y, const float* tmp, const void* b, const int32_t* indices, int64_t num_tokens,
                   int r, int n, int num_slices, int num_slots, int64_t y_stride, int64_t tmp_stride,
                   int64_t b_slot_stride, int dtype, void* stream);

/* ---- Delta toppings (additive in ABI 10): the DeltaW= half of the topping layers' ldmm(...) calls
 *      (nn/toppings/topping_layer.py) - a full-model delta W_finetuned - W_base per adapter slot, stored 4-bit and 2:4
 *      sparse (3 bits per dense weight), multiplied per row and added to the base projection's output.
 * The packed format (THIS library's; the reference's buffers are in triteia's Marlin tile order, which is not
 *      converted).  One projection, dense delta D[N, K] (output rows x input width, as the weights), per slot:
 *        codes  uint8 [N, K / 4]: byte g of row n is the group of columns 4 g .. 4 g + 3, of which two positions
 *               p0 < p1 are kept; low nibble = the code at p0, high nibble = the code at p1, codes in 0..15;
 *        meta   uint8 [N, K / 8]: byte m holds group 2 m in its low and group 2 m + 1 in its high nibble; a nibble is
 *               p0 | p1 << 2 and MUST have p0 < p1;
 *        scales [N] in `dtype`: D[n, 4 g + p] = scales[n] * (code - 8) at the two kept positions, 0 elsewhere.
 *      Stacked projections are stacked by rows (q | k | v, gate | up).  Slot strides: bytes for codes and meta,
 *      elements for scales.  A slot filled with code 8 (any valid meta, any finite scale) adds exactly 0: its rows of y
 *      are still rewritten, y + (+0.0), so a -0.0 there becomes +0.0 and every other value keeps its bits.
 * sp_delta_group: the stable counting sort of the rows t with 0 <= indices[t] < num_slots, by slot: slot_offsets int32
 *      [num_slots + 1], sorted_rows int32 [num_tokens] of which only the first slot_offsets[num_slots] entries are
 *      defined, ascending within a slot.  A row with any other index (the -1 of a base-model request, a padded graph
 *      row) appears nowhere.  No atomics: the order is a function of the indices alone.  One launch, also for
 *      num_tokens == 0 (slot_offsets then reads all zero).
 * sp_delta_mm: for every sorted row t of slot s, in place,
 *        y[t, n] = round_dtype( y[t, n] + scales_s[n] * sum_k x[t, k] * q_s[n, k] )        q = code - 8, an integer
 *      with ONE fp32 accumulation (the operands q are exact in fp16 / bf16), the scale applied once in fp32 behind the
 *      sum, one rounding.  The sum runs over super-steps of 256 columns dealt round-robin to 8 partial sums, each a
 *      chain of v_mfma_f32_16x16x32 (8 per super-step), folded in order: depth c(K) = 33 * 8 * ceil(ceil(K / 256) / 8)
 *      + 10 fp32 roundings at most.  A row that is in no group is neither read nor written and no address is formed
 *      from its index; every sorted row is checked against [0, num_tokens) first.  Every (t, n) has one writer provided
 *      sorted_rows names a row once (sp_delta_group does).  A slot without rows costs no weight traffic.
 * Batch invariance: the bits a row receives depend on that row's x and y, its slot's packed delta and (N, K) only - not
 *      on num_tokens, the row's position, its neighbours or how many rows its slot has.
 * SP_ERR_UNSUPPORTED: num_slots == 0 or > 64; num_tokens > 16384; (sp_delta_mm) a dtype other than fp16 / bf16, K not
 *      a positive multiple of 64, N not a positive multiple of 16 or above 1048560.
 * SP_ERR_INVALID_ARG before any launch: a NULL pointer, a negative size, x_stride < K, y_stride < N,
 *      codes_slot_stride < N K / 4, meta_slot_stride < N K / 8, scales_slot_stride < N; x or codes not 16-byte aligned,
 *      meta not 8-byte aligned, y or scales not 2-byte aligned, x_stride not a multiple of 8, codes_slot_stride not a
 *      multiple of 16, meta_slot_stride not a multiple of 8.  sp_delta_mm with num_tokens == 0 is SP_OK without a
 *      launch.  Like sp_gemm_skinny these entries sit on the decode step and do not ask the runtime whether their
 *      pointers are device memory.                                                                                 */
SP_API int sp_delta_group(int32_t* slot_offsets, int32_t* sorted_rows, const int32_t* indices, int64_t num_tokens,
                   int num_slots, void* stream);
SP_API int sp_delta_mm(void* y, const void* x, const void* codes, const void* meta, const void* scales,
                const int32_t* slot_offsets, const int32_t* sorted_rows, int64_t num_tokens, int num_slots, int N,
                int K, int64_t x_stride, int64_t y_stride, int64_t codes_slot_stride, int64_t meta_slot_stride,
                int64_t scales_slot_stride, int dtype, void* stream);

/* ---- Mixture of experts (additive in ABI 10): LlamaMoE.forward (nn/models/llama/llama_moe.py:98-120) as launches
 *      whose grids depend on (num_tokens, top_k, num_experts) and the widths alone; the grouping is read from device
 *      memory, so a captured sequence follows the routing of every replay.  T = num_tokens, K = top_k, E = num_experts.
 * sp_moe_route:   router_logits [T, E] in `dtype` (fp32, fp16 or bf16; row stride in elements).  topk_ids int32 [T, K]:
 *      the K largest logits of the row, largest first; among equal logits the LOWER expert index wins; NaN counts as
 *      the largest value.  Every id written is in [0, E) whatever the logits hold.  topk_weights fp32 [T, K]: the
 *      softmax over those K (torch.topk, then F.softmax(dtype=float).to(x.dtype), llama_moe.py:102-104), evaluated in
 *      fp64 in k order, rounded to fp32 and then to `dtype`.  expert_offsets int32 [E + 1] and sorted_pos int32 [T K]:
 *      the pairs t K + k ordered by expert and, within an expert, ascending - a stable counting sort, a function of
 *      the ids alone.  Two launches.
 * sp_moe_gate_up: h[p, :inter] = round(silu(round(x[t] . Wg[e]^T)) * round(x[t] . Wu[e]^T)) for sorted position p
 *      = pair t K + k of expert e; w13 [E, 2 inter, hidden] gate rows first, rows contiguous.  h [T K, inter] is
 *      indexed by SORTED POSITION.  The rounding points are those of sp_gemm_skinny followed by sp_silu_and_mul.
 * sp_moe_down:    tmp[t K + k, :hidden] = round(round(h[p] . W2[e]^T) * topk_weights[t, k]); w2 [E, hidden, inter].
 *      tmp [T K, hidden] is indexed by PAIR.
 * sp_moe_combine: out[t] = the K rows of tmp of token t, added from zero in ascending expert index, rounded to `dtype`
 *      after every addition (the reference's results[...] += expert(x) * weight sequence, llama_moe.py:111-118).
 * Batch invariance: the bits of a token's output depend on that token's input, its routing and the weights only - not
 *      on T, its row or how many rows an expert received (the reduction is split by its length alone).
 * sp_moe_block_rows: sorted positions a workgroup of the two products owns.  sp_moe_max_tokens: the largest T (16384).
 * SP_ERR_UNSUPPORTED: E == 0 or > 64; K == 0, > 8 or > E; T > sp_moe_max_tokens(); gate_up / down / combine with a
 *      dtype other than fp16 / bf16 (route: any of the three); hidden or inter not a positive multiple of 32.
 * SP_ERR_INVALID_ARG before any launch: a negative size, a NULL pointer, a stride below the width it spans,
 *      x / h / tmp / out strides or expert strides not a multiple of 8 and bases not 16-byte aligned where 16-byte
 *      vectors are read (x, w13, h, w2, tmp, out).  T == 0 is SP_OK without a launch.  Like sp_gemm_skinny these
 *      entries sit on the decode step and do not ask the runtime whether their pointers are device memory.        */
SP_API int sp_moe_block_rows(void);
SP_API int sp_moe_max_tokens(void);
SP_API int sp_moe_route(int32_t* topk_ids, float* topk_weights, int32_t* expert_offsets, int32_t* sorted_pos,
                 const void* router_logits, int64_t num_tokens, int num_experts, int top_k, int64_t logits_stride,
                 int dtype, void* stream);
SP_API int sp_moe_gate_up(void* h, const void* x, const void* w13, const int32_t* expert_offsets,
                   const int32_t* sorted_pos, int64_t num_tokens, int top_k, int num_experts, int hidden, int inter,
                   int64_t x_stride, int64_t h_stride, int64_t w_expert_stride, int dtype, void* stream);
SP_API int sp_moe_down(void* tmp, const void* h, const void* w2, const float* topk_weights,
                const int32_t* expert_offsets, const int32_t* sorted_pos, int64_t num_tokens, int top_k,
                int num_experts, int hidden, int inter, int64_t h_stride, int64_t tmp_stride,
                int64_t w_expert_stride, int dtype, void* stream);
SP_API int sp_moe_combine(void* out, const void* tmp, const int32_t* topk_ids, int64_t num_tokens, int top_k,
                   int num_experts, int hidden, int64_t tmp_stride, int64_t out_stride, int dtype, void* stream);

/* ---- Quantised mixture of experts (additive in ABI 10): the expert half of LlamaQuantisedMoE.forward
 *      (nn/models/llama/llama_quant_moe.py:204-257) and of the naive variant (llama_naive_quant_moe.py:140-163):
 *      top_k of num_experts compressed experts on top of a dense base MLP, out = sum_k w_k expert_k(x) + base_mlp(x).
 *      Routing and the sort are sp_moe_route's, unchanged.  T = num_tokens, K = top_k, E = num_experts, H = hidden,
 *      I = inter.  `rnd` = round to fp32, then to `dtype`.
 * The experts are stored in THIS library's packed format, the one stated under "Delta toppings" above (codes / meta /
 *      scales of a dense [N, red] matrix), stacked over the experts; the reference's qweight / meta / workspace triple
 *      is in triteia's Marlin tile order and is not converted.  Per projection:
 *        codes  uint8 [E, N, red / 4]     meta  uint8 [E, N, red / 8]     scales [E, N] in `dtype`
 *      gate_up: N = 2 I (gate rows first), red = H; down: N = H, red = I.  Expert strides: bytes for codes and meta,
 *      elements for scales.  An expert of code 8 (any valid meta, any finite scale) contributes exactly 0.
 * sp_qmoe_gate_up: h[p, n] = rnd( rnd(silu(rnd(sg[n] * G))) * rnd(su[n] * U) ),  G = sum_k x[t, k] q_e[n, k] and U the
 *      same sum over row I + n, for sorted position p = pair t K + k of expert e (x is gathered through sorted_pos,
 *      t = pair / K).  ONE fp32 accumulation per sum; the scale is multiplied once, in fp32, behind the sum.
 *      h [T K, I] is indexed by SORTED POSITION; rows at or past expert_offsets[E] are left untouched.
 * sp_qmoe_down:    tmp[t K + k, n] = rnd( rnd(s[n] * sum_j h[p, j] q_e[n, j]) * topk_weights[t, k] ).  tmp [T K, H] is
 *      indexed by PAIR.  topk_weights is fp32 holding values of `dtype`, as sp_moe_route writes it.
 * sp_qmoe_combine: acc = +0; for the K pairs of token t in the chosen order acc = rnd(acc + tmp[t K + j]); then
 *      out[t] = rnd(acc + base[t]).  order 0: ascending expert index, ties by k (the naive variant; sp_moe_combine's
 *      order).  order 1: j = 0 .. K - 1 (the sbmm variant).  out may alias base.  A pair whose id lies outside [0, E)
 *      is skipped.
 * Reduction order: sp_delta_mm's by definition (super-steps of 256 columns round-robin over 8 partial sums, 8
 *      v_mfma_f32_16x16x32 per super-step, folded in order): sp_qmoe_down with K = 1, ascending ids and weights 1.0
 *      writes the bits sp_delta_mm adds to a zeroed y.
 * Batch invariance: a token's bits depend on its input, its routing, the packed experts and (H, I) only - not on T,
 *      its row or how many rows an expert received.
 * Every offset read from device memory is clamped; every sorted entry and id is range-checked before an address is
 *      formed from it; byte offsets are 64-bit; every (row, n) has one writer; no atomics and no zero-fill launch.  An
 *      expert without rows costs no weight traffic.
 * sp_qmoe_weight_tiles: 16-row weight tiles a workgroup of the two products owns (a build-time figure; it changes no
 *      element's reduction order).
 * SP_ERR_UNSUPPORTED: a dtype other than fp16 / bf16; hidden or inter not a positive multiple of 64; E == 0 or > 64;
 *      K == 0, > 8 or > E; T > 16384; (combine) order not 0 or 1.
 * SP_ERR_INVALID_ARG before any launch: a NULL pointer, a negative size; a stride below the width it spans (x_stride
 *      < H, h_stride < I, tmp / base / out strides < H, codes / meta / scales expert strides below N red / 4, N red / 8,
 *      N); x, h, tmp, base, out or codes not 16-byte aligned, meta not 8-byte aligned, scales not 2-byte aligned;
 *      x / h / tmp / base / out strides not a multiple of 8, codes expert stride not a multiple of 16, meta expert
 *      stride not a multiple of 8; more than 65535 grid.y blocks.  T == 0 is SP_OK without a launch.  Like
 *      sp_gemm_skinny these entries sit on the decode step and do not ask the runtime whether their pointers are
 *      device memory.                                                                                              */
SP_API int sp_qmoe_weight_tiles(void);
SP_API int sp_qmoe_gate_up(void* h, const void* x, const void* codes, const void* meta, const void* scales,
                    const int32_t* expert_offsets, const int32_t* sorted_pos, int64_t num_tokens, int top_k,
                    int num_experts, int hidden, int inter, int64_t x_stride, int64_t h_stride,
                    int64_t codes_expert_stride, int64_t meta_expert_stride, int64_t scales_expert_stride, int dtype,
                    void* stream);
SP_API int sp_qmoe_down(void* tmp, const void* h, const void* codes, const void* meta, const void* scales,
                 const float* topk_weights, const int32_t* expert_offsets, const int32_t* sorted_pos,
                 int64_t num_tokens, int top_k, int num_experts, int hidden, int inter, int64_t h_stride,
                 int64_t tmp_stride, int64_t codes_expert_stride, int64_t meta_expert_stride,
                 int64_t scales_expert_stride, int dtype, void* stream);
SP_API int sp_qmoe_combine(void* out, const void* tmp, const void* base, const int32_t* topk_ids, int64_t num_tokens,
                    int top_k, int num_experts, int hidden, int64_t tmp_stride, int64_t base_stride,
                    int64_t out_stride, int order, int dtype, void* stream);

/* ---- Embedding requests (additive in ABI 10): the final norm of the decoder, Pooler(PoolingType.LAST) and
 *      F.normalize (nn/layers/pooler.py:38-50 behind nn/models/llama/llama.py:268) in one launch, on the num_seqs
 *      rows that matter.  One workgroup per sequence i:
 *        row_i  = extend_seq_lens[0] + ... + extend_seq_lens[i] - 1        (int32 lengths, int64 with idx64)
 *        n      = weight ? the row sp_fused_add_rmsnorm (residual given) / sp_rmsnorm (residual NULL) writes for
 *                          row_i, bit for bit : x[row_i]
 *        out[i] = normalize ? round(n / max(round(||n||_2), round(1e-12))) : n
 *      ("bit for bit": the norm entries sum the squares in one of two orders, chosen by whether base, stride and
 *      width of x, residual, weight AND of the buffer they write allow 16-byte accesses.  This entry chooses by x,
 *      residual and weight alone - its `out` is no counterpart of theirs - so it matches sp_fused_add_rmsnorm, which
 *      writes x itself, always, and sp_rmsnorm whenever that call's own `out` is 16-byte aligned with an out_stride
 *      that is a multiple of 16 bytes, or x already forces element accesses.)
 *      ||n||_2 is accumulated in fp32 in an order fixed by `hidden` alone, so a sequence's bits do not depend on
 *      num_seqs, on i or on the other rows; round() rounds to `dtype` (fp16: round(1e-12) = 0, an all-zero row gives
 *      NaN as torch's F.normalize does; a norm beyond the fp16 range gives zeros).  x and residual are NOT written.
 *      A sequence of length <= 0, or a row_i outside [0, num_tokens), forms no address: out[i] is zeros.
 *      Only row i itself is refused: the lengths are not validated as a whole, so a NEGATIVE length moves row_j of
 *      every later sequence j down without any warning, and those rows are then pooled from the wrong tokens (a zero
 *      length moves nothing).  Every workgroup adds extend_seq_lens[0..i] itself - num_seqs^2 / 2 index reads per
 *      launch in all, which is nothing at serving batch sizes and would want a prefix pass at tens of thousands.
 *      Any hidden; 16-byte accesses where base, stride and width allow, element accesses otherwise.  Strides in
 *      elements.  num_seqs == 0 is SP_OK without a launch.  SP_ERR_INVALID_ARG before any launch: out, x or
 *      extend_seq_lens NULL, a negative size, hidden <= 0, a stride below hidden, residual without weight, weight
 *      with eps <= 0.  SP_ERR_UNSUPPORTED: a dtype other than fp32 / fp16 / bf16.                                  */
SP_API int sp_embedding_pool(void* out, int64_t out_stride, const void* x, int64_t x_stride, const void* residual,
                      int64_t res_stride, const void* weight, float eps, const void* extend_seq_lens, int idx64,
                      int num_seqs, int64_t num_tokens, int hidden, int normalize, int dtype, void* stream);

/* ---- Direct all-reduce through IPC-mapped peer regions: fills GroupCoordinator.ca_comm
 *      (distributed/parallel_state.py:266-267, 326-347; the reference never constructs one and always
 *      calls NCCL, linear.py:1148-1149).  Each rank sp_ar_alloc()s one fine-grained region of
 *      sp_ar_flag_bytes() + 2 * data_bytes, exports it (64-byte IPC handle), and imports every peer's.
 *      sp_custom_all_reduce sums `num_elems` elements over the `world` ranks (one-shot up to 256 KiB,
 *      reduce-scatter + all-gather above); `regions[r]` = rank r's region as mapped in this process;
 *      calls are collective (every rank issues the same sequence; the call counters live in the regions,
 *      so the launch is graph-capturable - the role of pynccl inside the reference's graphs,
 *      parallel_state.py:256-302).
 *      Failure is collective: a peer barrier that waits longer than `timeout_us` (<= 0: 30 s) raises the
 *      status word of EVERY rank's region and the caller's `host_status` word (device pointer of the pinned
 *      word from sp_ar_host_status_alloc, or NULL), which the host reads as plain memory at every forward
 *      boundary; a launch that finds its region's status raised raises its own host word and stops
 *      waiting.  sp_ar_status reads the region's status word through a synchronising copy (check points).
 *      Opt-in (see allreduce.hip: not yet run across xGMI).  sp_ar_alloc / sp_ar_ipc_import /
 *      sp_ar_host_status_alloc are the only entries that allocate; the caller's object owns the memory.  */
SP_API size_t sp_ar_flag_bytes(void);
SP_API int sp_ar_alloc(void** ptr, size_t bytes);
SP_API int sp_ar_free(void* ptr);
SP_API int sp_ar_ipc_export(void* ptr, void* handle64);
SP_API int sp_ar_ipc_import(const void* handle64, void** ptr);
SP_API int sp_ar_ipc_close(void* ptr);
SP_API int sp_ar_status(const void* own_region, int* status);
SP_API int sp_ar_host_status_alloc(void** host_ptr, void** device_ptr);
SP_API int sp_ar_host_status_free(void* host_ptr);
SP_API int sp_custom_all_reduce(void* out, const void* in, int64_t num_elems, int dtype, void* const* regions,
                         int rank, int world, size_t data_bytes, int64_t timeout_us, void* host_status,
                         void* stream);

/* ---- Fused all-reduce + residual add + RMSNorm on the same regions: RowParallelLinear's all-reduce
 *      (nn/layers/linear.py:1148-1149) followed by the next RMSNorm(x, residual) of the decoder layer
 *      (nn/models/llama/llama.py:216, 222, 268 -> nn/layers/layernorm.py:22-32), 2 x layers per step.
 *      x [T, hidden]: this rank's partial sums in, the normalised activations out; residual [T, hidden]
 *      in/out.  Bit for bit  x <- sp_custom_all_reduce(x); sp_fused_add_rmsnorm(x, residual, w, eps)
 *      (one rounding of the fp32 rank-order sum, then the norm kernel's rounding points and summation
 *      order).  One-shot up to 256 KiB, else reduce-scatter by rows + gather of the bf16 sums with the
 *      norm applied on arrival.  Collective, graph-capturable, same failure protocol as above.
 *      SP_ERR_UNSUPPORTED (caller runs the two-step form): hidden not a multiple of the 16-byte vector or
 *      above 8192 elements, unaligned pointers/strides.  Strides in elements.                           */
SP_API int sp_fused_allreduce_add_rmsnorm(void* x, void* residual, const void* weight, int64_t num_tokens,
                                   int hidden, int64_t x_stride, int64_t res_stride, float eps, int dtype,
                                   void* const* regions, int rank, int world, size_t data_bytes,
                                   int64_t timeout_us, void* host_status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCRATCHPAD_HIP_H */
