// causal.hip — causal grouped-query attention that appends to a key / value cache, and the device end of a greedy decode step
// (PaddleOCR-VL's text decoder behind reference core/image/ocr_detection.py:886-962; include/mtx_hip.h, mtx_causal_attn_args / mtx_greedy_args).
//
//   prefill (rows > 1)  4 waves x 16 query rows of ONE head per workgroup, 32-key tiles, v_mfma_f32_16x16x32.  Both products are computed
//                       transposed as in attention.hip's small kernel (S^T = K Q^T, O^T = V^T P^T): the 16 lanes l & 15 are the query rows, a
//                       lane's S^T values are already the B operand of the second product.  K fragments come straight from memory (16 bytes
//                       per lane: the cache below `pos`, the launch's own rows from there on), V goes through LDS row-major and is read with
//                       the hardware transpose.  The softmax weights reach the matrix pipe as TWO 16-bit halves (p = hi + lo, the low half of
//                       f16 scaled by 2^12 into the normal range) with an accumulator each, so that the sum is an fp32 sum of products good
//                       to 16+ bits of p, not of p rounded to 8 or 11 bits: the op's contract is ONE rounding, and the step kernel below
//                       keeps p in fp32.
//   step (rows == 1)    a streaming kernel.  Workgroup (split, kv head, chunk of G query heads): 16 lanes share a key (16 x 16 bytes = the
//                       128-wide head), the 16 lane groups walk the split's 64 keys 16 at a time, every key / value chunk is read ONCE and
//                       used for all G query heads of the group.  The workgroup's state (m, l, acc[128]) per head goes to the workspace
//                       write-through; the workgroup that draws the last ticket merges the records in key order (mtx_device.h, hand-offs).
//   greedy pick         arg max of the fp32 logits in 4096-wide chunks (value, lowest index), then one wave that folds the chunks and
//                       advances the 16-byte decode state.  Two launches: the second starts a launch boundary after the first.
//   slot-batched step   the step and the pick for up to MTX_SLOTS_MAX independent sequences in one launch each (mtx_causal_step_batch_args /
//                       mtx_greedy_batch_args): the slot is folded into the grid, every slot has its own cache, workspace region and lane of
//                       the int32 [5][8] state block; the step's body is causal_step_body.inc, included in both step kernels, so a slot's
//                       result is bit for bit the single op's.  A finished or empty slot leaves before any barrier or ticket.
//   packed prompts      the prefill for up to MTX_SLOTS_MAX prompts packed row-wise into one qkv buffer, each into its own empty slot cache, in
//                       one launch (mtx_causal_prefill_slots_args): the boundaries are a DEVICE table of row offsets, the grid is sized from
//                       the buffer's capacity, a workgroup finds its prompt by walking the table; the body is causal_prefill_body.inc, included
//                       in both prefill kernels, so a prompt's rows and cache are bit for bit the single op's at pos = 0.
#include "mtx_device.h"
#include <limits.h>

namespace mtx {

constexpr int CA_D = 128;
constexpr int CA_TQ = MTX_CAUSAL_TQ;
constexpr int CA_TK = MTX_CAUSAL_TK;
constexpr int CA_S = MTX_CAUSAL_S;
constexpr int CA_REC = MTX_CAUSAL_REC;
constexpr int CA_VROW = CA_D + 16;        // LDS row of the V tile in elements: 72 dwords, so the 8 rows a half wave's transpose read touches fall on 8 x 8 distinct banks
constexpr float CA_NEG = -1.0e30f;        // running maximum before the first key (finite: exp(CA_NEG - m) is 0, never NaN)
static_assert(CA_TQ == 64 && CA_TK == 32 && CA_S % 16 == 0 && CA_REC >= 4 + CA_D, "tile constants of include/mtx_hip.h");

template <typename T>
__global__ __launch_bounds__(256) void causal_prefill_kernel(mtx_causal_attn_args p) {
#define CA_PREFILL_POS *p.pos
#define CA_PREFILL_QB blockIdx.x
#include "causal_prefill_body.inc"
#undef CA_PREFILL_POS
#undef CA_PREFILL_QB
}

// ---- the step --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ca_load8(const __bf16* p, float (&f)[8]) { unpack8<__bf16>(*reinterpret_cast<const u32x4*>(p), f); }
__device__ __forceinline__ void ca_load8(const _Float16* p, float (&f)[8]) { unpack8<_Float16>(*reinterpret_cast<const u32x4*>(p), f); }

// merge the online-softmax state (m, l, acc) with another one
__device__ __forceinline__ void ca_merge(float& m, float& l, float (&acc)[8], float m2, float l2, const float (&acc2)[8]) {
  const float mn = m > m2 ? m : m2;
  const float f1 = __expf(m - mn), f2 = __expf(m2 - mn);
  l = l * f1 + l2 * f2;
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = acc[e] * f1 + acc2[e] * f2;
  m = mn;
}

// grid (splits of CA_S keys, kv heads, chunks of G query heads); gfull = heads / kv_heads = gridDim.z * G
template <typename T, int G>
__global__ __launch_bounds__(256) void causal_step_kernel(mtx_causal_attn_args p, int gfull) {
#define CA_STEP_Z (int)blockIdx.z
#define CA_STEP_Z_IS_0 blockIdx.z == 0
#define CA_STEP_NZ (int)gridDim.z
#include "causal_step_body.inc"
#undef CA_STEP_Z
#undef CA_STEP_Z_IS_0
#undef CA_STEP_NZ
}

int causal_attn_launch(const mtx_causal_attn_args* a, void* stream, const char** err) {
  if (!a->qkv || !a->k_cache || !a->v_cache || !a->pos || !a->o) { *err = "causal_attn: null operand"; return MTX_ERR_INVALID; }
  if (a->d != CA_D) { *err = "causal_attn: only head width 128 is built"; return MTX_ERR_UNSUPPORTED; }
  if (a->heads < 1 || a->kv_heads < 1 || a->heads % a->kv_heads) { *err = "causal_attn: heads must be a multiple of kv_heads"; return MTX_ERR_UNSUPPORTED; }
  if (a->heads > 65535 || a->rows < 1 || a->max_len < 1 || a->rows > a->max_len) { *err = "causal_attn: needs 1 <= rows <= max_len, heads <= 65535"; return MTX_ERR_INVALID; }
  const long qkv_w = ((long)a->heads + 2L * a->kv_heads) * CA_D;
  if (a->ld_qkv % 8 || a->ld_o % 8 || a->ld_qkv < qkv_w || a->ld_o < (long)a->heads * CA_D) { *err = "causal_attn: row strides must be multiples of 8 and cover the row"; return MTX_ERR_INVALID; }
  if ((((size_t)a->qkv | (size_t)a->k_cache | (size_t)a->v_cache | (size_t)a->o) & 15) != 0) { *err = "causal_attn: operands must be 16-byte aligned"; return MTX_ERR_INVALID; }
  if (a->dtype != MTX_BF16 && a->dtype != MTX_F16) { *err = "causal_attn: dtype must be bf16 or f16"; return MTX_ERR_INVALID; }
  if (a->rows > 1) {
    const dim3 grid((unsigned)((a->rows + CA_TQ - 1) / CA_TQ), (unsigned)a->heads);
    MTX_LAUNCH_T(a->dtype, causal_prefill_kernel, grid, dim3(256), stream, *a);
    return MTX_OK;
  }
  if (!a->workspace || ((size_t)a->workspace & 15) || a->workspace_bytes < (int64_t)MTX_CAUSAL_WS_BYTES(a->heads, a->max_len)) {
    *err = "causal_attn: the step (rows == 1) needs a zeroed workspace of MTX_CAUSAL_WS_BYTES(heads, max_len)"; return MTX_ERR_INVALID;
  }
  const int gfull = a->heads / a->kv_heads;
  const int g = gfull % 8 == 0 ? 8 : (gfull % 4 == 0 ? 4 : (gfull % 2 == 0 ? 2 : 1));      // query heads that share one pass over the keys
  const dim3 grid((unsigned)((a->max_len + CA_S - 1) / CA_S), (unsigned)a->kv_heads, (unsigned)(gfull / g));
  if (grid.y > 65535u || grid.z > 65535u) { *err = "causal_attn: too many heads"; return MTX_ERR_INVALID; }
  with_storage_type(a->dtype, [&](auto t) {
    typedef typename decltype(t)::type T;
    if (g == 8) MTX_LAUNCH((causal_step_kernel<T, 8>), grid, dim3(256), 0, stream, *a, gfull);
    else if (g == 4) MTX_LAUNCH((causal_step_kernel<T, 4>), grid, dim3(256), 0, stream, *a, gfull);
    else if (g == 2) MTX_LAUNCH((causal_step_kernel<T, 2>), grid, dim3(256), 0, stream, *a, gfull);
    else MTX_LAUNCH((causal_step_kernel<T, 1>), grid, dim3(256), 0, stream, *a, gfull);
  });
  return MTX_OK;
}

// ---- greedy pick -----------------------------------------------------------------------------------------------------------------------
// (value, index) order: the larger value wins, among equal values the lower index; a NaN compares false both ways and never replaces anything
__device__ __forceinline__ void gp_take(float& bv, int& bi, float v, int i) {
  if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}
__device__ __forceinline__ void gp_wave(float& bv, int& bi) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float v = __shfl_xor(bv, off, 64);
    const int i = __shfl_xor(bi, off, 64);
    gp_take(bv, bi, v, i);
  }
}

// one chunk of one row of logits -> its (value, lowest index) record
__device__ __forceinline__ void gp_chunk(const float* logits, int vocab, void* scratch) {
  __shared__ float wv[4];
  __shared__ int wi[4];
  const int tid = threadIdx.x;
  const long base = (long)blockIdx.x * MTX_GREEDY_CHUNK;
  float bv = -INFINITY;
  int bi = INT_MAX;
#pragma unroll 4
  for (int k = 0; k < MTX_GREEDY_CHUNK / 256; ++k) {
    const long i = base + tid + 256 * k;
    if (i < vocab) gp_take(bv, bi, logits[i], (int)i);
  }
  gp_wave(bv, bi);
  if ((tid & 63) == 0) { wv[tid >> 6] = bv; wi[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) gp_take(bv, bi, wv[w], wi[w]);
    float* rec = reinterpret_cast<float*>(scratch) + 2 * blockIdx.x;
    rec[0] = bv;
    reinterpret_cast<int*>(rec)[1] = bi;
  }
}

// One wave folds a row's chunk records and advances the sequence's state {pos, n_out, done, token}, whose fields lie ST words apart (1: the
// single op's int32[4]; MTX_SLOTS_MAX: one lane of the slot block).  The body of greedy_final_kernel and of its slot-batched twin, stamped
// into each (a macro, so that the single kernel stays the code it was): `p` = the kernel's args, SCRATCH / STATE / OUT = this row's record
// run, state and output row, ALSO = what else advances with pos.
#define GP_FINAL_BODY(ST, SCRATCH, STATE, OUT, ALSO)                                                                   \
  const int lane = threadIdx.x;                                                                                        \
  float bv = -INFINITY;                                                                                                \
  int bi = INT_MAX;                                                                                                    \
  for (int c = lane; c < chunks; c += 64) {                                                                            \
    const float* rec = reinterpret_cast<const float*>(SCRATCH) + 2 * c;                                                \
    gp_take(bv, bi, rec[0], reinterpret_cast<const int*>(rec)[1]);                                                     \
  }                                                                                                                    \
  gp_wave(bv, bi);                                                                                                     \
  if (lane != 0) return;                                                                                               \
  int* st = STATE;                           /* {pos, n_out, done, token} */                                           \
  if (st[2 * ST]) return;                    /* a finished sequence changes nothing */                                 \
  int n_out = st[1 * ST];                                                                                              \
  if (n_out < 0 || n_out >= p.max_new) { st[2 * ST] = 1; return; }      /* (a damaged state must not leave `out`) */    \
  const int t = bi == INT_MAX ? 0 : bi;      /* all NaN */                                                             \
  (OUT)[n_out++] = t;                                                                                                  \
  int done = n_out == p.max_new;                                                                                       \
  for (int e = 0; e < p.n_eos; ++e) done |= t == p.eos[e];                                                             \
  st[0] += p.advance;                                                                                                  \
  st[1 * ST] = n_out;                                                                                                  \
  st[2 * ST] = done;                                                                                                   \
  st[3 * ST] = t;                                                                                                      \
  ALSO

__global__ __launch_bounds__(256) void greedy_chunk_kernel(mtx_greedy_args p) {
  gp_chunk(p.logits, p.vocab, p.scratch);
}

__global__ __launch_bounds__(64) void greedy_final_kernel(mtx_greedy_args p, int chunks) {
  GP_FINAL_BODY(1, p.scratch, p.state, p.out, ;)
}

int greedy_launch(const mtx_greedy_args* a, void* stream, const char** err) {
  if (!a->logits || !a->state || !a->out || !a->scratch) { *err = "greedy_pick: null operand"; return MTX_ERR_INVALID; }
  if (a->vocab < 1 || a->max_new < 1 || a->n_eos < 0 || a->n_eos > 4) { *err = "greedy_pick: needs vocab >= 1, max_new >= 1, 0 <= n_eos <= 4"; return MTX_ERR_INVALID; }
  const int chunks = (int)(((long)a->vocab + MTX_GREEDY_CHUNK - 1) / MTX_GREEDY_CHUNK);
  MTX_LAUNCH(greedy_chunk_kernel, dim3((unsigned)chunks), dim3(256), 0, stream, *a);
  MTX_LAUNCH(greedy_final_kernel, dim3(1), dim3(64), 0, stream, *a, chunks);
  return MTX_OK;
}

// ---- the slot-batched step (MTX_OP_CAUSAL_STEP_BATCH, MTX_OP_GREEDY_BATCH) -----------------------------------------------------------------
// the same step for `slots` sequences: grid (splits, kv heads, slots * nz), nz = gfull / G chunks of query heads; slot s owns cache s,
// row s of qkv and o, and region s of the workspace (its own counters and records), so the slots never meet
template <typename T, int G>
__global__ __launch_bounds__(256) void causal_step_batch_kernel(mtx_causal_step_batch_args b, int gfull, int nz) {
  const int slot = (int)blockIdx.z / nz, zc = (int)blockIdx.z - slot * nz;
  if (b.state[MTX_SLOT_DONE * MTX_SLOTS_MAX + slot] != 0) return;      // (workgroup-uniform, before any barrier or ticket) a finished or empty slot sits out
  mtx_causal_attn_args p;
  p.qkv = reinterpret_cast<const T*>(b.qkv) + (long)slot * b.ld_qkv;
  p.k_cache = reinterpret_cast<T*>(b.k_cache) + (long)slot * b.cache_stride;
  p.v_cache = reinterpret_cast<T*>(b.v_cache) + (long)slot * b.cache_stride;
  p.pos = b.state + MTX_SLOT_POS * MTX_SLOTS_MAX + slot;               // the body reads it and leaves (as uniformly) unless 0 <= pos < max_len
  p.o = reinterpret_cast<T*>(b.o) + (long)slot * b.ld_o;
  p.rows = 1; p.heads = b.heads; p.kv_heads = b.kv_heads; p.d = b.d; p.max_len = b.max_len;
  p.ld_qkv = b.ld_qkv; p.ld_o = b.ld_o;
  p.scale = b.scale; p.dtype = b.dtype;
  p.workspace = reinterpret_cast<unsigned char*>(b.workspace) + (long)slot * (long)MTX_CAUSAL_WS_BYTES(b.heads, b.max_len);
  p.workspace_bytes = (int64_t)MTX_CAUSAL_WS_BYTES(b.heads, b.max_len);
#define CA_STEP_Z zc
#define CA_STEP_Z_IS_0 zc == 0
#define CA_STEP_NZ nz
#include "causal_step_body.inc"
#undef CA_STEP_Z
#undef CA_STEP_Z_IS_0
#undef CA_STEP_NZ
}

int causal_step_batch_launch(const mtx_causal_step_batch_args* a, void* stream, const char** err) {
  if (!a->qkv || !a->k_cache || !a->v_cache || !a->state || !a->o) { *err = "causal_step_batch: null operand"; return MTX_ERR_INVALID; }
  if (a->slots < 1 || a->slots > MTX_SLOTS_MAX) { *err = "causal_step_batch: needs 1 <= slots <= MTX_SLOTS_MAX"; return MTX_ERR_INVALID; }
  if (a->d != CA_D) { *err = "causal_step_batch: only head width 128 is built"; return MTX_ERR_UNSUPPORTED; }
  if (a->heads < 1 || a->kv_heads < 1 || a->heads % a->kv_heads) { *err = "causal_step_batch: heads must be a multiple of kv_heads"; return MTX_ERR_UNSUPPORTED; }
  if (a->heads > 65535 || a->max_len < 1) { *err = "causal_step_batch: needs max_len >= 1, heads <= 65535"; return MTX_ERR_INVALID; }
  const long qkv_w = ((long)a->heads + 2L * a->kv_heads) * CA_D;
  if (a->ld_qkv % 8 || a->ld_o % 8 || a->ld_qkv < qkv_w || a->ld_o < (long)a->heads * CA_D) { *err = "causal_step_batch: row strides must be multiples of 8 and cover the row"; return MTX_ERR_INVALID; }
  if (a->cache_stride % 8 || a->cache_stride < (long)a->max_len * a->kv_heads * CA_D) { *err = "causal_step_batch: cache_stride must be a multiple of 8 and cover one cache"; return MTX_ERR_INVALID; }
  if ((((size_t)a->qkv | (size_t)a->k_cache | (size_t)a->v_cache | (size_t)a->o) & 15) != 0) { *err = "causal_step_batch: operands must be 16-byte aligned"; return MTX_ERR_INVALID; }
  if (a->dtype != MTX_BF16 && a->dtype != MTX_F16) { *err = "causal_step_batch: dtype must be bf16 or f16"; return MTX_ERR_INVALID; }
  if (!a->workspace || ((size_t)a->workspace & 15) || a->workspace_bytes < (int64_t)a->slots * (int64_t)MTX_CAUSAL_WS_BYTES(a->heads, a->max_len)) {
    *err = "causal_step_batch: needs a zeroed workspace of slots * MTX_CAUSAL_WS_BYTES(heads, max_len)"; return MTX_ERR_INVALID;
  }
  const int gfull = a->heads / a->kv_heads;
  const int g = gfull % 8 == 0 ? 8 : (gfull % 4 == 0 ? 4 : (gfull % 2 == 0 ? 2 : 1));      // as the single step: the same instantiation per head layout
  const int nz = gfull / g;
  const dim3 grid((unsigned)((a->max_len + CA_S - 1) / CA_S), (unsigned)a->kv_heads, (unsigned)(nz * a->slots));
  if (grid.y > 65535u || grid.z > 65535u) { *err = "causal_step_batch: too many heads"; return MTX_ERR_INVALID; }
  with_storage_type(a->dtype, [&](auto t) {
    typedef typename decltype(t)::type T;
    if (g == 8) MTX_LAUNCH((causal_step_batch_kernel<T, 8>), grid, dim3(256), 0, stream, *a, gfull, nz);
    else if (g == 4) MTX_LAUNCH((causal_step_batch_kernel<T, 4>), grid, dim3(256), 0, stream, *a, gfull, nz);
    else if (g == 2) MTX_LAUNCH((causal_step_batch_kernel<T, 2>), grid, dim3(256), 0, stream, *a, gfull, nz);
    else MTX_LAUNCH((causal_step_batch_kernel<T, 1>), grid, dim3(256), 0, stream, *a, gfull, nz);
  });
  return MTX_OK;
}

// grid (chunks, slots): row blockIdx.y of the logits, its own run of `chunks` records.  (LANES = MTX_SLOTS_MAX; templates so that the
// module emits the two after every kernel it held before)
template <int LANES>
__global__ __launch_bounds__(256) void greedy_chunk_batch_kernel(mtx_greedy_batch_args p, int chunks) {
  const int slot = blockIdx.y;
  gp_chunk(p.logits + (long)slot * p.ld_logits, p.vocab, reinterpret_cast<float*>(p.scratch) + 2L * slot * chunks);
}

// grid (slots): one wave per slot
template <int LANES>
__global__ __launch_bounds__(64) void greedy_final_batch_kernel(mtx_greedy_batch_args p, int chunks) {
  const int slot = blockIdx.x;
  GP_FINAL_BODY(LANES, reinterpret_cast<const float*>(p.scratch) + 2L * slot * chunks, p.state + slot, p.out + (long)slot * p.max_new,
                st[MTX_SLOT_ROPE * LANES] += p.advance;)
}

int greedy_batch_launch(const mtx_greedy_batch_args* a, void* stream, const char** err) {
  if (!a->logits || !a->state || !a->out || !a->scratch) { *err = "greedy_pick_batch: null operand"; return MTX_ERR_INVALID; }
  if (a->slots < 1 || a->slots > MTX_SLOTS_MAX) { *err = "greedy_pick_batch: needs 1 <= slots <= MTX_SLOTS_MAX"; return MTX_ERR_INVALID; }
  if (a->vocab < 1 || a->max_new < 1 || a->n_eos < 0 || a->n_eos > 4 || a->ld_logits < a->vocab) {
    *err = "greedy_pick_batch: needs vocab >= 1, max_new >= 1, 0 <= n_eos <= 4, ld_logits >= vocab"; return MTX_ERR_INVALID;
  }
  const int chunks = (int)(((long)a->vocab + MTX_GREEDY_CHUNK - 1) / MTX_GREEDY_CHUNK);
  MTX_LAUNCH(greedy_chunk_batch_kernel<MTX_SLOTS_MAX>, dim3((unsigned)chunks, (unsigned)a->slots), dim3(256), 0, stream, *a, chunks);
  MTX_LAUNCH(greedy_final_batch_kernel<MTX_SLOTS_MAX>, dim3((unsigned)a->slots), dim3(64), 0, stream, *a, chunks);
  return MTX_OK;
}

// ---- the packed prompt pass (MTX_OP_CAUSAL_PREFILL_SLOTS) ------------------------------------------------------------------------------------
// causal_prefill_kernel for up to MTX_SLOTS_MAX prompts packed into one qkv buffer, prompt s = rows [seg[s], seg[s + 1]) of a DEVICE table,
// each into its own empty slot cache.  Grid (cap_rows / CA_TQ + MTX_SLOTS_MAX, heads): sum_s ceil(L_s / CA_TQ) never exceeds the first
// figure, so the launch does not depend on the lengths.  A workgroup walks the nine offsets, takes the slot its block index falls into and
// runs causal_prefill_body.inc on that slot's rows and cache at pos = 0.  A damaged table, a prompt longer than the cache or a surplus block
// leaves before any barrier.  (Templates behind every kernel the module held before.)
template <typename T>
__global__ __launch_bounds__(256) void causal_prefill_slots_kernel(mtx_causal_prefill_slots_args b) {
  long vb = blockIdx.x;
  // (workgroup-uniform) the table is checked whole before anything else is touched
  long prev = b.seg[0], row0 = 0, len = -1;
  int slot = 0;
  bool ok = prev >= 0;
#pragma unroll
  for (int i = 0; i < MTX_SLOTS_MAX; ++i) {
    const long next = b.seg[i + 1];
    ok = ok && next >= prev && next - prev <= (long)b.max_len;
    const long nb = (next - prev + CA_TQ - 1) / CA_TQ;
    if (ok && len < 0) {
      if (vb < nb) { row0 = prev; len = next - prev; slot = i; }
      else vb -= nb;
    }
    prev = next;
  }
  if (!ok || prev > (long)b.cap_rows || len < 0) return;
  mtx_causal_attn_args p;
  p.qkv = reinterpret_cast<const T*>(b.qkv) + row0 * b.ld_qkv;
  p.k_cache = reinterpret_cast<T*>(b.k_cache) + (long)slot * b.cache_stride;
  p.v_cache = reinterpret_cast<T*>(b.v_cache) + (long)slot * b.cache_stride;
  p.pos = nullptr;
  p.o = reinterpret_cast<T*>(b.o) + row0 * b.ld_o;
  p.rows = (int)len; p.heads = b.heads; p.kv_heads = b.kv_heads; p.d = b.d; p.max_len = b.max_len;
  p.ld_qkv = b.ld_qkv; p.ld_o = b.ld_o;
  p.scale = b.scale; p.dtype = b.dtype;
  p.workspace = nullptr; p.workspace_bytes = 0;
#define CA_PREFILL_POS 0
#define CA_PREFILL_QB (unsigned)vb
#include "causal_prefill_body.inc"
#undef CA_PREFILL_POS
#undef CA_PREFILL_QB
}

int causal_prefill_slots_launch(const mtx_causal_prefill_slots_args* a, void* stream, const char** err) {
  if (!a->qkv || !a->k_cache || !a->v_cache || !a->seg || !a->o) { *err = "causal_prefill_slots: null operand"; return MTX_ERR_INVALID; }
  if (a->d != CA_D) { *err = "causal_prefill_slots: only head width 128 is built"; return MTX_ERR_UNSUPPORTED; }
  if (a->heads < 1 || a->kv_heads < 1 || a->heads % a->kv_heads) { *err = "causal_prefill_slots: heads must be a multiple of kv_heads"; return MTX_ERR_UNSUPPORTED; }
  if (a->heads > 65535 || a->max_len < 1 || a->cap_rows < 1) { *err = "causal_prefill_slots: needs cap_rows >= 1, max_len >= 1, heads <= 65535"; return MTX_ERR_INVALID; }
  const long qkv_w = ((long)a->heads + 2L * a->kv_heads) * CA_D;
  if (a->ld_qkv % 8 || a->ld_o % 8 || a->ld_qkv < qkv_w || a->ld_o < (long)a->heads * CA_D) { *err = "causal_prefill_slots: row strides must be multiples of 8 and cover the row"; return MTX_ERR_INVALID; }
  if (a->cache_stride % 8 || a->cache_stride < (long)a->max_len * a->kv_heads * CA_D) { *err = "causal_prefill_slots: cache_stride must be a multiple of 8 and cover one cache"; return MTX_ERR_INVALID; }
  if ((((size_t)a->qkv | (size_t)a->k_cache | (size_t)a->v_cache | (size_t)a->o) & 15) != 0 || ((size_t)a->seg & 3) != 0) { *err = "causal_prefill_slots: operands must be 16-byte aligned"; return MTX_ERR_INVALID; }
  if (a->dtype != MTX_BF16 && a->dtype != MTX_F16) { *err = "causal_prefill_slots: dtype must be bf16 or f16"; return MTX_ERR_INVALID; }
  const dim3 grid((unsigned)(a->cap_rows / CA_TQ + MTX_SLOTS_MAX), (unsigned)a->heads);
  MTX_LAUNCH_T(a->dtype, causal_prefill_slots_kernel, grid, dim3(256), stream, *a);
  return MTX_OK;
}

}  // namespace mtx
