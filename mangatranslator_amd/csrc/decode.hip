// decode.hip — the two kernels of an autoregressive decode step (manga-ocr's BERT decoder behind reference core/ml/model_manager.py:835-904;
// include/mtx_hip.h, mtx_decode_attn_args / mtx_rowlin_args).
//
//   decode attention   one query per (row, head) over a key / value cache whose LENGTH LIVES IN DEVICE MEMORY, so that one captured step graph serves
//                      every token.  A beam reorder never moves cache data: the history of row r at position j is the slot src[j][r].
//                      One workgroup per (head, row); 8 lanes share a key (8 x 16 bytes = the 64-wide head), so the 32 lane groups of the workgroup walk
//                      the keys 32 at a time with an online softmax each, merged by shuffles inside a wave and through LDS across the four waves.
//   skinny-row linear  c[r, n] = act(alpha * sum_k a[r, k] w[n, k] + bias[n]) (+ res[r, n]) for at most 8 rows: weight streaming.  A wave owns NW
//                      output columns and reduces K inside itself (16-byte chunks, lane-strided), so N spreads over the whole chip where the 128-tile
//                      GEMM would put a 768-column linear on 6 workgroups.  Rounding contract of mtx_gemm.
#include "mtx_device.h"

namespace mtx {

constexpr int DEC_D = 64;                 // the only head width built
constexpr int DEC_MAX_ROWS = 8;
constexpr float DEC_NEG = -1.0e30f;       // running maximum of a lane group that has seen no key (finite: exp(DEC_NEG - m) is 0, never NaN)

// 8 consecutive elements of the storage type (16-bit: one 16-byte chunk; fp32 — the model's precision "high" — two) as floats, and back
template <typename T> __device__ __forceinline__ void load8(const T* p, float (&f)[8]) { unpack8<T>(*reinterpret_cast<const u32x4*>(p), f); }
template <> __device__ __forceinline__ void load8<float>(const float* p, float (&f)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) { f[e] = a[e]; f[4 + e] = b[e]; }
}
template <typename T> __device__ __forceinline__ void store8(T* p, const float (&f)[8]) { *reinterpret_cast<u32x4*>(p) = pack8<T>(f); }
template <> __device__ __forceinline__ void store8<float>(float* p, const float (&f)[8]) {
  *reinterpret_cast<f32x4*>(p) = f32x4{f[0], f[1], f[2], f[3]};
  *reinterpret_cast<f32x4*>(p + 4) = f32x4{f[4], f[5], f[6], f[7]};
}
// storage-type dispatch of this file: bf16, f16 and fp32
template <typename F>
static inline bool with_decode_type(int dtype, F&& f) {
  if (dtype == MTX_F32) { f(TypeTag<float>{}); return true; }
  return with_storage_type(dtype, f);
}

// merge the online-softmax state (m, l, acc) with another one
__device__ __forceinline__ void dec_merge(float& m, float& l, float (&acc)[8], float m2, float l2, const float (&acc2)[8]) {
  const float mn = m > m2 ? m : m2;
  const float f1 = __expf(m - mn), f2 = __expf(m2 - mn);
  l = l * f1 + l2 * f2;
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = acc[e] * f1 + acc2[e] * f2;
  m = mn;
}

template <typename T>
__global__ __launch_bounds__(256) void decode_attn_kernel(mtx_decode_attn_args p) {
#include "decode_attn_body.inc"
}

int decode_attn_launch(const mtx_decode_attn_args* a, void* stream, const char** err) {
  if (!a->qkv || !a->k_cache || !a->v_cache || !a->pos || !a->src || !a->o) { *err = "decode_attn: null operand"; return MTX_ERR_INVALID; }
  if (a->d != DEC_D) { *err = "decode_attn: only head width 64 is built"; return MTX_ERR_UNSUPPORTED; }
  if (a->rows < 1 || a->rows > a->slots || a->slots > DEC_MAX_ROWS) { *err = "decode_attn: needs 1 <= rows <= slots <= 8"; return MTX_ERR_INVALID; }
  if (a->heads < 1 || a->heads > 65535 || a->max_len < 1) { *err = "decode_attn: bad heads / max_len"; return MTX_ERR_INVALID; }
  if (a->ld_qkv % 8 || a->ld_o % 8 || a->ld_qkv < 3L * a->heads * DEC_D || a->ld_o < (long)a->heads * DEC_D) { *err = "decode_attn: row strides must be multiples of 8 and cover the row"; return MTX_ERR_INVALID; }
  if ((((size_t)a->qkv | (size_t)a->k_cache | (size_t)a->v_cache | (size_t)a->o) & 15) != 0) { *err = "decode_attn: operands must be 16-byte aligned"; return MTX_ERR_INVALID; }
  const dim3 grid((unsigned)a->heads, (unsigned)a->rows);
  if (!with_decode_type(a->dtype, [&](auto t) { MTX_LAUNCH((decode_attn_kernel<typename decltype(t)::type>), grid, dim3(256), 0, stream, *a); })) {
    *err = "decode_attn: dtype must be bf16, f16 or f32"; return MTX_ERR_INVALID;
  }
  return MTX_OK;
}

// ---- skinny-row linear ---------------------------------------------------------------------------------------------------------------------
// RT rows (rows >= p.rows read as zero and are not stored), NW columns per wave, 4 waves per workgroup.
template <typename T, int RT, int NW>
__global__ __launch_bounds__(256) void rowlin_kernel(mtx_rowlin_args p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long n0 = ((long)blockIdx.x * 4 + wave) * NW;
  if (n0 >= p.n) return;                                 // wave-uniform
  const T* A = reinterpret_cast<const T*>(p.a);
  const T* W = reinterpret_cast<const T*>(p.w);
  const long nch = p.k / 8;
  float acc[RT][NW];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int c = 0; c < NW; ++c) acc[r][c] = 0.f;
  for (long ch = lane; ch < nch; ch += 64) {
    float wf[NW][8];
#pragma unroll
    for (int c = 0; c < NW; ++c) {
      const long n = n0 + c < p.n ? n0 + c : p.n - 1;      // a wave's columns past N repeat the last one and are not stored
      load8<T>(W + n * p.ldw + ch * 8, wf[c]);
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      if (r < p.rows) {
        float af[8];
        load8<T>(A + (long)r * p.lda + ch * 8, af);
#pragma unroll
        for (int c = 0; c < NW; ++c)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[r][c] += af[e] * wf[c][e];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int c = 0; c < NW; ++c) acc[r][c] = wave_sum(acc[r][c]);
  // lane r * NW + c finishes output (r, n0 + c)
  float v = 0.f;
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int c = 0; c < NW; ++c) v = lane == r * NW + c ? acc[r][c] : v;
  const int r = lane / NW;
  const long n = n0 + lane % NW;
  if (lane >= RT * NW || r >= p.rows || n >= p.n) return;
  v = apply_act(v * p.alpha + (p.bias ? p.bias[n] : 0.f), p.act, p.act_param);
  if (p.out_dtype == MTX_F32) {
    if (p.res) v += to_f32(reinterpret_cast<const T*>(p.res)[(long)r * p.ldres + n]);
    reinterpret_cast<float*>(p.c)[(long)r * p.ldc + n] = v;
    return;
  }
  T t = from_f32<T>(v);                                   // round_T(act(alpha * acc + bias))
  if (p.res) t = from_f32<T>(to_f32(t) + to_f32(reinterpret_cast<const T*>(p.res)[(long)r * p.ldres + n]));      // the second rounding
  reinterpret_cast<T*>(p.c)[(long)r * p.ldc + n] = t;
}

int rowlin_launch(const mtx_rowlin_args* a0, void* stream, const char** err) {
  if (!a0->a || !a0->w || !a0->c) { *err = "rowlin: null operand"; return MTX_ERR_INVALID; }
  if (a0->rows < 1 || a0->rows > DEC_MAX_ROWS) { *err = "rowlin: needs 1 <= rows <= 8"; return MTX_ERR_INVALID; }
  if (a0->n < 1 || a0->k < 8 || a0->k % 8 || a0->lda % 8 || a0->ldw % 8 || a0->lda < a0->k || a0->ldw < a0->k) { *err = "rowlin: K, lda and ldw must be multiples of 8 that cover K"; return MTX_ERR_INVALID; }
  if ((((size_t)a0->a | (size_t)a0->w) & 15) != 0) { *err = "rowlin: a and w must be 16-byte aligned"; return MTX_ERR_INVALID; }
  if (a0->ldc < a0->n || (a0->res && a0->ldres < a0->n)) { *err = "rowlin: ldc / ldres must cover N"; return MTX_ERR_INVALID; }
  if (a0->out_dtype != MTX_F32 && a0->out_dtype != a0->dtype) { *err = "rowlin: out_dtype must be the storage type or fp32"; return MTX_ERR_INVALID; }
  mtx_rowlin_args a = *a0;
  if (a.alpha == 0.f) a.alpha = 1.f;                      // as mtx_gemm: an unset alpha means 1
  const int nw = a.n >= 4096 ? 4 : (a.n >= 2048 ? 2 : 1);
  const unsigned blocks = (unsigned)((a.n + 4L * nw - 1) / (4L * nw));
  const int rt = a.rows == 1 ? 1 : (a.rows <= 4 ? 4 : 8);
  if (!with_decode_type(a.dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
#define MTX_ROWLIN(RT, NW) MTX_LAUNCH((rowlin_kernel<T, RT, NW>), dim3(blocks), dim3(256), 0, stream, a)
#define MTX_ROWLIN_R(RT) do { if (nw == 4) MTX_ROWLIN(RT, 4); else if (nw == 2) MTX_ROWLIN(RT, 2); else MTX_ROWLIN(RT, 1); } while (0)
        if (rt == 1) MTX_ROWLIN_R(1);
        else if (rt == 4) MTX_ROWLIN_R(4);
        else MTX_ROWLIN_R(8);
#undef MTX_ROWLIN_R
#undef MTX_ROWLIN
      })) { *err = "rowlin: dtype must be bf16, f16 or f32"; return MTX_ERR_INVALID; }
  return MTX_OK;
}

// ---- the same two for S groups of B beams (MTX_OP_DECODE_ATTN_BATCH, MTX_OP_ROWLIN_WIDE) ------------------------------------------------------
// grid (heads, beams, groups): group blockIdx.z owns its caches, its ancestry table and its rows of qkv and o, so the groups never meet
template <typename T>
__global__ __launch_bounds__(256) void decode_attn_batch_kernel(mtx_decode_attn_batch_args b) {
  const int g = blockIdx.z;
  const int32_t* st = b.state + (long)g * b.state_stride;
  if (st[MTX_BEAM_DONE] != 0) return;                    // (workgroup-uniform, before the barrier) a finished or empty group sits out
  mtx_decode_attn_args p;
  p.qkv = reinterpret_cast<const T*>(b.qkv) + (long)g * b.beams * b.ld_qkv;
  p.k_cache = reinterpret_cast<T*>(b.k_cache) + (long)g * b.cache_stride;
  p.v_cache = reinterpret_cast<T*>(b.v_cache) + (long)g * b.cache_stride;
  p.pos = st + MTX_BEAM_POS;                             // the body reads it and leaves (as uniformly) unless 0 <= pos < max_len
  p.src = b.src + (long)g * b.src_stride;
  p.o = reinterpret_cast<T*>(b.o) + (long)g * b.beams * b.ld_o;
  p.rows = b.beams; p.slots = b.beams; p.heads = b.heads; p.d = b.d; p.max_len = b.max_len;
  p.ld_qkv = b.ld_qkv; p.ld_o = b.ld_o;
  p.scale = b.scale; p.dtype = b.dtype;
#include "decode_attn_body.inc"
}

int decode_attn_batch_launch(const mtx_decode_attn_batch_args* a, void* stream, const char** err) {
  if (!a->qkv || !a->k_cache || !a->v_cache || !a->state || !a->src || !a->o) { *err = "decode_attn_batch: null operand"; return MTX_ERR_INVALID; }
  if (a->d != DEC_D) { *err = "decode_attn_batch: only head width 64 is built"; return MTX_ERR_UNSUPPORTED; }
  if (a->groups < 1 || a->groups > MTX_SLOTS_MAX || a->beams < 1 || a->beams > MTX_BEAM_MAX) { *err = "decode_attn_batch: needs 1 <= groups <= MTX_SLOTS_MAX, 1 <= beams <= 8"; return MTX_ERR_INVALID; }
  if (a->heads < 1 || a->heads > 65535 || a->max_len < 1) { *err = "decode_attn_batch: bad heads / max_len"; return MTX_ERR_INVALID; }
  if (a->ld_qkv % 8 || a->ld_o % 8 || a->ld_qkv < 3L * a->heads * DEC_D || a->ld_o < (long)a->heads * DEC_D) { *err = "decode_attn_batch: row strides must be multiples of 8 and cover the row"; return MTX_ERR_INVALID; }
  if (a->cache_stride % 8 || a->cache_stride < (long)a->max_len * a->beams * a->heads * DEC_D) { *err = "decode_attn_batch: cache_stride must be a multiple of 8 and cover one cache"; return MTX_ERR_INVALID; }
  if (a->src_stride < (long)a->max_len * a->beams || a->state_stride < 2) { *err = "decode_attn_batch: src_stride / state_stride too short"; return MTX_ERR_INVALID; }
  if ((((size_t)a->qkv | (size_t)a->k_cache | (size_t)a->v_cache | (size_t)a->o) & 15) != 0) { *err = "decode_attn_batch: operands must be 16-byte aligned"; return MTX_ERR_INVALID; }
  const dim3 grid((unsigned)a->heads, (unsigned)a->beams, (unsigned)a->groups);
  if (!with_decode_type(a->dtype, [&](auto t) { MTX_LAUNCH((decode_attn_batch_kernel<typename decltype(t)::type>), grid, dim3(256), 0, stream, *a); })) {
    *err = "decode_attn_batch: dtype must be bf16, f16 or f32"; return MTX_ERR_INVALID;
  }
  return MTX_OK;
}

// The skinny-row linear for up to 32 rows: a wave owns NW columns for ALL RT rows, so the weights are read once whatever `rows` is.  Every
// output runs rowlin_kernel's arithmetic — the same chunks in the same order, the same eight multiply-adds, the same wave sum — which does
// not depend on RT or NW: row r is bit for bit the single op's.  RT * NW may exceed the 64 lanes of the finishing step: it is looped.
// One multiply-add of the wide kernel.  With 16-bit storage the product of two operands is exact in fp32, so a fused and an unfused
// multiply-add give the same bits and the plain expression serves.  With fp32 storage they do not, and the compiler's choice in
// rowlin_kernel<float, 1, NW> — the kernel a single row runs on, whose code is pinned — is: the product rounded before the sum everywhere,
// except in columns 0 and 1 of a wave's four at NW == 4, which are fused.  The wide kernel spells that choice out so that an fp32 row is the
// single op's bit for bit (the GPU tier holds it to that for all three column tilings); the simulator never fuses.
template <typename T, int NW>
__device__ __forceinline__ float rowlin_wide_mac(float acc, float a, float w, int c) { return acc + a * w; }
#ifndef MTX_EMU
__device__ __forceinline__ float rowlin_unfused(float acc, float a, float w) {
#pragma clang fp contract(off)
  const float prod = a * w;
  return acc + prod;
}
template <> __device__ __forceinline__ float rowlin_wide_mac<float, 1>(float acc, float a, float w, int) { return rowlin_unfused(acc, a, w); }
template <> __device__ __forceinline__ float rowlin_wide_mac<float, 2>(float acc, float a, float w, int) { return rowlin_unfused(acc, a, w); }
template <> __device__ __forceinline__ float rowlin_wide_mac<float, 4>(float acc, float a, float w, int c) {
  return c < 2 ? __builtin_fmaf(a, w, acc) : rowlin_unfused(acc, a, w);
}
#endif

template <typename T, int RT, int NW>
__global__ __launch_bounds__(256) void rowlin_wide_kernel(mtx_rowlin_args p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long n0 = ((long)blockIdx.x * 4 + wave) * NW;
  if (n0 >= p.n) return;                                 // wave-uniform
  const T* A = reinterpret_cast<const T*>(p.a);
  const T* W = reinterpret_cast<const T*>(p.w);
  const long nch = p.k / 8;
  float acc[RT][NW];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int c = 0; c < NW; ++c) acc[r][c] = 0.f;
  for (long ch = lane; ch < nch; ch += 64) {
    float wf[NW][8];
#pragma unroll
    for (int c = 0; c < NW; ++c) {
      const long n = n0 + c < p.n ? n0 + c : p.n - 1;      // a wave's columns past N repeat the last one and are not stored
      load8<T>(W + n * p.ldw + ch * 8, wf[c]);
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      if (r < p.rows) {
        float af[8];
        load8<T>(A + (long)r * p.lda + ch * 8, af);
#pragma unroll
        for (int c = 0; c < NW; ++c)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[r][c] = rowlin_wide_mac<T, NW>(acc[r][c], af[e], wf[c][e], c);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int c = 0; c < NW; ++c) acc[r][c] = wave_sum(acc[r][c]);
  // pass q: lane finishes output (r, n0 + c) with r * NW + c == q * 64 + lane
#pragma unroll
  for (int q = 0; q < (RT * NW + 63) / 64; ++q) {
    float v = 0.f;
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
      for (int c = 0; c < NW; ++c)
        if ((r * NW + c) / 64 == q) v = lane == (r * NW + c) % 64 ? acc[r][c] : v;
    const int idx = q * 64 + lane;
    const int r = idx / NW;
    const long n = n0 + idx % NW;
    if (idx >= RT * NW || r >= p.rows || n >= p.n) continue;
    v = apply_act(v * p.alpha + (p.bias ? p.bias[n] : 0.f), p.act, p.act_param);
    if (p.out_dtype == MTX_F32) {
      if (p.res) v += to_f32(reinterpret_cast<const T*>(p.res)[(long)r * p.ldres + n]);
      reinterpret_cast<float*>(p.c)[(long)r * p.ldc + n] = v;
      continue;
    }
    T t = from_f32<T>(v);                                   // round_T(act(alpha * acc + bias))
    if (p.res) t = from_f32<T>(to_f32(t) + to_f32(reinterpret_cast<const T*>(p.res)[(long)r * p.ldres + n]));      // the second rounding
    reinterpret_cast<T*>(p.c)[(long)r * p.ldc + n] = t;
  }
}

int rowlin_wide_launch(const mtx_rowlin_args* a0, void* stream, const char** err) {
  if (!a0->a || !a0->w || !a0->c) { *err = "rowlin_wide: null operand"; return MTX_ERR_INVALID; }
  if (a0->rows < 1 || a0->rows > MTX_WIDE_ROWS_MAX) { *err = "rowlin_wide: needs 1 <= rows <= 32"; return MTX_ERR_INVALID; }
  if (a0->n < 1 || a0->k < 8 || a0->k % 8 || a0->lda % 8 || a0->ldw % 8 || a0->lda < a0->k || a0->ldw < a0->k) { *err = "rowlin_wide: K, lda and ldw must be multiples of 8 that cover K"; return MTX_ERR_INVALID; }
  if ((((size_t)a0->a | (size_t)a0->w) & 15) != 0) { *err = "rowlin_wide: a and w must be 16-byte aligned"; return MTX_ERR_INVALID; }
  if (a0->ldc < a0->n || (a0->res && a0->ldres < a0->n)) { *err = "rowlin_wide: ldc / ldres must cover N"; return MTX_ERR_INVALID; }
  if (a0->out_dtype != MTX_F32 && a0->out_dtype != a0->dtype) { *err = "rowlin_wide: out_dtype must be the storage type or fp32"; return MTX_ERR_INVALID; }
  mtx_rowlin_args a = *a0;
  if (a.alpha == 0.f) a.alpha = 1.f;                      // as mtx_gemm: an unset alpha means 1
  const int nw = a.n >= 4096 ? 4 : (a.n >= 2048 ? 2 : 1); // the single op's column tiling
  const unsigned blocks = (unsigned)((a.n + 4L * nw - 1) / (4L * nw));
  const int rt = a.rows <= 8 ? 8 : (a.rows <= 16 ? 16 : 32);
  if (!with_decode_type(a.dtype, [&](auto t) {
        typedef typename decltype(t)::type T;
#define MTX_ROWLIN(RT, NW) MTX_LAUNCH((rowlin_wide_kernel<T, RT, NW>), dim3(blocks), dim3(256), 0, stream, a)
#define MTX_ROWLIN_R(RT) do { if (nw == 4) MTX_ROWLIN(RT, 4); else if (nw == 2) MTX_ROWLIN(RT, 2); else MTX_ROWLIN(RT, 1); } while (0)
        if (rt == 8) MTX_ROWLIN_R(8);
        else if (rt == 16) MTX_ROWLIN_R(16);
        else MTX_ROWLIN_R(32);
#undef MTX_ROWLIN_R
#undef MTX_ROWLIN
      })) { *err = "rowlin_wide: dtype must be bf16, f16 or f32"; return MTX_ERR_INVALID; }
  return MTX_OK;
}

}  // namespace mtx
