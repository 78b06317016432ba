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
  __shared__ float part[4][2 + DEC_D];
  const int h = blockIdx.x, r = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = tid & 7;                 // which 8 of the head's 64 elements
  const int grp = tid >> 3;                // 0..31: the keys j = grp, grp + 32, ...
  const int pos = *p.pos;
  if (pos < 0 || pos >= p.max_len) return;            // nothing is read or written for a position outside the cache
  const long hd = (long)p.heads * DEC_D;
  const T* row = reinterpret_cast<const T*>(p.qkv) + (long)r * p.ld_qkv + (long)h * DEC_D + sub * 8;
  T* KC = reinterpret_cast<T*>(p.k_cache);
  T* VC = reinterpret_cast<T*>(p.v_cache);
  float q[8], k_own[8], v_own[8];
  load8<T>(row, q);
  load8<T>(row + hd, k_own);
  load8<T>(row + 2 * hd, v_own);
  if (grp == 0) {                           // this row's k and v go to its own slot at `pos` (nobody reads that position in this launch)
    const long at = ((long)pos * p.slots + r) * hd + (long)h * DEC_D + sub * 8;
    store8<T>(KC + at, k_own);              // (values of the storage type: the round trip through float is exact)
    store8<T>(VC + at, v_own);
  }
  float m = DEC_NEG, l = 0.f, acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int j0 = 0; j0 <= pos; j0 += 32) {             // wave-uniform trip count: every lane reaches the shuffles
    const int j = j0 + grp;
    float kf[8], vf[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { kf[e] = k_own[e]; vf[e] = v_own[e]; }
    if (j < pos) {
      int slot = p.src[(long)j * p.slots + r];
      slot = slot < 0 ? 0 : (slot >= p.slots ? p.slots - 1 : slot);          // a damaged table must not leave the cache
      const long at = ((long)j * p.slots + slot) * hd + (long)h * DEC_D + sub * 8;
      load8<T>(KC + at, kf);
      load8<T>(VC + at, vf);
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += q[e] * kf[e];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (j <= pos) {
      s *= p.scale;
      const float mn = s > m ? s : m;
      const float f = __expf(m - mn), w = __expf(s - mn);
      l = l * f + w;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = acc[e] * f + w * vf[e];
      m = mn;
    }
  }
  // the 8 lane groups of a wave, then the 4 waves
#pragma unroll
  for (int off = 8; off <= 32; off <<= 1) {
    const float m2 = __shfl_xor(m, off, 64), l2 = __shfl_xor(l, off, 64);
    float a2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a2[e] = __shfl_xor(acc[e], off, 64);
    dec_merge(m, l, acc, m2, l2, a2);
  }
  if (lane < 8) {
    if (sub == 0) { part[wave][0] = m; part[wave][1] = l; }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[wave][2 + sub * 8 + e] = acc[e];
  }
  __syncthreads();
  if (tid < 8) {
    m = part[0][0]; l = part[0][1];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = part[0][2 + sub * 8 + e];
    for (int w = 1; w < 4; ++w) {
      float a2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) a2[e] = part[w][2 + sub * 8 + e];
      dec_merge(m, l, acc, part[w][0], part[w][1], a2);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = acc[e] / l;          // l >= 1: the key at the running maximum weighs exp(0)
    store8<T>(reinterpret_cast<T*>(p.o) + (long)r * p.ld_o + (long)h * DEC_D + sub * 8, acc);
  }
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

}  // namespace mtx
