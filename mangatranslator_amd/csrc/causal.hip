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

// p in [0, 1] as two 16-bit halves: p ~ hi + lo * LoScale<T>::inv
template <typename T> struct LoScale;
template <> struct LoScale<__bf16> { static constexpr float mul = 1.f, inv = 1.f; };
template <> struct LoScale<_Float16> { static constexpr float mul = 4096.f, inv = 1.f / 4096.f; };
template <typename T> __device__ __forceinline__ void p_split(float p, T& hi, T& lo);
template <> __device__ __forceinline__ void p_split<__bf16>(float p, __bf16& hi, __bf16& lo) {
  hi = (__bf16)p;
  lo = (__bf16)(p - (float)hi);
}
template <> __device__ __forceinline__ void p_split<_Float16>(float p, _Float16& hi, _Float16& lo) {
  hi = p < 6.103515625e-5f ? (_Float16)0.f : (_Float16)p;          // below 2^-14 the high half would be subnormal: the scaled low half takes it all
  lo = (_Float16)((p - (float)hi) * 4096.f);
}

template <typename T>
__global__ __launch_bounds__(256) void causal_prefill_kernel(mtx_causal_attn_args p) {
  typedef typename Traits<T>::v8 v8;
  typedef typename Traits<T>::v4 v4;
  __shared__ u32x4 Vs4[CA_TK * CA_VROW / 8];
  T* Vs = reinterpret_cast<T*>(Vs4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, q4 = lane >> 4;
  const int pos = *p.pos;
  if (pos < 0 || pos > p.max_len - p.rows) return;                 // (workgroup-uniform) nothing is read or written outside the cache
  const int G = p.heads / p.kv_heads;
  const int h = blockIdx.y, kvh = h / G;
  const int q0 = blockIdx.x * CA_TQ;
  const long kvw = (long)p.kv_heads * CA_D;
  const T* QKV = reinterpret_cast<const T*>(p.qkv);
  const long koff = (long)p.heads * CA_D + (long)kvh * CA_D, voff = koff + kvw;
  T* KC = reinterpret_cast<T*>(p.k_cache) + (long)kvh * CA_D;
  T* VC = reinterpret_cast<T*>(p.v_cache) + (long)kvh * CA_D;

  // the rows' k and v go to cache[pos + i], once per kv head (nobody reads those positions in this launch)
  if (h % G == 0) {
    for (int it = tid; it < CA_TQ * 32; it += 256) {
      const int ch = it & 15, row = (it >> 4) & (CA_TQ - 1), which = it >> 10;
      const int qi = q0 + row;
      if (qi < p.rows) {
        const T* src = QKV + (long)qi * p.ld_qkv + (which ? voff : koff) + ch * 8;
        T* dst = (which ? VC : KC) + (long)(pos + qi) * kvw + ch * 8;
        *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
      }
    }
  }

  const int qw0 = q0 + wave * 16;                                   // the wave's first query row
  const bool wave_active = qw0 < p.rows;
  const int qi = qw0 + l15;
  const int qc = qi < p.rows ? qi : p.rows - 1;                     // rows past the end compute on the last row and are not stored
  const int kmax = pos + p.rows - 1;                                // the last key of the launch
  const int wave_last = pos + (qw0 + 15 < p.rows ? qw0 + 15 : p.rows - 1);      // the last key any row of this wave may see
  const int wg_last = pos + (q0 + CA_TQ - 1 < p.rows ? q0 + CA_TQ - 1 : p.rows - 1);
  const int ntiles = wg_last / CA_TK + 1;                           // key tiles wholly in the future are skipped

  v8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const v8*>(QKV + (long)qc * p.ld_qkv + (long)h * CA_D + ks * 32 + q4 * 8);

  f32x4 ohi[8], olo[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) { ohi[d] = f32x4{0.f, 0.f, 0.f, 0.f}; olo[d] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  float m = CA_NEG, l = 0.f;

  for (int t = 0; t < ntiles; ++t) {
    const int j0 = t * CA_TK;
    __syncthreads();                                                // the previous tile's V reads are done
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int idx = tid + it * 256, ch = idx & 15, row = idx >> 4;
      int j = j0 + row;
      j = j < kmax ? j : kmax;                                      // keys past the launch repeat the last one: their weight is 0
      const T* src = j < pos ? VC + (long)j * kvw : QKV + (long)(j - pos) * p.ld_qkv + voff;
      *reinterpret_cast<u32x4*>(Vs + row * CA_VROW + ch * 8) = *reinterpret_cast<const u32x4*>(src + ch * 8);
    }
    __syncthreads();
    if (!wave_active || j0 > wave_last) continue;                   // (wave-uniform) this wave's rows end before the tile

    // ---- S^T = K Q^T: sacc[s][r] is key j0 + 16 s + 4 q4 + r for query row l15
    f32x4 sacc[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      sacc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
      int j = j0 + s * 16 + l15;
      j = j < kmax ? j : kmax;
      const T* kp = (j < pos ? KC + (long)j * kvw : QKV + (long)(j - pos) * p.ld_qkv + koff) + q4 * 8;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) sacc[s] = Traits<T>::mfma(*reinterpret_cast<const v8*>(kp + ks * 32), qf[ks], sacc[s]);
    }

    // ---- online softmax; the mask is causal: key j counts for row i iff j <= pos + i
    float sc[8];
    float tmax = CA_NEG;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int key = j0 + (e >> 2) * 16 + q4 * 4 + (e & 3);
      const float s = key <= pos + qc ? sacc[e >> 2][e & 3] * p.scale : CA_NEG;
      sc[e] = s;
      tmax = s > tmax ? s : tmax;
    }
    { const float o1 = __shfl_xor(tmax, 16, 64); tmax = o1 > tmax ? o1 : tmax; }
    { const float o2 = __shfl_xor(tmax, 32, 64); tmax = o2 > tmax ? o2 : tmax; }
    const float mnew = tmax > m ? tmax : m;
    const float alpha = __expf(m - mnew);
    m = mnew;
    v8 phi, plo;
    float psum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int key = j0 + (e >> 2) * 16 + q4 * 4 + (e & 3);
      const float pv = key <= pos + qc ? __expf(sc[e] - mnew) : 0.f;      // (a masked key weighs 0 even while the row has seen no key at all)
      psum += pv;
      T hi, lo;
      p_split<T>(pv, hi, lo);
      phi[e] = hi; plo[e] = lo;                                     // k-slot 8 q4 + e  <->  key j0 + (e < 4 ? 4 q4 + e : 16 + 4 q4 + e - 4)
    }
    l = l * alpha + psum;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
#pragma unroll
      for (int r = 0; r < 4; ++r) { ohi[d][r] *= alpha; olo[d][r] *= alpha; }
    }

    // ---- O^T += V^T P^T: lane (l15, q4) receives V[4 q4 + 0..3][16 d + l15] and V[16 + 4 q4 + 0..3][16 d + l15]
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      const T* a = Vs + (q4 * 4 + (l15 >> 2)) * CA_VROW + d * 16 + (l15 & 3) * 4;
      const v4 v0 = lds_read_tr16<T>(a);
      const v4 v1 = lds_read_tr16<T>(a + 16 * CA_VROW);
      v8 vf;
      vf[0] = v0[0]; vf[1] = v0[1]; vf[2] = v0[2]; vf[3] = v0[3];
      vf[4] = v1[0]; vf[5] = v1[1]; vf[6] = v1[2]; vf[7] = v1[3];
      ohi[d] = Traits<T>::mfma(vf, phi, ohi[d]);
      olo[d] = Traits<T>::mfma(vf, plo, olo[d]);
    }
  }

  // ---- row sums across the 4 quads, normalise, store 4 consecutive d per lane
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (qi < p.rows) {
    T* O = reinterpret_cast<T*>(p.o) + (long)qi * p.ld_o + (long)h * CA_D + q4 * 4;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      v4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = from_f32<T>((ohi[d][r] + olo[d][r] * LoScale<T>::inv) / l);      // l >= 1: the key at the running maximum weighs exp(0)
      *reinterpret_cast<v4*>(O + d * 16) = o;
    }
  }
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
  __shared__ float part[4][G][CA_REC];
  __shared__ int last_flag;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = tid & 15;                  // which 8 of the head's 128 elements
  const int grp = tid >> 4;                  // 0..15: the keys j = j0 + grp
  const int pos = *p.pos;
  if (pos < 0 || pos >= p.max_len) return;   // (workgroup-uniform)
  const int split = blockIdx.x, n_active = pos / CA_S + 1;
  if (split >= n_active) return;             // splits wholly in the future draw no ticket
  const int kvh = blockIdx.y;
  const int h0 = kvh * gfull + (int)blockIdx.z * G;
  const int nsplit = (int)gridDim.x;
  const long kvw = (long)p.kv_heads * CA_D;
  const T* row = reinterpret_cast<const T*>(p.qkv);
  T* KC = reinterpret_cast<T*>(p.k_cache) + (long)kvh * CA_D + sub * 8;
  T* VC = reinterpret_cast<T*>(p.v_cache) + (long)kvh * CA_D + sub * 8;
  float q[G][8], k_own[8], v_own[8];
#pragma unroll
  for (int g = 0; g < G; ++g) ca_load8(row + (long)(h0 + g) * CA_D + sub * 8, q[g]);
  ca_load8(row + (long)p.heads * CA_D + (long)kvh * CA_D + sub * 8, k_own);
  ca_load8(row + (long)p.heads * CA_D + kvw + (long)kvh * CA_D + sub * 8, v_own);
  if (split == n_active - 1 && blockIdx.z == 0 && grp == 0) {      // the row's k and v go to cache[pos] (nobody reads that position in this launch)
    *reinterpret_cast<u32x4*>(KC + (long)pos * kvw) = pack8<T>(k_own);            // (values of the storage type: the round trip through float is exact)
    *reinterpret_cast<u32x4*>(VC + (long)pos * kvw) = pack8<T>(v_own);
  }
  float m[G], l[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = CA_NEG; l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
  }
  const int jbeg = split * CA_S;
  const int jend = jbeg + CA_S < pos + 1 ? jbeg + CA_S : pos + 1;
  for (int j0 = jbeg; j0 < jend; j0 += 16) {                        // workgroup-uniform trip count: every lane reaches the shuffles
    const int j = j0 + grp;
    float kf[8], vf[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { kf[e] = k_own[e]; vf[e] = v_own[e]; }
    if (j < pos) {
      ca_load8(KC + (long)j * kvw, kf);
      ca_load8(VC + (long)j * kvw, vf);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) s += q[g][e] * kf[e];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      s += __shfl_xor(s, 8, 64);
      if (j < jend) {
        s *= p.scale;
        const float mn = s > m[g] ? s : m[g];
        const float f = __expf(m[g] - mn), w = __expf(s - mn);
        l[g] = l[g] * f + w;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][e] = acc[g][e] * f + w * vf[e];
        m[g] = mn;
      }
    }
  }
  // the 4 lane groups of a wave, then the 4 waves
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float m2 = __shfl_xor(m[g], off, 64), l2 = __shfl_xor(l[g], off, 64);
      float a2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) a2[e] = __shfl_xor(acc[g][e], off, 64);
      ca_merge(m[g], l[g], acc[g], m2, l2, a2);
    }
    if (lane < 16) {
      if (sub == 0) { part[wave][g][0] = m[g]; part[wave][g][1] = l[g]; }
#pragma unroll
      for (int e = 0; e < 8; ++e) part[wave][g][4 + sub * 8 + e] = acc[g][e];
    }
  }
  __syncthreads();
  unsigned* counter = reinterpret_cast<unsigned*>(p.workspace) + (kvh * (int)gridDim.z + (int)blockIdx.z);
  float* recs = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(p.workspace) + (((long)p.heads * 4 + 255) / 256) * 256);
  const int g = tid >> 4;                    // threads 0 .. 16 G - 1 finish: 16 lanes per query head
  float fm = CA_NEG, fl = 0.f, facc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) facc[e] = 0.f;
  if (g < G) {
    fm = part[0][g][0]; fl = part[0][g][1];
#pragma unroll
    for (int e = 0; e < 8; ++e) facc[e] = part[0][g][4 + sub * 8 + e];
    for (int w = 1; w < 4; ++w) {
      float a2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) a2[e] = part[w][g][4 + sub * 8 + e];
      ca_merge(fm, fl, facc, part[w][g][0], part[w][g][1], a2);
    }
    float* rec = recs + ((long)(h0 + g) * nsplit + split) * CA_REC;
    if (sub == 0) { agent_store(rec, fm); agent_store(rec + 1, fl); }
#pragma unroll
    for (int e = 0; e < 8; ++e) agent_store(rec + 4 + sub * 8 + e, facc[e]);
  }
  MTX_WAIT_VMEM();                                       // every storing wave drains its write-through stores
  __syncthreads();
  if (tid == 0) last_flag = agent_ticket(counter) + 1 == (unsigned)n_active;
  __syncthreads();
  if (!last_flag) return;                                // (workgroup-uniform)
  // ---- the last arriver: the records of this head chunk, merged in key order whoever came last
  if (tid == 0) { agent_acquire(); agent_store(counter, 0u); }      // zero again for the next launch (a launch boundary away)
  __syncthreads();
  if (g < G) {
    const float* r0 = recs + (long)(h0 + g) * nsplit * CA_REC;
    fm = r0[0]; fl = r0[1];
#pragma unroll
    for (int e = 0; e < 8; ++e) facc[e] = r0[4 + sub * 8 + e];
    for (int s = 1; s < n_active; ++s) {
      const float* r = r0 + (long)s * CA_REC;
      float a2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) a2[e] = r[4 + sub * 8 + e];
      ca_merge(fm, fl, facc, r[0], r[1], a2);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) facc[e] = facc[e] / fl;           // fl >= 1: the key at the running maximum weighs exp(0)
    *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(p.o) + (long)(h0 + g) * CA_D + sub * 8) = pack8<T>(facc);
  }
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

__global__ __launch_bounds__(256) void greedy_chunk_kernel(mtx_greedy_args p) {
  __shared__ float wv[4];
  __shared__ int wi[4];
  const int tid = threadIdx.x;
  const long base = (long)blockIdx.x * MTX_GREEDY_CHUNK;
  float bv = -INFINITY;
  int bi = INT_MAX;
#pragma unroll 4
  for (int k = 0; k < MTX_GREEDY_CHUNK / 256; ++k) {
    const long i = base + tid + 256 * k;
    if (i < p.vocab) gp_take(bv, bi, p.logits[i], (int)i);
  }
  gp_wave(bv, bi);
  if ((tid & 63) == 0) { wv[tid >> 6] = bv; wi[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) gp_take(bv, bi, wv[w], wi[w]);
    float* rec = reinterpret_cast<float*>(p.scratch) + 2 * blockIdx.x;
    rec[0] = bv;
    reinterpret_cast<int*>(rec)[1] = bi;
  }
}

__global__ __launch_bounds__(64) void greedy_final_kernel(mtx_greedy_args p, int chunks) {
  const int lane = threadIdx.x;
  float bv = -INFINITY;
  int bi = INT_MAX;
  for (int c = lane; c < chunks; c += 64) {
    const float* rec = reinterpret_cast<const float*>(p.scratch) + 2 * c;
    gp_take(bv, bi, rec[0], reinterpret_cast<const int*>(rec)[1]);
  }
  gp_wave(bv, bi);
  if (lane != 0) return;
  int* st = p.state;                         // {pos, n_out, done, token}
  if (st[2]) return;                         // a finished sequence changes nothing
  int n_out = st[1];
  if (n_out < 0 || n_out >= p.max_new) { st[2] = 1; return; }      // (a damaged state must not leave `out`)
  const int t = bi == INT_MAX ? 0 : bi;      // all NaN
  p.out[n_out++] = t;
  int done = n_out == p.max_new;
  for (int e = 0; e < p.n_eos; ++e) done |= t == p.eos[e];
  st[0] += p.advance;
  st[1] = n_out;
  st[2] = done;
  st[3] = t;
}

int greedy_launch(const mtx_greedy_args* a, void* stream, const char** err) {
  if (!a->logits || !a->state || !a->out || !a->scratch) { *err = "greedy_pick: null operand"; return MTX_ERR_INVALID; }
  if (a->vocab < 1 || a->max_new < 1 || a->n_eos < 0 || a->n_eos > 4) { *err = "greedy_pick: needs vocab >= 1, max_new >= 1, 0 <= n_eos <= 4"; return MTX_ERR_INVALID; }
  const int chunks = (int)(((long)a->vocab + MTX_GREEDY_CHUNK - 1) / MTX_GREEDY_CHUNK);
  MTX_LAUNCH(greedy_chunk_kernel, dim3((unsigned)chunks), dim3(256), 0, stream, *a);
  MTX_LAUNCH(greedy_final_kernel, dim3(1), dim3(64), 0, stream, *a, chunks);
  return MTX_OK;
}

}  // namespace mtx
