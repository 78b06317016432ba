// relattn.hip — attention with an additive Toeplitz bias and a device-side key count (MTX_OP_REL_ATTN; include/mtx_hip.h, mtx_rel_attn_args):
// the one attention of FLUX's prompt encoders.  Qwen3 and CLIP pass the causal table (0 on and below the diagonal, masked above), T5 its
// bucketed relative-position bias; Qwen3 also limits the keys to the prompt's real tokens.
//
//   shape   causal.hip's prefill kernel without the cache: 4 waves x 16 query rows of ONE head per workgroup, 32-key tiles,
//           v_mfma_f32_16x16x32, both products transposed (S^T = K Q^T, O^T = V^T P^T) so that a lane's S^T values are already the B operand
//           of the second product.  K fragments come straight from memory (16 bytes per lane), V goes through LDS row-major and is read with
//           the hardware transpose, the softmax weights reach the matrix pipe as a high and a low 16-bit half (mtx_device.h, p_split).
//           D = 64 / 128 is the template parameter: 2 / 4 k-steps for the scores, 4 / 8 accumulator blocks for the output.
//   bias    a head's table row is 4-byte aligned only, so its 2 s - 1 floats are staged in LDS once per workgroup; entry j - i + s - 1 is
//           added AFTER the scale.  An entry <= MTX_REL_MASKED and a key >= n_keys never enter the maximum and weigh exactly 0; the running
//           maximum starts at a finite sentinel, so a row that has seen no key yet rescales by exp(0) and a row that never sees one ends
//           with l = 0 and is stored as zeros.
//   no cache, no tile skipping: s <= 1024, and a skip rule would need a promise about the table.
#include "mtx_device.h"

namespace mtx {

constexpr int RA_TQ = MTX_REL_ATTN_TQ;
constexpr int RA_TK = 32;
constexpr int RA_SMAX = MTX_REL_ATTN_SMAX;
constexpr float RA_NEG = -1.0e30f;        // running maximum before the first visible key (finite: exp(RA_NEG - RA_NEG) is 1, never NaN)
static_assert(RA_TQ == 64 && RA_SMAX == 1024, "tile constants of include/mtx_hip.h");

// grid (query blocks of RA_TQ rows, heads)
template <typename T, int D>
__global__ __launch_bounds__(256) void rel_attn_kernel(mtx_rel_attn_args p) {
  typedef typename Traits<T>::v8 v8;
  typedef typename Traits<T>::v4 v4;
  constexpr int KS = D / 32, DB = D / 16, CH = D / 8;
  constexpr int VROW = D + 16;            // LDS row of the V tile in elements: 72 / 40 dwords, so the 8 rows a half wave's transpose read touches fall on 8 x 8 distinct banks
  __shared__ u32x4 Vs4[RA_TK * VROW / 8];
  __shared__ float rels[2 * RA_SMAX];
  T* Vs = reinterpret_cast<T*>(Vs4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, q4 = lane >> 4;
  const int s = p.s;
  int nk = s;
  if (p.n_keys) { const int n = *p.n_keys; nk = n < s ? n : s; }
  nk = __builtin_amdgcn_readfirstlane(nk < 0 ? 0 : nk);             // (workgroup-uniform) the keys that count: [0, nk)
  const int G = p.heads / p.kv_heads;
  const int h = blockIdx.y, kvh = h / G;
  const int q0 = blockIdx.x * RA_TQ;
  const T* Q = reinterpret_cast<const T*>(p.q) + (long)h * p.q_hs;
  const T* K = reinterpret_cast<const T*>(p.k) + (long)kvh * p.k_hs;
  const T* V = reinterpret_cast<const T*>(p.v) + (long)kvh * p.v_hs;
  const bool biased = p.rel != nullptr;

  // the head's table row: entries 0 .. 2 s - 2 (read after the tile loop's barriers)
  if (biased) {
    const float* rel = p.rel + (long)h * p.ld_rel;
    for (int i = tid; i < 2 * s - 1; i += 256) rels[i] = rel[i];
  }

  const int qw0 = q0 + wave * 16;                                   // the wave's first query row
  const bool wave_active = qw0 < s;
  const int qi = qw0 + l15;
  const int qc = qi < s ? qi : s - 1;                               // rows past the end compute on the last row and are not stored
  const int kmax = nk - 1;                                          // the last key that is read
  const int ntiles = (nk + RA_TK - 1) / RA_TK;

  v8 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const v8*>(Q + (long)qc * p.q_ss + ks * 32 + q4 * 8);

  f32x4 ohi[DB], olo[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) { ohi[d] = f32x4{0.f, 0.f, 0.f, 0.f}; olo[d] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  float m = RA_NEG, l = 0.f;

  for (int t = 0; t < ntiles; ++t) {
    const int j0 = t * RA_TK;
    __syncthreads();                                                // the previous tile's V reads are done
#pragma unroll
    for (int it = 0; it < RA_TK * CH / 256; ++it) {
      const int idx = tid + it * 256, ch = idx % CH, row = idx / CH;
      int j = j0 + row;
      j = j < kmax ? j : kmax;                                      // keys past the limit repeat the last one: their weight is 0
      *reinterpret_cast<u32x4*>(Vs + row * VROW + ch * 8) = *reinterpret_cast<const u32x4*>(V + (long)j * p.v_ss + ch * 8);
    }
    __syncthreads();
    if (!wave_active) continue;                                     // (wave-uniform) the sequence ends before this wave's rows

    // ---- S^T = K Q^T: sacc[s][r] is key j0 + 16 s + 4 q4 + r for query row l15
    f32x4 sacc[2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      sacc[sb] = f32x4{0.f, 0.f, 0.f, 0.f};
      int j = j0 + sb * 16 + l15;
      j = j < kmax ? j : kmax;
      const T* kp = K + (long)j * p.k_ss + q4 * 8;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) sacc[sb] = Traits<T>::mfma(*reinterpret_cast<const v8*>(kp + ks * 32), qf[ks], sacc[sb]);
    }

    // ---- online softmax; key j counts for row i iff j < nk and the table entry j - i + s - 1 is above MTX_REL_MASKED
    float sc[8];
    unsigned seen = 0;
    float tmax = RA_NEG;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int key = j0 + (e >> 2) * 16 + q4 * 4 + (e & 3);
      bool vis = key < nk;
      float b = 0.f;
      if (biased) {
        b = rels[vis ? key - qc + s - 1 : 0];
        vis = vis && b > MTX_REL_MASKED;
      }
      const float v = vis ? sacc[e >> 2][e & 3] * p.scale + b : RA_NEG;
      seen |= vis ? 1u << e : 0u;
      sc[e] = v;
      tmax = v > tmax ? v : tmax;
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
      const float pv = (seen >> e) & 1u ? __expf(sc[e] - mnew) : 0.f;      // (a masked key weighs 0 even while the row has seen no key at all)
      psum += pv;
      T hi, lo;
      p_split<T>(pv, hi, lo);
      phi[e] = hi; plo[e] = lo;                                     // k-slot 8 q4 + e  <->  key j0 + (e < 4 ? 4 q4 + e : 16 + 4 q4 + e - 4)
    }
    l = l * alpha + psum;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
#pragma unroll
      for (int r = 0; r < 4; ++r) { ohi[d][r] *= alpha; olo[d][r] *= alpha; }
    }

    // ---- O^T += V^T P^T: lane (l15, q4) receives V[4 q4 + 0..3][16 d + l15] and V[16 + 4 q4 + 0..3][16 d + l15]
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      const T* a = Vs + (q4 * 4 + (l15 >> 2)) * VROW + d * 16 + (l15 & 3) * 4;
      const v4 v0 = lds_read_tr16<T>(a);
      const v4 v1 = lds_read_tr16<T>(a + 16 * VROW);
      v8 vf;
      vf[0] = v0[0]; vf[1] = v0[1]; vf[2] = v0[2]; vf[3] = v0[3];
      vf[4] = v1[0]; vf[5] = v1[1]; vf[6] = v1[2]; vf[7] = v1[3];
      ohi[d] = Traits<T>::mfma(vf, phi, ohi[d]);
      olo[d] = Traits<T>::mfma(vf, plo, olo[d]);
    }
  }

  // ---- row sums across the 4 quads, normalise, store 4 consecutive d per lane; a row without a visible key has l = 0 and stores zeros
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (qi < s) {
    T* O = reinterpret_cast<T*>(p.o) + (long)qi * p.o_ss + (long)h * p.o_hs + q4 * 4;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      v4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = from_f32<T>(l > 0.f ? (ohi[d][r] + olo[d][r] * LoScale<T>::inv) / l : 0.f);
      *reinterpret_cast<v4*>(O + d * 16) = o;
    }
  }
}

int rel_attn_launch(const mtx_rel_attn_args* a, void* stream, const char** err) {
  if (!a->q || !a->k || !a->v || !a->o) { *err = "rel_attn: null operand"; return MTX_ERR_INVALID; }
  if (a->dtype != MTX_BF16 && a->dtype != MTX_F16) { *err = "rel_attn: dtype must be bf16 or f16"; return MTX_ERR_INVALID; }
  if (a->d != 64 && a->d != 128) { *err = "rel_attn: only head widths 64 and 128 are built"; return MTX_ERR_UNSUPPORTED; }
  if (a->s < 1 || a->s > RA_SMAX) { *err = "rel_attn: needs 1 <= s <= MTX_REL_ATTN_SMAX"; return MTX_ERR_UNSUPPORTED; }
  if (a->heads < 1 || a->kv_heads < 1 || a->heads % a->kv_heads) { *err = "rel_attn: heads must be a multiple of kv_heads"; return MTX_ERR_UNSUPPORTED; }
  if (a->heads > 65535) { *err = "rel_attn: heads <= 65535"; return MTX_ERR_INVALID; }
  if (a->rel && (a->ld_rel < 2L * a->s - 1 || ((size_t)a->rel & 3) != 0)) { *err = "rel_attn: the table needs ld_rel >= 2 s - 1 and 4-byte alignment"; return MTX_ERR_INVALID; }
  if (((size_t)a->n_keys & 3) != 0) { *err = "rel_attn: n_keys must be 4-byte aligned"; return MTX_ERR_INVALID; }
  if ((((size_t)a->q | (size_t)a->k | (size_t)a->v | (size_t)a->o) & 15) != 0) { *err = "rel_attn: operands must be 16-byte aligned"; return MTX_ERR_INVALID; }
  if ((a->q_ss | a->q_hs | a->k_ss | a->k_hs | a->v_ss | a->v_hs | a->o_ss | a->o_hs) % 8 != 0) { *err = "rel_attn: strides must be multiples of 8"; return MTX_ERR_INVALID; }
  const dim3 grid((unsigned)((a->s + RA_TQ - 1) / RA_TQ), (unsigned)a->heads);
  with_storage_type(a->dtype, [&](auto t) {
    typedef typename decltype(t)::type T;
    if (a->d == 64) MTX_LAUNCH((rel_attn_kernel<T, 64>), grid, dim3(256), 0, stream, *a);
    else MTX_LAUNCH((rel_attn_kernel<T, 128>), grid, dim3(256), 0, stream, *a);
  });
  return MTX_OK;
}

}  // namespace mtx
