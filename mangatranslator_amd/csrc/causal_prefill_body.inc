// causal_prefill_body.inc — one (head, 64-query block) of one prompt's causal attention: the body of causal_prefill_kernel and of
// causal_prefill_slots_kernel (causal.hip), included inside each so that the single-sequence kernel stays, token for token, the code it was.
// In scope at the point of inclusion: T, `p` (mtx_causal_attn_args holding THAT sequence's operands) and the macros CA_PREFILL_POS (the
// positions already cached) and CA_PREFILL_QB (the query block inside the sequence); the head is blockIdx.y.
  typedef typename Traits<T>::v8 v8;
  typedef typename Traits<T>::v4 v4;
  __shared__ u32x4 Vs4[CA_TK * CA_VROW / 8];
  T* Vs = reinterpret_cast<T*>(Vs4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, q4 = lane >> 4;
  const int pos = CA_PREFILL_POS;
  if (pos < 0 || pos > p.max_len - p.rows) return;                 // (workgroup-uniform) nothing is read or written outside the cache
  const int G = p.heads / p.kv_heads;
  const int h = blockIdx.y, kvh = h / G;
  const int q0 = CA_PREFILL_QB * CA_TQ;
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
