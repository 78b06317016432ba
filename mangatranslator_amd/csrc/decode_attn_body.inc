// decode_attn_body.inc — the body of decode_attn_kernel<T> (csrc/decode.hip), stamped into it and into its group-batched twin so that both run
// the same code: `p` = an mtx_decode_attn_args (the twin fills one for its group), blockIdx.x = head, blockIdx.y = row.
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
