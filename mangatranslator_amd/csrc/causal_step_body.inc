// causal_step_body.inc — one sequence's decode step: the body of causal_step_kernel and of causal_step_batch_kernel (causal.hip), included
// inside each so that the single-sequence kernel stays, token for token, the code it was.  In scope at the point of inclusion: T, G,
// `p` (mtx_causal_attn_args holding THAT sequence's operands), `gfull`, and the macros CA_STEP_Z (this workgroup's chunk of G query heads),
// CA_STEP_Z_IS_0 and CA_STEP_NZ (chunks per kv head).
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
  const int h0 = kvh * gfull + CA_STEP_Z * G;
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
  if (split == n_active - 1 && CA_STEP_Z_IS_0 && grp == 0) {      // the row's k and v go to cache[pos] (nobody reads that position in this launch)
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
  unsigned* counter = reinterpret_cast<unsigned*>(p.workspace) + (kvh * CA_STEP_NZ + CA_STEP_Z);
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
