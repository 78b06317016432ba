// attn_body.inc — one (head, 128-query block) of the short attention kernel: the body of attn_kernel and of attn_seg_kernel (attention.hip),
// included inside each so that the single-sequence kernel stays, token for token, the code it was.  In scope at the point of inclusion: T, DP,
// `p` (AttnParams holding THAT sequence's operands, lengths and strides) and the macros ATTN_BODY_BH (batch * heads + head) and ATTN_BODY_QB
// (the query block inside the sequence).
  typedef typename Traits<T>::v8 v8;
  typedef typename Traits<T>::v4 v4;
  constexpr int KST = DP / 32;                 // k-steps of the S^T product
  constexpr int DF = DP / 16;                  // d fragments of O^T
  constexpr int SLOTS = DP <= 64 ? 8 : 16;
  constexpr int KROW = SLOTS * 16;             // bytes per K row in LDS
  constexpr int K_BYTES = AT_KV * KROW;
  constexpr int VT_BYTES = DP * 128;           // [DP rows][64 keys] T
  __shared__ __attribute__((aligned(16))) unsigned char smem[K_BYTES + VT_BYTES];
  unsigned char* Ks = smem;
  unsigned char* Vt = smem + K_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, q4 = lane >> 4;
  const long bh = ATTN_BODY_BH;
  const long qb = ATTN_BODY_QB;
  const long b = bh / p.heads, h = bh % p.heads;
  const long q0 = qb * AT_QB + wv * AT_QW;
  const T* Q = reinterpret_cast<const T*>(p.q) + b * p.q_bs + h * p.q_hs;
  const T* K = reinterpret_cast<const T*>(p.k) + b * p.k_bs + h * p.k_hs;
  const T* V = reinterpret_cast<const T*>(p.v) + b * p.v_bs + h * p.v_hs;
  T* O = reinterpret_cast<T*>(p.o) + b * p.o_bs + h * p.o_hs;
  const int dch = (int)(p.d / 8);              // valid 16-byte chunks per row

  // Q fragments (B operand: col = query row, 8 consecutive d per lane), kept in registers
  v8 qf[2][KST];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int ks = 0; ks < KST; ++ks) {
      const long qr = q0 + f * 16 + l15;
      const int ch = ks * 4 + q4;
      u32x4 raw = u32x4{0u, 0u, 0u, 0u};
      if (qr < p.sq && ch < dch) raw = *reinterpret_cast<const u32x4*>(Q + qr * p.q_ss + ch * 8);
      qf[f][ks] = __builtin_bit_cast(v8, raw);
    }

  f32x4 oacc[2][DF];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int d = 0; d < DF; ++d) oacc[f][d] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mrun[2] = {-1.0e30f, -1.0e30f};
  float lrun[2] = {0.f, 0.f};

  constexpr int KCH = AT_KV * (DP / 8);        // 16-byte chunks per K (or V) tile
  constexpr int NLD = (KCH + 255) / 256;
  u32x4 rk[NLD], rv[NLD];
  auto load_tile = [&](long k0) {
#pragma unroll
    for (int it = 0; it < NLD; ++it) {
      const int idx = tid + it * 256;
      const int ch = idx % (DP / 8), row = idx / (DP / 8);
      u32x4 a = u32x4{0u, 0u, 0u, 0u}, c = u32x4{0u, 0u, 0u, 0u};
      if (idx < KCH && k0 + row < p.sk && ch < dch) {
        a = *reinterpret_cast<const u32x4*>(K + (k0 + row) * p.k_ss + ch * 8);
        c = *reinterpret_cast<const u32x4*>(V + (k0 + row) * p.v_ss + ch * 8);
      }
      rk[it] = a; rv[it] = c;
    }
  };

  const long ntiles = (p.sk + AT_KV - 1) / AT_KV;
  load_tile(0);
  for (long t = 0; t < ntiles; ++t) {
    const long k0 = t * AT_KV;
    __syncthreads();
#pragma unroll
    for (int it = 0; it < NLD; ++it) {
      const int idx = tid + it * 256;
      if (idx < KCH) {
        const int ch = idx % (DP / 8), row = idx / (DP / 8);
        *reinterpret_cast<u32x4*>(Ks + row * KROW + ((ch ^ (row & (SLOTS - 1))) << 4)) = rk[it];
        // V transposed: Vt[d][key], 8-byte granules (4 keys) XOR-swizzled by (d & 15)
        const typename Traits<T>::v8 vv = __builtin_bit_cast(v8, rv[it]);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int dr = ch * 8 + e;
          *reinterpret_cast<T*>(Vt + dr * 128 + ((((row >> 2) ^ (dr & 15))) << 3) + ((row & 3) << 1)) = vv[e];
        }
      }
    }
    __syncthreads();
    if (t + 1 < ntiles) load_tile(k0 + AT_KV);

    // ---- S^T = K Q^T : sacc[f][kf] holds keys kf*16 + q4*4 + r for query f*16 + l15 -----------
    f32x4 sacc[2][4];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int kf = 0; kf < 4; ++kf) sacc[f][kf] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KST; ++ks) {
      const int ch = ks * 4 + q4;
#pragma unroll
      for (int kf = 0; kf < 4; ++kf) {
        const int row = kf * 16 + l15;
        const v8 kfr = *reinterpret_cast<const v8*>(Ks + row * KROW + ((ch ^ (row & (SLOTS - 1))) << 4));
#pragma unroll
        for (int f = 0; f < 2; ++f) sacc[f][kf] = Traits<T>::mfma(kfr, qf[f][ks], sacc[f][kf]);
      }
    }

    // ---- online softmax (base-2), lane-local per query row --------------------------------------
    v8 pb[2][2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      float tmax = -1.0e30f;
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long key = k0 + kf * 16 + q4 * 4 + r;
          float s = sacc[f][kf][r] * p.scale_log2;
          if (key >= p.sk) s = -1.0e30f;
          sacc[f][kf][r] = s;
          tmax = s > tmax ? s : tmax;
        }
      { float o1 = __shfl_xor(tmax, 16, 64); tmax = o1 > tmax ? o1 : tmax; }
      { float o2 = __shfl_xor(tmax, 32, 64); tmax = o2 > tmax ? o2 : tmax; }
      const float mnew = tmax > mrun[f] ? tmax : mrun[f];
      const float alpha = exp2f(mrun[f] - mnew);
      mrun[f] = mnew;
      float psum = 0.f;
#pragma unroll
      for (int kf = 0; kf < 4; ++kf)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv = exp2f(sacc[f][kf][r] - mnew);
          psum += pv;
          // B operand of O^T = V^T P^T: k-slot q4*8 + e  <->  key (kk*32) + (e<4 ? q4*4+e : 16+q4*4+e-4)
          pb[f][kf >> 1][(kf & 1) * 4 + r] = from_f32<T>(pv);
        }
      lrun[f] = lrun[f] * alpha + psum;
#pragma unroll
      for (int d = 0; d < DF; ++d) {
        oacc[f][d][0] *= alpha; oacc[f][d][1] *= alpha; oacc[f][d][2] *= alpha; oacc[f][d][3] *= alpha;
      }
    }

    // ---- O^T += V^T P^T ------------------------------------------------------------------------
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int d = 0; d < DF; ++d) {
        const int dr = d * 16 + l15;
        const int g0 = kk * 8 + q4;            // granule of keys kk*32 + q4*4 .. +3
        const int g1 = kk * 8 + 4 + q4;        // granule of keys kk*32 + 16 + q4*4 .. +3
        const v4 lo = *reinterpret_cast<const v4*>(Vt + dr * 128 + ((g0 ^ (dr & 15)) << 3));
        const v4 hi = *reinterpret_cast<const v4*>(Vt + dr * 128 + ((g1 ^ (dr & 15)) << 3));
        v8 vf;
        vf[0] = lo[0]; vf[1] = lo[1]; vf[2] = lo[2]; vf[3] = lo[3];
        vf[4] = hi[0]; vf[5] = hi[1]; vf[6] = hi[2]; vf[7] = hi[3];
#pragma unroll
        for (int f = 0; f < 2; ++f) oacc[f][d] = Traits<T>::mfma(vf, pb[f][kk], oacc[f][d]);
      }
    }
  }

  // ---- finish: row sums across the 4 quads, normalise, store 4 consecutive d per lane ----------
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    float l = lrun[f];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    const long qr = q0 + f * 16 + l15;
    if (qr < p.sq) {
#pragma unroll
      for (int d = 0; d < DF; ++d) {
        const int dc = d * 16 + q4 * 4;
        if (dc < p.d) {
          v4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = from_f32<T>(oacc[f][d][r] * inv);
          *reinterpret_cast<v4*>(O + qr * p.o_ss + dc) = o;
        }
      }
    }
  }
