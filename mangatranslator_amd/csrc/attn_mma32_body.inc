// attn_mma32_body.inc — the long-sequence attention kernel, stamped by attention.hip once per variant:
//
//   kernel                     Q8  WIDE  DEEP  K8  V8
//   attn_mma32_kernel           0    0     0    0   0     token for token the kernel as it was first tuned and measured
//   attn_mma32_q8_kernel        1    0     0    0   0
//   attn_mma32_q8d_kernel       1    0   0x44   0   0
//   attn_mma32_d_kernel         0    1   0x44   0   0     the FLUX graphs' form
//   attn_mma32_k8_kernel        0    1   0x44   1   0
//   attn_mma32_k8q_kernel       1    0   0x44   1   0
//   attn_mma32_k8v8q_kernel     1    0   0x44   1   1
//
// ATTN_MMA32_NAME and all five switches are defined by the includer before every inclusion and undefined at the end of this file.
//   Q8    the rows leave as the MX fp8 operand of the next linear (mtx_attn_args.q8) instead of 16-bit rows
//   WIDE  the 16-bit rows leave as 8 x 16-byte stores per lane instead of 16 x 8-byte ones (not read when Q8 is set)
//   DEEP  fragment reads ahead of the MFMAs in the pre-scaled tile step: K k-steps ahead | V MFMAs ahead << 4 (attn_bias_tile)
//   K8    the scores come from plain e4m3 copies of q and k (mtx_attn_args.q_f8 / k_f8) on the MX-scaled fp8 matrix instruction: four
//         MFMAs of K = 64 per tile instead of sixteen of K = 16; a K tile is 8 KiB of LDS.  PRESCALED and DEEP only.
//   V8    (with K8) P V on the fp8 instruction too: V^T tiles come as e4m3 [d][64 keys] in accumulator key order (MTX_EW_V_F8T), 8 KiB per tile
// An include rather than a template flag or a shared device function on purpose: both of those changed the register allocation and the
// schedule of the 16-bit kernel (5 % of its instruction sequence moved, compared with `hipcc -S`), and that kernel is 30 % of a page's
// GPU time.  A variant is a new line of the table; tools/isa_diff.py shows that the others did not move.
// PRESCALED (MTX_ATTN_Q_PRESCALED, the FLUX graphs): q carries scale * log2(e); the S^T accumulators start at minus the running maximum
// and no maximum is taken on the hot path (attn_bias_tile).  Otherwise the classic online softmax of attn_mma32_tile.
#if !defined(ATTN_MMA32_NAME) || !defined(ATTN_MMA32_Q8) || !defined(ATTN_MMA32_WIDE) || !defined(ATTN_MMA32_DEEP) || !defined(ATTN_MMA32_K8) || !defined(ATTN_MMA32_V8)
#error "attn_mma32_body.inc: define ATTN_MMA32_NAME, _Q8, _WIDE, _DEEP, _K8 and _V8 before every inclusion"
#endif
template <typename T, int DP, bool PRESCALED>
__global__ __launch_bounds__(512) void ATTN_MMA32_NAME(AttnParams p) {
  constexpr bool BIAS = PRESCALED;
#if ATTN_MMA32_K8
  static_assert(PRESCALED && ATTN_MMA32_DEEP, "the fp8-score form exists for pre-scaled q and the deep-prefetch loop");
#endif
  using v8 [[maybe_unused]] = typename Traits<T>::v8;
  using v4 [[maybe_unused]] = typename Traits<T>::v4;
  [[maybe_unused]] constexpr int KS = DP / 16; // k-steps of S^T
  constexpr int DB = DP / 32;                  // 32-row blocks of O^T
  constexpr int ROWB = DP * 2;                 // bytes per K / V row
  constexpr int CPR = DP / 8;                  // 16-byte chunks per row
  constexpr int TILE_B = AB_KV * ROWB;
  constexpr int NLD = AB_KV * CPR / 512;       // chunks per thread per operand per tile
  static_assert(DP == 128, "swizzles are written for 256-byte rows");
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * TILE_B];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, hi = lane >> 5;
  unsigned vb, part = 0, nparts = 1;
  const unsigned bidx = blockIdx.x;
  if (bidx < p.n_full) vb = xcd_remap(bidx, p.n_full);
  else { const unsigned i = bidx - p.n_full; vb = p.n_full + i / p.split; part = i % p.split; nparts = p.split; }
  const long bh = vb / p.qblocks, qb = vb % p.qblocks;
  const long b = bh / p.heads, h = bh % p.heads;
  const long q0 = qb * AB_QB + wv * 32;
  const T* Q = reinterpret_cast<const T*>(p.q) + b * p.q_bs + h * p.q_hs;
  const T* K = reinterpret_cast<const T*>(p.k) + b * p.k_bs + h * p.k_hs;
  const T* V = reinterpret_cast<const T*>(p.v) + b * p.v_bs + h * p.v_hs;
  T* O = reinterpret_cast<T*>(p.o) + b * p.o_bs + h * p.o_hs;

#if ATTN_MMA32_K8
  // Q^T fragments of the fp8 instruction (B operand: column = query l31; the lane holds bytes 64 ks + 32 hi + 0..31 of its row — the K
  // fragments use the same assignment, and with one scale for all blocks any assignment that is the same on both sides gives the same sum)
  i32x8 qf[2];
  {
    const long qr = q0 + l31;
    const unsigned char* Q8 = p.qf8 + h * DP;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      u32x4 lo = u32x4{0u, 0u, 0u, 0u}, hv = lo;
      if (qr < p.sq) {
        lo = *reinterpret_cast<const u32x4*>(Q8 + qr * p.qf8_ss + ks * 64 + hi * 32);
        hv = *reinterpret_cast<const u32x4*>(Q8 + qr * p.qf8_ss + ks * 64 + hi * 32 + 16);
      }
      qf[ks] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hv[0], (int)hv[1], (int)hv[2], (int)hv[3]};
    }
  }
  (void)Q; (void)K;
#else
  // Q^T fragments (B operand: column = query l31, k = d 16*ks + 8*hi + j)
  v8 qf[KS];
  {
    const long qr = q0 + l31;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      u32x4 raw = u32x4{0u, 0u, 0u, 0u};
      if (qr < p.sq) raw = *reinterpret_cast<const u32x4*>(Q + qr * p.q_ss + ks * 16 + hi * 8);
      qf[ks] = __builtin_bit_cast(v8, raw);
      if (BIAS) {                              // Q <- Q * scale * log2(e), rounded back to the storage type
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[ks][e] = from_f32<T>(to_f32(qf[ks][e]) * p.scale_log2);
      }
    }
  }
#endif

  f32x16 oacc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[d][r] = 0.f;
  float m_raw = BIAS ? 0.f : -1.0e30f, lsum = 0.f;     // BIAS: m_raw holds M in log2 units
  const float c = p.scale_log2;
  const float thr = 8.0f / c;                  // refresh the max when a row's tile max grows by > 2^8
  f32x16 minit;
#pragma unroll
  for (int r = 0; r < 16; ++r) minit[r] = 0.f;
  bool first = true;

  // ---- global -> register staging through buffer descriptors (no per-load predicates, no 64-bit VALU math)
#if ATTN_MMA32_K8
  const BufView kb_ = make_buf(p.kf8 + h * DP, (unsigned)((p.sk - 1) * p.kf8_ss + DP));
  // a K tile is 64 rows of 128 bytes: one 16-byte chunk per thread; chunk ^= (row >> 1) & 7 (two rows span the 64 banks)
  const unsigned k8off = (unsigned)((tid >> 3) * p.kf8_ss + (tid & 7) * 16);
  const int k8sw = (tid >> 3) * 128 + (((tid & 7) ^ ((tid >> 4) & 7)) << 4);
  u32x4 rk8;
#else
  const BufView kb_ = make_buf(K, (unsigned)(((p.sk - 1) * p.k_ss + DP) * sizeof(T)));
#endif
#if ATTN_MMA32_V8
  static_assert(ATTN_MMA32_K8, "fp8 P V comes with fp8 scores");
  const long sk_pad = (p.sk + AB_KV - 1) / AB_KV * AB_KV;
  const BufView vb_ = make_buf(p.vf8 + (size_t)h * DP * p.vf8_ld, (unsigned)((DP - 1) * p.vf8_ld + sk_pad));
  // a V^T tile is 128 d-rows of 64 bytes: one 16-byte chunk per thread; chunk ^= (d >> 2) & 3 (four rows span the 64 banks)
  const unsigned v8off = (unsigned)((tid >> 2) * p.vf8_ld + (tid & 3) * 16);
  const int v8sw = TILE_B + (tid >> 2) * 64 + (((tid & 3) ^ ((tid >> 4) & 3)) << 4);
  u32x4 rv8;
  (void)V;
#else
  const BufView vb_ = make_buf(V, (unsigned)(((p.sk - 1) * p.v_ss + DP) * sizeof(T)));
#endif
  unsigned kvoff[NLD], vvoff[NLD];
  int ksw[NLD], vsw[NLD];
#pragma unroll
  for (int it = 0; it < NLD; ++it) {
    const int idx = tid + it * 512;
    const int ch = idx % CPR, row = idx / CPR;
    kvoff[it] = (unsigned)((row * p.k_ss + ch * 8) * sizeof(T));
    vvoff[it] = (unsigned)((row * p.v_ss + ch * 8) * sizeof(T));
    ksw[it] = row * ROWB + ((ch ^ (row & 15)) << 4);
    vsw[it] = TILE_B + row * ROWB + ((ch ^ ((row & 3) << 2)) << 4);
  }
#if ATTN_MMA32_V8
  const unsigned k_step = (unsigned)(AB_KV * p.kf8_ss);
  auto load_tile = [&](long t) {
    rk8 = buf_load16(kb_, k8off, (unsigned)t * k_step);
    rv8 = buf_load16(vb_, v8off, (unsigned)t * AB_KV);
  };
  auto store_tile = [&](int stage) {
    *reinterpret_cast<u32x4*>(smem + stage * 2 * TILE_B + k8sw) = rk8;
    *reinterpret_cast<u32x4*>(smem + stage * 2 * TILE_B + v8sw) = rv8;
  };
  (void)kvoff; (void)ksw; (void)vvoff; (void)vsw;
#elif ATTN_MMA32_K8
  const unsigned k_step = (unsigned)(AB_KV * p.kf8_ss), v_step = (unsigned)(AB_KV * p.v_ss * sizeof(T));
  u32x4 rv[NLD];
  auto load_tile = [&](long t) {
    rk8 = buf_load16(kb_, k8off, (unsigned)t * k_step);
#pragma unroll
    for (int it = 0; it < NLD; ++it) rv[it] = buf_load16(vb_, vvoff[it], (unsigned)t * v_step);
  };
  auto store_tile = [&](int stage) {
    *reinterpret_cast<u32x4*>(smem + stage * 2 * TILE_B + k8sw) = rk8;
#pragma unroll
    for (int it = 0; it < NLD; ++it) *reinterpret_cast<u32x4*>(smem + stage * 2 * TILE_B + vsw[it]) = rv[it];
  };
  (void)kvoff; (void)ksw;
#else
  const unsigned k_step = (unsigned)(AB_KV * p.k_ss * sizeof(T)), v_step = (unsigned)(AB_KV * p.v_ss * sizeof(T));
  u32x4 rk[NLD], rv[NLD];
  auto load_tile = [&](long t) {
#pragma unroll
    for (int it = 0; it < NLD; ++it) {
      rk[it] = buf_load16(kb_, kvoff[it], (unsigned)t * k_step);
      rv[it] = buf_load16(vb_, vvoff[it], (unsigned)t * v_step);
    }
  };
  auto store_tile = [&](int stage) {
#pragma unroll
    for (int it = 0; it < NLD; ++it) {
      *reinterpret_cast<u32x4*>(smem + stage * 2 * TILE_B + ksw[it]) = rk[it];
      *reinterpret_cast<u32x4*>(smem + stage * 2 * TILE_B + vsw[it]) = rv[it];
    }
  };
#endif

  // ---- loop-invariant LDS fragment addresses (byte offsets inside a stage) ---------------------------------
  // K: row l31 (+32*kb), chunk (2*ks + hi) ^ (l31 & 15)
#if ATTN_MMA32_K8
  // fp8 K: row l31 (+32*kb) of 128 bytes, logical chunks 4 ks + 2 hi and + 1 (the lane's 32 bytes of k-step ks), chunk ^= (row >> 1) & 7
  int kaddr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) kaddr[i] = l31 * 128 + (((4 * (i >> 1) + 2 * hi + (i & 1)) ^ ((l31 >> 1) & 7)) << 4);
  const int qk_scale_b = 127 + p.qk_f8_exp;
#else
  int kaddr[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) kaddr[ks] = l31 * ROWB + (((2 * ks + hi) ^ (l31 & 15)) << 4);
#endif
  // V^T by transpose reads: 16-lane group g1 covers d 16*g1..+15 of a 32-row block; lane i of the group
  // addresses key 4*hi + (i>>2) (+ step base), d 4*(i&3)..+3; chunk swizzle 4*(key & 3) = 4*(i>>2)
#if ATTN_MMA32_V8
  // fp8 V^T: d-row l31 (+32 per block) of 64 bytes; the lane's kb = 0 keys are logical chunk hi, its kb = 1 keys chunk 2 + hi
  int vaddr[2];
  vaddr[0] = l31 * 64 + ((hi ^ ((l31 >> 2) & 3)) << 4);
  vaddr[1] = l31 * 64 + (((2 + hi) ^ ((l31 >> 2) & 3)) << 4);
#else
  int vaddr[DB];
  {
    const int ti = lane & 15, g1 = (lane >> 4) & 1;
    const int vrow = hi * 4 + (ti >> 2);
#pragma unroll
    for (int d = 0; d < DB; ++d)
      vaddr[d] = vrow * ROWB + (((4 * d + 2 * g1 + ((ti & 3) >> 1)) ^ ((ti >> 2) << 2)) << 4) + (ti & 1) * 8;
  }
#endif

  const long ntiles_all = (p.sk + AB_KV - 1) / AB_KV;
  const long t_begin = part * ntiles_all / nparts, ntiles = (part + 1) * ntiles_all / nparts;    // this workgroup's key tiles
  const long kv_last = ntiles == ntiles_all ? p.sk - (ntiles_all - 1) * AB_KV : AB_KV;     // valid keys in its last tile
  // the key-tile loop, written once and expanded with the tile step `ATTN_TILE` of the pass at hand
#define ATTN_MMA32_LOOP() do { \
    load_tile(t_begin); \
    store_tile(0); \
    __syncthreads(); \
    long t = t_begin; \
    /* full tiles, two per iteration so the LDS stage is a compile-time constant */ \
    for (; t + 2 < ntiles; t += 2) { \
      load_tile(t + 1); \
      ATTN_TILE(0, false, AB_KV); \
      store_tile(1); \
      MTX_LDS_BARRIER(); \
      load_tile(t + 2); \
      ATTN_TILE(1, false, AB_KV); \
      store_tile(0); \
      MTX_LDS_BARRIER(); \
    } \
    /* one or two tiles left; the very last one may be ragged */ \
    if (t + 2 == ntiles) { \
      load_tile(t + 1); \
      ATTN_TILE(0, false, AB_KV); \
      store_tile(1); \
      MTX_LDS_BARRIER(); \
      if (kv_last < AB_KV) ATTN_TILE(1, true, kv_last); \
      else ATTN_TILE(1, false, AB_KV); \
    } else { \
      if (kv_last < AB_KV) ATTN_TILE(0, true, kv_last); \
      else ATTN_TILE(0, false, AB_KV); \
    } \
  } while (0)
#if ATTN_MMA32_V8
#define ATTN_TILE(ST, RAG, KV) attn_bias_tile_k8v8<T, DP, ST, RAG>(smem, qf, oacc, m_raw, lsum, minit, first, kaddr, vaddr, KV, hi, qk_scale_b)
  (void)thr;
#elif ATTN_MMA32_K8
#define ATTN_TILE(ST, RAG, KV) attn_bias_tile_k8<T, DP, ST, RAG, ATTN_MMA32_DEEP>(smem, qf, oacc, m_raw, lsum, minit, first, kaddr, vaddr, KV, hi, qk_scale_b)
  (void)thr;
#else
#define ATTN_TILE(ST, RAG, KV) do { if constexpr (BIAS) attn_bias_tile<T, DP, ST, RAG, ATTN_MMA32_DEEP>(smem, qf, oacc, m_raw, lsum, minit, first, kaddr, vaddr, KV, hi); \
                                    else attn_mma32_tile<T, DP, ST, RAG>(smem, qf, oacc, m_raw, lsum, c, thr, kaddr, vaddr, KV, hi); } while (0)
#endif
  ATTN_MMA32_LOOP();
#undef ATTN_TILE
#define ATTN_ROW_SUM() half_sum(lsum)
#undef ATTN_MMA32_LOOP

  if (nparts > 1) {
    // ---- key-split tail: leave the unnormalised O^T (fp32), the row maximum and the row sum for the merge kernel
    const unsigned slot = bidx - p.n_full;
    const int row = wv * 32 + l31;
    float* PO = p.part_o + ((size_t)slot * AB_QB + row) * DP;
    const float lrow = ATTN_ROW_SUM();
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 o = {oacc[d][g * 4 + 0], oacc[d][g * 4 + 1], oacc[d][g * 4 + 2], oacc[d][g * 4 + 3]};
        *reinterpret_cast<f32x4*>(PO + d * 32 + g * 8 + hi * 4) = o;
      }
    if (hi == 0) { p.part_ml[((size_t)slot * AB_QB + row) * 2] = BIAS ? m_raw / c : m_raw; p.part_ml[((size_t)slot * AB_QB + row) * 2 + 1] = lrow; }
    return;
  }

  // ---- finish: the two lane halves of a row add their partial sums; 4 consecutive d per store -----------
  const float l = ATTN_ROW_SUM();
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  const long qr = q0 + l31;
#if ATTN_MMA32_Q8
  // MX e4m3 + E8M0 of the row rounded to the storage type, exactly what quant_mx_kernel makes of the 16-bit output: a 32-wide block of the
  // head dim lives in this lane (16 values) and in lane ^ 32 (the other 16), the layout of mx_quantize_halfpair; the four scale bytes of
  // the head's 128 columns are one word
  (void)O;
  unsigned word = 0;
#pragma unroll
  for (int d = 0; d < DB; ++d) {
    float hv[16];
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) { hv[e] = to_f32(from_f32<T>(oacc[d][e] * inv)); const float v = fabsf(hv[e]); amax = v > amax ? v : amax; }
    int eb;
    const u32x4 out = mx_quantize_halfpair(hv, amax, hi, eb);
    if (qr < p.sq) *reinterpret_cast<u32x4*>(p.q8 + (size_t)qr * p.ldq8 + h * DP + d * 32 + hi * 16) = out;
    word |= (unsigned)eb << (8 * d);
  }
  if (qr < p.sq && hi == 0) p.q8_scale[(size_t)h * (DP / 128) * p.lds_q8 + qr] = word;
#elif ATTN_MMA32_WIDE
  // lanes l and l ^ 32 hold 4 + 4 of every 8 consecutive columns: they trade two dwords (v_permlane32_swap) and each stores 16 contiguous bytes
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      v4 x, y;
#pragma unroll
      for (int r = 0; r < 4; ++r) { x[r] = from_f32<T>(oacc[d][gp * 8 + r] * inv); y[r] = from_f32<T>(oacc[d][gp * 8 + 4 + r] * inv); }
      const u32x2 xw = __builtin_bit_cast(u32x2, x), yw = __builtin_bit_cast(u32x2, y);
      uint32_t x0 = xw[0], x1 = xw[1], y0 = yw[0], y1 = yw[1];
      half_pair_exchange(x0, y0);
      half_pair_exchange(x1, y1);
      if (qr < p.sq) *reinterpret_cast<u32x4*>(O + qr * p.o_ss + d * 32 + gp * 16 + hi * 8) = u32x4{x0, x1, y0, y1};
    }
#else
  if (qr < p.sq) {
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        v4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = from_f32<T>(oacc[d][g * 4 + r] * inv);
        *reinterpret_cast<v4*>(O + qr * p.o_ss + d * 32 + g * 8 + hi * 4) = o;
      }
  }
#endif
#undef ATTN_ROW_SUM
}
#undef ATTN_MMA32_NAME
#undef ATTN_MMA32_Q8
#undef ATTN_MMA32_WIDE
#undef ATTN_MMA32_DEEP
#undef ATTN_MMA32_K8
#undef ATTN_MMA32_V8
