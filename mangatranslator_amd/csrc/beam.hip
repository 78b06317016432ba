// beam.hip — one iteration of manga-ocr's beam search per group, on the device (include/mtx_hip.h, mtx_beam_step_args; the arithmetic is that of
// core/ml/manga_ocr.py `beam_search`, which restates transformers' `_beam_search`).  Three launches:
//   beam_lse_kernel     grid (rows): a row's maximum and log(sum exp(x - max)), reduced in a fixed order
//   beam_cand_kernel    grid (ceil(chunks / 4), rows): a wave owns MTX_BEAM_CHUNK logits of one row, turns them into candidate scores
//                       ((x - max) - log sum, the n-gram ban, + running score) and writes its best `keep` in selection order
//   beam_final_kernel   grid (groups), one wave: the top `keep` of the group's records, then the bookkeeping of the iteration
// Every selection runs in the one order of the header's rule — value, then position — so a round takes "the best entry after the one taken
// last": nothing is marked, and equal inputs give equal bytes.
#include "mtx_device.h"
#include <climits>

namespace mtx {

constexpr int BEAM_KEEP_MAX = 5 * MTX_BEAM_MAX;          // max(2, 1 + n_eos) * beams, n_eos <= 4
constexpr int BEAM_PER_LANE = MTX_BEAM_CHUNK / 64;

// a comes before b in selection order
__device__ __forceinline__ bool beam_before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }
// (bv, bi) <- (v, i) if (v, i) lies after the entry taken last (pv, pi) and before the best so far; bi < 0: nothing yet
__device__ __forceinline__ void beam_take(float& bv, int& bi, float v, int i, float pv, int pi) {
  if (i < 0 || !beam_before(pv, pi, v, i)) return;
  if (bi < 0 || beam_before(v, i, bv, bi)) { bv = v; bi = i; }
}
__device__ __forceinline__ void beam_wave_best(float& bv, int& bi) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float v = __shfl_xor(bv, off, 64);
    const int i = __shfl_xor(bi, off, 64);
    if (i >= 0 && (bi < 0 || beam_before(v, i, bv, bi))) { bv = v; bi = i; }
  }
}
__device__ __forceinline__ float beam_clean(float x) { return x != x ? -INFINITY : x; }      // a NaN logit counts as -inf

__global__ __launch_bounds__(256) void beam_lse_kernel(mtx_beam_step_args p) {
  __shared__ float red[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int32_t* st = p.state + (long)(row / p.beams) * p.state_stride;
  if (st[MTX_BEAM_DONE] != 0) return;                    // workgroup-uniform
  const float* x = p.logits + (long)row * p.ld_logits;
  float m = -INFINITY;
  for (int i = tid; i < p.vocab; i += 256) { const float v = beam_clean(x[i]); m = v > m ? v : m; }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { const float o = __shfl_xor(m, off, 64); m = o > m ? o : m; }
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  m = red[0];
  for (int w = 1; w < 4; ++w) m = red[w] > m ? red[w] : m;
  __syncthreads();
  float s = 0.f;
  if (m > -INFINITY && m < INFINITY)
    for (int i = tid; i < p.vocab; i += 256) s += expf(beam_clean(x[i]) - m);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    s = ((red[0] + red[1]) + red[2]) + red[3];
    float* rec = reinterpret_cast<float*>(p.scratch) + 2L * row;
    rec[0] = m;                                          // not finite: the row has no finite logit (beam_final_kernel ends the group)
    rec[1] = logf(s);
  }
}

__global__ __launch_bounds__(256) void beam_cand_kernel(mtx_beam_step_args p, int chunks, int keep) {
  const int row = blockIdx.y, lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= chunks) return;                           // wave-uniform; no barrier in this kernel
  const int g = row / p.beams, b = row - g * p.beams;
  const int32_t* st = p.state + (long)g * p.state_stride;
  if (st[MTX_BEAM_DONE] != 0) return;
  const int pos = st[MTX_BEAM_POS];
  if (pos < 0 || pos + 2 > p.max_len || pos + 2 > p.max_length) return;      // beam_final_kernel ends such a group
  const float* lse = reinterpret_cast<const float*>(p.scratch) + 2L * row;
  const float m = lse[0], ls = lse[1];
  const float rs = reinterpret_cast<const float*>(st)[MTX_BEAM_RSCORE + b];
  const float* x = p.logits + (long)row * p.ld_logits;
  const int base = chunk * MTX_BEAM_CHUNK;
  float v[BEAM_PER_LANE];
#pragma unroll
  for (int e = 0; e < BEAM_PER_LANE; ++e) {
    const int t = base + e * 64 + lane;
    v[e] = t < p.vocab ? (beam_clean(x[t]) - m) - ls : 0.f;
  }
  // the n-gram ban: token seq[i + n - 1] wherever seq[i .. i + n - 2] equals the last n - 1 tokens
  const int n = p.ngram, len = pos + 1;
  if (n > 0 && len + 1 >= n) {
    const int32_t* seq = st + MTX_BEAM_RUNNING(p.beams, p.max_len) + (long)b * p.max_len;
    for (int i = 0; i + n <= len; ++i) {
      bool same = true;
      for (int k = 0; k + 1 < n; ++k) same = same && seq[i + k] == seq[len + 1 - n + k];
      const int t = seq[i + n - 1];
      if (same && t >= base && t < base + MTX_BEAM_CHUNK) {
#pragma unroll
        for (int e = 0; e < BEAM_PER_LANE; ++e) v[e] = t == base + e * 64 + lane ? -INFINITY : v[e];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < BEAM_PER_LANE; ++e) v[e] = v[e] + rs;
  // the chunk's best `keep` in selection order; the position is the flat index beam * vocab + token
  float* rec = reinterpret_cast<float*>(p.scratch) + 2L * p.groups * p.beams + 2L * ((long)row * chunks + chunk) * keep;
  float pv = INFINITY;
  int pi = -1;
  for (int k = 0; k < keep; ++k) {
    float bv = 0.f;
    int bi = -1;
#pragma unroll
    for (int e = 0; e < BEAM_PER_LANE; ++e) {
      const int t = base + e * 64 + lane;
      beam_take(bv, bi, v[e], t < p.vocab ? b * p.vocab + t : -1, pv, pi);
    }
    beam_wave_best(bv, bi);
    if (lane == 0) { rec[2 * k] = bv; reinterpret_cast<int*>(rec)[2 * k + 1] = bi; }
    pv = bv; pi = bi;
    if (bi < 0) {                                        // the chunk is exhausted: the remaining records are empty
      for (int k2 = k + 1 + lane; k2 < keep; k2 += 64) reinterpret_cast<int*>(rec)[2 * k2 + 1] = -1;
      break;
    }
  }
}

__global__ __launch_bounds__(64) void beam_final_kernel(mtx_beam_step_args p, int chunks, int keep) {
  __shared__ float top_v[BEAM_KEEP_MAX];
  __shared__ int top_i[BEAM_KEEP_MAX];
  __shared__ int s_beam[BEAM_KEEP_MAX], s_tok[BEAM_KEEP_MAX];
  __shared__ int s_nxt[MTX_BEAM_MAX], s_pick[MTX_BEAM_MAX], s_flen[MTX_BEAM_MAX], s_go;
  const int g = blockIdx.x, lane = threadIdx.x;
  const int B = p.beams, V = p.vocab, L = p.max_len;
  int32_t* st = p.state + (long)g * p.state_stride;
  float* stf = reinterpret_cast<float*>(st);
  if (st[MTX_BEAM_DONE] != 0) return;                    // a finished group changes nothing
  const int pos = st[MTX_BEAM_POS];
  const float* lse = reinterpret_cast<const float*>(p.scratch) + 2L * g * B;
  bool bad = pos < 0 || pos + 2 > L || pos + 2 > p.max_length;
  for (int b = 0; b < B && !bad; ++b) bad = !(lse[2 * b] > -INFINITY && lse[2 * b] < INFINITY);
  if (bad) { if (lane == 0) st[MTX_BEAM_DONE] = 2; return; }
  const int cur_len = pos + 1;
  // ---- the top `keep` of the group's records
  const float* rec = reinterpret_cast<const float*>(p.scratch) + 2L * p.groups * B + 2L * (long)g * B * chunks * keep;
  const int n_rec = B * chunks * keep;
  float pv = INFINITY;
  int pi = -1;
  for (int k = 0; k < keep; ++k) {
    float bv = 0.f;
    int bi = -1;
    for (int i = lane; i < n_rec; i += 64) beam_take(bv, bi, rec[2 * i], reinterpret_cast<const int*>(rec)[2 * i + 1], pv, pi);
    beam_wave_best(bv, bi);
    if (lane == 0) { top_v[k] = bv; top_i[k] = bi; }
    pv = bv; pi = bi;
  }
  __syncthreads();
  int32_t* run = st + MTX_BEAM_RUNNING(B, L);
  int32_t* fin = st + MTX_BEAM_FIN(B, L);
  int32_t* stage = st + MTX_BEAM_STAGE(B, L);
  int32_t* src = st + MTX_BEAM_SRC(B, L);
  // ---- the iteration's decisions, by one lane in beam_search's order
  if (lane == 0) {
    float masked[BEAM_KEEP_MAX], sc[BEAM_KEEP_MAX];
    bool hits[BEAM_KEEP_MAX];
    bool all_hits = true, all_done = true;
    for (int b = 0; b < B; ++b) all_done = all_done && st[MTX_BEAM_FDONE + b] != 0;
    const bool unsat = st[MTX_BEAM_UNSAT] != 0;
    const float full = (all_done && p.early == 1) ? 1.f : 0.f;
    const float div = p.len_pow[cur_len - 1];            // (cur_len + 1 - 1) ** length_penalty
    for (int i = 0; i < keep; ++i) {
      int idx = top_i[i];
      idx = idx < 0 ? 0 : idx;                           // (beams * vocab >= keep: every round found an entry)
      const int bm = idx / V, t = idx - bm * V;
      s_beam[i] = bm; s_tok[i] = t;
      bool hit = cur_len + 1 >= p.max_length;
      for (int e = 0; e < p.n_eos; ++e) hit = hit || t == p.eos[e];
      hits[i] = hit;
      all_hits = all_hits && hit;
      masked[i] = top_v[i] + (hit ? 1.f : 0.f) * -1.0e9f;
      const bool just = hit && i < B;
      float s = top_v[i] / div;
      s = s + full * -1.0e9f;
      s = s + (unsat ? 0.f : 1.f) * -1.0e9f;
      s = s + (just ? 0.f : 1.f) * -1.0e9f;
      sc[i] = s;
    }
    // the running beams of the next step: the best B of `masked`, value then rank
    float new_rs[MTX_BEAM_MAX];
    {
      float qv = INFINITY;
      int qi = -1;
      for (int r = 0; r < B; ++r) {
        float bv = 0.f;
        int bi = -1;
        for (int i = 0; i < keep; ++i) beam_take(bv, bi, masked[i], i, qv, qi);
        s_nxt[r] = bi; new_rs[r] = bv;
        qv = bv; qi = bi;
      }
    }
    // the finished set: the best B of [finished | candidates], value then position
    float new_fs[MTX_BEAM_MAX];
    int new_fd[MTX_BEAM_MAX];
    {
      float qv = INFINITY;
      int qi = -1;
      for (int r = 0; r < B; ++r) {
        float bv = 0.f;
        int bi = -1;
        for (int i = 0; i < B; ++i) beam_take(bv, bi, stf[MTX_BEAM_FSCORE + i], i, qv, qi);
        for (int i = 0; i < keep; ++i) beam_take(bv, bi, sc[i], B + i, qv, qi);
        s_pick[r] = bi; new_fs[r] = bv;
        if (bi < B) {
          int fl = st[MTX_BEAM_FLEN + bi];
          new_fd[r] = st[MTX_BEAM_FDONE + bi] != 0;
          s_flen[r] = fl < 1 ? 1 : (fl > L ? L : fl);
        } else {
          new_fd[r] = (hits[bi - B] && bi - B < B) ? 1 : 0;
          s_flen[r] = cur_len + 1;
        }
        qv = bv; qi = bi;
      }
    }
    bool all_done2 = true;
    float min_fs = new_fs[0];
    for (int r = 0; r < B; ++r) {
      stf[MTX_BEAM_RSCORE + r] = new_rs[r];
      stf[MTX_BEAM_FSCORE + r] = new_fs[r];
      st[MTX_BEAM_FDONE + r] = new_fd[r];
      st[MTX_BEAM_FLEN + r] = s_flen[r];
      st[MTX_BEAM_PARENT + r] = s_beam[s_nxt[r]];
      all_done2 = all_done2 && new_fd[r];
      min_fs = new_fs[r] < min_fs ? new_fs[r] : min_fs;
    }
    // can a running beam still beat the worst finished one?  (cur_len has advanced by one)
    const int best_len = (p.early == 2 && p.lp_positive) ? p.max_length - 1 : cur_len;
    const float best_running = new_rs[0] / p.len_pow[best_len - 1];
    bool any = false;
    for (int r = 0; r < B; ++r) any = any || best_running > (new_fd[r] ? min_fs : -1.0e9f);
    const bool unsat2 = unsat && any;
    st[MTX_BEAM_UNSAT] = unsat2 ? 1 : 0;
    s_go = (unsat2 && !(all_done2 && p.early == 1) && !all_hits) ? 1 : 0;
  }
  __syncthreads();
  // ---- the finished hypotheses (from the OLD running rows), through the staging area
  for (int r = 0; r < B; ++r) {
    const int pk = s_pick[r], n = s_flen[r];
    if (pk < B) {
      for (int j = lane; j < n; j += 64) stage[(long)r * L + j] = fin[(long)pk * L + j];
    } else {
      const int32_t* from = run + (long)s_beam[pk - B] * L;
      for (int j = lane; j < n; j += 64) stage[(long)r * L + j] = j < cur_len ? from[j] : s_tok[pk - B];
    }
  }
  __syncthreads();
  for (int r = 0; r < B; ++r)
    for (int j = lane; j < s_flen[r]; j += 64) fin[(long)r * L + j] = stage[(long)r * L + j];
  __syncthreads();
  // ---- the running rows reordered by parent and extended
  for (int r = 0; r < B; ++r) {
    const int c = s_nxt[r];
    const int32_t* from = run + (long)s_beam[c] * L;
    for (int j = lane; j <= cur_len; j += 64) stage[(long)r * L + j] = j < cur_len ? from[j] : s_tok[c];
  }
  __syncthreads();
  for (int r = 0; r < B; ++r)
    for (int j = lane; j <= cur_len; j += 64) run[(long)r * L + j] = stage[(long)r * L + j];
  // ---- the ancestry table: one lane owns a whole position's B entries
  for (int j = lane; j <= pos; j += 64) {
    int old[MTX_BEAM_MAX];
    for (int r = 0; r < B; ++r) {
      const int s = src[(long)j * B + r];
      old[r] = j == pos ? r : (s < 0 ? 0 : (s >= B ? B - 1 : s));
    }
    for (int r = 0; r < B; ++r) src[(long)j * B + r] = old[s_beam[s_nxt[r]]];
  }
  if (lane < B) {
    p.tok_idx[g * B + lane] = s_tok[s_nxt[lane]];
    p.pos_idx[g * B + lane] = pos + 1;
  }
  __syncthreads();
  if (!s_go) {
    const int n = s_flen[0];
    for (int j = lane; j < n; j += 64) st[MTX_BEAM_OUT + j] = fin[j];
  }
  if (lane == 0) {
    st[MTX_BEAM_POS] = pos + 1;
    if (!s_go) { st[MTX_BEAM_OUT_LEN] = s_flen[0]; st[MTX_BEAM_DONE] = 1; }
  }
}

int beam_step_launch(const mtx_beam_step_args* a, void* stream, const char** err) {
  if (!a->logits || !a->state || !a->tok_idx || !a->pos_idx || !a->len_pow || !a->scratch) { *err = "beam_step: null operand"; return MTX_ERR_INVALID; }
  if (a->groups < 1 || a->groups > MTX_SLOTS_MAX || a->beams < 1 || a->beams > MTX_BEAM_MAX) { *err = "beam_step: needs 1 <= groups <= MTX_SLOTS_MAX, 1 <= beams <= 8"; return MTX_ERR_INVALID; }
  if (a->n_eos < 1 || a->n_eos > 4 || a->vocab < 2 || a->ld_logits < a->vocab) { *err = "beam_step: needs 1 <= n_eos <= 4, vocab >= 2, ld_logits >= vocab"; return MTX_ERR_INVALID; }
  const int keep = (a->n_eos + 1 > 2 ? a->n_eos + 1 : 2) * a->beams;
  if ((long)a->beams * a->vocab < keep || (long)a->beams * a->vocab > INT_MAX) { *err = "beam_step: beams * vocab must hold max(2, 1 + n_eos) * beams candidates and fit 31 bits"; return MTX_ERR_INVALID; }
  if (a->max_len < 2 || a->max_length < 2 || a->max_length > a->max_len) { *err = "beam_step: needs 2 <= max_length <= max_len"; return MTX_ERR_INVALID; }
  if (a->early < 0 || a->early > 2 || a->ngram < 0) { *err = "beam_step: early must be 0, 1 or 2 and ngram >= 0"; return MTX_ERR_INVALID; }
  if (a->state_stride < (int64_t)MTX_BEAM_STATE_WORDS(a->beams, a->max_len)) { *err = "beam_step: state_stride below MTX_BEAM_STATE_WORDS(beams, max_len)"; return MTX_ERR_INVALID; }
  const int rows = a->groups * a->beams;
  const int chunks = (a->vocab + MTX_BEAM_CHUNK - 1) / MTX_BEAM_CHUNK;
  MTX_LAUNCH(beam_lse_kernel, dim3((unsigned)rows), dim3(256), 0, stream, *a);
  MTX_LAUNCH(beam_cand_kernel, dim3((unsigned)((chunks + 3) / 4), (unsigned)rows), dim3(256), 0, stream, *a, chunks, keep);
  MTX_LAUNCH(beam_final_kernel, dim3((unsigned)a->groups), dim3(64), 0, stream, *a, chunks, keep);
  return MTX_OK;
}

}  // namespace mtx
