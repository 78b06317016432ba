// dettail.hip — the tail of a YOLO-family detector call on the device (include/mtx_hip.h, mtx_det_tail_args): score filter, class-aware greedy
// NMS and the rescale to page coordinates, in the fp32 operations and the order of core/ml/yolo.py `YoloSegHip._finish` / `nms_xyxy`.
// Four launches, all of fixed size, every count read from device memory:
//   det_compact_kernel   grid (ceil(anchors / 256)): a thread owns a row; rows with score > conf are appended (atomicAdd on an int) as
//                        (sort key, class) records.  The append order varies from run to run; nothing after the sort depends on it
//   det_sort_kernel      one workgroup: bitonic sort of the keys in LDS — (score bits descending, row ascending), all keys distinct — then
//                        the sorted records: offset corners, area, score, class, row.  Resets the counter for the next call
//   det_pairs_kernel     grid (CAP / 64, CAP / 64), upper triangle: a lane owns row i and builds the 64-bit word "which j of this column block,
//                        j > i, would i suppress"
//   det_scan_kernel      one wave: walks the rows in order, 64 at a time — the diagonal word decides inside a block, the kept rows' other words
//                        are OR-ed into the removed set afterwards, so no load depends on a decision — and writes boxes, scores, classes,
//                        row indices and the mask coefficients of the kept rows
// Suppression is an exact threshold decision: no expression here may be contracted into an FMA or reassociated, and `/` is the correctly
// rounded division (hipcc's default for fp32; the simulator's clang build computes IEEE fp32 too).
#include "mtx_device.h"

#pragma clang fp contract(off)

namespace mtx {

constexpr int DT_CAP = MTX_DET_TAIL_CAP;
constexpr int DT_WORDS = DT_CAP / 64;            // 64-bit words per row of the suppression matrix
constexpr int DT_KEEP = MTX_DET_TAIL_MAX_KEEP;
static_assert(DT_WORDS <= 64 && (DT_CAP & (DT_CAP - 1)) == 0, "the scan keeps one removed-word per lane; the sort needs a power of two");

struct DetWs {
  int* hdr;                        // [0] append counter, [1] n (sorted candidates), [2] overflow
  unsigned long long* keys;        // appended: (~orderable score bits) << 32 | row
  int* ccls;                       // appended: class of the record in the same slot
  f32x4* sbox;                     // sorted: offset corners x + cls * 7680
  float* sarea; float* sscore; int* scls; int* srow;
  unsigned long long* pairs;       // [CAP][DT_WORDS], only words at or right of the diagonal of rows < n are ever written or read
};
__device__ __forceinline__ DetWs det_ws(void* workspace) {
  unsigned char* b = reinterpret_cast<unsigned char*>(workspace);
  DetWs w;
  w.hdr = reinterpret_cast<int*>(b); b += 16;
  w.keys = reinterpret_cast<unsigned long long*>(b); b += (size_t)DT_CAP * 8;
  w.ccls = reinterpret_cast<int*>(b); b += (size_t)DT_CAP * 4;
  w.sbox = reinterpret_cast<f32x4*>(b); b += (size_t)DT_CAP * 16;
  w.sarea = reinterpret_cast<float*>(b); b += (size_t)DT_CAP * 4;
  w.sscore = reinterpret_cast<float*>(b); b += (size_t)DT_CAP * 4;
  w.scls = reinterpret_cast<int*>(b); b += (size_t)DT_CAP * 4;
  w.srow = reinterpret_cast<int*>(b); b += (size_t)DT_CAP * 4;
  w.pairs = reinterpret_cast<unsigned long long*>(b);
  return w;
}

// fp32 bits -> unsigned that orders like the value (negative values below positive ones)
__device__ __forceinline__ unsigned det_orderable(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float det_from_orderable(unsigned o) {
  return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__global__ __launch_bounds__(256) void det_compact_kernel(mtx_det_tail_args p) {
  const int row = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (row >= p.anchors) return;
  const float conf = reinterpret_cast<const float*>(p.params)[MTX_DET_TAIL_P_CONF];
  const float* x = p.decoded + (long)row * p.ld + 4;
  float best = x[0];
  int cls = 0;
  bool nan = best != best;
  for (int c = 1; c < p.nc; ++c) {
    const float v = x[c];
    nan = nan || v != v;
    if (v > best) { best = v; cls = c; }               // strictly: the lowest class that attains the maximum
  }
  if (nan || !(best > conf)) return;
  const DetWs w = det_ws(p.workspace);
  const int slot = atomicAdd(w.hdr, 1);
  if (slot >= DT_CAP) return;                          // the counter keeps counting: det_sort_kernel reports the overflow
  w.keys[slot] = ((unsigned long long)(~det_orderable(best)) << 32) | (unsigned)row;
  w.ccls[slot] = cls;
}

__global__ __launch_bounds__(512) void det_sort_kernel(mtx_det_tail_args p) {
  __shared__ unsigned long long s_key[DT_CAP];
  __shared__ int s_slot[DT_CAP];
  const int tid = threadIdx.x;
  const DetWs w = det_ws(p.workspace);
  int32_t* out = reinterpret_cast<int32_t*>(p.out);
  const int count = w.hdr[0];
  const int max_det = reinterpret_cast<const int32_t*>(p.params)[MTX_DET_TAIL_P_MAX_DET];
  const bool overflow = count > DT_CAP || max_det < 1 || max_det > p.max_keep;
  const int n = overflow ? 0 : count;
  __syncthreads();                                     // every thread has read the counter before it is reset
  if (tid == 0) {
    w.hdr[0] = 0; w.hdr[1] = n; w.hdr[2] = overflow ? 1 : 0;
    out[MTX_DET_TAIL_KEPT] = 0; out[MTX_DET_TAIL_CAND] = count; out[MTX_DET_TAIL_OVERFLOW] = overflow ? 1 : 0; out[3] = 0;
  }
  if (n == 0) return;                                  // workgroup-uniform
  int np2 = 2;
  while (np2 < n) np2 <<= 1;                           // <= DT_CAP
  for (int i = tid; i < np2; i += 512) { s_key[i] = i < n ? w.keys[i] : ~0ull; s_slot[i] = i; }
  __syncthreads();
  for (int k = 2; k <= np2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (tid < (np2 >> 1)) {
        const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), q = i + j;
        const unsigned long long a = s_key[i], b = s_key[q];
        if ((a > b) == ((i & k) == 0)) {
          s_key[i] = b; s_key[q] = a;
          const int t = s_slot[i]; s_slot[i] = s_slot[q]; s_slot[q] = t;
        }
      }
      __syncthreads();
    }
  for (int i = tid; i < n; i += 512) {
    const unsigned long long key = s_key[i];
    const int row = (int)(unsigned)(key & 0xffffffffull);
    const int cls = w.ccls[s_slot[i]];
    const float* d = p.decoded + (long)row * p.ld;
    const float off = (float)cls * 7680.0f;
    const float x1 = d[0] + off, y1 = d[1] + off, x2 = d[2] + off, y2 = d[3] + off;
    w.sbox[i] = f32x4{x1, y1, x2, y2};
    w.sarea[i] = (x2 - x1) * (y2 - y1);
    w.sscore[i] = det_from_orderable(~(unsigned)(key >> 32));
    w.scls[i] = cls;
    w.srow[i] = row;
  }
}

// would a kept box a suppress b?  nms_xyxy's expressions in its order; a NaN (0 / 0 of two empty boxes) compares false
__device__ __forceinline__ bool det_suppresses(const f32x4& a, float area_a, const f32x4& b, float area_b, float thr) {
  const float wx = (a[2] < b[2] ? a[2] : b[2]) - (a[0] > b[0] ? a[0] : b[0]);
  const float wy = (a[3] < b[3] ? a[3] : b[3]) - (a[1] > b[1] ? a[1] : b[1]);
  const float iw = wx > 0.f ? wx : 0.f, ih = wy > 0.f ? wy : 0.f;
  const float inter = iw * ih;
  const float iou = inter / ((area_a + area_b) - inter);
  return iou > thr;
}

__global__ __launch_bounds__(64) void det_pairs_kernel(mtx_det_tail_args p) {
  __shared__ f32x4 s_box[64];
  __shared__ float s_area[64];
  const int lane = threadIdx.x, bw = blockIdx.x, br = blockIdx.y;
  if (bw < br) return;                                 // below the diagonal
  const DetWs w = det_ws(p.workspace);
  const int n = w.hdr[1];
  if (br * 64 >= n || bw * 64 >= n) return;            // workgroup-uniform
  const float thr = reinterpret_cast<const float*>(p.params)[MTX_DET_TAIL_P_IOU];
  const int j0 = bw * 64, i = br * 64 + lane;
  if (j0 + lane < n) { s_box[lane] = w.sbox[j0 + lane]; s_area[lane] = w.sarea[j0 + lane]; }
  __syncthreads();
  if (i >= n) return;
  const f32x4 a = w.sbox[i];
  const float area_a = w.sarea[i];
  const int jn = n - j0 < 64 ? n - j0 : 64;
  unsigned long long word = 0ull;
  for (int t = 0; t < jn; ++t)
    if (j0 + t > i && det_suppresses(a, area_a, s_box[t], s_area[t], thr)) word |= 1ull << t;
  w.pairs[(long)i * DT_WORDS + bw] = word;
}

// np.clip's element rule: min(max(x, lo), hi) with a NaN passed through
__device__ __forceinline__ float det_clip(float v, float lo, float hi) {
  v = (v > lo || v != v) ? v : lo;
  return (v < hi || v != v) ? v : hi;
}

template <typename T>
__global__ __launch_bounds__(64) void det_scan_kernel(mtx_det_tail_args p) {
  __shared__ unsigned long long s_words[DT_WORDS][65];        // [word][row of the block]; 65: the lanes of the OR pass hit different banks
  __shared__ int s_kept[DT_KEEP];
  const int lane = threadIdx.x;
  const DetWs w = det_ws(p.workspace);
  if (w.hdr[2]) return;                                // overflow: nothing else is written
  int32_t* out = reinterpret_cast<int32_t*>(p.out);
  const int32_t* pi = reinterpret_cast<const int32_t*>(p.params);
  const float* pf = reinterpret_cast<const float*>(p.params);
  const int n = w.hdr[1];
  const int max_det = pi[MTX_DET_TAIL_P_MAX_DET];       // 1 .. max_keep <= DT_KEEP (det_sort_kernel reports anything else as overflow)
  const int nw = (n + 63) >> 6;
  unsigned long long rem = 0ull;                       // lane l < nw: the removed bits of word l
  int k = 0;
  for (int b = 0; b < nw && k < max_det; ++b) {
    const int i = b * 64 + lane;
#pragma unroll
    for (int c = 0; c < DT_WORDS; ++c)
      if (c >= b && c < nw) s_words[c][lane] = i < n ? w.pairs[(long)i * DT_WORDS + c] : 0ull;
    __syncthreads();
    unsigned long long cur = __shfl(rem, b, 64);
    unsigned long long keptbits = 0ull;
    const int lim = n - b * 64 < 64 ? n - b * 64 : 64;
    for (int t = 0; t < lim && k < max_det; ++t)       // every lane walks the block alike: `cur`, `keptbits` and k are wave-uniform
      if (!((cur >> t) & 1ull)) {
        keptbits |= 1ull << t;
        cur |= s_words[b][t];
        if (lane == 0) s_kept[k] = b * 64 + t;
        ++k;
      }
    if (lane > b && lane < nw)
      for (int t = 0; t < lim; ++t)
        if ((keptbits >> t) & 1ull) rem |= s_words[lane][t];
    __syncthreads();
  }
  const int kept = k;
  if (lane == 0) out[MTX_DET_TAIL_KEPT] = kept;
  const float gain = pf[MTX_DET_TAIL_P_GAIN], padw = pf[MTX_DET_TAIL_P_PADW], padh = pf[MTX_DET_TAIL_P_PADH];
  const float w0 = (float)pi[MTX_DET_TAIL_P_W0], h0 = (float)pi[MTX_DET_TAIL_P_H0];
  const int mk = p.max_keep;
  float* boxes = reinterpret_cast<float*>(out + MTX_DET_TAIL_BOXES);
  float* conf = reinterpret_cast<float*>(out + MTX_DET_TAIL_CONF(mk));
  float* cls = reinterpret_cast<float*>(out + MTX_DET_TAIL_CLS(mk));
  int32_t* rows = out + MTX_DET_TAIL_ROWS(mk);
  for (int r = lane; r < mk; r += 64) {
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, sc = 0.f, cl = 0.f;
    int row = 0;
    if (r < kept) {
      const int i = s_kept[r];
      row = w.srow[i];
      const float* d = p.decoded + (long)row * p.ld;
      x1 = det_clip((d[0] - padw) / gain, 0.f, w0);
      y1 = det_clip((d[1] - padh) / gain, 0.f, h0);
      x2 = det_clip((d[2] - padw) / gain, 0.f, w0);
      y2 = det_clip((d[3] - padh) / gain, 0.f, h0);
      sc = w.sscore[i];
      cl = (float)w.scls[i];
    }
    boxes[4 * r + 0] = x1; boxes[4 * r + 1] = y1; boxes[4 * r + 2] = x2; boxes[4 * r + 3] = y2;
    conf[r] = sc; cls[r] = cl; rows[r] = row;
  }
  const int nm = p.nm;
  if (nm <= 0) return;
  // mask coefficients: nm <= 64 -> 64 / nm rows per pass, a lane keeps its column; wider rows -> one row per pass, columns strided
  T* coef = reinterpret_cast<T*>(p.coef);
  const int per = nm <= 64 ? 64 / nm : 1;
  const int sub = nm <= 64 ? lane / nm : 0, c0 = nm <= 64 ? lane - sub * nm : lane, cstep = nm <= 64 ? nm : 64;
  if (sub >= per) return;
  for (int r = sub; r < mk; r += per) {
    const float* d = r < kept ? p.decoded + (long)w.srow[s_kept[r]] * p.ld + 4 + p.nc : nullptr;
    for (int c = c0; c < nm; c += cstep) coef[(long)r * nm + c] = d ? (T)d[c] : (T)0.f;      // a plain cast: round to nearest even, no saturation
  }
}

int det_tail_launch(const mtx_det_tail_args* a, void* stream, const char** err) {
  if (!a->decoded || !a->params || !a->out || !a->workspace) { *err = "detector_tail: null operand"; return MTX_ERR_INVALID; }
  if (a->anchors < 1 || a->nc < 1 || a->nm < 0 || a->ld < 4 + (int64_t)a->nc + a->nm) { *err = "detector_tail: needs anchors >= 1, nc >= 1, nm >= 0, ld >= 4 + nc + nm"; return MTX_ERR_INVALID; }
  if (a->max_keep < 1 || a->max_keep > MTX_DET_TAIL_MAX_KEEP) { *err = "detector_tail: max_keep outside 1 .. MTX_DET_TAIL_MAX_KEEP"; return MTX_ERR_INVALID; }
  if (a->workspace_bytes < (int64_t)MTX_DET_TAIL_WS_BYTES || (reinterpret_cast<uintptr_t>(a->workspace) & 15)) { *err = "detector_tail: workspace below MTX_DET_TAIL_WS_BYTES or not 16-byte aligned"; return MTX_ERR_INVALID; }
  if (a->nm > 0 && (!a->coef || (a->dtype != MTX_BF16 && a->dtype != MTX_F16))) { *err = "detector_tail: mask coefficients need a bf16 / f16 coef buffer"; return MTX_ERR_INVALID; }
  MTX_LAUNCH(det_compact_kernel, dim3((unsigned)((a->anchors + 255) / 256)), dim3(256), 0, stream, *a);
  MTX_LAUNCH(det_sort_kernel, dim3(1), dim3(512), 0, stream, *a);
  MTX_LAUNCH(det_pairs_kernel, dim3((unsigned)DT_WORDS, (unsigned)DT_WORDS), dim3(64), 0, stream, *a);
  if (!MTX_LAUNCH_T(a->nm > 0 ? a->dtype : MTX_F16, det_scan_kernel, dim3(1), dim3(64), stream, *a)) { *err = "detector_tail: dtype"; return MTX_ERR_INVALID; }
  return MTX_OK;
}

}  // namespace mtx
