// textcolor.hip — pixel half of the rendered-text colour probe of the outside-speech-bubble stage on gfx950 (include/mtx_hip.h
// mtx_textcolor_args; reference core/outside_text_processor.py:1096-1165).
//
// The reference runs, per text region on the CPU: cv2 RGB -> Lab of the crop, the distance map to the border ring's median, its 95th
// percentile, a contrast mask, a 3x3 close and a 2x2 erode, contours, and the median RGB under the cleaned mask.  Here all regions of a page
// go through each launch, restricted to their own crops like the cleaning chain of clean.hip: one thread per crop pixel, coalesced along
// x, the page read in place.  Integer work throughout, so every result is exact:
//   DIST  d2 per pixel + the order statistics the percentile needs (coarse 768-bin histogram of d2 >> 8, then a 256-bin histogram of the
//         low byte inside the bins that hold the wanted ranks: LDS atomics per block, one global add per non-empty bin)
//   MASK  threshold, close, erode — each thread recomputes its 6 x 6 neighbourhood from d2 as row bit masks (no intermediate planes)
//   HIST  R / G / B histograms under the mask the host's contour step filled
#include "mtx_device.h"
#include "lab8.h"

namespace mtx {

// crop pixel -> (region, x, y); returns false past the end of the crop
__device__ __forceinline__ bool tc_pixel(const mtx_textcolor_args& a, int& x, int& y, int& w, int& h, int& X, int& Y, long& o) {
  const int* r = a.rois + blockIdx.y * 4;
  w = r[2]; h = r[3];
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)w * h) return false;
  x = (int)(idx % w); y = (int)(idx / w);
  X = r[0] + x; Y = r[1] + y;
  o = a.offsets[blockIdx.y] + idx;
  return true;
}

// page pixel, black outside the page (PIL's crop pads with zeros)
__device__ __forceinline__ void tc_rgb(const mtx_textcolor_args& a, int X, int Y, int& r, int& g, int& b) {
  r = g = b = 0;
  if (X >= 0 && X < a.page_w && Y >= 0 && Y < a.page_h) {
    const unsigned char* px = reinterpret_cast<const unsigned char*>(a.page_rgb) + ((size_t)Y * a.page_w + X) * 3;
    r = px[0]; g = px[1]; b = px[2];
  }
}

__global__ __launch_bounds__(256) void tc_dist_kernel(mtx_textcolor_args a) {
  __shared__ int hist[768];
  for (int i = threadIdx.x; i < 768; i += 256) hist[i] = 0;
  __syncthreads();
  int x, y, w, h, X, Y; long o;
  if (tc_pixel(a, x, y, w, h, X, Y, o)) {
    int r, g, b, L, A, B;
    tc_rgb(a, X, Y, r, g, b);
    rgb_to_lab8(Lab8Tables{a.gamma_tab, a.cbrt_tab, a.lab_coef, a.cbrt_n}, r, g, b, L, A, B);
    const int* bg = a.bg_lab + blockIdx.y * 3;
    const int dl = L - bg[0], da = A - bg[1], db = B - bg[2];
    const int d = dl * dl + da * da + db * db;
    a.d2[o] = d;
    atomicAdd(&hist[d >> 8], 1);
  }
  __syncthreads();
  int* st = a.stats + (size_t)blockIdx.y * MTX_TC_STATS + MTX_TC_STAT_COARSE;
  for (int i = threadIdx.x; i < 768; i += 256)
    if (hist[i]) atomicAdd(st + i, hist[i]);
}

// per region: the coarse bin that holds each wanted rank, and the rank's position inside that bin
__global__ __launch_bounds__(256) void tc_select_coarse_kernel(mtx_textcolor_args a) {
  __shared__ int part[256], before[256];
  int* st = a.stats + (size_t)blockIdx.x * MTX_TC_STATS;
  const int t = threadIdx.x;
  const int c0 = st[MTX_TC_STAT_COARSE + 3 * t], c1 = st[MTX_TC_STAT_COARSE + 3 * t + 1], c2 = st[MTX_TC_STAT_COARSE + 3 * t + 2];
  part[t] = c0 + c1 + c2;
  __syncthreads();
  if (t == 0) {
    int s = 0;
    for (int i = 0; i < 256; ++i) { before[i] = s; s += part[i]; }
  }
  __syncthreads();
  const int lo = before[t], hi = lo + part[t];
  for (int j = 0; j < MTX_TC_RANKS; ++j) {
    const int rank = a.ranks[blockIdx.x * MTX_TC_RANKS + j];
    if (rank >= lo && rank < hi) {
      int r = rank - lo, bin = 3 * t;
      if (r >= c0) { r -= c0; ++bin; if (r >= c1) { r -= c1; ++bin; } }
      st[MTX_TC_STAT_SEL + 2 * j] = bin;
      st[MTX_TC_STAT_SEL + 2 * j + 1] = r;
    }
  }
}

// low-byte histograms inside the selected coarse bins (ranks ascend, so equal bins are neighbours: the first of a run owns the histogram)
__global__ __launch_bounds__(256) void tc_fine_kernel(mtx_textcolor_args a) {
  __shared__ int hist[MTX_TC_RANKS * 256];
  for (int i = threadIdx.x; i < MTX_TC_RANKS * 256; i += 256) hist[i] = 0;
  __syncthreads();
  int* st = a.stats + (size_t)blockIdx.y * MTX_TC_STATS;
  int x, y, w, h, X, Y; long o;
  if (tc_pixel(a, x, y, w, h, X, Y, o)) {
    const int d = a.d2[o], c = d >> 8;
    const int* sel = st + MTX_TC_STAT_SEL;
#pragma unroll
    for (int j = 0; j < MTX_TC_RANKS; ++j)
      if (sel[2 * j] == c && (j == 0 || sel[2 * j - 2] != c)) atomicAdd(&hist[j * 256 + (d & 255)], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < MTX_TC_RANKS * 256; i += 256)
    if (hist[i]) atomicAdd(st + MTX_TC_STAT_FINE + i, hist[i]);
}

__global__ __launch_bounds__(64) void tc_select_fine_kernel(mtx_textcolor_args a) {
  int* st = a.stats + (size_t)blockIdx.x * MTX_TC_STATS;
  const int j = threadIdx.x;
  if (j < MTX_TC_RANKS) {
    const int* sel = st + MTX_TC_STAT_SEL;
    int owner = j;
    while (owner > 0 && sel[2 * owner - 2] == sel[2 * j]) --owner;
    const int* fine = st + MTX_TC_STAT_FINE + owner * 256;
    const int r = sel[2 * j + 1];
    int s = 0, k = 0;
    for (; k < 255; ++k) { s += fine[k]; if (s > r) break; }
    st[MTX_TC_STAT_ORDER + j] = (sel[2 * j] << 8) | k;
  }
}

// contrast mask -> 3x3 close -> 2x2 erode (anchor (1, 1): offsets {-1, 0}).  Row j of the 6 x 6 window is crop row y - 3 + j, bit i is
// crop column x - 3 + i; `v` marks the pixels inside the crop, which alone take part in a maximum / minimum.
__global__ __launch_bounds__(256) void tc_mask_kernel(mtx_textcolor_args a) {
  int x, y, w, h, X, Y; long o;
  if (!tc_pixel(a, x, y, w, h, X, Y, o)) return;
  const long base = a.offsets[blockIdx.y];
  const int cut = a.cutoff[blockIdx.y];
  unsigned t[6], v[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int yy = y - 3 + j;
    unsigned tj = 0, vj = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const int xx = x - 3 + i;
      if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
        vj |= 1u << i;
        if (a.d2[base + (long)yy * w + xx] > cut) tj |= 1u << i;
      }
    }
    t[j] = tj; v[j] = vj;
  }
  unsigned e[6];                                     // dilated, rows 1..4 (bits 1..4 complete); outside the crop: neutral for the erosion
#pragma unroll
  for (int j = 1; j <= 4; ++j) {
    const unsigned r = t[j - 1] | t[j] | t[j + 1];
    e[j] = (r | (r << 1) | (r >> 1)) | ~v[j];
  }
  unsigned f = ~0u;                                  // closed, rows 2..3 (bits 2..3 complete), folded by the 2x2 erosion
#pragma unroll
  for (int j = 2; j <= 3; ++j) {
    const unsigned q = e[j - 1] & e[j] & e[j + 1];
    f &= (q & (q << 1) & (q >> 1)) | ~v[j];
  }
  a.mask[o] = ((f >> 2) & (f >> 3) & 1u) ? 255 : 0;
}

__global__ __launch_bounds__(256) void tc_hist_kernel(mtx_textcolor_args a) {
  __shared__ int hist[768];
  for (int i = threadIdx.x; i < 768; i += 256) hist[i] = 0;
  __syncthreads();
  int x, y, w, h, X, Y; long o;
  if (tc_pixel(a, x, y, w, h, X, Y, o) && a.mask[o]) {
    int r, g, b;
    tc_rgb(a, X, Y, r, g, b);
    atomicAdd(&hist[r], 1); atomicAdd(&hist[256 + g], 1); atomicAdd(&hist[512 + b], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 768; i += 256)
    if (hist[i]) atomicAdd(a.hist + (size_t)blockIdx.y * 768 + i, hist[i]);
}

static void tc_zero(int* p, size_t words, void* stream) {
#ifdef MTX_EMU
  memset(p, 0, words * sizeof(int));
#else
  zero_words_async(p, words * sizeof(int), stream);        // a kernel, not a memset node (mtx_device.h)
#endif
}

int textcolor_launch(const mtx_textcolor_args* a, void* stream, const char** err) {
  if (!a->rois || !a->offsets) { *err = "text_color: null rois / offsets"; return MTX_ERR_INVALID; }
  if (a->n < 1 || a->max_pixels < 1) return MTX_OK;
  if (a->n > 65535 || a->page_h < 1 || a->page_w < 1) { *err = "text_color: 1 .. 65535 regions of a non-empty page"; return MTX_ERR_INVALID; }
  const dim3 grid((unsigned)((a->max_pixels + 255) / 256), (unsigned)a->n);
  switch (a->phase) {
    case MTX_TC_DIST:
      if (!a->page_rgb || !a->bg_lab || !a->ranks || !a->d2 || !a->stats || !a->gamma_tab || !a->cbrt_tab || !a->lab_coef || a->cbrt_n < 1) {
        *err = "text_color (DIST): page / bg_lab / ranks / d2 / stats / tables"; return MTX_ERR_INVALID;
      }
      tc_zero(a->stats, (size_t)a->n * MTX_TC_STATS, stream);
      MTX_LAUNCH(tc_dist_kernel, grid, dim3(256), 0, stream, *a);
      MTX_LAUNCH(tc_select_coarse_kernel, dim3((unsigned)a->n), dim3(256), 0, stream, *a);
      MTX_LAUNCH(tc_fine_kernel, grid, dim3(256), 0, stream, *a);
      MTX_LAUNCH(tc_select_fine_kernel, dim3((unsigned)a->n), dim3(64), 0, stream, *a);
      return MTX_OK;
    case MTX_TC_MASK:
      if (!a->d2 || !a->cutoff || !a->mask) { *err = "text_color (MASK): d2 / cutoff / mask"; return MTX_ERR_INVALID; }
      MTX_LAUNCH(tc_mask_kernel, grid, dim3(256), 0, stream, *a);
      return MTX_OK;
    case MTX_TC_HIST:
      if (!a->page_rgb || !a->mask || !a->hist) { *err = "text_color (HIST): page / mask / hist"; return MTX_ERR_INVALID; }
      tc_zero(a->hist, (size_t)a->n * 768, stream);
      MTX_LAUNCH(tc_hist_kernel, grid, dim3(256), 0, stream, *a);
      return MTX_OK;
    default:
      *err = "text_color: unknown phase"; return MTX_ERR_INVALID;
  }
}

}  // namespace mtx
