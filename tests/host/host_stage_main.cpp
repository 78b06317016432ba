// host_stage_main.cpp — stand-alone driver of the host half of the page stage (csrc/host_contours.cpp, csrc/host_png.cpp) for
// tests/test_host_sanitized.py, which builds it with -fsanitize=address,undefined and runs it as a child process.
//
//   host_stage_main <case file> <result file>
//
// Case file: records, little endian, each `int32 op` followed by the op's fields (below) and its payload bytes.  Every input and
// output buffer is a heap block of exactly the size the callee may touch, so a read or write past it is an AddressSanitizer report.
// Output blocks are pre-filled with 0xAB where the test wants to see what was left alone.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../include/mtx_hip.h"

namespace {

struct Reader {
  FILE* f;
  template <class T> T get() {
    T v;
    if (fread(&v, sizeof v, 1, f) != 1) { fprintf(stderr, "case file: truncated record\n"); exit(3); }
    return v;
  }
  std::unique_ptr<uint8_t[]> bytes(size_t n) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
    if (n && fread(p.get(), 1, n, f) != n) { fprintf(stderr, "case file: truncated payload\n"); exit(3); }
    return p;
  }
};

struct Writer {
  FILE* f;
  template <class T> void put(T v) { if (fwrite(&v, sizeof v, 1, f) != 1) exit(4); }
  void bytes(const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) exit(4); }
};

enum { OP_TEXT_MASK = 1, OP_FILL = 2, OP_OUTLINE = 3, OP_CHAMFER = 4, OP_PNG = 5 };

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]); return 2; }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) { fprintf(stderr, "cannot open the case or the result file\n"); return 2; }
  Reader r{in};
  Writer w{out};
  int records = 0;
  for (;;) {
    int32_t op;
    if (fread(&op, sizeof op, 1, in) != 1) break;
    ++records;
    switch (op) {
      case OP_TEXT_MASK: {                      // w h ox oy page_w page_h, double min_area, thr[w*h], eroded[w*h] -> rc, final[w*h], bbox[4]
        const int W = r.get<int32_t>(), H = r.get<int32_t>(), ox = r.get<int32_t>(), oy = r.get<int32_t>(), pw = r.get<int32_t>(), ph = r.get<int32_t>();
        const double min_area = r.get<double>();
        const size_t n = (size_t)W * H;
        auto thr = r.bytes(n), ero = r.bytes(n);
        std::unique_ptr<uint8_t[]> fin(new uint8_t[n]);
        memset(fin.get(), 0xAB, n);
        std::unique_ptr<int[]> bbox(new int[4]);
        for (int i = 0; i < 4; ++i) bbox[i] = -77;
        const int rc = mtx_host_text_mask(thr.get(), ero.get(), W, H, ox, oy, pw, ph, min_area, fin.get(), bbox.get());
        w.put<int32_t>(rc); w.bytes(fin.get(), n); w.bytes(bbox.get(), 4 * sizeof(int));
        break;
      }
      case OP_FILL: {                           // w h, double min_area, mask[w*h] -> rc, out[w*h]
        const int W = r.get<int32_t>(), H = r.get<int32_t>();
        const double min_area = r.get<double>();
        const size_t n = (size_t)W * H;
        auto mask = r.bytes(n);
        std::unique_ptr<uint8_t[]> o(new uint8_t[n]);
        memset(o.get(), 0xAB, n);
        const int rc = mtx_host_fill_components(mask.get(), W, H, min_area, o.get());
        w.put<int32_t>(rc); w.bytes(o.get(), n);
        break;
      }
      case OP_OUTLINE: {                        // w h cap, mask[w*h] -> rc, xy[2*cap]   (cap 0: a null output pointer)
        const int W = r.get<int32_t>(), H = r.get<int32_t>(), cap = r.get<int32_t>();
        auto mask = r.bytes((size_t)W * H);
        std::unique_ptr<int[]> xy(cap > 0 ? new int[2 * (size_t)cap] : nullptr);
        for (int i = 0; i < 2 * cap; ++i) xy[i] = -77;
        const int rc = mtx_host_mask_outline(mask.get(), W, H, xy.get(), cap);
        w.put<int32_t>(rc); w.bytes(xy.get(), 2 * (size_t)cap * sizeof(int));
        break;
      }
      case OP_CHAMFER: {                        // w h, src[w*h] -> rc, dist[w*h] float32
        const int W = r.get<int32_t>(), H = r.get<int32_t>();
        const size_t n = (size_t)W * H;
        auto src = r.bytes(n);
        std::unique_ptr<float[]> d(new float[n]);
        for (size_t i = 0; i < n; ++i) d[i] = -1.0f;
        const int rc = mtx_host_chamfer_l2_5x5(src.get(), W, H, d.get());
        w.put<int32_t>(rc); w.bytes(d.get(), n * sizeof(float));
        break;
      }
      case OP_PNG: {                            // w h channels level threads reduce, pixels -> size with no buffer; exact-capacity rc + file; one-short rc + untouched flag
        const int W = r.get<int32_t>(), H = r.get<int32_t>(), ch = r.get<int32_t>(), level = r.get<int32_t>(), threads = r.get<int32_t>(), reduce = r.get<int32_t>();
        auto px = r.bytes((size_t)W * H * ch);
        const int64_t size = mtx_host_png_encode(px.get(), W, H, ch, level, threads, reduce, nullptr, 0);        // capacity zero: the size alone
        w.put<int64_t>(size);
        if (size <= 0) break;
        std::unique_ptr<uint8_t[]> exact(new uint8_t[(size_t)size]);
        const int64_t rc_exact = mtx_host_png_encode(px.get(), W, H, ch, level, threads, reduce, exact.get(), size);
        w.put<int64_t>(rc_exact); w.bytes(exact.get(), (size_t)size);
        std::unique_ptr<uint8_t[]> small(new uint8_t[(size_t)size - 1]);
        memset(small.get(), 0xAB, (size_t)size - 1);
        const int64_t rc_short = mtx_host_png_encode(px.get(), W, H, ch, level, threads, reduce, small.get(), size - 1);
        int32_t untouched = 1;
        for (int64_t i = 0; i < size - 1; ++i) if (small[i] != 0xAB) untouched = 0;
        w.put<int64_t>(rc_short); w.put<int32_t>(untouched);
        break;
      }
      default:
        fprintf(stderr, "case file: unknown op %d in record %d\n", op, records);
        return 3;
    }
  }
  fclose(in);
  if (fclose(out) != 0) return 4;
  printf("%d records\n", records);
  return 0;
}
