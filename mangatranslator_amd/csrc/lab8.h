// lab8.h — OpenCV's fixed-point 8-bit RGB -> Lab (cv2.cvtColor(COLOR_RGB2LAB) on uint8), shared by pagetail.hip (luminance match) and
// textcolor.hip (text-colour probe).  Integer tables from core/image/color.py, uploaded once by the caller: exact.
#pragma once
#include "mtx_device.h"

namespace mtx {

struct Lab8Tables { const int32_t* gamma_tab; const int32_t* cbrt_tab; const int32_t* lab_coef; int cbrt_n; };

__device__ __forceinline__ void rgb_to_lab8(const Lab8Tables& t, int r8, int g8, int b8, int& L, int& A, int& B) {
  const int r = t.gamma_tab[r8], g = t.gamma_tab[g8], b = t.gamma_tab[b8];
  int f[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int xyz = (r * t.lab_coef[c * 3] + g * t.lab_coef[c * 3 + 1] + b * t.lab_coef[c * 3 + 2] + (1 << 11)) >> 12;
    xyz = xyz < 0 ? 0 : (xyz > t.cbrt_n - 1 ? t.cbrt_n - 1 : xyz);
    f[c] = t.cbrt_tab[xyz];
  }
  const int lshift = -((16 * 255 * (1 << 15) + 50) / 100), h2 = 1 << 14;
  L = (((116 * 255 + 50) / 100) * f[1] + lshift + h2) >> 15;
  A = (500 * (f[0] - f[1]) + 128 * (1 << 15) + h2) >> 15;
  B = (200 * (f[1] - f[2]) + 128 * (1 << 15) + h2) >> 15;
  L = L < 0 ? 0 : (L > 255 ? 255 : L); A = A < 0 ? 0 : (A > 255 ? 255 : A); B = B < 0 ? 0 : (B > 255 ? 255 : B);
}

}  // namespace mtx
