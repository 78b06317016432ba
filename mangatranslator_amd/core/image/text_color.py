"""Rendered-text colour probe of the OSB (outside-speech-bubble) stage — SURVEY.md §8 row f3; reference
core/outside_text_processor.py:1096-1165, which runs per text region on the CPU through OpenCV:

    Lab distance of every crop pixel to the border ring's median -> 95th percentile -> contrast threshold max(30, 0.6 * p95) ->
    3x3 close -> 2x2 erode -> external contours of area >= 4, filled -> median RGB of what is left (>= 10 pixels) ->
    snapped to black / white when its HSV saturation is below 25

Here the pixel work runs on the device for all regions of a page at once (csrc/textcolor.hip, `mtx_text_color`, phases DIST / MASK /
HIST), the contour step on the host in native code on the small crop masks (`mtx_host_fill_components`).  Everything the device hands
back is an exact integer: squared Lab distances, their order statistics around the percentile's rank, histograms.  The float32 part
of the reference expression (square roots, `np.percentile`, `max(30, p95 * 0.6)`) is evaluated by numpy itself on the host from those
integers, then turned back into an integer cut-off on the squared distance, so the mask is the reference's mask bit for bit.

Per page: one upload of the page (or adoption of a device tensor), three `mtx_text_color` calls whatever the number of regions, two
small read-backs (order statistics, histograms) and one round trip of the byte masks for the contour step.  There is no host
fallback: without the library this raises like every other kernel path."""
import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from ...hip import abi
from ...hip.lib import get_library
from ...utils.exceptions import ModelError
from .color import rgb_to_lab_u8
from .device_tail import get_device_tail

MIN_CONTRAST = 30
CONTRAST_OF_P95 = 0.6
MIN_COMPONENT_AREA = 4
MIN_TEXT_PIXELS = 10
SATURATION_SNAP = 25
MAX_D2 = 3 * 255 * 255

# `launches` = calls of `mtx_text_color`; each issues a fixed kernel sequence over ALL regions (grid row = region), so the count per
# page does not depend on the number of regions
stats = {"pages": 0, "regions": 0, "launches": 0}

Region = Tuple[Tuple[int, int, int, int], Sequence[int]]


def hsv_saturation(r: int, g: int, b: int) -> int:
    """S of OpenCV's 8-bit RGB -> HSV (fixed point: (v - min) * round(255 * 4096 / v), descaled by 12 bits)"""
    v, mn = max(r, g, b), min(r, g, b)
    if v == 0:
        return 0
    return ((v - mn) * int(round((255 << 12) / float(v))) + (1 << 11)) >> 12


def snap_low_saturation(rgb: Tuple[int, int, int]) -> Tuple[int, int, int]:
    if hsv_saturation(*rgb) < SATURATION_SNAP:
        return (0, 0, 0) if max(rgb) < 128 else (255, 255, 255)
    return rgb


def _ranks(n: int) -> np.ndarray:
    """the four ranks around 0.95 * (n - 1): numpy forms that index in the array's own float32, which may land one rank beside the
    float64 value; the window covers either"""
    r0 = int(np.floor(0.95 * (n - 1)))
    return np.clip(np.array([r0 - 1, r0, r0 + 1, r0 + 2], np.int64), 0, n - 1).astype(np.int32)


def contrast_cutoff(n: int, ranks: np.ndarray, order_d2: np.ndarray):
    """(cut-off on d2, p95, threshold): the reference's `np.percentile(dist_map, 95)` and `max(30, p95 * 0.6)`, evaluated by numpy on a
    stand-in for the sorted distance map that agrees with it at every rank the percentile can read; the cut-off is the largest d2
    whose float32 root is not above the threshold, so `d2 > cutoff` is `dist_map > threshold`"""
    roots = np.sqrt(order_d2.astype(np.float32))
    stand_in = np.empty(n, np.float32)
    stand_in[:] = roots[0]
    for k in (1, 2, 3):
        stand_in[int(ranks[k]):] = roots[k]
    p95 = np.percentile(stand_in, 95)
    threshold = max(MIN_CONTRAST, p95 * CONTRAST_OF_P95)

    def above(c: int) -> bool:
        return bool((np.sqrt(np.array([c], np.float32)) > threshold)[0])
    c = int(min(max(float(threshold), 0.0) ** 2, MAX_D2))
    while c < MAX_D2 and not above(c + 1):
        c += 1
    while c >= 0 and above(c):
        c -= 1
    return c, p95, threshold


def median_from_hist(hist: np.ndarray) -> int:
    """`int(np.median(values))` of the 8-bit values a 256-bin histogram counts (even counts: mean of the two middle values, truncated)"""
    cum = np.cumsum(hist)
    n = int(cum[-1])
    lo = int(np.searchsorted(cum, (n - 1) // 2, side="right"))
    hi = int(np.searchsorted(cum, n // 2, side="right"))
    return (lo + hi) // 2


def _page_tensor(page_rgb, dev) -> torch.Tensor:
    if torch.is_tensor(page_rgb):
        t = page_rgb
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] < 3:
            raise ValueError("page tensor must be uint8 [H, W, 3]")
        return t[..., :3].to(dev).contiguous()
    if isinstance(page_rgb, Image.Image):
        page_rgb = np.array(page_rgb.convert("RGB"))
    arr = np.asarray(page_rgb)
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] < 3:
        raise ValueError("page must be uint8 [H, W, 3]")
    return torch.from_numpy(np.ascontiguousarray(arr[..., :3])).to(dev)


def probe_text_colors(page_rgb, regions: Sequence[Region], lib=None, device=None, trace: Optional[list] = None) -> List[Optional[Tuple[int, int, int]]]:
    """Text colour of every region `((x0, y0, x1, y1), bg_rgb)` of one page (numpy / PIL / uint8 device tensor, RGB), or None where the
    reference finds none (fewer than 10 text pixels).  Rectangle pixels outside the page count as black, as `Image.crop` pads them.
    `trace` (tests): a list that receives, per launched region, dict(index, d2, cutoff, p95, threshold, mask, filled)."""
    out: List[Optional[Tuple[int, int, int]]] = [None] * len(regions)
    live = []
    for i, (rect, _) in enumerate(regions):
        x0, y0, x1, y1 = (int(v) for v in rect)
        if x1 > x0 and y1 > y0:
            live.append(i)
    if not live:
        return out
    lib = lib if lib is not None else get_library()
    if device is None:
        device = page_rgb.device if torch.is_tensor(page_rgb) and not lib.is_simulator else ("cpu" if lib.is_simulator else "cuda")
    dev = torch.device(device)
    if (dev.type == "cuda") == bool(lib.is_simulator):
        raise ModelError(f"text colour probe: device {dev} does not match the kernel library ({'simulator' if lib.is_simulator else 'gfx950'})")
    page = _page_tensor(page_rgb, dev)
    H, W = int(page.shape[0]), int(page.shape[1])
    n = len(live)
    rois = np.zeros((n, 4), np.int32)
    offsets = np.zeros(n, np.int64)
    bg_lab = np.zeros((n, 3), np.int32)
    ranks = np.zeros((n, abi.TC_RANKS), np.int32)
    total = 0
    for k, i in enumerate(live):
        (x0, y0, x1, y1), bg = regions[i]
        rois[k] = (int(x0), int(y0), int(x1) - int(x0), int(y1) - int(y0))
        offsets[k] = total
        area = int(rois[k, 2]) * int(rois[k, 3])
        total += area
        bg_lab[k] = rgb_to_lab_u8(np.asarray(bg, dtype=np.int64).astype(np.uint8).reshape(1, 1, 3))[0, 0]
        ranks[k] = _ranks(area)
    areas = rois[:, 2].astype(np.int64) * rois[:, 3]
    if total >= 2 ** 31 or int(areas.max()) >= 2 ** 31 - 256:
        raise ModelError("text colour probe: regions of a page exceed 2^31 pixels")
    tail = get_device_tail(lib, dev)
    up = lambda a: torch.from_numpy(a).to(dev)
    rois_d, off_d, bg_d, ranks_d = up(rois), up(offsets), up(bg_lab), up(ranks)
    d2 = torch.empty(total, dtype=torch.int32, device=dev)
    mask = torch.empty(total, dtype=torch.uint8, device=dev)
    st = torch.empty((n, abi.TC_STATS), dtype=torch.int32, device=dev)
    hist = torch.empty((n, 768), dtype=torch.int32, device=dev)
    a = abi.TextColorArgs()
    a.page_rgb, a.rois, a.offsets, a.bg_lab, a.ranks = page.data_ptr(), rois_d.data_ptr(), off_d.data_ptr(), bg_d.data_ptr(), ranks_d.data_ptr()
    a.d2, a.mask, a.stats, a.hist = d2.data_ptr(), mask.data_ptr(), st.data_ptr(), hist.data_ptr()
    a.gamma_tab, a.cbrt_tab, a.lab_coef, a.cbrt_n = tail._gamma.data_ptr(), tail._cbrt.data_ptr(), tail._coef.data_ptr(), int(tail._cbrt.numel())
    a.n, a.page_h, a.page_w, a.max_pixels = n, H, W, int(areas.max())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream if (dev.type == "cuda" and not lib.is_simulator) else 0)

    def run(phase):
        a.phase = phase
        lib.check(lib.mtx_text_color(C.byref(a), stream), "mtx_text_color")
        stats["launches"] += 1

    stats["pages"] += 1
    stats["regions"] += n
    run(abi.TC_DIST)
    order = st[:, abi.TC_STAT_ORDER:abi.TC_STAT_ORDER + abi.TC_RANKS].cpu().numpy()
    cut = np.zeros(n, np.int32)
    floats = []
    for k in range(n):
        c, p95, thr = contrast_cutoff(int(areas[k]), ranks[k], order[k])
        cut[k] = c
        floats.append((p95, thr))
    cut_d = up(cut)
    a.cutoff = cut_d.data_ptr()
    run(abi.TC_MASK)
    mask_h = np.array(mask.cpu().numpy())                   # a copy: on a CPU device (simulator) the tensor's own memory is reused below
    filled_h = np.zeros_like(mask_h)
    for k in range(n):
        o, w, h = int(offsets[k]), int(rois[k, 2]), int(rois[k, 3])
        src = mask_h[o:o + w * h]
        if not src.any():
            continue
        rc = lib.mtx_host_fill_components(src.ctypes.data, w, h, float(MIN_COMPONENT_AREA), filled_h[o:o + w * h].ctypes.data)
        if rc < 0:
            raise ModelError(f"mtx_host_fill_components failed ({rc})")
    mask.copy_(torch.from_numpy(filled_h))
    run(abi.TC_HIST)
    hist_h = hist.cpu().numpy().reshape(n, 3, 256)
    d2_h = d2.cpu().numpy() if trace is not None else None
    for k, i in enumerate(live):
        if int(hist_h[k, 0].sum()) >= MIN_TEXT_PIXELS:
            out[i] = snap_low_saturation(tuple(median_from_hist(hist_h[k, c]) for c in range(3)))
        if trace is not None:
            o, w, h = int(offsets[k]), int(rois[k, 2]), int(rois[k, 3])
            trace.append(dict(index=i, d2=d2_h[o:o + w * h].reshape(h, w), order=order[k].copy(), cutoff=int(cut[k]), p95=floats[k][0],
                              threshold=floats[k][1], mask=mask_h[o:o + w * h].reshape(h, w), filled=filled_h[o:o + w * h].reshape(h, w),
                              text_pixels=int(hist_h[k, 0].sum())))
    return out
