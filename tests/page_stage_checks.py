"""Exact-input checks of the kernels that write the bytes of the finished page — csrc/clean.hip (bubble cleaning), csrc/textcolor.hip (the
text-colour probe) and csrc/pagetail.hip (resample, composite, Lab luminance match, feather weight) — shared by the simulator tier
(tests/test_page_stage_sim.py) and the GPU tier (tests/test_page_stage_gpu.py).

Every check feeds a kernel inputs whose correct output is known exactly, stage by stage, and compares with a witness that shares no code
with the kernel: oracle/cleaning_ref.py, oracle/cv2_color_ref.py (a per-pixel loop: subsets only), numpy, scipy, torch's CPU resize, closed
forms, and core/image/color.py (the host path the kernels replace) where a full-size witness is needed.  Integer results: equal.  The one
float leg (Lab -> RGB of the luminance match) has a stated bound, see `check_lab_remap`."""
import ctypes as C
import math
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

from mangatranslator_amd.core.image import cleaning as cl
from mangatranslator_amd.core.image import color as hc
from mangatranslator_amd.core.image import inpainting as ip
from mangatranslator_amd.core.image.device_tail import DeviceTail, aten_aa_bilinear_tables
from mangatranslator_amd.core.image.text_color import _ranks
from mangatranslator_amd.hip import abi
from oracle import cleaning_ref as cr
from oracle import cv2_color_ref as cv


def _dev(lib):
    return torch.device("cpu") if lib.is_simulator else torch.device("cuda:0")


def _stream(lib, dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream if (dev.type == "cuda" and not lib.is_simulator) else 0)


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# =================================================================================================================================
# 1. cleaning: mtx_bubble_clean through cleaning._run_pixel_half
# =================================================================================================================================
CLEAN_H, CLEAN_W = 40, 52
CLEAN_PAGES = ("noise", "flat128", "rows127_129", "just_under_128", "stripes", "ramp", "white", "black")
CLEAN_ELEMENTS = (((7, 7), (5, 5)), ((1, 1), (1, 1)), ((15, 15), (9, 3)), ((3, 11), (5, 5)))
CLEAN_SHRINKS = (0.0, 0.5, 1.0, 1.4, 2.1969, 2.2, 3.0, 6.5)          # on and beside the chamfer weights 1, 1.4, 2.1969
CLEAN_MASK_NAMES = ("top-left rectangle", "bottom-right rectangle stored as 1", "single pixel", "whole page", "1-px line",
                    "ellipse with a hole", "empty", "checkerboard")
FIXED_THRESHOLD = 200


def clean_cases():
    """48 fixed (page, element pair, otsu, shrink) combinations: every page six times, every element pair twelve times, every shrink six
    times, Otsu on and off 24 times each — walked with strides that are coprime to the list lengths so the factors do not move in step"""
    out = []
    for k in range(48):
        out.append((CLEAN_PAGES[k % 8], CLEAN_ELEMENTS[(k // 2 + k // 8) % 4], bool((k + k // 16) % 2), CLEAN_SHRINKS[(3 * k + k // 8) % 8]))
    assert {c[0] for c in out} == set(CLEAN_PAGES) and {c[1] for c in out} == set(CLEAN_ELEMENTS) and {c[3] for c in out} == set(CLEAN_SHRINKS)
    assert {c[2] for c in out} == {False, True} and len(set(out)) == 48
    return out


@lru_cache(maxsize=None)
def clean_masks():
    H, W = CLEAN_H, CLEAN_W
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((8, H, W), np.uint8)
    m[0, 0:9, 0:12] = 255
    m[1, H - 8:, W - 11:] = 1
    m[2, 20, 30] = 255
    m[3] = 255
    m[4, 12, 5:41] = 255
    ell = ((xx - 26) / 17.0) ** 2 + ((yy - 21) / 11.0) ** 2 <= 1.0
    hole = ((xx - 24) / 6.0) ** 2 + ((yy - 20) / 4.0) ** 2 <= 1.0
    m[5][ell & ~hole] = 255
    m[7][((xx + yy) % 2 == 0) & (xx >= 6) & (xx < 47) & (yy >= 4) & (yy < 35)] = 255
    return m


@lru_cache(maxsize=None)
def clean_page(name):
    """BGR page [40, 52, 3]"""
    H, W = CLEAN_H, CLEAN_W
    yy, xx = np.mgrid[0:H, 0:W]
    grey = lambda g: np.repeat(np.asarray(g, np.uint8)[..., None], 3, axis=2)       # equal channels: BGR2GRAY is the identity
    if name == "noise":
        page = np.random.default_rng(11).integers(0, 256, (H, W, 3), dtype=np.uint8)
    elif name == "flat128":
        page = grey(np.full((H, W), 128))                                           # mean exactly 128: a white bubble
    elif name == "rows127_129":
        page = grey(np.where(yy % 2 == 0, 127, 129))
    elif name == "just_under_128":
        g = np.full((H, W), 128, np.uint8)
        for m in clean_masks():                                                     # the first pixel of every mask one level lower:
            ys, xs = np.nonzero(m)                                                  # every bubble's mean is a hair under 128, a black bubble
            if ys.size:
                g[ys[0], xs[0]] = 127
        page = grey(g)
    elif name == "stripes":
        page = grey(np.where((xx // 4) % 2 == 0, 60, 190))                          # an Otsu histogram of two spikes: ties in the variance
    elif name == "ramp":
        page = np.stack([(xx * 5) % 256, (yy * 6 + xx) % 256, 255 - (xx * 4 + yy) % 256], -1).astype(np.uint8)
    elif name == "white":
        page = grey(np.full((H, W), 255))
    elif name == "black":
        page = grey(np.zeros((H, W)))
    else:
        raise KeyError(name)
    return np.ascontiguousarray(page)


@lru_cache(maxsize=None)
def _oracle_morph(mask_key, ksize, dilate):
    """whole-page dilation / erosion of one of the fixed masks (the cache key names the mask set and index)"""
    base = np.where(_mask_by_key(mask_key) > 0, 255, 0).astype(np.uint8)
    k = cr.ellipse_kernel(ksize)
    return cr.dilate(base, k) if dilate else cr.erode(base, k)


@lru_cache(maxsize=None)
def _oracle_dist(mask_key, dil_ksize):
    """the oracle's two-pass chamfer transform of the dilated mask — a Python loop per pixel, so computed once per (mask, element)"""
    return cr.distance_transform_l2_5x5(_oracle_morph(mask_key, dil_ksize, True))


_MASK_SETS = {}


def _mask_by_key(key):
    return _MASK_SETS[key[0]][key[1]]


def oracle_stages(page_bgr, set_name, index, dil_ksize, ero_ksize, use_otsu, shrink, threshold=FIXED_THRESHOLD):
    """the stages of oracle/cleaning_ref.process_single_bubble on the WHOLE page, statement by statement, kept apart"""
    key = (set_name, index)
    base = np.where(_mask_by_key(key) > 0, 255, 0).astype(np.uint8)
    gray = cr.bgr_to_gray(page_bgr)
    masked = gray[base == 255]
    black = bool(masked.size > 0 and float(np.mean(masked)) < cr.GRAYSCALE_MIDPOINT)
    roi_mask = _oracle_morph(key, dil_ksize, True)
    roi = roi_mask == 255
    roi_gray = np.where(roi, gray, 0).astype(np.uint8)
    v = (255 - roi_gray) if black else roi_gray
    if use_otsu:
        thr = int(cr.otsu_threshold(v[roi])) if roi.any() else 0                     # an empty ROI has no histogram: the kernel writes 0
    else:
        thr = threshold
    above = np.where(v > thr, 255, 0).astype(np.uint8) & roi_mask
    dist = _oracle_dist(key, dil_ksize)
    shrunk = np.where(dist >= np.float32(shrink), 255, 0).astype(np.uint8)
    return dict(base=base, roi=roi_mask, eroded=_oracle_morph(key, ero_ksize, False), above=above, thresholded=above & shrunk, shrunk=shrunk, dist=dist,
                hist=np.bincount(v[roi].ravel(), minlength=256), gsum=int(masked.astype(np.int64).sum()), gcount=int(masked.size), black=int(black), thr=thr)


def assert_clean_planes(crops, i, want, tag):
    """every plane and statistic of bubble i against the oracle's whole-page stages cut to the crop"""
    x0, y0, w, h = (int(v) for v in crops.rois[i])
    outside = np.ones(want["roi"].shape, bool)
    outside[y0:y0 + h, x0:x0 + w] = False
    # the kernel treats "outside the crop" as background: that only holds when the oracle has nothing there
    assert not want["roi"][outside].any() and not want["thresholded"][outside].any(), f"{tag}: the oracle's ROI leaves the crop {crops.rois[i]}"
    for name in ("base", "roi", "eroded", "thresholded", "shrunk"):
        got, ref = crops.plane(name, i), want[name][y0:y0 + h, x0:x0 + w]
        assert np.array_equal(got, ref), f"{tag}: plane {name} differs on {(got != ref).sum()} of {ref.size} px, first at {np.argwhere(got != ref)[0]}"
    st = crops.stats[i]
    assert np.array_equal(st[:256], want["hist"]), f"{tag}: histogram differs in bins {np.nonzero(st[:256] != want['hist'])[0][:8]}"
    assert (int(st[256]), int(st[257])) == (want["gsum"], want["gcount"]), f"{tag}: grey sum / count {st[256]}, {st[257]} != {want['gsum']}, {want['gcount']}"
    assert int(st[258]) == want["black"], f"{tag}: polarity {st[258]} != {want['black']}"
    assert int(st[259]) == want["thr"], f"{tag}: threshold {st[259]} != {want['thr']}"


def check_clean_case(lib, page_name, elements, use_otsu, shrink):
    """one launch over the 8 masks of the 40 x 52 page; the masks' crops differ in size, so the grid has blocks past a small bubble's end"""
    _MASK_SETS.setdefault("fixed", clean_masks())
    dk, ek = elements
    page, masks = clean_page(page_name), clean_masks()
    crops, box = cl._run_pixel_half(lib, str(_dev(lib)), page, np.array(masks), cl.ellipse_rows(dk), cl.ellipse_rows(ek), FIXED_THRESHOLD, use_otsu, shrink, None, 1.0)
    assert [bool(b) for b in box[:, 4]] == [False] * 6 + [True, False]
    assert len({(int(r[2]), int(r[3])) for r in crops.rois}) >= 5
    blacks = []
    for i in range(8):
        want = oracle_stages(page, "fixed", i, dk, ek, use_otsu, shrink)
        assert_clean_planes(crops, i, want, f"{page_name} {dk}/{ek} otsu={use_otsu} shrink={shrink} mask '{CLEAN_MASK_NAMES[i]}'")
        blacks.append(want["black"])
    return blacks


def check_clean_polarity_pages(lib):
    """the inputs prove themselves: the flat-128 page is white everywhere and the page one level under it is black everywhere"""
    assert check_clean_case(lib, "flat128", CLEAN_ELEMENTS[0], False, 1.0) == [0] * 8
    assert check_clean_case(lib, "just_under_128", CLEAN_ELEMENTS[0], False, 1.0) == [1, 1, 1, 1, 1, 1, 0, 1]


def check_clean_junction_zones(lib):
    """two neighbouring bubbles near the page's top edge (their zones are clipped by it) and a third, far one without a zone; shrink 5 with
    the junction minimum 1 against the oracle's adaptive_shrink_mask, then with the junction minimum equal to the shrink (zones without effect)"""
    H, W = 64, 96
    masks = np.zeros((3, H, W), np.uint8)
    masks[0, 3:30, 8:40] = 255
    masks[1, 5:34, 44:80] = 255
    masks[2, 44:60, 10:30] = 255
    bboxes = [(8, 3, 39, 29), (44, 5, 79, 33), (10, 44, 29, 59)]
    neighbors = [[bboxes[1]], [bboxes[0]], [bboxes[0], bboxes[1]]]
    zones = [cl._junction_zones(bboxes[i], neighbors[i], 1.0, W, H) for i in range(3)]
    assert zones[0] and zones[1] and not zones[2], zones
    assert zones[0][0][1] == 0 and max(bboxes[0][1], bboxes[1][1]) - cl.JUNCTION_ADJACENCY_MARGIN < 0, "the zone must be clipped by the page edge"
    _MASK_SETS["junction"] = masks
    page = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    dk, ek = (7, 7), (5, 5)
    changed = 0
    for jmin in (1.0, 5.0):
        crops, _ = cl._run_pixel_half(lib, str(_dev(lib)), page, masks, cl.ellipse_rows(dk), cl.ellipse_rows(ek), FIXED_THRESHOLD, False, 5.0, zones, jmin)
        for i in range(3):
            want = oracle_stages(page, "junction", i, dk, ek, False, 5.0)
            if jmin == 1.0:
                want["shrunk"] = cr.adaptive_shrink_mask(want["roi"], 5.0, bboxes[i], neighbors[i], 1.0)
                changed += int((want["shrunk"] != np.where(want["dist"] >= np.float32(5.0), 255, 0)).sum())
                want["thresholded"] = want["above"] & want["shrunk"]
            assert_clean_planes(crops, i, want, f"junction minimum {jmin}, bubble {i}")
    assert changed > 50, "the zones must relax the shrink somewhere"


def check_clean_sweep_count(lib):
    """`sweeps = ceil(shrink) + 1` where it is tightest: a 150 x 150 rectangle with dilation (1, 1) (ROI == base).  Inside a rectangle the
    chamfer distance to the nearest background pixel is the 1-based distance k to the nearest side (a straight run of k unit steps; every
    other move costs more per row or column crossed), so shrunk = {k >= ceil(s)}.  The second rectangle touches the page's left edge, where
    outside the page counts as far: that side is not counted."""
    H, W = 170, 180
    page = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for x0 in (15, 0):
        mask = np.zeros((1, H, W), np.uint8)
        mask[0, 10:160, x0:x0 + 150] = 255
        k = np.minimum(np.minimum(yy - 10, 159 - yy), x0 + 149 - xx) + 1
        if x0 > 0:
            k = np.minimum(k, xx - x0 + 1)
        inside = mask[0] == 255
        for s in (1.0, 31.5, 63.0, 64.0):
            crops, _ = cl._run_pixel_half(lib, str(_dev(lib)), page, mask, cl.ellipse_rows((1, 1)), cl.ellipse_rows((1, 1)), FIXED_THRESHOLD, False, s, None, 1.0)
            cx, cy, w, h = (int(v) for v in crops.rois[0])
            want = np.where(inside & (k >= math.ceil(s)), 255, 0).astype(np.uint8)
            assert not want[~inside].any() and np.array_equal(crops.plane("roi", 0), mask[0][cy:cy + h, cx:cx + w])
            got = crops.plane("shrunk", 0)
            assert np.array_equal(got, want[cy:cy + h, cx:cx + w]), f"rectangle at x = {x0}, shrink {s}: {(got != want[cy:cy + h, cx:cx + w]).sum()} px differ"
            assert want.any() == (math.ceil(s) <= 75)


class _LaunchTwice:
    """the kernel library with `mtx_bubble_clean` issued twice on the same arguments, hence on the same buffers"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def mtx_bubble_clean(self, args, stream):
        rc = self._lib.mtx_bubble_clean(args, stream)
        return rc if rc else self._lib.mtx_bubble_clean(args, stream)


def check_clean_cross_block_atomics(lib):
    """a bubble of 115 600 pixels (452 blocks adding into one histogram, sum and count) beside one of 9, on a noise page: the statistics
    equal numpy's; a second launch on the same buffers gives the same result, which is the in-launch zeroing of `stats`"""
    H, W = 360, 380
    page = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
    masks = np.zeros((2, H, W), np.uint8)
    masks[0, 10:350, 12:352] = 255
    masks[1, 20:23, 360:363] = 255
    dil, ero = cl.ellipse_rows((7, 7)), cl.ellipse_rows((5, 5))
    gray = cr.bgr_to_gray(page).astype(np.int64)
    runs = []
    for library in (lib, _LaunchTwice(lib)):
        crops, _ = cl._run_pixel_half(library, str(_dev(lib)), page, masks, dil, ero, FIXED_THRESHOLD, True, 2.0, None, 1.0)
        for i in range(2):
            x0, y0, w, h = (int(v) for v in crops.rois[i])
            base = masks[i] != 0
            black = gray[base].mean() < 128
            roi = cr.dilate(np.where(base, 255, 0).astype(np.uint8), cr.ellipse_kernel((7, 7))) == 255
            assert np.array_equal(crops.plane("roi", i) != 0, roi[y0:y0 + h, x0:x0 + w]) and roi.sum() == (crops.plane("roi", i) != 0).sum()
            st = crops.stats[i]
            assert (int(st[256]), int(st[257])) == (int(gray[base].sum()), int(base.sum())), f"bubble {i}: grey sum / count"
            assert int(st[258]) == int(black)
            assert np.array_equal(st[:256], np.bincount((255 - gray[roi]) if black else gray[roi], minlength=256)), f"bubble {i}: histogram"
            assert int(st[259]) == int(cr.otsu_threshold(((255 - gray[roi]) if black else gray[roi]).astype(np.uint8)))
        assert int(masks[0].astype(bool).sum()) >= 100000
        runs.append(crops)
    assert np.array_equal(runs[0].stats, runs[1].stats)
    for name in ("base", "roi", "eroded", "thresholded", "shrunk"):
        assert np.array_equal(runs[0].planes[name], runs[1].planes[name]), name


# =================================================================================================================================
# the colour chart
# =================================================================================================================================
CHART_FULL = 1536                       # 2 359 296 pixels: one grid-stride trip more than the tail kernels' cap of 8192 blocks x 256
N_CORNERS_AND_GREYS = 8 + 256


@lru_cache(maxsize=None)
def _chart_colours():
    lv52, lv16, all256 = np.arange(52) * 5, np.arange(16) * 17, np.arange(256)
    parts = [np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)]), np.repeat(all256[:, None], 3, axis=1),
             np.stack(np.meshgrid(lv52, lv52, lv52, indexing="ij"), -1).reshape(-1, 3)]
    for ch in range(3):                                                  # each channel's 256 levels crossed with 16 levels of the other two
        g = np.stack(np.meshgrid(all256, lv16, lv16, indexing="ij"), -1).reshape(-1, 3)
        order = {0: (0, 1, 2), 1: (1, 0, 2), 2: (1, 2, 0)}[ch]
        parts.append(g[:, order])
    n = sum(len(p) for p in parts)
    parts.append(np.random.default_rng(21).integers(0, 256, (CHART_FULL * CHART_FULL - n, 3)))
    return np.concatenate(parts).astype(np.uint8)


@lru_cache(maxsize=None)
def chart(size):
    """RGB [size, size, 3]: the first size^2 colours of the chart — the 8 cube corners, the grey axis, the 52-level lattice (52^3), each
    channel's 256 levels x 16 x 16 levels of the others, seeded colours for the rest.  1536 holds everything; 512 (simulator tier) holds the
    corners, the grey axis, the whole lattice and the red and most of the green crossings."""
    return np.ascontiguousarray(_chart_colours()[:size * size].reshape(size, size, 3))


@lru_cache(maxsize=None)
def chart_lab(size):
    """int32 Lab of the chart through the host path the kernels replace (core/image/color.py)"""
    return hc.rgb_to_lab_u8(chart(size)).astype(np.int32)


def _d2(lab, bg):
    return ((lab.astype(np.int64) - np.asarray(bg, np.int64)) ** 2).sum(-1).astype(np.int32)


def _padded_crop(page, x0, y0, w, h):
    """the page's rectangle, black outside the page (as PIL's crop pads)"""
    H, W = page.shape[:2]
    out = np.zeros((h, w, 3), np.uint8)
    xa, ya, xb, yb = max(x0, 0), max(y0, 0), min(x0 + w, W), min(y0 + h, H)
    if xb > xa and yb > ya:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = page[ya:yb, xa:xb]
    return out


# =================================================================================================================================
# 2. text colour: the phases of mtx_text_color called directly on authored buffers
# =================================================================================================================================
class TextColorLaunch:
    """buffers of one `mtx_text_color` problem: regions (x, y, w, h) of a page, `gap` unused elements between the regions' crops"""

    def __init__(self, lib, page, rois, gap=0):
        from mangatranslator_amd.core.image.device_tail import get_device_tail
        self.lib, self.dev = lib, _dev(lib)
        self.rois = np.asarray(rois, np.int32).reshape(-1, 4)
        self.n = len(self.rois)
        self.areas = self.rois[:, 2].astype(np.int64) * self.rois[:, 3]
        self.offsets = np.concatenate([[0], np.cumsum(self.areas + gap)[:-1]]).astype(np.int64)
        self.total = int(self.offsets[-1] + self.areas[-1] + gap)
        self.page = _up(page, self.dev)
        self.tail = get_device_tail(lib, self.dev)
        self.t = dict(rois=_up(self.rois, self.dev), offsets=_up(self.offsets, self.dev))
        a = self.args = abi.TextColorArgs()
        a.page_rgb, a.rois, a.offsets = self.page.data_ptr(), self.t["rois"].data_ptr(), self.t["offsets"].data_ptr()
        a.gamma_tab, a.cbrt_tab, a.lab_coef, a.cbrt_n = self.tail._gamma.data_ptr(), self.tail._cbrt.data_ptr(), self.tail._coef.data_ptr(), int(self.tail._cbrt.numel())
        a.n, a.page_h, a.page_w, a.max_pixels = self.n, int(page.shape[0]), int(page.shape[1]), int(self.areas.max())

    def put(self, name, array):
        self.t[name] = _up(array, self.dev)
        setattr(self.args, name, self.t[name].data_ptr())
        return self.t[name]

    def run(self, phase):
        self.args.phase = phase
        self.lib.check(self.lib.mtx_text_color(C.byref(self.args), _stream(self.lib, self.dev)), "mtx_text_color")

    def get(self, name):
        return np.array(self.t[name].cpu().numpy())

    def crop(self, flat, k):
        o, (x, y, w, h) = int(self.offsets[k]), (int(v) for v in self.rois[k])
        return flat[o:o + w * h].reshape(h, w)


def _run_dist(lib, page, rois, bg_lab):
    """DIST over the regions -> (launch, d2 flat, order statistics [n, 4], ranks [n, 4]); stats pre-filled with garbage: the launch zeroes them"""
    L = TextColorLaunch(lib, page, rois)
    ranks = np.stack([_ranks(int(a)) for a in L.areas])
    L.put("bg_lab", np.asarray(bg_lab, np.int32).reshape(-1, 3))
    L.put("ranks", ranks)
    L.put("d2", np.full(L.total, -1, np.int32))
    L.put("stats", np.full((L.n, abi.TC_STATS), 12345, np.int32))
    L.run(abi.TC_DIST)
    return L, L.get("d2"), L.get("stats")[:, abi.TC_STAT_ORDER:abi.TC_STAT_ORDER + abi.TC_RANKS], ranks


def check_tc_dist_chart(lib, size):
    """d2 of the whole chart under three backgrounds equals numpy's from core/image/color.rgb_to_lab_u8, and from the per-pixel oracle
    (oracle/cv2_color_ref.py) on the corners, the grey axis and 4096 seeded positions; a fourth region crosses the page edge by 3 px on two
    sides and reads black there.  The order statistics of these large regions are checked on the way."""
    page, lab = chart(size), chart_lab(size)
    rng = np.random.default_rng(31)
    bgs = [(0, 128, 128), (255, 128, 128), tuple(int(v) for v in rng.integers(0, 256, 3)), tuple(int(v) for v in rng.integers(0, 256, 3))]
    edge = (size - 37, size - 29, 40, 32)
    L, d2, order, ranks = _run_dist(lib, page, [(0, 0, size, size)] * 3 + [edge], bgs)
    pick = np.concatenate([np.arange(N_CORNERS_AND_GREYS), rng.choice(size * size, 4096, replace=False)])
    assert len(pick) >= 4096
    lab_cv = cv.rgb_to_lab_u8(page.reshape(-1, 1, 3)[pick]).reshape(-1, 3)
    assert np.array_equal(lab_cv, lab.reshape(-1, 3)[pick]), "the two host witnesses disagree"
    for k in range(3):
        got, want = L.crop(d2, k), _d2(lab, bgs[k])
        assert np.array_equal(got, want), f"background {bgs[k]}: d2 differs on {(got != want).sum()} px"
        assert np.array_equal(got.reshape(-1)[pick], _d2(lab_cv, bgs[k])), f"background {bgs[k]}: d2 differs from the per-pixel oracle"
        assert np.array_equal(order[k], np.sort(want, axis=None)[ranks[k]]), f"background {bgs[k]}: order statistics {order[k]}"
    crop = _padded_crop(page, *edge)
    assert not crop[:, -3:].any() and not crop[-3:].any() and crop[:-3, :-3].any()
    want = _d2(hc.rgb_to_lab_u8(crop), bgs[3])
    assert np.array_equal(L.crop(d2, 3), want), "the region across the page edge"
    assert np.array_equal(order[3], np.sort(want, axis=None)[ranks[3]])


def _stack_regions(colour_lists):
    """a page that holds each list of colours as its own w x h rectangle (rows of up to 257 px, stacked), and the regions"""
    Wp = 257
    rows, rois = [], []
    y = 0
    for cols in colour_lists:
        cols = np.asarray(cols, np.uint8).reshape(-1, 3)
        n = len(cols)
        w = n if n <= Wp else next(d for d in range(Wp, 0, -1) if n % d == 0)
        h = n // w
        block = np.zeros((h, Wp, 3), np.uint8)
        block[:, :w] = cols.reshape(h, w, 3)
        rows.append(block)
        rois.append((0, y, w, h))
        y += h
    return np.ascontiguousarray(np.concatenate(rows)), rois


def check_tc_order_edges(lib, size):
    """rank selection at its edges, on regions built from chart colours whose d2 the DIST check pins: all ranks in one coarse and one fine
    bin; each wanted rank on the last pixel of the first colour and on the first pixel of the second; wanted ranks in one coarse bin but
    different fine bins; the highest fine bin a sum of three squares can reach (254: 255 is 7 mod 8, which no such sum is); the largest d2
    the chart offers"""
    colours, lab = chart(size).reshape(-1, 3), chart_lab(size).reshape(-1, 3)
    bg = (0, 128, 128)
    d2 = _d2(lab, bg)
    rng = np.random.default_rng(41)
    regions, labels = [], []
    flat = int(rng.integers(0, len(colours)))
    for n in (1, 2, 3, 255, 256, 257):
        regions.append(np.repeat(colours[flat][None], n, axis=0)); labels.append(f"flat, {n} px")
    lo, hi = int(np.argmin(d2)), int(np.argmax(d2))
    assert d2[hi] >> 8 != d2[lo] >> 8
    n = 240
    for j, rank in enumerate(_ranks(n)):
        for first in (int(rank) + 1, int(rank)):                     # the rank is the last pixel of the first colour / the first of the second
            idx = np.array([lo] * first + [hi] * (n - first))
            regions.append(colours[rng.permutation(idx)]); labels.append(f"two colours, {first} + {n - first}, rank {j}")
    # five distinct d2 in one coarse bin: ranks 93, 94, 95, 96 of 100 pixels each on its own value
    uniq = np.unique(d2)
    coarse, counts = np.unique(uniq >> 8, return_counts=True)
    rich = int(coarse[np.argmax(counts >= 5)])
    assert (counts >= 5).any()
    vals = uniq[(uniq >> 8) == rich][:5]
    five = [int(np.nonzero(d2 == v)[0][0]) for v in vals]
    assert tuple(_ranks(100)) == (93, 94, 95, 96)
    idx = np.array([five[0]] * 93 + [five[1], five[2], five[3]] + [five[4]] * 4)
    regions.append(colours[rng.permutation(idx)]); labels.append("one coarse bin, four fine bins")
    # fine bin 255 cannot be filled: d2 is a sum of three squares, which is never 7 mod 8 (Legendre), and 255 is.  The chart agrees; the
    # highest fine bin that can be reached is 254, alone in a region and above another fine bin of its coarse bin
    assert not ((d2 & 7) == 7).any()
    top = np.nonzero((d2 & 255) == 254)[0]
    assert top.size, "the chart must hold a colour with d2 & 255 == 254"
    regions.append(np.repeat(colours[top[0]][None], 33, axis=0)); labels.append("fine bin 254, flat")
    below = np.nonzero((d2 >> 8 == d2[top[0]] >> 8) & ((d2 & 255) < 254))[0]
    assert below.size
    idx = np.array([int(below[0])] * 95 + [int(top[0])] * 5)
    regions.append(colours[rng.permutation(idx)]); labels.append("fine bin 254 above another fine bin")
    regions.append(np.repeat(colours[hi][None], 7, axis=0)); labels.append("the largest d2")
    page, rois = _stack_regions(regions)
    L, got_d2, order, ranks = _run_dist(lib, page, rois, [bg] * len(rois))
    for k, cols in enumerate(regions):
        want = _d2(hc.rgb_to_lab_u8(cols), bg)
        assert np.array_equal(L.crop(got_d2, k).reshape(-1), want), labels[k]
        assert np.array_equal(order[k], np.sort(want)[ranks[k]]), f"{labels[k]}: order statistics {order[k]}, wanted {np.sort(want)[ranks[k]]}"
    return len(regions)


def check_tc_many_regions(lib, size, n=300):
    """300 regions of mixed sizes (1 x 1 to 40 x 30) in one launch, each with its own background: `blockIdx.y` indexing, per-region zeroing"""
    page, lab = chart(size), chart_lab(size)
    rng = np.random.default_rng(51)
    rois = []
    for k in range(n):
        w, h = (1, 1) if k == 0 else (40, 30) if k == 1 else (int(rng.integers(1, 41)), int(rng.integers(1, 31)))
        rois.append((int(rng.integers(0, size - w + 1)), int(rng.integers(0, size - h + 1)), w, h))
    bgs = rng.integers(0, 256, (n, 3))
    L, d2, order, ranks = _run_dist(lib, page, rois, bgs)
    for k, (x, y, w, h) in enumerate(rois):
        want = _d2(lab[y:y + h, x:x + w], bgs[k])
        assert np.array_equal(L.crop(d2, k), want), f"region {k} {rois[k]}: d2"
        assert np.array_equal(order[k], np.sort(want, axis=None)[ranks[k]]), f"region {k} {rois[k]}: order statistics"
    return n


def _mask_patterns():
    """9 060 binary crops: every pattern on 3 x 3, 2 x 5, 3 x 4 and 1 x 7, 3 000 seeded 4 x 4 patterns, 300 seeded crops up to 11 x 39 (every
    other one transposed)"""
    out = []
    for h, w in ((3, 3), (2, 5), (3, 4), (1, 7)):
        bits = (np.arange(1 << (h * w))[:, None] >> np.arange(h * w)[None, :]) & 1
        out += [b.reshape(h, w).astype(np.uint8) for b in bits]
    rng = np.random.default_rng(61)
    out += [rng.integers(0, 2, (4, 4)).astype(np.uint8) for _ in range(3000)]
    for k in range(300):
        h, w = int(rng.integers(1, 12)), int(rng.integers(1, 40))
        c = (rng.random((h, w)) < rng.uniform(0.1, 0.9)).astype(np.uint8)
        out.append(np.ascontiguousarray(c.T) if k % 2 else c)
    return out


def _close_then_erode(c):
    k3 = np.ones((3, 3), np.uint8)
    return cr.erode(cr.erode(cr.dilate(c, k3), k3), np.ones((2, 2), np.uint8))


def check_tc_mask(lib):
    """MASK on authored d2 planes of 50 and 150 at the cut-offs 100, 149 (150 is above) and 150 (nothing is above): each crop its own region,
    equal to the oracle's close-then-erode; the mask buffer is pre-filled with 7, no 7 remains inside a crop and the gaps keep theirs"""
    pats = _mask_patterns()
    assert len(pats) == 9060
    GAP = 5
    rois = [(0, 0, p.shape[1], p.shape[0]) for p in pats]
    L = TextColorLaunch(lib, np.zeros((40, 40, 3), np.uint8), rois, gap=GAP)
    d2 = np.full(L.total, 1 << 20, np.int32)                             # the gaps read as "far above": a read past a crop would show
    in_crop = np.zeros(L.total, bool)
    for k, p in enumerate(pats):
        o = int(L.offsets[k])
        d2[o:o + p.size] = np.where(p.reshape(-1) != 0, 150, 50)
        in_crop[o:o + p.size] = True
    L.put("d2", d2)
    want_set = [_close_then_erode(p * np.uint8(255)) for p in pats]
    zero = {}
    for cut in (100, 149, 150):
        L.put("cutoff", np.full(L.n, cut, np.int32))
        L.put("mask", np.full(L.total, 7, np.uint8))
        L.run(abi.TC_MASK)
        got = L.get("mask")
        assert not (got[in_crop] == 7).any(), "a crop byte was left unwritten"
        assert (got[~in_crop] == 7).all(), "a byte between two crops was written"
        for k, p in enumerate(pats):
            if cut == 150:
                want = zero.setdefault(p.shape, _close_then_erode(np.zeros(p.shape, np.uint8)))
            else:
                want = want_set[k]
            g = L.crop(got, k)
            assert np.array_equal(g, want), f"cut-off {cut}, crop {k} {p.shape}:\n{p}\ngot\n{g // 255}\nwanted\n{want // 255}"
    return len(pats)


def check_tc_hist(lib, size):
    """HIST under authored masks (stripes, one pixel, empty, full) over chart regions, two of them across the page edge: the 768 counts equal
    numpy's per-channel bincount of the padded crop; the output is pre-filled with garbage (the launch zeroes it)"""
    page = chart(size)
    rois = [(5, 7, 64, 48), (100, 200, 33, 17), (300, 40, 25, 25), (0, 0, 257, 3), (size - 30, 50, 34, 21), (-3, size - 10, 40, 13)]
    kinds = ["stripes", "one pixel", "empty", "full", "stripes", "full"]
    L = TextColorLaunch(lib, page, rois, gap=3)
    mask = np.full(L.total, 255, np.uint8)
    masks = []
    for k, (x, y, w, h) in enumerate(rois):
        yy, xx = np.mgrid[0:h, 0:w]
        m = {"stripes": (xx + 2 * yy) % 3 == 0, "one pixel": (xx == w - 1) & (yy == h - 1), "empty": np.zeros((h, w), bool), "full": np.ones((h, w), bool)}[kinds[k]]
        masks.append(m)
        mask[int(L.offsets[k]):int(L.offsets[k]) + w * h] = np.where(m.reshape(-1), 255 if k % 2 else 1, 0)
    L.put("mask", mask)
    L.put("hist", np.full((L.n, 768), 999, np.int32))
    L.run(abi.TC_HIST)
    got = L.get("hist")
    for k, (x, y, w, h) in enumerate(rois):
        px = _padded_crop(page, x, y, w, h)[masks[k]]
        want = np.concatenate([np.bincount(px[:, c], minlength=256) for c in range(3)])
        assert np.array_equal(got[k], want), f"region {k} ({kinds[k]}, {rois[k]}): {np.nonzero(got[k] != want)[0][:8]}"
    return len(rois)


# =================================================================================================================================
# 3. page tail: mtx_page_tail through DeviceTail and direct calls
# =================================================================================================================================
def _antidiagonal_mask(size):
    yy, xx = np.mgrid[0:size, 0:size]
    return np.where((xx + yy) % 3 == 0, 255, 0).astype(np.uint8)           # every third anti-diagonal masked


def _lab_stats(tail, src, other, mask):
    sums = torch.full((9,), 0, dtype=torch.int64, device=tail.device)
    a = tail._lab_args(abi.TAIL_LAB_STATS, src, mask)
    a.dst = src.data_ptr()
    a.other, a.ld_other, a.sums = other.data_ptr(), other.shape[1] * 3, sums.data_ptr()
    tail._run(a)
    return [int(v) for v in sums.cpu().tolist()]


def check_lab_stats(lib, size):
    """the nine context sums over the chart and its vertical flip equal numpy's int64 sums; all masked: zero; nothing masked: n = pixels"""
    dev = _dev(lib)
    tail = DeviceTail(lib, dev)
    src, other = chart(size), np.ascontiguousarray(chart(size)[::-1])
    ls, lo = chart_lab(size).astype(np.int64), chart_lab(size)[::-1].astype(np.int64)
    src_d, other_d = _up(src, dev), _up(other, dev)
    for name, mask in (("anti-diagonals", _antidiagonal_mask(size)), ("all masked", np.full((size, size), 1, np.uint8)), ("unmasked", np.zeros((size, size), np.uint8))):
        ctx = mask == 0
        want = [int(ctx.sum()), int(ls[..., 0][ctx].sum()), int((ls[..., 0][ctx] ** 2).sum()), int(ls[..., 1][ctx].sum()), int(ls[..., 2][ctx].sum()),
                int(lo[..., 0][ctx].sum()), int((lo[..., 0][ctx] ** 2).sum()), int(lo[..., 1][ctx].sum()), int(lo[..., 2][ctx].sum())]
        got = _lab_stats(tail, src_d, other_d, _up(mask, dev))
        assert got == want, f"{name}: {got} != {want}"
        if name == "all masked":
            assert got == [0] * 9
        if name == "unmasked":
            assert got[0] == size * size


# {g_mean, gain, o_mean, shift_a, shift_b, use_a, use_b}
REMAP_PARAMS = {                        # clip_high: L and a clip at 255, b at 0; clip_low_b_off: L clips at 0, b's shift must be ignored
    "identity": (0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0),
    "clip_high": (0.0, 2.0, 60.0, 100.0, -100.0, 1.0, 1.0),
    "clip_low_b_off": (200.0, 1.5, 10.0, -5.0, 50.0, 1.0, 0.0),
    "fractional": (117.3, 0.83, 131.7, 2.4, -3.6, 1.0, 1.0),
}
REMAP_MAX_SHARE = 1e-3


def remap_lab_f32(lab_u8, params):
    """the reference's remap (core/image/inpainting.py `_match_luminance`) in numpy float32, its operation order, its truncation to uint8"""
    f32 = np.float32
    g_mean, gain, o_mean, sa, sb, use_a, use_b = (f32(v) for v in params)
    lab = lab_u8.astype(f32)
    lab[..., 0] = np.clip((lab[..., 0] - g_mean) * gain + o_mean, 0, 255)
    if use_a != 0:
        lab[..., 1] = np.clip(lab[..., 1] + sa, 0, 255)
    if use_b != 0:
        lab[..., 2] = np.clip(lab[..., 2] + sb, 0, 255)
    return lab.astype(np.uint8)


def lab_to_rgb_f64(lab_u8):
    """Lab -> sRGB bytes with the formulas and decimal constants of core/image/color.lab_to_rgb_u8, every step in float64"""
    v = lab_u8.astype(np.float64)
    L, A, B = v[..., 0] * (100.0 / 255.0), v[..., 1] - 128.0, v[..., 2] - 128.0
    low = L <= 0.008856 * 903.3
    fy_hi = (L + 16.0) / 116.0
    y = np.where(low, L / 903.3, fy_hi ** 3)
    fy = np.where(low, 7.787 * (L / 903.3) + 16.0 / 116.0, fy_hi)
    inv_f = lambda f: np.where(f <= 7.787 * 0.008856 + 16.0 / 116.0, (f - 16.0 / 116.0) / 7.787, f ** 3)
    x, z = inv_f(fy + A / 500.0) * 0.950456, inv_f(fy - B / 200.0) * 1.088754
    M = ((3.240479, -1.53715, -0.498535), (-0.969256, 1.875991, 0.041556), (0.055648, -0.204043, 1.057311))
    out = np.empty(lab_u8.shape, np.uint8)
    for r in range(3):
        lin = np.clip(M[r][0] * x + M[r][1] * y + M[r][2] * z, 0.0, 1.0)
        g = np.where(lin <= 0.0031308, lin * 12.92, 1.055 * np.power(lin, 1.0 / 2.4) - 0.055)
        out[..., r] = np.clip(np.rint(g * 255.0), 0, 255)
    return out


@lru_cache(maxsize=None)
def _remap_witness(size, name):
    """(float64-evaluated witness, host float32 path) of the chart with every pixel remapped by the named parameter set"""
    lab = remap_lab_f32(chart_lab(size).astype(np.uint8), REMAP_PARAMS[name])
    return lab_to_rgb_f64(lab), hc.lab_to_rgb_u8(lab)


def _share(got, want):
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    return int(d.max()) if d.size else 0, float((d != 0).mean()) if d.size else 0.0


def check_lab_remap(lib, size, name):
    """LAB_REMAP of the chart with one parameter set, under an all-ones mask and under the anti-diagonal mask.  Witness: the remap in numpy
    float32 with the reference's order and truncation, then Lab -> RGB evaluated in float64.  Conditions: no byte off by more than one
    level; at most 1e-3 of the bytes differ; unmasked pixels obey both against the identity.  The cap is a condition, not a measurement:
    the host float32 path differs from the float64 evaluation on fewer than 2.5e-5 of these bytes (asserted below, so the inputs prove
    themselves), while the smallest real error — one level in L under the sparse mask — moves 0.11 of them.
    Returns {mask name: (device share, host float32 share)}."""
    dev = _dev(lib)
    tail = DeviceTail(lib, dev)
    src = _up(chart(size), dev)
    remapped, host_remapped = _remap_witness(size, name)
    identity, host_identity = _remap_witness(size, "identity")
    params = torch.tensor(list(REMAP_PARAMS[name]) + [0.0], dtype=torch.float32).to(dev)
    out_shares = {}
    for mask_name, mask in (("all ones", np.ones((size, size), np.uint8)), ("anti-diagonals", _antidiagonal_mask(size))):
        m = mask != 0
        want = np.where(m[..., None], remapped, identity)
        host = np.where(m[..., None], host_remapped, host_identity)
        host_max, host_share = _share(host, want)
        assert host_max <= 1 and host_share <= REMAP_MAX_SHARE, f"{name}, {mask_name}: the host float32 path itself is off: max {host_max}, share {host_share:.3g}"
        mask_d = _up(mask, dev)
        out = torch.full((size, size, 3), 77, dtype=torch.uint8, device=dev)
        a = tail._lab_args(abi.TAIL_LAB_REMAP, src, mask_d)
        a.dst, a.ld_dst, a.params = out.data_ptr(), size * 3, params.data_ptr()
        tail._run(a)
        got = out.cpu().numpy()
        dmax, share = _share(got, want)
        print(f"lab remap '{name}', mask {mask_name}, {size} x {size}: device share {share:.3g} (max {dmax}), host float32 share {host_share:.3g}")
        assert dmax <= 1, f"{name}, {mask_name}: a byte is off by {dmax} levels"
        assert share <= REMAP_MAX_SHARE, f"{name}, {mask_name}: {share:.3g} of the bytes differ"
        umax, ushare = _share(got[~m], identity[~m])
        assert umax <= 1 and ushare <= REMAP_MAX_SHARE, f"{name}, {mask_name}: unmasked pixels: max {umax}, share {ushare:.3g}"
        out_shares[mask_name] = (share, host_share)
    return out_shares


def check_composite_exact(lib):
    """every (patch byte, page byte) pair at alpha 0, 1, the smallest subnormal, nextafter(1, 0), 0.5 and seeded values, on 3- and 4-channel
    pages, the window on the page's last row and column: equal to `composite_u8`"""
    dev = _dev(lib)
    tail = DeviceTail(lib, dev)
    ii, jj = np.mgrid[0:256, 0:256]
    patch = np.stack([(ii + 85 * c) & 255 for c in range(3)], -1).astype(np.uint8)
    rng = np.random.default_rng(71)
    alphas = [np.full((256, 256), v, np.float32) for v in (0.0, 1.0, np.float32(1e-45), np.nextafter(np.float32(1), np.float32(0)), 0.5)]
    alphas.append(rng.random((256, 256), dtype=np.float32))
    assert alphas[2][0, 0] > 0 and alphas[3][0, 0] < 1
    PH, PW, x, y = 300, 280, 24, 44
    n = 0
    for page_c in (3, 4):
        page = rng.integers(0, 256, (PH, PW, page_c), dtype=np.uint8)
        page[y:, x:] = np.stack([(jj + 51 * c) & 255 for c in range(page_c)], -1).astype(np.uint8)
        for alpha in alphas:
            ref = ip.composite_u8(page, patch, alpha, x, y)
            got = tail.composite(_up(page.copy(), dev), _up(patch, dev), _up(alpha, dev), x, y).cpu().numpy()
            assert np.array_equal(got, ref), f"{page_c}-channel page, alpha {alpha[0, 0]}: {(got != ref).sum()} bytes differ"
            n += 1
    return n


def check_feather_extremes(lib):
    """the feather weight at the largest radius the launcher takes (254) on a 40 x 300 crop with one masked pixel (in the first row, then in the
    last row and column: the window's bounds checks), and radius 1 on a 1 x 1 and a 1 x 600 crop, against `_crop_alpha` as float32 bit patterns"""
    dev = _dev(lib)
    tail = DeviceTail(lib, dev)
    for (h, w), (py, px), R in (((40, 300), (0, 31), 254), ((40, 300), (39, 299), 254), ((1, 1), (0, 0), 1), ((1, 600), (0, 299), 1)):
        m = np.zeros((h, w), bool)
        m[py, px] = True
        ref = ip.FluxKleinInpainter._crop_alpha(m, R)
        got = tail.feather(_up(m.astype(np.uint8), dev), R).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.astype(np.float32).view(np.uint32)), \
            f"{h} x {w}, R = {R}: {(got != ref).sum()} weights differ"
        assert R == 1 or (ref > 0).sum() > 10000


def _resample_pass(lib, dev, src, n_out, axis):
    """one pass of the 16-bit-tap form of RESAMPLE: axis 0 = horizontal, 1 = vertical"""
    H, W, Cn = src.shape
    b, taps, ksize, bits = aten_aa_bilinear_tables(W if axis == 0 else H, n_out)
    oh, ow = (H, n_out) if axis == 0 else (n_out, W)
    out = torch.full((oh, ow, Cn), 99, dtype=torch.uint8, device=dev)
    bd, td = _up(b, dev), _up(taps, dev)
    a = abi.TailArgs()
    a.kind, a.src, a.dst = abi.TAIL_RESAMPLE, src.data_ptr(), out.data_ptr()
    a.out_h, a.out_w, a.c, a.ld_src, a.ld_dst = oh, ow, Cn, W * Cn, ow * Cn
    a.bounds, a.coeff, a.ksize, a.axis, a.src_row0, a.coeff_bits = bd.data_ptr(), td.data_ptr(), ksize, axis, 0, bits
    lib.check(lib.mtx_page_tail(C.byref(a), _stream(lib, dev)), "mtx_page_tail")
    return out, bits


def check_resample_16bit(lib):
    """the 16-bit-tap resample (ATen's uint8 antialiased bilinear) on a 97 x 61 image of 0 / 255 checkers, both axes, down and up, against
    torch's CPU `interpolate(antialias=True)` on uint8"""
    dev = _dev(lib)
    H, W = 97, 61
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([((xx // 8 + yy // 8) % 2) * 255, ((xx + yy) % 2) * 255, ((xx // 3 + yy // 11) % 2) * 255], -1).astype(np.uint8)
    src = _up(img, dev)
    seen_bits = set()
    for oh, ow in ((40, 23), (150, 131), (97, 30), (200, 61), (31, 140)):
        t = torch.from_numpy(img).permute(2, 0, 1)[None]
        want = F.interpolate(t, (oh, ow), mode="bilinear", antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()
        cur = src
        if ow != W:
            cur, bits = _resample_pass(lib, dev, cur, ow, 0)
            seen_bits.add(bits)
        if oh != H:
            cur, bits = _resample_pass(lib, dev, cur, oh, 1)
            seen_bits.add(bits)
        got = cur.cpu().numpy()
        assert np.array_equal(got, want), f"97 x 61 -> {oh} x {ow}: {(got != want).sum()} bytes differ"
        assert want.min() == 0 and want.max() == 255
    assert all(0 < b < 22 for b in seen_bits) and len(seen_bits) >= 2
