"""Shared by tests/test_text_color_sim.py (CPU, kernel simulator) and tests/test_osb_payload_gpu.py (MI355X): the reference's text-colour
expression (core/outside_text_processor.py:1096-1165) restated over the oracle primitives (oracle/cv2_color_ref.py, oracle/cleaning_ref.py)
and numpy, seeded pages with text-like strokes, and the exact comparison of `probe_text_colors` against it — distance map, percentile,
threshold, the mask after MASK and after the fill byte for byte, and the colour."""
import sys
from pathlib import Path

import numpy as np
from PIL import Image

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle import cleaning_ref as cr  # noqa: E402
from oracle import cv2_color_ref as cc  # noqa: E402


def lab_u8(rgb: np.ndarray) -> np.ndarray:
    """oracle RGB -> Lab (a per-pixel Python loop) through the image's distinct colours"""
    flat = np.ascontiguousarray(rgb.reshape(-1, 3))
    uniq, inv = np.unique(flat, axis=0, return_inverse=True)
    return cc.rgb_to_lab_u8(uniq.reshape(-1, 1, 3)).reshape(-1, 3)[np.asarray(inv).reshape(-1)].reshape(rgb.shape)


def reference_probe(page: np.ndarray, rect, bg_rgb):
    """the reference's statements, cv2 calls replaced by the oracle's restatements; returns dict(color, dist, p95, threshold, mask, filled)"""
    crop_rgb = np.array(Image.fromarray(page).crop(tuple(int(v) for v in rect)).convert("RGB"))
    bg = np.asarray(bg_rgb).astype(np.uint8)
    bg_lab = lab_u8(np.uint8([[bg]]))[0][0]
    crop_lab = lab_u8(crop_rgb).astype(np.float32)
    dist_map = np.linalg.norm(crop_lab - bg_lab.astype(np.float32), axis=2)
    p95 = np.percentile(dist_map, 95)
    threshold = max(30, p95 * 0.6)
    contrast = (dist_map > threshold).astype(np.uint8) * 255
    k3 = np.ones((3, 3), np.uint8)
    contrast = cr.erode(cr.dilate(contrast, k3), k3)                       # MORPH_CLOSE
    contrast = cr.erode(contrast, np.ones((2, 2), np.uint8), iterations=1)
    clean = np.zeros_like(contrast)
    for cnt in cr.find_external_contours(contrast):
        if cr.contour_area(cnt) >= 4:
            clean |= cr.draw_filled([cnt], contrast.shape)
    px = crop_rgb[clean == 255]
    color = None
    if len(px) >= 10:
        color = tuple(int(v) for v in np.median(px, axis=0).astype(int))
        if cr.bgr_pixel_saturation(color[2], color[1], color[0]) < 25:
            color = (0, 0, 0) if max(color) < 128 else (255, 255, 255)
    return dict(color=color, dist=dist_map, p95=p95, threshold=threshold, mask=contrast, filled=clean)


def seeded_page(seed: int, w: int, h: int) -> np.ndarray:
    """colour page from a small palette: flat and textured blocks, a few speckles"""
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (48, 3)).astype(np.uint8)
    pal[:4] = [[255, 255, 255], [0, 0, 0], [128, 128, 128], [250, 250, 245]]
    yy, xx = np.mgrid[0:h, 0:w]
    idx = ((xx // 61 + 3 * (yy // 47)) % 12).astype(np.int64)
    tex = (xx * 7 + yy * 13) % 5 == 0
    idx = np.where(tex & ((xx // 61) % 2 == 1), idx + 12, idx)
    page = pal[idx]
    sp = rng.random((h, w)) < 0.002
    page[sp] = pal[rng.integers(24, 48, int(sp.sum()))]
    return np.ascontiguousarray(page)


def draw_strokes(page: np.ndarray, rect, color, thick: int, rng) -> None:
    """a few horizontal and vertical bars inside rect (clipped to the page)"""
    H, W = page.shape[:2]
    x0, y0, x1, y1 = (int(v) for v in rect)
    for k in range(3):
        y = y0 + (k + 1) * (y1 - y0) // 4
        ya, yb, xa, xb = max(0, y), min(H, y + thick), max(0, x0 + 2), min(W, x1 - 2)
        if yb > ya and xb > xa:
            page[ya:yb, xa:xb] = color
    x = x0 + int(rng.integers(2, max(3, x1 - x0 - 2)))
    xa, xb, ya, yb = max(0, x), min(W, x + thick), max(0, y0 + 1), min(H, y1 - 1)
    if yb > ya and xb > xa:
        page[ya:yb, xa:xb] = color


def random_regions(seed: int, page: np.ndarray, n: int, max_w: int = 300, max_h: int = 200):
    """n seeded rectangles (1 x 1 up to max_w x max_h, some touching or crossing the page edge) with strokes drawn into the page, and a
    background colour each (the colour of the rectangle's corner pixel, or a random one)"""
    rng = np.random.default_rng(seed)
    H, W = page.shape[:2]
    stroke_colors = [(200, 30, 30), (30, 60, 200), (90, 90, 90), (240, 240, 235), (20, 150, 40), (250, 220, 0), (10, 10, 10)]
    regions = []
    for k in range(n):
        if k == 0:
            w, h = 1, 1
        elif k == 1:
            w, h = max_w, max_h
        elif k == 2:
            w, h = 2, 37
        else:
            w, h = int(rng.integers(1, max_w + 1)), int(rng.integers(1, max_h + 1))
        x0, y0 = int(rng.integers(0, max(1, W - w + 1))), int(rng.integers(0, max(1, H - h + 1)))
        if k % 5 == 3:
            x0 = 0
        if k % 5 == 4:
            x0, y0 = W - w, H - h
        if k % 7 == 6:
            x0, y0 = W - w + 3, -2                                            # crosses the page edge: black padding
        rect = (x0, y0, x0 + w, y0 + h)
        draw_strokes(page, rect, stroke_colors[k % len(stroke_colors)], int(rng.integers(1, 7)), rng)
        if k % 3 == 0:
            bg = tuple(int(v) for v in rng.integers(0, 256, 3))
        else:
            bg = tuple(int(v) for v in page[min(H - 1, max(0, y0)), min(W - 1, max(0, x0))])
        regions.append((rect, bg))
    return regions


def assert_probe_matches(page: np.ndarray, regions, lib, device=None, page_arg=None):
    """runs the probe once for all regions; compares every stage of every region with the restatement; returns the colours"""
    from mangatranslator_amd.core.image.text_color import probe_text_colors
    trace = []
    got = probe_text_colors(page if page_arg is None else page_arg, regions, lib=lib, device=device, trace=trace)
    assert len(got) == len(regions) and len(trace) == len(regions)
    for t in trace:
        rect, bg = regions[t["index"]]
        ref = reference_probe(page, rect, bg)
        tag = f"region {t['index']} {rect}"
        assert np.array_equal(np.sqrt(t["d2"].astype(np.float32)), ref["dist"]), tag
        assert type(t["p95"]) is type(ref["p95"]) and t["p95"] == ref["p95"], tag
        assert type(t["threshold"]) is type(ref["threshold"]) and t["threshold"] == ref["threshold"], tag
        assert np.array_equal(t["d2"] > t["cutoff"], ref["dist"] > ref["threshold"]), tag
        assert np.array_equal(t["mask"], ref["mask"]), tag
        assert np.array_equal(t["filled"], ref["filled"]), tag
        assert got[t["index"]] == ref["color"], tag
    return got
