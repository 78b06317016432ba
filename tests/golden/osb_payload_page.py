"""The synthetic page + canned detector outputs + stand-in inpainter of the OSB PAYLOAD golden (translation payload, rendered-text
colours, `needs_text_background`, grouped FLUX), shared by the generator (tests/golden/make_osb_payload_goldens.py, which runs the
REFERENCE on it) and the tests (tests/test_osb_payload.py, tests/test_osb_payload_gpu.py, tests/test_integration_osb.py).

The page of osb_page.py does not exercise the colour probe: its 2-pixel strokes do not survive the 2x2 erode and the area test.  This
one carries 5-pixel strokes in colours that are kept (saturated, on white / texture / grey / near-black), colours that are snapped to
black / white (grey and near-white on texture), faint strokes on a flat block whose 95th-percentile distance stays below 50, so the
floor of 30 decides, and boxes with 2-pixel strokes (no colour)."""
import types

import numpy as np
from PIL import Image

import osb_page

W, H = osb_page.W, osb_page.H
BUBBLES, TEXT_FREE, PANELS, SEED = osb_page.BUBBLES, osb_page.TEXT_FREE, osb_page.PANELS, osb_page.SEED
FLAT_BLOCK = (308, 182, 398, 300)           # x0, y0, x1, y1 of a flat (200, 180, 160) block that holds the low-contrast box
# text boxes as the (stand-in) OSB text model reports them, and what is drawn into each: (stroke colour or None = by background, thickness)
OSB = osb_page.OSB + [[320.0, 196.0, 386.0, 288.0]]     # R10 on the flat block, faint strokes -> solid ring, flat fill
OSB_CONF = osb_page.OSB_CONF + [0.75]
STROKES = [((200, 30, 30), 5),              # R0  saturated red on white                  -> colour kept
           ((30, 60, 200), 5),              # R1  saturated blue on texture (group of two) -> colour kept
           ((30, 60, 200), 5),              # R1b
           ((90, 90, 90), 5),               # R2  grey on texture                          -> snapped to black
           ((240, 240, 235), 5),            # R3  near-white on texture                    -> snapped to white
           ((20, 150, 40), 5),              # R4  green on grey 120                        -> colour kept
           ((250, 220, 0), 5),              # R5  yellow on near-black                     -> colour kept
           (None, 2),                       # R6  hugging bubble B1: nothing left after the guard mask
           (None, 2),                       # R7  2-pixel strokes                          -> no colour
           ((200, 30, 30), 5),              # R8  the per-region FLUX call raises
           (None, 2),                       # R9  2-pixel strokes, FLUX hands the page back -> no colour
           ((150, 132, 115), 5)]            # R10 faint on the flat block: p95 distance 46 < 50 -> the floor of 30 decides; colour kept


def make_page() -> Image.Image:
    yy, xx = np.mgrid[0:H, 0:W]
    tex = ((xx * 7 + yy * 13) % 97 + 80).astype(np.uint8)                   # deterministic non-solid texture
    page = np.stack([tex, np.roll(tex, 5, axis=1), np.roll(tex, 9, axis=0)], axis=-1)
    page[0:180, 0:360] = 255                                                # white area (bubble B0 and R0 live here)
    page[360:450, 230:370] = 120                                            # grey block (not 128: BT.601 luma of 128 sits on the dark / light border)
    page[420:480, 0:140] = 5                                                # near-black block
    page[20:130, 410:570] = 250                                             # near-white area around bubble B1
    fx0, fy0, fx1, fy1 = FLAT_BLOCK
    page[fy0:fy1, fx0:fx1] = (200, 180, 160)
    for (x0, y0, x1, y1), (color, thick) in zip(OSB, STROKES):
        for k in range(3):
            y = int(y0 + (k + 1) * (y1 - y0) / 4)
            c = color if color is not None else ((20,) * 3 if page[y, int(x0) + 3, 0] > 60 else (230,) * 3)
            page[y:y + thick, int(x0) + 3:max(int(x0) + 4, int(x1) - 3)] = c
    return Image.fromarray(page)


bubble_data = osb_page.bubble_data


def make_config(coordinator, method="flux_kontext", upscale_method="none", osb_min_side_pixels=120, test_mode=False, **over):
    cfg = osb_page.make_config(coordinator, method, **over)
    cfg.translation = types.SimpleNamespace(upscale_method=upscale_method, osb_min_side_pixels=osb_min_side_pixels)
    cfg.test_mode = test_mode
    return cfg


# tag -> (inpainting method, coordinator?, image format, config keywords, grouped call fails?)
RUNS = {
    "flux": ("flux_kontext", True, "PNG", dict(upscale_method="none"), False),
    "none_mode": ("none", True, "JPEG", dict(upscale_method="lanczos"), False),
    "opencv_model": ("opencv", False, "PNG", dict(upscale_method="model"), False),
    "group_coordinator": ("flux_kontext", True, "PNG", dict(upscale_method="model", test_mode=True, flux_group_regions=True), False),
    "group_no_coordinator": ("flux_kontext", False, "JPEG", dict(upscale_method="other", flux_group_regions=True), False),
    "group_raises": ("flux_kontext", True, "PNG", dict(upscale_method="none", flux_group_regions=True), True),
}


class StandInInpainter:
    """osb_page's deterministic stand-in (paints the clipped mask with a function of position and seed; the region whose clip box starts
    at x = 215 raises, the one starting at x = 212 hands the page back untouched), which also records `ocr_params` and, with
    `fail_group` set, raises on the grouped call"""
    calls = []
    fail_group = False

    def __init__(self, **kw):
        self.kw = kw

    def inpaint_mask(self, image_pil, mask_np, seed=1, verbose=False, ocr_params=None, strict_mask_clipping=False, composite_clip_bbox=None):
        m = np.asarray(mask_np).astype(bool).copy()
        ys, xs = np.nonzero(m)
        StandInInpainter.calls.append(dict(seed=int(seed), clip=[int(v) for v in composite_clip_bbox] if composite_clip_bbox else None,
                                           mask_bbox=[int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1], area=int(m.sum()),
                                           strict=bool(strict_mask_clipping), ocr_params=dict(ocr_params) if ocr_params else None))
        if ocr_params and ocr_params.get("type") == "outside_text_group" and StandInInpainter.fail_group:
            raise RuntimeError("stand-in group failure")
        if composite_clip_bbox and composite_clip_bbox[0] == 215:
            raise RuntimeError("stand-in failure")
        if composite_clip_bbox and composite_clip_bbox[0] == 212:
            return image_pil
        if strict_mask_clipping and composite_clip_bbox:
            x0, y0, x1, y1 = composite_clip_bbox
            clip = np.zeros_like(m)
            clip[max(0, y0):max(0, y1), max(0, x0):max(0, x1)] = True
            m &= clip
        arr = np.array(image_pil.convert("RGB"))
        ys, xs = np.nonzero(m)
        for c in range(3):
            arr[ys, xs, c] = (xs * 3 + ys * 5 + seed * 7 + c * 40) % 256
        return Image.fromarray(arr)


def sorted_calls():
    return sorted(StandInInpainter.calls, key=lambda c: (c["seed"], c["ocr_params"] is not None))
