"""CPU tier, kernel simulator: the text-colour probe (`core/image/text_color.py` over csrc/textcolor.hip and `mtx_host_fill_components`)
equals, exactly, the reference's expression (core/outside_text_processor.py:1096-1165) restated in tests/text_color_checks.py from
the oracle primitives and numpy — on the regions of the payload fixture page and on seeded random rectangles (1 x 1 up to 300 x 200,
some touching or crossing the page edge).  Every stage is compared: squared distances, the percentile and threshold numpy computes from
the device's order statistics (type and value), the mask after MASK and after the contour fill byte for byte, the colour."""
import sys
from pathlib import Path

import numpy as np
import pytest

G = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(G))
import osb_payload_page as pp  # noqa: E402
import text_color_checks as tc  # noqa: E402

from mangatranslator_amd.core import outside_text_processor as otp  # noqa: E402
from mangatranslator_amd.core.image import text_color  # noqa: E402


def fixture_regions():
    page = pp.make_page()
    regions = []
    for box in pp.OSB:
        x0, y0, x1, y1 = (int(v) for v in box)
        ring = otp.border_ring_pixels(page, x0, y0, x1, y1, pp.W, pp.H)
        regions.append(((x0, y0, x1, y1), tuple(int(v) for v in np.median(ring, axis=0).astype(np.uint8))))
    return np.array(page), regions


def test_fixture_regions_match_the_restatement(emu_lib):
    page, regions = fixture_regions()
    got = tc.assert_probe_matches(page, regions, emu_lib)
    found = [c for c in got if c is not None]
    snapped = [c for c in found if c in ((0, 0, 0), (255, 255, 255))]
    assert len(found) >= 5 and len(snapped) >= 2 and len(found) - len(snapped) >= 2 and len(found) < len(got), got


def test_random_rectangles_match_the_restatement(emu_lib):
    page = tc.seeded_page(5, 640, 480)
    regions = tc.random_regions(9, page, 20)
    sizes = {(r[2] - r[0], r[3] - r[1]) for r, _ in regions}
    assert (1, 1) in sizes and (300, 200) in sizes
    assert any(r[0] < 0 or r[1] < 0 or r[2] > 640 or r[3] > 480 for r, _ in regions)
    got = tc.assert_probe_matches(page, regions, emu_lib)
    assert sum(c is not None for c in got) >= 8


def test_degenerate_rectangles_need_no_launch(emu_lib):
    page = tc.seeded_page(1, 64, 48)
    before = dict(text_color.stats)
    assert text_color.probe_text_colors(page, [((5, 5, 5, 20), (0, 0, 0)), ((9, 9, 3, 12), (1, 2, 3))], lib=emu_lib) == [None, None]
    assert text_color.probe_text_colors(page, [], lib=emu_lib) == []
    assert text_color.stats == before
    got = text_color.probe_text_colors(page, [((5, 5, 5, 20), (0, 0, 0)), ((0, 0, 64, 48), (255, 255, 255))], lib=emu_lib)
    assert got[0] is None and text_color.stats["launches"] == before["launches"] + 3 and text_color.stats["regions"] == before["regions"] + 1


def test_launch_count_does_not_depend_on_the_region_count(emu_lib):
    page = tc.seeded_page(2, 320, 240)
    regions = tc.random_regions(4, page, 12, max_w=80, max_h=60)
    n0 = text_color.stats["launches"]
    text_color.probe_text_colors(page, regions[:1], lib=emu_lib)
    one = text_color.stats["launches"] - n0
    text_color.probe_text_colors(page, regions, lib=emu_lib)
    assert text_color.stats["launches"] - n0 - one == one == 3


@pytest.mark.parametrize("n", [1, 2, 3, 20, 21, 41, 1000, 60000])
def test_percentile_from_order_statistics(n):
    """the host step alone: `np.percentile` of a random float32 distance map == the stand-in built from four order statistics"""
    rng = np.random.default_rng(n)
    d2 = rng.integers(0, 195076, n).astype(np.int32)
    ranks = text_color._ranks(n)
    order = np.sort(d2)[ranks]
    cut, p95, thr = text_color.contrast_cutoff(n, ranks, order)
    dist = np.sqrt(d2.astype(np.float32))
    want = np.percentile(dist, 95)
    assert type(p95) is type(want) and p95 == want
    assert np.array_equal(d2 > cut, dist > max(30, want * 0.6))


def test_median_and_snap():
    h = np.zeros(256, np.int64)
    h[[10, 20, 31]] = [1, 1, 2]
    assert text_color.median_from_hist(h) == int(np.median([10, 20, 31, 31]))
    h[200] = 1
    assert text_color.median_from_hist(h) == 31
    assert text_color.snap_low_saturation((90, 90, 90)) == (0, 0, 0) and text_color.snap_low_saturation((240, 240, 235)) == (255, 255, 255)
    assert text_color.snap_low_saturation((200, 30, 30)) == (200, 30, 30) and text_color.snap_low_saturation((0, 0, 0)) == (0, 0, 0)
