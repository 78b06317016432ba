"""MI355X tier: the text-colour probe on the product library (csrc/textcolor.hip on gfx950) — the comparisons of
tests/test_text_color_sim.py (fixture regions and seeded random rectangles vs the restatement of the reference's expression, every stage
exact) and of tests/test_osb_payload.py (the reference's golden runs of the OSB stage with the payload), plus one seeded page of
2048 x 3072 with 24 regions.  Reads nothing outside the repository."""
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch

G = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(G))
import text_color_checks as tc  # noqa: E402
from test_osb_payload import GOLD, Rig, check_run  # noqa: E402
from test_text_color_sim import fixture_regions  # noqa: E402

from mangatranslator_amd.core.image import text_color  # noqa: E402

pytestmark = pytest.mark.gpu


def test_fixture_regions_match_the_restatement_on_gpu(hip_lib):
    page, regions = fixture_regions()
    got = tc.assert_probe_matches(page, regions, hip_lib, device="cuda")
    assert sum(c is not None for c in got) >= 5


def test_random_rectangles_match_the_restatement_on_gpu(hip_lib):
    page = tc.seeded_page(5, 640, 480)
    regions = tc.random_regions(9, page, 20)
    got = tc.assert_probe_matches(page, regions, hip_lib, device="cuda")
    assert sum(c is not None for c in got) >= 8


@pytest.mark.parametrize("tag", list(GOLD))
def test_payload_matches_reference_on_gpu(monkeypatch, hip_lib, tag):
    check_run(Rig(monkeypatch, hip_lib), tag)


def test_large_page_24_regions(hip_lib):
    """2048 x 3072, 24 regions: exact against the restatement, the page adopted as a device tensor; the launch count for 24 regions is
    the count for one; for the record, the probe's wall time next to the host restatement's"""
    W, H = 2048, 3072
    page = tc.seeded_page(17, W, H)
    regions = tc.random_regions(23, page, 24)
    page_d = torch.from_numpy(page).to("cuda")
    n0 = text_color.stats["launches"]
    text_color.probe_text_colors(page_d, regions[1:2], lib=hip_lib)                       # also warms the tables up
    one = text_color.stats["launches"] - n0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = text_color.probe_text_colors(page_d, regions, lib=hip_lib)
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    assert text_color.stats["launches"] - n0 - one == one == 3
    t0 = time.perf_counter()
    want = [tc.reference_probe(page, rect, bg)["color"] for rect, bg in regions]
    t_host = time.perf_counter() - t0
    print(f"text colour probe, 2048x3072, 24 regions ({sum((r[2] - r[0]) * (r[3] - r[1]) for r, _ in regions)} crop pixels): "
          f"device path {t_dev * 1e3:.2f} ms (3 launches + host contour step), host restatement (numpy + Python contours) {t_host * 1e3:.1f} ms")
    assert got == want
    assert tc.assert_probe_matches(page, regions, hip_lib, page_arg=page_d) == want
    assert sum(c is not None for c in got) >= 10
