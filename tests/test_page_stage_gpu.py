"""GPU tier: the exact-input checks of the page-stage byte kernels (tests/page_stage_checks.py) on gfx950 — csrc/clean.hip, csrc/textcolor.hip
and csrc/pagetail.hip, every kernel stage by stage against the oracles, numpy, scipy and torch's CPU resize.  The colour chart is
1536 x 1536 = 2 359 296 pixels: the tail kernels' grid is capped at 8192 blocks of 256, so their grid-stride loop takes a second trip."""
import pytest

import page_stage_checks as ps

pytestmark = pytest.mark.gpu

CHART = ps.CHART_FULL


# ---- cleaning ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page, elements, otsu, shrink", ps.clean_cases())
def test_clean_planes_and_statistics(hip_lib, page, elements, otsu, shrink):
    ps.check_clean_case(hip_lib, page, elements, otsu, shrink)


def test_clean_polarity_at_the_midpoint(hip_lib):
    ps.check_clean_polarity_pages(hip_lib)


def test_clean_junction_zones(hip_lib):
    ps.check_clean_junction_zones(hip_lib)


def test_clean_sweep_count_closed_form(hip_lib):
    ps.check_clean_sweep_count(hip_lib)


def test_clean_cross_block_atomics_and_relaunch(hip_lib):
    ps.check_clean_cross_block_atomics(hip_lib)


# ---- text colour ------------------------------------------------------------------------------------------------------------------
def test_text_color_dist_on_the_chart(hip_lib):
    ps.check_tc_dist_chart(hip_lib, CHART)


def test_text_color_rank_selection_edges(hip_lib):
    assert ps.check_tc_order_edges(hip_lib, CHART) >= 17


def test_text_color_300_regions_in_one_launch(hip_lib):
    ps.check_tc_many_regions(hip_lib, CHART)


def test_text_color_mask_morphology(hip_lib):
    assert ps.check_tc_mask(hip_lib) == 9060


def test_text_color_hist(hip_lib):
    ps.check_tc_hist(hip_lib, CHART)


# ---- page tail --------------------------------------------------------------------------------------------------------------------
def test_lab_sums(hip_lib):
    ps.check_lab_stats(hip_lib, CHART)


@pytest.mark.parametrize("name", list(ps.REMAP_PARAMS))
def test_lab_remap(hip_lib, name):
    ps.check_lab_remap(hip_lib, CHART, name)


def test_composite_every_byte_pair(hip_lib):
    assert ps.check_composite_exact(hip_lib) == 12


def test_feather_extreme_radii(hip_lib):
    ps.check_feather_extremes(hip_lib)


def test_resample_16_bit_taps(hip_lib):
    ps.check_resample_16bit(hip_lib)
