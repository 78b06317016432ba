"""CPU tier, kernel simulator: the exact-input checks of the page-stage byte kernels (tests/page_stage_checks.py) — csrc/clean.hip,
csrc/textcolor.hip and csrc/pagetail.hip, every kernel stage by stage against the oracles, numpy, scipy and torch's CPU resize.  The colour
chart is 512 x 512 here (the GPU tier runs 1536 x 1536, one grid-stride trip more than the tail kernels' block cap)."""
import pytest

import page_stage_checks as ps

CHART = 512


# ---- cleaning ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page, elements, otsu, shrink", ps.clean_cases())
def test_clean_planes_and_statistics(emu_lib, page, elements, otsu, shrink):
    ps.check_clean_case(emu_lib, page, elements, otsu, shrink)


def test_clean_polarity_at_the_midpoint(emu_lib):
    ps.check_clean_polarity_pages(emu_lib)


def test_clean_junction_zones(emu_lib):
    ps.check_clean_junction_zones(emu_lib)


def test_clean_sweep_count_closed_form(emu_lib):
    ps.check_clean_sweep_count(emu_lib)


def test_clean_cross_block_atomics_and_relaunch(emu_lib):
    ps.check_clean_cross_block_atomics(emu_lib)


# ---- text colour ------------------------------------------------------------------------------------------------------------------
def test_text_color_dist_on_the_chart(emu_lib):
    ps.check_tc_dist_chart(emu_lib, CHART)


def test_text_color_rank_selection_edges(emu_lib):
    assert ps.check_tc_order_edges(emu_lib, CHART) >= 17


def test_text_color_300_regions_in_one_launch(emu_lib):
    ps.check_tc_many_regions(emu_lib, CHART)


def test_text_color_mask_morphology(emu_lib):
    assert ps.check_tc_mask(emu_lib) == 9060


def test_text_color_hist(emu_lib):
    ps.check_tc_hist(emu_lib, CHART)


# ---- page tail --------------------------------------------------------------------------------------------------------------------
def test_lab_sums(emu_lib):
    ps.check_lab_stats(emu_lib, CHART)


@pytest.mark.parametrize("name", list(ps.REMAP_PARAMS))
def test_lab_remap(emu_lib, name):
    ps.check_lab_remap(emu_lib, CHART, name)


def test_composite_every_byte_pair(emu_lib):
    assert ps.check_composite_exact(emu_lib) == 12


def test_feather_extreme_radii(emu_lib):
    ps.check_feather_extremes(emu_lib)


def test_resample_16_bit_taps(emu_lib):
    ps.check_resample_16bit(emu_lib)
