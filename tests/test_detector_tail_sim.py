"""CPU tier of the detector tail (csrc/dettail.hip through the kernel simulator): every check of tests/detector_tail_checks.py on `emu_lib`,
device "cpu".  The yardstick is the host path of the same model class; all comparisons are exact."""
import pytest

import detector_tail_checks as dc


def test_empty_single_and_identical_rows(emu_lib):
    dc.check_empty_single_identical(emu_lib, "cpu")


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_word_and_sort_pad_boundaries(emu_lib, n):
    dc.check_word_and_pad_boundaries(emu_lib, "cpu", n)


def test_greedy_chain_keeps_what_a_suppressed_box_would_have_suppressed(emu_lib):
    dc.check_greedy_chain(emu_lib, "cpu")


def test_exact_threshold_and_degenerate_boxes(emu_lib):
    dc.check_exact_threshold_and_degenerate(emu_lib, "cpu")


def test_classes_are_kept_apart(emu_lib):
    dc.check_classes(emu_lib, "cpu")


def test_truncation_to_max_det(emu_lib):
    dc.check_truncation(emu_lib, "cpu")


def test_clamping_to_the_page(emu_lib):
    dc.check_clamping(emu_lib, "cpu")


def test_mask_coefficients_round_as_torch_does(emu_lib):
    dc.check_coefficients(emu_lib, "cpu")


def test_overflow_falls_back_to_the_host_path(emu_lib):
    dc.check_overflow(emu_lib, "cpu")


def test_changed_thresholds_reuse_the_plan(emu_lib):
    dc.check_changed_thresholds(emu_lib, "cpu")


def test_device_tail_does_not_run_the_host_nms(emu_lib, monkeypatch):
    dc.check_path_selection(emu_lib, "cpu", monkeypatch)


@pytest.mark.parametrize("family,seg,seed", [("11", True, 2), ("11", False, 0), ("12", False, 3)])
def test_end_to_end_equals_the_host_tail(emu_lib, family, seg, seed):
    dc.check_end_to_end(emu_lib, "cpu", family, seg, seed)


def test_detector_batcher_gets_the_device_tail_per_ticket(emu_lib):
    dc.check_batcher(emu_lib, "cpu")


def test_constructor_refuses_an_unknown_tail(emu_lib):
    dc.check_constructor(emu_lib, "cpu")


def test_manager_switch_reaches_the_model(emu_lib, monkeypatch):
    dc.check_manager_switch(emu_lib, monkeypatch)
