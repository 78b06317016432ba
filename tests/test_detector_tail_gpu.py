"""GPU tier of the detector tail (csrc/dettail.hip on the MI355X): every check of tests/detector_tail_checks.py on `hip_lib`, device "cuda", plus
what only hardware shows — the captured plan replayed with byte-identical results whatever order the workgroups appended candidates in, and
the bubble detector's real row count, where the compaction spans many workgroups.  The yardstick is the host path; all comparisons are exact."""
import numpy as np
import pytest
import torch

import detector_tail_checks as dc
from mangatranslator_amd.core.ml.yolo import YoloSegHip
from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.plan import PlanBuilder

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_empty_single_and_identical_rows(hip_lib):
    dc.check_empty_single_identical(hip_lib, DEV)


@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_word_and_sort_pad_boundaries(hip_lib, n):
    dc.check_word_and_pad_boundaries(hip_lib, DEV, n)


def test_greedy_chain_keeps_what_a_suppressed_box_would_have_suppressed(hip_lib):
    dc.check_greedy_chain(hip_lib, DEV)


def test_exact_threshold_and_degenerate_boxes(hip_lib):
    dc.check_exact_threshold_and_degenerate(hip_lib, DEV)


def test_classes_are_kept_apart(hip_lib):
    dc.check_classes(hip_lib, DEV)


def test_truncation_to_max_det(hip_lib):
    dc.check_truncation(hip_lib, DEV)


def test_clamping_to_the_page(hip_lib):
    dc.check_clamping(hip_lib, DEV)


def test_mask_coefficients_round_as_torch_does(hip_lib):
    dc.check_coefficients(hip_lib, DEV)


def test_overflow_falls_back_to_the_host_path(hip_lib):
    dc.check_overflow(hip_lib, DEV)


def test_changed_thresholds_reuse_the_plan(hip_lib):
    dc.check_changed_thresholds(hip_lib, DEV)


def test_device_tail_does_not_run_the_host_nms(hip_lib, monkeypatch):
    dc.check_path_selection(hip_lib, DEV, monkeypatch)


@pytest.mark.parametrize("family,seg,seed", [("11", True, 2), ("11", False, 0), ("12", False, 3)])
def test_end_to_end_equals_the_host_tail(hip_lib, family, seg, seed):
    dc.check_end_to_end(hip_lib, DEV, family, seg, seed)


def test_detector_batcher_gets_the_device_tail_per_ticket(hip_lib):
    dc.check_batcher(hip_lib, DEV)


def test_constructor_refuses_an_unknown_tail(hip_lib):
    dc.check_constructor(hip_lib, DEV)


def test_manager_switch_reaches_the_model(hip_lib, monkeypatch):
    dc.check_manager_switch(hip_lib, monkeypatch)


def _params(bufs, conf, iou, max_det):
    gain, padw, padh = YoloSegHip._page_scale(dc.LP, dc.H0, dc.W0)
    p = np.zeros(abi.DET_TAIL_PARAM_WORDS, np.int32)
    f = p.view(np.float32)
    f[abi.DET_TAIL_P_CONF], f[abi.DET_TAIL_P_IOU], p[abi.DET_TAIL_P_MAX_DET] = conf, iou, max_det
    f[abi.DET_TAIL_P_GAIN], f[abi.DET_TAIL_P_PADW], f[abi.DET_TAIL_P_PADH] = gain, padw, padh
    p[abi.DET_TAIL_P_W0], p[abi.DET_TAIL_P_H0] = dc.W0, dc.H0
    bufs.params.copy_(torch.from_numpy(p))


def test_replays_of_the_captured_plan_give_identical_bytes(hip_lib):
    """the 129-candidate set through the captured op eight times: the append order of the compaction varies, the result block must not"""
    rows = torch.from_numpy(dc.clustered(129, seed=129)).to(DEV)
    pb = PlanBuilder(hip_lib, DEV, abi.F16)
    bufs = pb.detector_tail(rows, nc=1, nm=0)
    plan = pb.build()
    _params(bufs, 0.25, 0.5, 300)
    blocks = []
    for _ in range(8):
        plan.run(graph=True)
        torch.cuda.synchronize()
        blocks.append(bufs.out.clone())
    host = dc.finish(dc.pair(hip_lib, DEV)[0], rows.cpu().numpy(), 0.25, 0.5, 300)
    kept = int(blocks[0][abi.DET_TAIL_KEPT])
    assert blocks[0][:4].tolist() == [len(host.boxes), 129, 0, 0]
    assert torch.equal(bufs.boxes[:kept], host.boxes.xyxy)
    for i, b in enumerate(blocks[1:], 1):
        assert torch.equal(b, blocks[0]), f"replay {i} differs from replay 0"


def test_bubble_detector_row_count_spans_many_workgroups(hip_lib):
    """35 700 rows (the 1600 x 1088 letterbox of the bubble detector), about 200 candidates spread over all of them, segmentation head"""
    rng = np.random.default_rng(11)
    A, n, nm = 35700, 200, 32
    cand = dc.clustered(n, seed=200, extra=0, centres=8)
    rows = np.zeros((A, 4 + 1 + nm), np.float32)
    rows[:, :4] = rng.uniform(0, 60, (A, 4))
    rows[:, 4] = rng.uniform(0, 0.1, A)
    rows[:, 5:] = rng.normal(0, 1, (A, nm))
    at = np.sort(rng.choice(A, n, replace=False))
    at[0], at[-1] = 0, A - 1                                     # the first and the last row are candidates
    rows[at, :5] = cand
    mh, md = dc.pair(hip_lib, DEV, 1, True)
    host = dc.finish(mh, rows, 0.25, 0.5, 300, dc.proto_for(mh))
    dev = dc.finish(md, rows, 0.25, 0.5, 300, dc.proto_for(md))
    assert 8 <= len(host.boxes) < n
    dc.assert_same(host, dev, "35 700 rows")
    assert dc.state_of(md, dev) == [len(host.boxes), n, 0, 0]
