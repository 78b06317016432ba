"""CPU tier: the YOLO11 / YOLO12 graphs (core/ml/yolo11.py) on the kernel simulator vs the fp32 oracle, nano scale on a small page."""
import yolo11_checks as yc


def test_yolo11n_detect(emu_lib):
    yc.check(emu_lib, "cpu", "11", "n", False)


def test_yolo11n_seg(emu_lib):
    yc.check(emu_lib, "cpu", "11", "n", True, h=192, w=128, imgsz=128, seed=2)


def test_yolo12n_detect(emu_lib):
    """A2C2f blocks with area attention (4 areas at P4): 64 x 96 letterbox -> 4 x 6 = 24 positions at P4, 6 per area"""
    yc.check(emu_lib, "cpu", "12", "n", False, seed=3)


def test_detector_batcher_matches_single_calls(emu_lib):
    """cross-page batches through one detector graph (core/ml/detector_batch.py): YOLO11 and YOLO12 (area attention), 3 pages in a batch of 4,
    4 pages in batches of 2 (both buffer sets in flight), and 5 pages submitted and collected from their own threads (sets reused)"""
    yc.check_batched(emu_lib, "cpu", family="11")
    yc.check_batched(emu_lib, "cpu", family="12", pages=4, batch=2, seed=1)
    yc.check_batched(emu_lib, "cpu", family="11", pages=5, batch=2, seed=2, threads=True)


def test_detector_batcher_survives_a_failed_submit(emu_lib):
    """a submit that fails after it took its slot (here: the launch of a full batch raises) gives the slot back — the next pages go through and get the
    one-page call's results"""
    import numpy as np
    import pytest
    import torch
    from mangatranslator_amd.core.ml.detector_batch import DetectorBatcher
    from mangatranslator_amd.core.ml.yolo11 import Yolo11Hip
    from oracle import yolo11_ref as yr
    net = yr.make_model("11", "n", 1, False, seed=4)
    hip = Yolo11Hip(net.state_dict(), device="cpu", lib=emu_lib)
    pages = [yc.make_page(96, 64, 9 + i) for i in range(2)]
    want = [hip(p, conf=0.05, imgsz=64)[0] for p in pages]
    bat = DetectorBatcher(hip, batch=1)
    real, state = bat._run, {"fail": True}

    def flaky(b):
        if state.pop("fail", False):
            raise RuntimeError("injected launch failure")
        return real(b)
    bat._run = flaky
    with pytest.raises(RuntimeError, match="injected"):
        bat.submit(pages[0], conf=0.05, imgsz=64)
    for p, w in zip(pages, want):          # both buffer sets are usable afterwards
        got = bat(p, conf=0.05, imgsz=64)[0]
        assert (w.boxes is None) == (got.boxes is None)
        if w.boxes is not None:
            assert torch.equal(w.boxes.xyxy, got.boxes.xyxy) and torch.equal(w.boxes.conf, got.boxes.conf)
    assert all(s.filled == 0 and not s.launched for s in bat._sets[(96, 64, 64)])


def _equal_boxes(want, got):
    import torch
    assert want.boxes is not None and got.boxes is not None, "the page produced no box: the comparison is empty"
    for f in ("xyxy", "conf", "cls"):
        assert torch.equal(getattr(want.boxes, f), getattr(got.boxes, f)), f"boxes.{f} differ between the batched and the one-page call"


OTHER_SIZES = ((32, 64), (64, 32), (30, 64), (64, 30))      # four more page sizes: with (96, 64) one more than the wrapper keeps buffer sets for


def _batcher_and_page(emu_lib, seed):
    from mangatranslator_amd.core.ml.detector_batch import DetectorBatcher
    from mangatranslator_amd.core.ml.yolo11 import Yolo11Hip
    from oracle import yolo11_ref as yr
    hip = Yolo11Hip(yr.make_model("11", "n", 1, False, seed=seed).state_dict(), device="cpu", lib=emu_lib)
    page = yc.make_page(96, 64, seed + 1)
    return hip, DetectorBatcher(hip, batch=2), page, hip(page, conf=0.05, imgsz=64)[0]


def test_detector_batcher_keeps_the_sets_of_a_held_ticket(emu_lib):
    """a page's ticket is held (batch not full, as `submit_panels` holds it) while pages of four other sizes go through the same wrapper: the held
    page's buffer sets are not the ones the cache closes, and its boxes are the one-page call's bytes.  (Before buffer sets were pinned while
    in use this sequence raised `ModelError: mtx_plan_run: null plan` in `collect`: the fifth size evicted and destroyed the held ticket's plan.)"""
    hip, bat, page, want = _batcher_and_page(emu_lib, seed=5)
    held = bat.submit(page, conf=0.05, imgsz=64)
    for i, (h, w) in enumerate(OTHER_SIZES):
        bat(yc.make_page(h, w, 20 + i), conf=0.05, imgsz=64)
    assert (96, 64, 64) in bat._sets and OTHER_SIZES[0] + (64,) not in bat._sets and len(bat._sets) == 4, "the least recently used IDLE size went instead"
    _equal_boxes(want, bat.collect(held)[0])
    bat(yc.make_page(28, 64, 30), conf=0.05, imgsz=64)          # drained: the next new size brings the cache back to its bound
    assert len(bat._sets) == 4 and (96, 64, 64) not in bat._sets and not bat._filling


def test_detector_batcher_forgets_a_set_that_reset_without_launching(emu_lib):
    """a ticket closed before its batch was launched frees its set AND ends that set's turn as the one being filled; after other sizes evicted the
    key, the next page of the first size builds fresh sets and gets the one-page call's bytes (not a slot of a destroyed set)"""
    hip, bat, page, want = _batcher_and_page(emu_lib, seed=6)
    dropped = bat.submit(page, conf=0.05, imgsz=64)
    first = dropped.batch
    dropped.close()
    assert not first.launched and first.filled == 0 and not bat._filling
    for i, (h, w) in enumerate(OTHER_SIZES):
        bat(yc.make_page(h, w, 40 + i), conf=0.05, imgsz=64)
    assert (96, 64, 64) not in bat._sets and not first.plan._h, "the idle key was evicted and its plans destroyed"
    again = bat.submit(page, conf=0.05, imgsz=64)
    assert again.batch is not first
    _equal_boxes(want, bat.collect(again)[0])
    bat.close()
    assert len(bat._sets) == 0 and not again.batch.plan._h


def test_packed_weights_match_the_recorded_digests(emu_lib):
    """`YoloSegHip._put`, shared by both families (YOLO11 / YOLO12 round the output channels up to 8): every `W[name]` — weight, bias, cout, k — of
    the seeded YOLOv8n-seg, YOLO11n, YOLO11n-seg and YOLO12n state dicts is bit for bit what the two separate packers produced"""
    import json
    from pathlib import Path
    want = json.loads((Path(__file__).resolve().parent / "golden" / "yolo_pack_digests.json").read_text())
    assert yc.pack_digests(emu_lib) == want
