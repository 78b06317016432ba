"""CPU tier: RT-DETR-v2 graphs on the kernel simulator vs HF RTDetrV2ForObjectDetection (tiny geometry)."""
import rtdetr_checks as rc


def test_rtdetr_tiny(emu_lib):
    rc.check_raw(emu_lib, "cpu", hw=(64, 96))


def test_rtdetr_call_shape(emu_lib):
    rc.check_call_shape(emu_lib, "cpu")


def test_oracle_pre_post_matches_reference_adapter():
    """goldens from the REFERENCE's RTDetrYOLOAdapter around HF's RTDetrImageProcessor (tests/golden/make_rtdetr_adapter_golden.py): the
    restated resize / rescale / sigmoid / top-k over queries x classes / box scaling / threshold of oracle.rtdetr_ref.predict"""
    import json
    from pathlib import Path
    import numpy as np
    import torch
    from PIL import Image
    from oracle import rtdetr_ref
    g = json.loads((Path(__file__).resolve().parent / "golden" / "rtdetr_adapter.json").read_text())
    model, _ = rtdetr_ref.make_model("tiny_test", seed=g["model_seed"])
    rtdetr_ref.spread_class_scores(model)
    page = (np.random.default_rng(g["page_seed"]).random(tuple(g["page_shape"])) * 255).astype(np.uint8)
    pil = Image.fromarray(np.ascontiguousarray(page[..., ::-1]))
    for tag, run in g["runs"].items():
        xyxy, scores, labels = rtdetr_ref.predict(model, pil, conf=run["conf"], imgsz=g["imgsz"])
        assert len(scores) == len(run["scores"]), tag
        assert torch.allclose(scores, torch.tensor(run["scores"]), atol=2e-6), tag
        assert labels.tolist() == [int(c) for c in run["cls"]], tag
        assert torch.allclose(xyxy, torch.tensor(run["xyxy"]).reshape(-1, 4), atol=2e-3), tag
    assert len(g["runs"]["bgr_mid"]["scores"]) == 10 and g["runs"]["bgr_lo"]["xyxy"] == g["runs"]["pil_lo"]["xyxy"]


def test_rtdetr_batcher_matches_single_calls(emu_lib):
    """RT-DETR's backbone + encoder shared by the pages of a batch (core/ml/detector_batch.py RTDetrBatcher): 3 pages in a batch of 4, 4 pages in
    batches of 2, 5 pages from their own threads — boxes, scores and classes are the one-page call's bytes"""
    rc.check_batched(emu_lib, "cpu")
    rc.check_batched(emu_lib, "cpu", pages=4, batch=2, seed=2)
    rc.check_batched(emu_lib, "cpu", pages=5, batch=2, seed=3, threads=True)


def test_rtdetr_batcher_keeps_the_sets_of_a_held_ticket(emu_lib):
    """the held-ticket sequence of tests/test_yolo11_sim.py for RTDetrBatcher, the sizes passed through `imgsz`: one page submitted and held,
    pages at four other sizes through the same wrapper, then the first collected — the one-page call's bytes.  (Before buffer sets were pinned
    while in use this raised `ModelError: mtx_plan_run: null plan`: the fifth size destroyed the held ticket's encoder and decoder plans.)"""
    import numpy as np
    import torch
    from mangatranslator_amd.core.ml.detector_batch import RTDetrBatcher
    from mangatranslator_amd.core.ml.rtdetr import RTDetrHip
    from oracle import rtdetr_ref as rr
    m, cfg = rr.make_model("tiny_test", 1)
    model = RTDetrHip(m.state_dict(), cfg, "cpu", lib=emu_lib, graph=False, names={0: "a", 1: "b", 2: "c"})
    rng = np.random.default_rng(6)
    page = (rng.random((100, 140, 3)) * 255).astype(np.uint8)
    want = model(page, conf=0.2, imgsz=96)[0]
    bat = RTDetrBatcher(model, batch=2)
    held = bat.submit(page, conf=0.2, imgsz=96)
    for size in (64, 128, 160, 192):
        bat((rng.random((100, 140, 3)) * 255).astype(np.uint8), conf=0.2, imgsz=size)
    assert (96, 96, "rtdetr") in bat._sets and (64, 64, "rtdetr") not in bat._sets and len(bat._sets) == 4      # the least recently used IDLE size went instead
    got = bat.collect(held)[0]
    assert len(want.boxes) > 0, "the page produced no box: the comparison is empty"
    for f in ("xyxy", "conf", "cls"):
        assert torch.equal(getattr(want.boxes, f), getattr(got.boxes, f)), f"boxes.{f} differ between the batched and the one-page call"
    assert got.orig_shape == want.orig_shape and got.names == want.names
