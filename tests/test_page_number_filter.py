"""The OSB stage's page-number filter (`enable_page_number_filtering`) against the reference: tests/golden/page_number_filter.json holds what the
REFERENCE `prepare_outside_text_work` (core/outside_text_processor.py:287-349) asked its recogniser and which regions it kept, in which order, on the
page of tests/golden/osb_page.py with scripted recogniser answers (tests/golden/make_page_number_goldens.py).  Here the same scripted callable sits
in the manager's manga-ocr slot and the stage must take identical crops and keep identical survivors."""
import json
import sys
import types
from pathlib import Path

import pytest
import torch

G = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(G))
import osb_page  # noqa: E402

from mangatranslator_amd.core import outside_text_processor as otp  # noqa: E402
from mangatranslator_amd.core.image import ocr_detection  # noqa: E402
from mangatranslator_amd.core.ml.model_manager import ModelType, get_model_manager  # noqa: E402
from mangatranslator_amd.utils.exceptions import ValidationError  # noqa: E402

GOLD = json.loads((G / "page_number_filter.json").read_text(encoding="utf-8"))


class _Boxes:
    def __init__(self, xyxy, conf):
        self.xyxy, self.conf, self.cls = torch.tensor(xyxy, dtype=torch.float32).reshape(-1, 4), torch.tensor(conf, dtype=torch.float32), torch.zeros(len(conf))


@pytest.fixture
def stage(monkeypatch):
    """the detectors' stand-ins of tests/test_osb_stage.py; the recogniser comes from the REAL manager's slot"""
    def boom(*a, **k):
        raise RuntimeError("bubbles are provided: no bubble detector may run")
    real = get_model_manager()
    osb_model = lambda *a, **k: [types.SimpleNamespace(boxes=_Boxes(osb_page.OSB, osb_page.OSB_CONF))]
    mgr = types.SimpleNamespace(load_yolo_speech_bubble=boom, load_rtdetr_conjoined_bubble=boom, load_yolo_osbtext=lambda token=None: osb_model, device="cpu",
                                get_manga_ocr=real.get_manga_ocr)
    monkeypatch.setattr(ocr_detection, "get_model_manager", lambda: mgr)
    before = real.models.get(ModelType.MANGA_OCR)
    yield real
    real.models[ModelType.MANGA_OCR] = before


@pytest.mark.parametrize("tag", list(GOLD))
def test_filter_matches_reference(stage, tag):
    gold = GOLD[tag]
    answers, seen = list(gold["answers"]), []

    def recogniser(img):
        seen.append(img.size)
        return answers[len(seen) - 1]
    stage.models[ModelType.MANGA_OCR] = recogniser
    page = osb_page.make_page()
    boxes, plain_crop = [], page.crop
    page.crop = lambda box=None: (boxes.append([int(v) for v in box]), plain_crop(box))[1]
    cfg = osb_page.make_config(None, "flux_kontext", enable_page_number_filtering=True, **gold["over"])
    work = otp.prepare_outside_text_work(page, cfg, "page.png", "PNG", bubble_data=osb_page.bubble_data(), text_free_boxes=osb_page.TEXT_FREE, panels=osb_page.PANELS)
    n = len(gold["crops"])
    assert len(seen) == n and boxes[:n] == gold["crops"]
    assert seen == [(b[2] - b[0], b[3] - b[1]) for b in gold["crops"]]
    assert [[[float(v) for v in b], float(c)] for b, c in work.raw_outside_text_results] == gold["raw"]
    assert [[[int(v) for v in b], float(c)] for b, c in work.outside_text_results] == gold["results"]


def test_filter_without_a_recogniser_is_refused_before_detection(stage, monkeypatch):
    stage.models[ModelType.MANGA_OCR] = None
    monkeypatch.setattr(ocr_detection.OutsideTextDetector, "detect_outside_text", lambda *a, **k: pytest.fail("detection ran"))
    with pytest.raises(ValidationError):
        otp.prepare_outside_text_work(osb_page.make_page(), osb_page.make_config(None, enable_page_number_filtering=True), "p.png", "PNG")


def test_page_number_pattern():
    yes = ["12", " 7 ", "Page 20", "page.3", "p. 3", "P.12", "p3", "１２"]
    no = ["ｐ．３", "あ１", "", "[OCR FAILED]", "12a", "pp 3", "page"]
    assert all(otp.PAGE_NUMBER_RE.match(t) for t in yes) and not any(otp.PAGE_NUMBER_RE.match(t) for t in no)
