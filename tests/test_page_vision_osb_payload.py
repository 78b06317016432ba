"""`process_page_vision(..., osb_payload=True)`: the keyword reaches the OSB stage's prepare half and the entries come back under
`info["outside_text"]`; without it the stage is called exactly as before and `info` carries no such key."""
import numpy as np
from PIL import Image

from mangatranslator_amd.core import outside_text_processor as otp
from mangatranslator_amd.core import pipeline
from mangatranslator_amd.core.image import cleaning, detection
from test_page_vision import _config


def _rig(monkeypatch, seen):
    def prepare(page, config, image_path, image_format, verbose=False, bubble_data=None, text_free_boxes=None, panels=None, **kw):
        seen.append(kw)
        return ("work", page, kw.get("build_payload"))

    def finish(work):
        return work[1], ([{"bbox": (1, 2, 3, 4), "is_outside_text": True}] if work[2] else [])
    monkeypatch.setattr(detection, "detect_speech_bubbles", lambda *a, **k: ([], []))
    monkeypatch.setattr(otp, "prepare_outside_text_work", prepare)
    monkeypatch.setattr(otp, "finish_outside_text_work", finish)
    monkeypatch.setattr(cleaning, "clean_speech_bubbles", lambda *a, **k: (_ for _ in ()).throw(AssertionError("no bubbles: cleaning must not run")))


def test_payload_keyword_travels_and_entries_come_back(monkeypatch):
    seen = []
    _rig(monkeypatch, seen)
    cfg = _config()
    cfg.output.upscale_final_image = False
    page = Image.fromarray(np.full((20, 30, 3), 200, np.uint8))
    _, info = pipeline.process_page_vision(page, cfg)
    assert seen == [{}] and "outside_text" not in info
    _, info = pipeline.process_page_vision(page, cfg, osb_payload=True)
    assert seen[1] == {"build_payload": True} and info["outside_text"] == [{"bbox": (1, 2, 3, 4), "is_outside_text": True}]
    state = pipeline.process_page_vision_front(page, cfg, osb_payload=True)
    assert state["osb_payload"] is True and pipeline.process_page_vision_back(state)[1]["outside_text"]
