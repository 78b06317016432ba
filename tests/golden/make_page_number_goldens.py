"""Golden of the OSB stage's page-number filter: the REFERENCE `prepare_outside_text_work` (core/outside_text_processor.py:217-636, the filter
is :287-349) run on the page of tests/golden/osb_page.py with `enable_page_number_filtering=True` and `extract_text_with_manga_ocr` replaced
by a scripted list of recogniser answers.

    python tests/golden/make_page_number_goldens.py      # rewrites tests/golden/page_number_filter.json (data only)

Per run the file holds the boxes handed to the recogniser (in order), the answers it was scripted to give, and the surviving regions in the
reference's order (safe regions first, then the suspicious ones that were no page number).  Only this generator reads the reference; the test
(tests/test_page_number_filter.py) reads the committed file."""
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
import make_goldens as mg  # noqa: E402,F401  (stubbed import of the reference package)
import osb_page  # noqa: E402
from core import outside_text_processor as ref  # noqa: E402
from core.image import ocr_detection as refdet  # noqa: E402

SCRIPT = ["１２", "12", "Page 20", "p. 3", "ｐ．３", "あ１", "", "[OCR FAILED]"]
# tag -> (config overrides, index of the first scripted answer used)
RUNS = {
    "wide_margin": (dict(page_filter_margin_threshold=0.3, page_filter_min_area_ratio=0.05), 0),
    "clamped": (dict(page_filter_margin_threshold=5.0, page_filter_min_area_ratio=5.0), 2),            # both clamp: 0.3 and 0.2
    "edge": (dict(page_filter_margin_threshold=0.25, page_filter_min_area_ratio=0.02), 2),            # a centre ON the margin line, areas on both sides
    "nothing_suspicious": (dict(page_filter_margin_threshold=0.0, page_filter_min_area_ratio=0.05), 0),
}


def main():
    from scipy import ndimage
    refdet.cv2 = types.SimpleNamespace(cvtColor=lambda a, code: np.ascontiguousarray(a[..., ::-1]), COLOR_RGB2BGR=4, COLOR_BGR2RGB=4)
    ref.cv2 = types.SimpleNamespace(dilate=lambda img, k, iterations=1: ndimage.maximum_filter(np.asarray(img), size=k.shape[0], mode="constant", cval=0))
    ref._build_outside_text_data = lambda **kw: []

    class Boxes:
        def __init__(self, xyxy, conf):
            self.xyxy, self.conf, self.cls = torch.tensor(xyxy, dtype=torch.float32).reshape(-1, 4), torch.tensor(conf, dtype=torch.float32), torch.zeros(len(conf))

    osb_model = lambda *a, **k: [types.SimpleNamespace(boxes=Boxes(osb_page.OSB, osb_page.OSB_CONF))]

    def boom(*a, **k):
        raise RuntimeError("bubbles are provided: no bubble detector may run")

    class Paths(dict):
        def __missing__(self, k):
            return "model.pt"

    mgr = types.SimpleNamespace(load_yolo_speech_bubble=boom, load_rtdetr_conjoined_bubble=boom, load_yolo_osbtext=lambda token=None: osb_model,
                                model_paths=Paths(), device="cpu")
    none = lambda *a, **k: None
    refdet.get_model_manager = lambda: mgr
    refdet.get_cache = lambda: types.SimpleNamespace(get_yolo_cache_key=none, get_yolo_detection=none, set_yolo_detection=none)
    refdet.get_best_device = lambda: "cpu"

    out = {}
    for tag, (over, first) in RUNS.items():
        page = osb_page.make_page()
        boxes, asked = [], []
        plain_crop = page.crop
        page.crop = lambda box=None: (boxes.append([int(v) for v in box]), plain_crop(box))[1]       # every crop the stage takes, in order

        def scripted(images, verbose=False):
            asked.append((len(boxes), len(images)))
            return [SCRIPT[(first + i) % len(SCRIPT)] for i in range(len(images))]
        ref.extract_text_with_manga_ocr = scripted
        cfg = osb_page.make_config(None, "flux_kontext", enable_page_number_filtering=True, **over)
        work = ref.prepare_outside_text_work(page, cfg, "page.png", "PNG", bubble_data=osb_page.bubble_data(), text_free_boxes=osb_page.TEXT_FREE,
                                             panels=osb_page.PANELS)
        assert len(asked) <= 1
        n = asked[0][1] if asked else 0
        assert not asked or asked[0][0] == n, "the recogniser's crops are the first crops the stage takes"
        out[tag] = dict(over=over, crops=boxes[:n], answers=[SCRIPT[(first + i) % len(SCRIPT)] for i in range(n)],
                        raw=[[[float(v) for v in b], float(c)] for b, c in work.raw_outside_text_results],
                        results=[[[int(v) for v in b], float(c)] for b, c in work.outside_text_results])
    # the fixture must make the filter do something
    assert len(out["wide_margin"]["crops"]) >= 6 and len(out["wide_margin"]["raw"]) < len(out["nothing_suspicious"]["raw"])
    assert 0 < len(out["edge"]["crops"]) < len(out["wide_margin"]["crops"]) and out["nothing_suspicious"]["crops"] == []
    assert out["clamped"]["crops"] == out["wide_margin"]["crops"]
    json.dump(out, open(HERE / "page_number_filter.json", "w"), indent=0, ensure_ascii=False)
    print({t: (len(v["crops"]), len(v["raw"])) for t, v in out.items()})


if __name__ == "__main__":
    main()
