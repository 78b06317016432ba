"""Goldens of the OSB stage's translation payload, rendered-text colours and grouped FLUX: the REFERENCE `prepare_outside_text_work` +
`finish_outside_text_work` (core/outside_text_processor.py:217-1691, with `_build_outside_text_data` :61-175, the colour probe
:1096-1165 and `_apply_inpaint_render_metadata` :178-214 left in place) run on the page of tests/golden/osb_payload_page.py.

    python tests/golden/make_osb_payload_goldens.py      # rewrites tests/golden/osb_payload.json / osb_payload.npz

Stand-ins, as for the rest of the stage (make_goldens.gen_osb_stage, make_bubble_crop_goldens): the inpainter (deterministic), the 2x
model (make_goldens.fake_upscaler), and `cv2` = the namespace of cv2_shim.py (every primitive served by oracle/cleaning_ref.py /
oracle/cv2_color_ref.py), extended HERE with what the colour probe and the payload call on top of it: `morphologyEx(MORPH_CLOSE)` =
the shim's dilate then erode, `COLOR_RGB2HSV` = the shim's BGR form on the flipped pixel, `imencode` = a recorder of the array it is
handed.  So the FLOW is pinned (which pixels are compared with what, which mask is cleaned how, which colour lands in which entry);
the cv2 primitives stay "parity unpinned" like the rest of SURVEY.md §8 rows a5 / f4.  `np.percentile` is wrapped to record the type
and value of `p95` and `p95 * 0.6`: a NumPy with another promotion rule shows up as a golden mismatch.

Only this generator reads the reference; the tests read the committed fixtures."""
import hashlib
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
import make_goldens as mg  # noqa: E402  (stubbed import of the reference package)
import make_cache_goldens  # noqa: E402,F401  (fontTools stubs + the reference UnifiedCache import)
import cv2_shim  # noqa: E402
import osb_payload_page as pp  # noqa: E402
from core import batch_coordinator  # noqa: E402
from core import outside_text_processor as ref  # noqa: E402
from core.caching import UnifiedCache  # noqa: E402
from core.image import image_utils as refu  # noqa: E402
from core.image import ocr_detection as refdet  # noqa: E402

MORPH_CLOSE, COLOR_RGB2HSV = 3, 41


def sha(a) -> str:
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.tobytes()).hexdigest()


class RecordingNumpy:
    """numpy, with `percentile` noting what the reference's threshold expression sees"""

    def __init__(self):
        self.seen = []

    def __getattr__(self, name):
        return getattr(np, name)

    def percentile(self, a, q, *args, **kw):
        p = np.percentile(a, q, *args, **kw)
        scaled = p * 0.6
        self.seen.append([type(p).__name__, float(p), type(scaled).__name__, float(scaled), int(np.asarray(a).size)])
        return p


def main():
    from scipy import ndimage
    captured = []
    shim = dict(vars(cv2_shim.namespace))

    def cvt(a, code):
        if code == COLOR_RGB2HSV:
            return cv2_shim.cvtColor(np.asarray(a)[..., ::-1], cv2_shim.COLOR_BGR2HSV)
        return cv2_shim.cvtColor(a, code)

    def morphology_ex(src, op, kernel):
        assert op == MORPH_CLOSE
        return cv2_shim.erode(cv2_shim.dilate(src, kernel), kernel)

    def bubble_dilate(img, k, iterations=1):
        if k.shape[0] == 11:             # the page-sized bubble guard: a zero-padded maximum filter == cv2's default constant border
            return ndimage.maximum_filter(np.asarray(img), size=11, mode="constant", cval=0)
        return cv2_shim.dilate(img, k, iterations)

    shim.update(cvtColor=cvt, morphologyEx=morphology_ex, MORPH_CLOSE=MORPH_CLOSE, COLOR_RGB2HSV=COLOR_RGB2HSV, dilate=bubble_dilate,
                imencode=lambda ext, arr: (captured.append((ext, np.asarray(arr).copy())) or True, b"x"))
    ref.cv2 = types.SimpleNamespace(**shim)
    refu.cv2 = ref.cv2
    refdet.cv2 = types.SimpleNamespace(cvtColor=lambda a, code: np.ascontiguousarray(a[..., ::-1]), COLOR_RGB2BGR=4, COLOR_BGR2RGB=4)
    ref.FluxKontextInpainter = pp.StandInInpainter
    rec = RecordingNumpy()
    ref.np = rec
    cache = UnifiedCache()
    refu.get_cache = lambda: cache
    passes = [0]

    def model(t):
        passes[0] += 1
        return mg.fake_upscaler(t)
    ref.get_model_manager = lambda: types.SimpleNamespace(load_upscale=lambda verbose=False: model, load_upscale_lite=lambda verbose=False: model,
                                                          clear_cache=lambda: None)

    class Boxes:
        def __init__(self, xyxy, conf):
            self.xyxy, self.conf, self.cls = torch.tensor(xyxy, dtype=torch.float32).reshape(-1, 4), torch.tensor(conf, dtype=torch.float32), torch.zeros(len(conf))

    osb_model = lambda *a, **k: [types.SimpleNamespace(boxes=Boxes(pp.OSB, pp.OSB_CONF))]

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

    page = pp.make_page()
    out, arrays = {}, {}
    for tag, (method, with_coord, fmt, kw, fail_group) in pp.RUNS.items():
        coord = batch_coordinator.BatchRequestCoordinator(2) if with_coord else None
        cfg = pp.make_config(coord, method, **kw)
        pp.StandInInpainter.calls, pp.StandInInpainter.fail_group = [], fail_group
        captured.clear()
        rec.seen = []
        n0 = passes[0]
        work = ref.prepare_outside_text_work(page, cfg, "page.png", fmt, bubble_data=pp.bubble_data(), text_free_boxes=pp.TEXT_FREE, panels=pp.PANELS)
        prepared = [dict(text_color_rgb=d["text_color_rgb"], needs_text_background=d["needs_text_background"]) for d in work.outside_text_data]
        final, data = ref.finish_outside_text_work(work)
        assert data is work.outside_text_data and len(data) == len(captured) == len(pp.OSB)
        entries = []
        for d, (ext, enc) in zip(data, captured):
            color = d["text_color_rgb"]
            entries.append(dict(keys=list(d), bbox=[int(v) for v in d["bbox"]], original_bbox=[int(v) for v in d["original_bbox"]],
                                confidence=float(d["confidence"]), is_outside_text=d["is_outside_text"], mime_type=d["mime_type"],
                                is_dark_text=bool(d["is_dark_text"]), text_color_rgb=None if color is None else [int(v) for v in color],
                                aspect_ratio=float(d["aspect_ratio"]), needs_text_background=bool(d["needs_text_background"]),
                                crop_shape=list(np.asarray(d["original_crop_pil"]).shape), crop_sha256=sha(np.asarray(d["original_crop_pil"])),
                                ext=ext, encoded_shape=list(enc.shape), encoded_sha256=sha(enc)))
        arrays[f"{tag}_final"] = np.asarray(final.convert("RGB"))
        out[tag] = dict(method=method, coordinator=with_coord, image_format=fmt, config=kw, fail_group=fail_group, model_passes=passes[0] - n0,
                        prepared=prepared, data=entries, percentiles=rec.seen, calls=pp.sorted_calls())
    # the fixture must make the probe do something (the comparison cannot be emptied by an edit of the page)
    colors = [e["text_color_rgb"] for e in out["flux"]["data"]]
    found = [c for c in colors if c is not None]
    snapped = [c for c in found if c in ([0, 0, 0], [255, 255, 255])]
    assert len(found) >= 5 and len(snapped) >= 2 and len(found) - len(snapped) >= 2 and len(found) < len(colors), colors
    assert any(p[1] < 50 for p in out["flux"]["percentiles"]), "no region whose p95 lets the floor of 30 decide"
    assert any(e["needs_text_background"] for e in out["none_mode"]["data"])
    assert any(c["ocr_params"] for c in out["group_coordinator"]["calls"]) and any(c["ocr_params"] for c in out["group_raises"]["calls"])
    json.dump(out, open(HERE / "osb_payload.json", "w"), indent=0)
    np.savez_compressed(HERE / "osb_payload.npz", **arrays)
    print({t: (len(v["calls"]), v["model_passes"], [e["text_color_rgb"] for e in v["data"]]) for t, v in out.items()})


if __name__ == "__main__":
    main()
