"""bench.py's plain / --full split and --dump-outputs (host logic only)."""
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch
from PIL import Image

spec = importlib.util.spec_from_file_location("bench_mod_outputs", Path(__file__).resolve().parents[1] / "bench.py")
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def _parse(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = _parse(monkeypatch, ["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def _page_outputs():
    g = torch.Generator().manual_seed(0)
    det = types.SimpleNamespace(boxes=types.SimpleNamespace(xyxy=torch.rand(3, 4, generator=g) * 100, conf=torch.rand(3, generator=g),
                                                            cls=torch.zeros(3)),
                                masks=types.SimpleNamespace(data=torch.rand(3, 600, 700, generator=g) > 0.5))
    rt = types.SimpleNamespace(boxes=types.SimpleNamespace(xyxy=torch.ones(0, 4), conf=torch.ones(0), cls=torch.ones(0)))
    none = types.SimpleNamespace(boxes=None, masks=None)
    return {"detect": det, "detect2": rt, "detect_panel": none, "segment": (torch.rand(2, 32, 48, generator=g) > 0.5).to(torch.uint8),
            "inpaint": Image.fromarray(np.full((40, 30, 3), 7, np.uint8)), "upscale": torch.randint(0, 255, (1200, 1000, 3), dtype=torch.uint8, generator=g),
            "clean": [None, (np.ones((4, 4), np.uint8), (255, 255, 255), False, None, (1, 2, 3, 4))]}


def test_dump_outputs_names_dtypes_and_budget(tmp_path):
    outs = _page_outputs()
    bench.dump_outputs(outs, tmp_path / "a")
    files = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    # detectors that found nothing (detect2, detect_panel) leave no file: every file written holds data
    assert set(files) == {"detect_boxes", "detect_masks", "segment", "inpaint", "upscale", "clean_1_0", "clean_1_1", "clean_1_2", "clean_1_4"}
    assert all(v.dtype == np.float32 and v.size > 0 for v in files.values())
    assert files["detect_boxes"].shape == (3, 6)
    np.testing.assert_array_equal(files["detect_boxes"][:, :4], outs["detect"].boxes.xyxy.numpy())
    assert files["clean_1_1"].tolist() == [255, 255, 255] and files["clean_1_4"].shape == (4,)
    assert files["segment"].shape == (2, 32, 48) and files["inpaint"].shape == (40, 30, 3) and float(files["inpaint"].max()) == 7.0
    # arrays above the cap are a seeded sample of their elements, the same positions on every call
    assert files["upscale"].shape == (bench.DUMP_MAX_ELEMS,) and files["detect_masks"].shape == (bench.DUMP_MAX_ELEMS,)
    up = outs["upscale"].float().numpy().reshape(-1)
    assert np.isin(files["upscale"], up).all()
    bench.dump_outputs(outs, tmp_path / "b")
    for name, v in files.items():
        np.testing.assert_array_equal(v, np.load(tmp_path / "b" / f"{name}.npy"))
    assert sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy")) <= bench.DUMP_BUDGET_BYTES


def test_dump_outputs_stays_within_budget_with_many_arrays(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 20)
    bench.dump_outputs({f"s{i}": torch.zeros(300, 300) for i in range(12)}, tmp_path)
    assert sum(p.stat().st_size for p in tmp_path.glob("*.npy")) <= 1 << 20
