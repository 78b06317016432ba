"""The detector tail on the device (csrc/dettail.hip, MTX_OP_DET_TAIL; `YoloSegHip(tail="device")`) against the host path (`tail="host"`:
torch row maximum, numpy NMS and rescale — the yardstick, never the code under test), written once and run on the simulator
(tests/test_detector_tail_sim.py) and on the GPU (tests/test_detector_tail_gpu.py).  Every comparison is `torch.equal`: there is no tolerance.

The row sets are built by hand as the fp32 rows MTX_OP_YOLO_DECODE writes, [anchors][4 + nc + nm], and go through `_finish` of a host-tail
and a device-tail model made from one tiny state dict; each set first asserts ON THE HOST RESULT that it exercises what it claims."""
from types import SimpleNamespace

import numpy as np
import torch

from mangatranslator_amd.core.ml import yolo as yolo_mod
from mangatranslator_amd.core.ml.yolo import letterbox_params
from mangatranslator_amd.core.ml.yolo11 import Yolo11Hip
from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.plan import Act
from mangatranslator_amd.utils.exceptions import ModelError
from oracle import yolo11_ref as yr

H0, W0, IMGSZ = 96, 64, 64          # a 64 x 64 letterbox with 10 px of padding left: gain 2 / 3 (no power of two), padw 10, padh 0
LP = letterbox_params(H0, W0, IMGSZ)
CAP = abi.DET_TAIL_CAP

_models = {}


def pair(lib, device, nc=1, seg=False):
    """(host-tail model, device-tail model) of one seeded nano state dict; only their methods and head geometry are used by the row-set checks"""
    key = (id(lib), str(device), nc, seg)
    if key not in _models:
        sd = yr.make_model("11", "n", nc, seg, seed=5).state_dict()
        _models[key] = (Yolo11Hip(sd, device=device, lib=lib, tail="host"), Yolo11Hip(sd, device=device, lib=lib, tail="device"))
    return _models[key]


def rows_of(boxes, scores, coef=None):
    """decoded rows [A][4 + nc + nm] fp32 from boxes [A, 4], scores [A] or [A, nc] and optional coefficients [A, nm]"""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    scores = np.asarray(scores, np.float32).reshape(len(boxes), -1)
    parts = [boxes, scores] + ([np.asarray(coef, np.float32).reshape(len(boxes), -1)] if coef is not None else [])
    return np.ascontiguousarray(np.concatenate(parts, 1))


def proto_for(model, seed=0):
    """a prototype grid for the letterbox (stride 4) in the model's storage type"""
    g = torch.Generator().manual_seed(seed)
    mh, mw, nm = LP["H"] // 4, LP["W"] // 4, model.a["nm"]
    return Act(torch.randn(1, mh, mw, nm, generator=g).to(model.device, model.tdt), 1, mh, mw, nm)


def finish(model, rows, conf, iou, max_det, proto=None):
    view = SimpleNamespace(decoded=torch.from_numpy(rows).to(model.device), proto=proto)
    res = model._finish(view, LP, (H0, W0), conf, iou, max_det)[0]
    res._view = view          # keeps the rows alive while the caller looks at plan caches keyed by their address
    return res


def n_boxes(res):
    return 0 if res.boxes is None else len(res.boxes)


def assert_same(host, dev, what=""):
    assert (host.boxes is None) == (dev.boxes is None), f"{what}: one path has boxes, the other none"
    assert (host.masks is None) == (dev.masks is None), f"{what}: one path has masks, the other none"
    assert host.orig_shape == dev.orig_shape and host.names == dev.names
    if host.boxes is not None:
        for f in ("xyxy", "conf", "cls"):
            a, b = getattr(host.boxes, f), getattr(dev.boxes, f)
            assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: boxes.{f} {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}"
            assert torch.equal(a, b), f"{what}: boxes.{f} differ\nhost {a}\ndevice {b}"
    if host.masks is not None:
        assert torch.equal(host.masks.data, dev.masks.data), f"{what}: masks differ"


def both(lib, device, rows, conf, iou, max_det=300, nc=1, seg=False, what=""):
    mh, md = pair(lib, device, nc, seg)
    ph, pd = (proto_for(mh), proto_for(md)) if seg else (None, None)
    host = finish(mh, rows, conf, iou, max_det, ph)
    dev = finish(md, rows, conf, iou, max_det, pd)
    assert_same(host, dev, what)
    return host, dev


def state_of(model, res):
    """[kept, candidates, overflow, 0] the op left for the rows of `res`"""
    dec = res._view.decoded
    tp = model._tail_plans.get((dec.data_ptr(), int(dec.shape[0]), int(dec.stride(0))))
    assert tp is not None, "no tail plan was recorded for these rows"
    return tp.bufs.state.tolist()


def clustered(n, seed, extra=37, centres=6, spread=1.5, size=12.0):
    """n candidates (distinct scores in 0.3 .. 0.99) around `centres` centres of the letterbox plus `extra` rows below any threshold, rows shuffled"""
    rng = np.random.default_rng(seed)
    cx = np.array([10, 30, 50, 10, 30, 50, 20, 40][:centres], np.float32) if centres <= 8 else rng.uniform(0, 600, centres).astype(np.float32)
    cy = np.array([12, 12, 12, 44, 44, 44, 28, 28][:centres], np.float32) if centres <= 8 else rng.uniform(0, 600, centres).astype(np.float32)
    which = np.arange(n) % centres
    c = np.stack([cx[which], cy[which]], 1) + rng.uniform(-spread, spread, (n, 2)).astype(np.float32)
    half = (size / 2 + rng.uniform(-0.5, 0.5, (n, 2))).astype(np.float32)
    boxes = np.concatenate([c - half, c + half], 1).astype(np.float32)
    scores = rng.permutation(np.linspace(0.3, 0.99, n)).astype(np.float32)
    assert len(np.unique(scores)) == n
    boxes = np.concatenate([boxes, rng.uniform(0, 60, (extra, 4)).astype(np.float32)])
    scores = np.concatenate([scores, rng.uniform(0.0, 0.1, extra).astype(np.float32)])
    order = rng.permutation(n + extra)
    return rows_of(boxes[order], scores[order])


# ---- the row sets ---------------------------------------------------------------------------------------------------------------------------

def check_empty_single_identical(lib, device):
    none = rows_of(np.tile([[5, 5, 20, 20]], (50, 1)), np.full(50, 0.1))
    host, _ = both(lib, device, none, 0.5, 0.7, what="no candidate")
    assert host.boxes is None
    one = none.copy()
    one[17, 4] = 0.9
    host, dev = both(lib, device, one, 0.5, 0.7, what="one candidate")
    assert n_boxes(host) == 1 and n_boxes(dev) == 1
    same = rows_of(np.tile([[5, 5, 20, 20]], (40, 1)), np.full(40, 0.9))
    host, _ = both(lib, device, same, 0.5, 0.7, what="all identical")
    assert n_boxes(host) == 1
    # equal scores, boxes apart: the order is the row order
    grid = np.array([[12 * i, 0, 12 * i + 8, 8] for i in range(5)], np.float32)
    host, _ = both(lib, device, rows_of(grid[[3, 0, 4, 1, 2]], np.full(5, 0.8)), 0.5, 0.7, what="equal scores")
    assert n_boxes(host) == 5
    x2 = host.boxes.xyxy[:, 2].cpu().numpy()
    assert np.argsort(np.argsort(x2, kind="stable"), kind="stable").tolist() == [3, 0, 4, 1, 2], "equal scores keep the row order"


def check_word_and_pad_boundaries(lib, device, n):
    rows = clustered(n, seed=n)
    host, dev = both(lib, device, rows, 0.25, 0.5, what=f"{n} candidates")
    kept = n_boxes(host)
    assert kept >= 6 and n - kept >= n // 2, f"{n} candidates: the host kept {kept}; the set must keep at least 6 and suppress at least half"
    md = pair(lib, device)[1]
    assert state_of(md, dev) == [kept, n, 0, 0]


def check_greedy_chain(lib, device):
    rows = rows_of([[0, 0, 10, 10], [3, 0, 13, 10], [6, 0, 16, 10]], [0.9, 0.8, 0.7])      # IoU(A, B) = IoU(B, C) = 7 / 13, IoU(A, C) = 4 / 16
    host, _ = both(lib, device, rows, 0.25, 0.4, what="greedy chain")
    assert host.boxes.conf.cpu().tolist() == [float(np.float32(0.9)), float(np.float32(0.7))], "the host keeps A and C: B, itself suppressed, suppresses nothing"


def check_exact_threshold_and_degenerate(lib, device):
    pairs_ = rows_of([[0, 0, 3, 1], [1, 0, 4, 1]], [0.9, 0.8])                              # inter 2, union 3 + 3 - 2: IoU exactly 0.5
    host, _ = both(lib, device, pairs_, 0.25, 0.5, what="IoU == threshold")
    assert n_boxes(host) == 2
    host, _ = both(lib, device, pairs_, 0.25, 0.49, what="IoU above threshold")
    assert n_boxes(host) == 1
    points = rows_of([[5, 5, 5, 5], [5, 5, 5, 5]], [0.9, 0.8])                              # 0 / 0: NaN compares false
    host, _ = both(lib, device, points, 0.25, 0.5, what="zero-area boxes")
    assert n_boxes(host) == 2
    c32 = np.float32(0.3)
    edge = rows_of([[0, 0, 8, 8], [20, 0, 28, 8], [40, 0, 48, 8]], [c32, np.nextafter(c32, np.float32(1)), np.nextafter(c32, np.float32(0))])
    host, _ = both(lib, device, edge, 0.3, 0.5, what="score == float32(conf)")
    assert n_boxes(host) == 1 and host.boxes.conf.cpu().numpy()[0] == np.nextafter(c32, np.float32(1)), "only the score one ulp above float32(conf) is a candidate"


def check_classes(lib, device):
    box = [4, 4, 30, 30]
    diff = rows_of([box, box], [[0.9, 0.1, 0.2], [0.15, 0.05, 0.8]])
    host, _ = both(lib, device, diff, 0.25, 0.5, nc=3, what="identical boxes, two classes")
    assert n_boxes(host) == 2 and host.boxes.cls.cpu().tolist() == [0.0, 2.0]
    same = rows_of([box, box, box], [[0.1, 0.9, 0.2], [0.15, 0.8, 0.05], [0.3, 0.2, 0.7]])
    host, _ = both(lib, device, same, 0.25, 0.5, nc=3, what="identical boxes, one class twice")
    assert n_boxes(host) == 2 and host.boxes.cls.cpu().tolist() == [1.0, 2.0]


def check_truncation(lib, device):
    boxes = [[12 * (i % 5), 12 * (i // 5), 12 * (i % 5) + 8, 12 * (i // 5) + 8] for i in range(20)]
    rows = rows_of(boxes, np.linspace(0.4, 0.95, 20))
    host, _ = both(lib, device, rows, 0.25, 0.5, what="20 kept")
    assert n_boxes(host) == 20
    host, dev = both(lib, device, rows, 0.25, 0.5, max_det=7, what="max_det 7")
    assert n_boxes(host) == 7
    assert state_of(pair(lib, device)[1], dev) == [7, 20, 0, 0]


def check_clamping(lib, device):
    rows = rows_of([[-5, -7, 70, 75], [2, -3, 40, 30], [30, 20, 90, 64.5]], [0.9, 0.8, 0.7])
    host, _ = both(lib, device, rows, 0.25, 0.99, what="clamping")
    xy = host.boxes.xyxy.cpu().numpy()
    assert n_boxes(host) == 3 and (xy[:, [0, 1]] == 0).any() and (xy[:, 2] == W0).any() and (xy[:, 3] == H0).any()
    assert (xy != np.round(xy)).any(), "the gain is no power of two: some coordinate must be a rounded quotient"


def check_coefficients(lib, device):
    rng = np.random.default_rng(3)
    n, nm = 24, 32
    boxes = [[12 * (i % 5), 12 * (i // 5), 12 * (i % 5) + 10, 12 * (i // 5) + 10] for i in range(n)]
    coef = rng.normal(0, 1, (n, nm)).astype(np.float32)
    # ties of the f16 grid (to even: down, then up), values that land on f16 subnormals, ties between subnormals, below half the smallest one
    coef[0, :8] = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -25, 5 * 2.0 ** -25, 2.0 ** -26, -(1 + 2.0 ** -11)]
    coef[1, :4] = [6.0e-8, 6.1e-5, -3.0e-6, 1.0e-7]
    assert (torch.from_numpy(coef).to(torch.float16).float().numpy() != coef).any()
    rows = rows_of(boxes, np.linspace(0.4, 0.95, n), coef)
    host, dev = both(lib, device, rows, 0.25, 0.5, seg=True, what="mask coefficients")
    assert n_boxes(host) == n and host.masks is not None and int(host.masks.data.sum()) > 0
    mh, md = pair(lib, device, 1, True)
    ch, cd = [[v for k, v in m._mask_plans.items() if k[0] == n][-1] for m in (mh, md)]
    assert torch.equal(ch.coef.view(torch.int16), cd.coef.view(torch.int16)), "the mask GEMM's coefficient operand differs in its f16 bytes"
    want = torch.from_numpy(coef[np.argsort(-rows[:, 4], kind="stable")]).to(torch.float16)
    assert torch.equal(cd.coef[:n].cpu().view(torch.int16), want.view(torch.int16))


def check_overflow(lib, device):
    md = pair(lib, device)[1]
    for n, over in ((CAP, 0), (CAP + 1, 1)):
        rows = clustered(n, seed=n, extra=11, centres=40, spread=2.0)
        host, dev = both(lib, device, rows, 0.25, 0.5, what=f"{n} candidates")
        assert n_boxes(host) >= 20
        st = state_of(md, dev)
        assert st[abi.DET_TAIL_CAND] == n and st[abi.DET_TAIL_OVERFLOW] == over, st
        assert st[abi.DET_TAIL_KEPT] == (0 if over else n_boxes(host))
    # a max_det beyond the result block's capacity takes the host path as well
    rows = clustered(65, seed=1)
    both(lib, device, rows, 0.25, 0.99, max_det=abi.DET_TAIL_MAX_KEEP + 1, what="max_det above max_keep")


def check_changed_thresholds(lib, device):
    mh, md = pair(lib, device)
    rows = clustered(129, seed=7)
    view = SimpleNamespace(decoded=torch.from_numpy(rows).to(md.device), proto=None)
    counts, plans = [], []
    for conf, iou, max_det in ((0.25, 0.5, 300), (0.6, 0.3, 5), (0.25, 0.5, 300)):
        dev = md._finish(view, LP, (H0, W0), conf, iou, max_det)[0]
        host = mh._finish(view, LP, (H0, W0), conf, iou, max_det)[0]
        assert_same(host, dev, f"conf {conf} iou {iou} max_det {max_det}")
        counts.append(n_boxes(host))
        plans.append(len(md._tail_plans))
    assert counts[0] == counts[2] > counts[1] == 5
    assert plans[0] == plans[1] == plans[2], "a change of thresholds rebuilt the tail plan"


def check_path_selection(lib, device, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("nms_xyxy ran")
    mh, md = pair(lib, device)
    rows = clustered(65, seed=2)
    want = finish(mh, rows, 0.25, 0.5, 300)
    monkeypatch.setattr(yolo_mod, "nms_xyxy", boom)
    assert_same(want, finish(md, rows, 0.25, 0.5, 300), "device tail with the host NMS disabled")
    try:
        finish(mh, rows, 0.25, 0.5, 300)
    except AssertionError as e:
        assert "nms_xyxy ran" in str(e)
    else:
        raise AssertionError("the host tail did not go through nms_xyxy")


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------

def _net(family, seg, seed):
    from oracle import yolo_ref
    from yolo11_checks import make_page
    net = yr.make_model(family, "n", 1, seg, seed=seed)
    x, _ = yolo_ref.letterbox(make_page(H0, W0, seed + 1), IMGSZ)
    yr.calibrate(net, x)
    return net.state_dict()


def check_end_to_end(lib, device, family="11", seg=False, seed=0):
    from yolo11_checks import make_page
    sd = _net(family, seg, seed)
    host_m, dev_m = Yolo11Hip(sd, device=device, lib=lib), Yolo11Hip(sd, device=device, lib=lib, tail="device")
    assert host_m.tail == "host"
    page = make_page(H0, W0, seed + 1)
    host, dev = host_m(page, conf=0.05, imgsz=IMGSZ)[0], dev_m(page, conf=0.05, imgsz=IMGSZ)[0]
    assert n_boxes(host) >= 2, "the page gives the host path fewer than two boxes: the comparison shows nothing"
    assert_same(host, dev, f"YOLO{family}n{'-seg' if seg else ''}")
    assert len(dev_m._tail_plans) == 1
    return n_boxes(host)


def check_batcher(lib, device, pages=3, batch=4, seed=0):
    from mangatranslator_amd.core.ml.detector_batch import DetectorBatcher
    from yolo11_checks import make_page
    sd = _net("11", False, seed)
    host_m, dev_m = Yolo11Hip(sd, device=device, lib=lib), Yolo11Hip(sd, device=device, lib=lib, tail="device")
    imgs = [make_page(H0, W0, seed + 1 + i) for i in range(pages)]
    want = [host_m(im, conf=0.05, imgsz=IMGSZ)[0] for im in imgs]
    bat = DetectorBatcher(dev_m, batch=batch)
    tickets = [bat.submit(im, conf=0.05, imgsz=IMGSZ) for im in imgs]
    got = [bat.collect(t)[0] for t in tickets]
    assert bat.stats == dict(pages=pages, launches=1)
    for i, (a, b) in enumerate(zip(want, got)):
        assert n_boxes(a) >= 2
        assert_same(a, b, f"page {i} of the batch")
    assert len(dev_m._tail_plans) == pages, "one tail plan per slot of the batched plan's decoded rows"
    bat.close()


# ---- constructor and switch -----------------------------------------------------------------------------------------------------------------

def check_constructor(lib, device):
    sd = yr.make_model("11", "n", 1, False, seed=5).state_dict()
    try:
        Yolo11Hip(sd, device=device, lib=lib, tail="gpu")
    except ModelError as e:
        assert "tail" in str(e)
    else:
        raise AssertionError('tail="gpu" was accepted')


def check_manager_switch(lib, monkeypatch):
    import mangatranslator_amd.hip.lib as libmod
    from mangatranslator_amd.core.ml import model_manager as mm
    monkeypatch.setattr(libmod, "_lib", lib)
    monkeypatch.setattr(mm, "_model_manager", None)
    monkeypatch.setattr(mm.ModelManager, "_instance", None)
    m = mm.get_model_manager()
    assert m.detector_tail == "host"
    sd = yr.make_model("11", "n", 1, False, seed=5).state_dict()
    assert m._detector_from_state_dict(sd, default_names={0: "x"}).tail == "host"
    m.detector_tail = "device"
    model = m._detector_from_state_dict(sd, default_names={0: "x"})
    assert model.tail == "device" and isinstance(model, Yolo11Hip)
    from oracle import yolo_ref
    v8 = m._detector_from_state_dict(yolo_ref.make_model("n", 1, 0).state_dict(), default_names={0: "x"})
    assert v8.tail == "device" and type(v8) is yolo_mod.YoloSegHip
    m.detector_tail = "gpu"
    try:
        m._detector_from_state_dict(sd)
    except ModelError as e:
        assert "detector_tail" in str(e)
    else:
        raise AssertionError('detector_tail = "gpu" was accepted')
