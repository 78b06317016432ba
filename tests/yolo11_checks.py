"""YOLO11 / YOLO12 parity: libmtx_hip graphs (core/ml/yolo11.py) vs the fp32 CPU oracle (oracle/yolo11_ref.py): decoded head (boxes,
scores, mask coefficients), final boxes after NMS, retina masks for the seg variant."""
import numpy as np
import torch

from mangatranslator_amd.core.ml.yolo11 import Yolo11Hip
from oracle import yolo11_ref as yr


def make_page(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    page = np.stack([(xx * 3 + yy) % 256, (xx + yy * 2) % 256, (xx * yy // 7) % 256], -1).astype(np.float32)
    page += rng.normal(0, 12, page.shape)
    return np.clip(page, 0, 255).astype(np.uint8)


stats = {}      # figures of the last check (recorded by the GPU tests)
ORACLE_THREADS = 128    # CPU threads while the seeded network is conditioned (see check): the count the recorded figures (profiles/*_parity.json) were taken with


def check(lib, device, family="11", scale="n", seg=False, h=96, w=64, imgsz=64, seed=0, nc=1, tol=2e-2, mask_tol=0.03, n_det=12):
    from oracle import yolo_ref
    # The seeded network is conditioned on its own CPU activations and then rounded to f16.  With the host's thread count the sums change, and
    # with them thousands of the rounded weights and the worst anchor of the GPU check: a fixed thread count takes the host's core count out of it.
    n_threads = torch.get_num_threads()
    torch.set_num_threads(ORACLE_THREADS)
    net = yr.make_model(family, scale, nc, seg, seed=seed)
    page = make_page(h, w, seed + 1)
    x, lp = yolo_ref.letterbox(page, imgsz)
    yr.calibrate(net, x)                  # every layer's output zero-mean / unit-spread on this page: the features stay input-dependent at depth
    # a random-weight head saturates: rescale the last conv of the box / class branches so their logits have unit spread, as a trained
    # head's do — otherwise the DFL expectation and the sigmoid amplify f16 rounding into whole bins (same device as yolo_checks.py)
    head = net.model[-1]
    grabbed = {}
    hooks = [head.cv2[l][1].register_forward_hook(lambda m, i, o, l=l: grabbed.__setitem__(("b", l), o)) for l in range(3)]
    hooks += [head.cv3[l][1].register_forward_hook(lambda m, i, o, l=l: grabbed.__setitem__(("c", l), o)) for l in range(3)]
    net(x)
    for hk in hooks:
        hk.remove()
    with torch.no_grad():
        for l in range(3):
            sb = head.cv2[l][2](grabbed[("b", l)]).std().item()
            head.cv2[l][2].weight.div_(sb); head.cv2[l][2].bias.div_(sb)
            sc_ = head.cv3[l][2](grabbed[("c", l)]).std().item()
            head.cv3[l][2].weight.div_(sc_); head.cv3[l][2].bias.fill_(-1.0)
        for p_ in net.parameters():
            p_.copy_(p_.to(torch.float16).float())
    torch.set_num_threads(n_threads)
    hip = Yolo11Hip(net.state_dict(), device=device, lib=lib, names={i: f"c{i}" for i in range(nc)})
    assert hip.a["family"] == family and hip.a["seg"] == seg
    pred, _ = net(x)
    scores = pred[0, 4:4 + nc].max(0).values
    conf = float(scores.sort(descending=True).values[min(n_det, scores.numel() - 1)])      # about a dozen candidates pass
    ref = yr.predict(net, page, imgsz=imgsz, conf=conf)
    res = hip(page, conf=conf, imgsz=imgsz)[0]
    plan, _ = hip._plans[(h, w, imgsz)]
    dec = plan.decoded.float().cpu().t()
    want = ref["pred"]
    box_err = (dec[:4] - want[:4]).abs().max().item()                      # letterboxed pixels
    box_med = (dec[:4] - want[:4]).abs().median().item()
    e_cls = (dec[4:4 + nc] - want[4:4 + nc]).abs().max().item()
    # The DFL decode turns rounding of the box logits into fractions of a BIN, and a bin is one stride wide: the same logit error is four
    # times the pixels at stride 32 that it is at stride 8.  So the bound on the worst anchor is stated per pyramid level, in bins —
    # 0.08 of a bin (0.64 / 1.28 / 2.56 px at strides 8 / 16 / 32) — beside the median (0.05 px) and the 99.9th percentile (1.5 px).  (Until round 5
    # one flat 2.0 px on the maximum over all levels: YOLO11-L sat at 1.96, i.e. at 0.061 bin of its stride-32 level, and moved across it
    # with a 1-ulp-but-one-sided change in the SiLU epilogues (csrc/mtx_device.h div_by_1p); the per-level figures are printed and recorded:
    # YOLO11-L 0.041 / 0.043 / 0.061 bin, 99.9 % 1.10 px; YOLO11m-seg 0.029 / 0.043 / 0.024, 0.31 px; YOLO12x 99.9 % 0.37 px.)
    err_px = (dec[:4] - want[:4]).abs().max(0).values                       # per anchor
    strides, n_lvl = (8, 16, 32), [(lp["H"] // st) * (lp["W"] // st) for st in (8, 16, 32)]
    assert sum(n_lvl) == err_px.numel(), (n_lvl, err_px.numel())
    lvl_bins, a0 = [], 0
    for st, n_ in zip(strides, n_lvl):
        lvl_bins.append(err_px[a0:a0 + n_].max().item() / st)
        a0 += n_
    box_p999 = torch.quantile(err_px, 0.999).item()
    stats.update(box_err_px=box_err, box_median_px=box_med, box_p999_px=box_p999, box_err_bins_by_stride=dict(zip(strides, [round(v, 4) for v in lvl_bins])))
    print(f"YOLO{family}{scale}{'-seg' if seg else ''} @{lp['W']}x{lp['H']}: decoded boxes max {box_err:.3f} px (median {box_med:.4f}, 99.9 % {box_p999:.3f}; "
          f"worst anchor per level {', '.join(f'{v:.3f} bin @ stride {st}' for st, v in zip(strides, lvl_bins))}), class score abs err {e_cls:.4f}")
    # round 6: the box branch's last convolution and the DFL expectation run on fp32 logits (mtx_yolo_decode_args.box_f32), and the flat bound on
    # the worst anchor of any level is back beside the per-level one
    assert box_err < 2.0 and max(lvl_bins) < 0.08 and box_p999 < 1.5 and box_med < 0.05 and e_cls < tol
    if seg:
        e_mc = ((dec[4 + nc:] - want[4 + nc:]).abs().max() / want[4 + nc:].abs().max()).item()
        assert e_mc < 2 * tol, e_mc
    n_ref = len(ref["boxes"])
    got = res.boxes.xyxy.cpu().numpy() if res.boxes is not None else np.zeros((0, 4), np.float32)
    assert abs(len(got) - n_ref) <= 2, (len(got), n_ref)                   # the same set, threshold ties aside: match by position
    matched, mism = 0, []
    got_conf = res.boxes.conf.cpu().numpy() if res.boxes is not None else np.zeros(0, np.float32)
    masks = res.masks.data.cpu().numpy().astype(bool) if (seg and len(got)) else None
    for i, rb in enumerate(ref["boxes"]):
        if not len(got):
            break
        d = np.abs(got - rb[None]).max(1)
        near = np.nonzero(d < 3.0)[0]                                      # boxes clipped to the page can coincide: tell them apart by score
        j = int(near[np.abs(got_conf[near] - ref["conf"][i]).argmin()]) if len(near) else int(d.argmin())
        if d[j] < 3.0:
            matched += 1
            # two overlapping candidates whose scores tie within f16 rounding may swap places in the NMS order: the surviving box is
            # then a NEIGHBOUR anchor's (a pixel or two away, unrelated mask coefficients in a seeded network).  Masks are compared
            # where the survivor is the same anchor, i.e. its box agrees to within the decoded-box error.
            if seg and d[j] < max(0.6, 3.0 * box_err / min(lp["H"] / h, lp["W"] / w)) and abs(got_conf[j] - ref["conf"][i]) < 3 * e_cls + 1e-4:
                mism.append(float((masks[j] != ref["masks"][i]).mean()))
    assert matched >= n_ref - 2, (matched, n_ref)
    if seg and n_ref:
        assert len(mism) >= max(1, n_ref // 2), (len(mism), n_ref)
        assert max(mism) < mask_tol, f"mask mismatch {max(mism):.4%}"
    return box_err, e_cls


def pack_digests(lib):
    """sha256 of everything `_pack` leaves in `W` (and `DW`) — names, padded weights and biases as stored (f16 / f32 bytes), `cout`, `k`, the qkv
    geometry — for the seeded YOLOv8n-seg, YOLO11n, YOLO11n-seg and YOLO12n state dicts of the simulator tests.  The recorded values
    (tests/golden/yolo_pack_digests.json, written by tests/golden/make_yolo_pack_digests.py) pin the packed layout."""
    import hashlib
    from mangatranslator_amd.core.ml.yolo import YoloSegHip
    from oracle import yolo_ref

    def feed(h, v):
        if torch.is_tensor(v):
            t = v.detach().cpu().contiguous()
            h.update(f"{t.dtype}{tuple(t.shape)}".encode())
            h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
        elif isinstance(v, (tuple, list)):
            for x in v:
                feed(h, x)
        else:
            h.update(repr(v).encode())

    def digest(model):
        h = hashlib.sha256()
        for table in (model.W, getattr(model, "DW", {})):
            for name in sorted(table):
                h.update(name.encode())
                feed(h, table[name])
        return h.hexdigest()

    out = {"yolov8n-seg": digest(YoloSegHip(yolo_ref.make_model("n", 1, 0).state_dict(), device="cpu", lib=lib))}
    for tag, (family, seg, seed) in {"yolo11n": ("11", False, 0), "yolo11n-seg": ("11", True, 2), "yolo12n": ("12", False, 3)}.items():
        out[tag] = digest(Yolo11Hip(yr.make_model(family, "n", 1, seg, seed=seed).state_dict(), device="cpu", lib=lib))
    return out


def check_batched(lib, device, family="11", scale="n", h=96, w=64, imgsz=64, pages=3, batch=4, seed=0, threads=False):
    """core/ml/detector_batch.py: `pages` different pages through ONE batched graph replay (DetectorBatcher) give, page by page, the bytes of the
    one-image call — decoded head rows and final boxes / scores / classes.  threads: every page submitted and collected by its own thread (the
    way the front halves of a batch run share a detector); otherwise all submits, then all collects, on this thread."""
    from mangatranslator_amd.core.ml.detector_batch import DetectorBatcher
    net = yr.make_model(family, scale, 1, False, seed=seed)
    from oracle import yolo_ref
    x, _ = yolo_ref.letterbox(make_page(h, w, seed + 1), imgsz)
    yr.calibrate(net, x)
    hip = Yolo11Hip(net.state_dict(), device=device, lib=lib)
    imgs = [make_page(h, w, seed + 1 + i) for i in range(pages)]
    singles, rows = [], []
    for im in imgs:
        r = hip(im, conf=0.05, imgsz=imgsz)[0]
        plan, _ = hip._plans[(h, w, imgsz)]
        singles.append(r)
        rows.append(plan.decoded.clone())
    bat = DetectorBatcher(hip, batch=batch)
    if threads:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=pages) as ex:
            got = list(ex.map(lambda im: bat(im, conf=0.05, imgsz=imgsz)[0], imgs))
    else:
        tickets = [bat.submit(im, conf=0.05, imgsz=imgsz) for im in imgs]
        held = [(t.batch, t.slot) for t in tickets]
        got = []
        for i, t in enumerate(tickets):
            b_, s_ = held[i]
            got.append(bat.collect(t)[0])
            assert torch.equal(b_.plan.decoded[s_], rows[i]), f"page {i}: decoded rows of the batched graph differ from the one-image graph"
        assert bat.stats["launches"] == (pages + batch - 1) // batch, bat.stats
    assert bat.stats["pages"] == pages
    n_boxes = 0
    for i, (a, b) in enumerate(zip(singles, got)):
        assert (a.boxes is None) == (b.boxes is None), f"page {i}"
        if a.boxes is not None:
            for f in ("xyxy", "conf", "cls"):
                assert torch.equal(getattr(a.boxes, f), getattr(b.boxes, f)), f"page {i}: boxes.{f} differ between the batched and the one-image call"
            n_boxes += len(a.boxes)
    assert n_boxes > 0, "no page produced a box: the comparison is empty"
    return bat.stats
