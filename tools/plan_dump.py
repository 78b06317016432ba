"""Op stream of a model's plans as text: one line per recorded op, for diffing two builds of the same model.

    python tools/plan_dump.py kontext --fp8 --cached --size 4 6 16
    python tools/plan_dump.py klein --fp8 qkv --size 22 24 16
    python tools/plan_dump.py sam2 --variant high --digest --weights
    python tools/plan_dump.py manga-ocr --variant f32 --weights

A line holds the op's label, kind and lane, every non-pointer field of its argument block (include/mtx_hip.h) and every pointer field as `0`
or `<buffer>+<byte offset>`.  A buffer is named by the ordinal of its first appearance in the dump plus its shape and dtype, never by its
address or its place in `plan._keep`: two builds that record the same ops over the same layout give the same text, whatever order they
allocated in.  Pointers are looked up in the buffers the plans keep alive (all the dumped plans together) and in every tensor reachable from the
model object; one that lies in none of them is an error.  `--weights` adds a digest of the packed weights themselves, so that a repacking that
keeps the launches but moves a byte shows too.

The command line builds the seeded toy networks of the test suite on the kernel simulator (tests/emu), so it needs no GPU.  The entries use only
the models' long-standing names (`plans`, `_pre_plan`, `_encoder`, `_stepper`, `plan_for`, ...): the file can be copied into an older checkout to
dump what that one builds."""
import argparse
import bisect
import ctypes as C
import hashlib
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

from mangatranslator_amd.hip import abi  # noqa: E402

_KIND_NAME = {getattr(abi, n): n[3:] for n in dir(abi) if n.startswith("OP_") and isinstance(getattr(abi, n), int)}


def tensors_of(obj, out=None, seen=None):
    """every tensor reachable from `obj` through dicts, sequences and the package's own small holder classes"""
    out, seen = ([] if out is None else out), (set() if seen is None else seen)
    if id(obj) in seen:
        return out
    seen.add(id(obj))
    if torch.is_tensor(obj):
        out.append(obj)
    elif isinstance(obj, dict):
        for v in obj.values():
            tensors_of(v, out, seen)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            tensors_of(v, out, seen)
    elif type(obj).__module__.startswith("mangatranslator_amd") and hasattr(obj, "__dict__"):
        tensors_of(vars(obj), out, seen)
    return out


def plan_family(plan):
    """a one-plan step, or the head / body / skip plans of the first-block cache"""
    return [plan] + [p for p in (getattr(plan, "body", None), getattr(plan, "skip", None)) if p is not None]


class _Buffers:
    def __init__(self, tensors):
        spans = {}
        for t in tensors:
            if t.numel():
                lo, n = t.data_ptr(), t.numel() * t.element_size()
                if lo not in spans or n > spans[lo][0]:                 # a view that starts where its base does: the base names the buffer
                    spans[lo] = (n, f"{tuple(t.shape)}:{str(t.dtype).replace('torch.', '')}")
        self.starts = sorted(spans)
        self.spans = spans
        self.names = {}

    def name(self, ptr, where):
        if not ptr:
            return "0"
        i = bisect.bisect_right(self.starts, ptr) - 1
        while i >= 0:                                                   # the nearest buffer below may be a view inside the one that holds ptr
            lo = self.starts[i]
            n, what = self.spans[lo]
            if ptr < lo + n:
                if lo not in self.names:
                    self.names[lo] = f"b{len(self.names)}{what}"
                return f"{self.names[lo]}+{ptr - lo}"
            i -= 1
        raise LookupError(f"{where}: pointer {ptr:#x} lies in no buffer of the plans or the model")


def _fields(args, where, bufs):
    out = []
    for name, ft in args._fields_:
        v = getattr(args, name)
        if ft is C.c_void_p:
            out.append(f"{name}={bufs.name(v, where + '.' + name)}")
        elif issubclass(ft, C.Array):
            items = [bufs.name(x, where + '.' + name) if ft._type_ is C.c_void_p else repr(x) for x in v]
            out.append(f"{name}=[{','.join(items)}]")
        else:
            out.append(f"{name}={v!r}")
    return out


def dump(plans, holder) -> list:
    """the lines of `plans` — a list of plans (labelled p0, p1, ...), or one plan, which stands for itself plus its `.body` / `.skip` where it is the
    head of a cached DiT build (labelled head / body / skip) — of the model `holder`: the model object itself, or anything that holds its weights"""
    if isinstance(plans, (list, tuple)):
        plans, parts = list(plans), [f"p{i}" for i in range(len(plans))]
    else:
        plans, parts = plan_family(plans), ("head", "body", "skip")
    bufs = _Buffers(tensors_of([p._keep for p in plans]) + tensors_of(holder))
    lines = []
    for part, p in zip(parts, plans):
        for i, (label, op) in enumerate(zip(p.labels, p.ops)):
            where = f"{part}[{i}] {label}"
            args = getattr(op.u, abi.UNION_FIELD[op.kind])
            lines.append(" ".join([part, label, _KIND_NAME.get(op.kind, str(op.kind)), f"lane={op.lane}"] + _fields(args, where, bufs)))
    return lines


def digest(lines) -> str:
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def _weights(obj, path, out, seen):
    """(path, tensor) of every tensor the model holds as a weight or table.  A tuple adds nothing to the path (its tensors keep their order, so a
    stored pair and the same pair with a None between hash alike); plans, their caches and lanes (hip/plan.py) hold activations, not weights."""
    if torch.is_tensor(obj):
        out.append((path, obj))
    if torch.is_tensor(obj) or id(obj) in seen:
        return
    seen.add(id(obj))
    if isinstance(obj, dict):
        for k, v in obj.items():
            _weights(v, f"{path}.{k}", out, seen)
    elif isinstance(obj, tuple):
        for v in obj:
            _weights(v, path, out, seen)
    elif isinstance(obj, list):
        for i, v in enumerate(obj):
            _weights(v, f"{path}.{i}", out, seen)
    elif type(obj).__module__.startswith("mangatranslator_amd.core") and hasattr(obj, "__dict__"):
        _weights(vars(obj), path, out, seen)


def weights_digest(holder) -> str:
    """SHA-256 over every weight tensor of `holder` (dtype, shape and bytes, as tests/yolo11_checks.py pack_digests feeds them), sorted by path"""
    found = []
    _weights(holder, "", found, set())
    h = hashlib.sha256()
    for path, t in sorted(found, key=lambda e: e[0]):
        t = t.detach().cpu().contiguous()
        h.update(f"{path}{t.dtype}{tuple(t.shape)}".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def simulator():
    import subprocess
    from mangatranslator_amd.hip.lib import _open_simulator_for_tests
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT / "mangatranslator_amd" / "csrc", check=True)
    return _open_simulator_for_tests(ROOT / "tests" / "emu" / "libmtx_emu.so")


# entry -> its variants (the first is the default)
VARIANTS = {"sam2": ("fast", "high"), "sam3": ("fast", "high"), "manga-ocr": ("f16", "f32"), "yolo": ("v8n-seg",), "yolo11": ("11n", "11n-seg", "12n"),
            "rtdetr": ("tiny_test",), "rcan": ("pool", "nopool"), "flux-vae": ("toy",)}


def _toy_dit(model, lib, size, fp8, cached, net, **dit_kw):
    h2, w2, t_txt = size
    if model == "klein":
        import flux2_checks as f2c
        t, v = f2c.models(**(net if net is not None else dict(d=256, heads=2, axes_dim=(32, 32, 32, 32), layers=1, single_layers=1)))
        dit, _ = f2c.hip_models(t, v, lib, "cpu", fp8=fp8, **dit_kw)
        return dit.plan_for(t_txt, h2, w2, h2, w2), dit
    import flux_checks as fc
    import kontext_fp8_checks as kc
    t, v = fc.models(**(net if net is not None else dict(layers=1, single_layers=1, **kc.HD128)))
    dit, _ = kc.hip_models(t, v, lib, "cpu", fp8=fp8, **dit_kw)
    return dit.plan_for(t_txt, h2, w2, 1, cached=cached), dit


def _toy_yolo(hip, h, w, imgsz):
    from mangatranslator_amd.core.ml.yolo import letterbox_params
    lp = letterbox_params(h, w, imgsz)
    net = hip._build(lp)
    return [net, hip._page_plan(net.img, h, w, lp)], hip


def toy_plan(model: str, lib, size=(4, 6, 16), fp8=False, cached=False, net=None, variant=None, **dit_kw):
    """(plans, holder) of one seeded toy network of the test suite (tests/*_checks.py) on `lib`, for `dump`: one plan for the DiT models "kontext" and
    "klein", a list of plans for the entries of VARIANTS"""
    if model in ("kontext", "klein"):
        return _toy_dit(model, lib, size, fp8, cached, net, **dit_kw)
    variant = variant or VARIANTS[model][0]
    if variant not in VARIANTS[model]:
        raise ValueError(f"{model}: variant {variant!r} is not one of {VARIANTS[model]}")
    if model in ("sam2", "sam3"):
        if model == "sam2":
            from mangatranslator_amd.core.ml.sam2 import Sam2Hip as cls
            from oracle import sam2_ref as src
            m, cfg = src.make_model("tiny_test", 0)
        else:
            import sam3_checks as src
            from mangatranslator_amd.core.ml.sam3 import Sam3Hip as cls
            m, cfg = src.make_model("tiny", 0)
        hip = cls(m.state_dict(), cfg, device="cpu", lib=lib, precision=variant)
        return list(hip.plans(2, 120, 260)), hip
    if model == "manga-ocr":
        import manga_ocr_checks as mc
        hip = mc.hip_model(lib, mc.oracle(0)[0], abi.F16 if variant == "f16" else abi.F32, 4)
        return [hip._pre_plan(50, 70), hip._encoder(), hip._stepper()], hip
    if model == "yolo":
        from mangatranslator_amd.core.ml.yolo import YoloSegHip
        from oracle import yolo_ref
        return _toy_yolo(YoloSegHip(yolo_ref.make_model("n", 1, 0).state_dict(), device="cpu", lib=lib), 160, 96, 128)
    if model == "yolo11":
        from mangatranslator_amd.core.ml.yolo11 import Yolo11Hip
        from oracle import yolo11_ref
        family, seg, seed, shape = {"11n": ("11", False, 0, (96, 64, 64)), "11n-seg": ("11", True, 2, (192, 128, 128)), "12n": ("12", False, 3, (96, 64, 64))}[variant]
        return _toy_yolo(Yolo11Hip(yolo11_ref.make_model(family, "n", 1, seg, seed=seed).state_dict(), device="cpu", lib=lib), *shape)
    if model == "rtdetr":
        from mangatranslator_amd.core.ml.rtdetr import RTDetrHip
        from oracle import rtdetr_ref
        m, cfg = rtdetr_ref.make_model("tiny_test", 0)
        hip = RTDetrHip(m.state_dict(), cfg, "cpu", lib=lib, graph=False)
        return list(hip.plans(64, 96)), hip
    if model == "rcan":
        from mangatranslator_amd.core.ml.rcan import RCANUpscaler
        from oracle.rcan_ref import make_state_dict
        hip = RCANUpscaler(make_state_dict(n_feats=64, n_resgroups=2, n_resblocks=2, seed=0), device="cpu", lib=lib, pool_before_conv=variant == "pool")
        return [hip.plan_for(1, 20, 36)], hip
    if model == "flux-vae":
        import flux_checks as fc
        _, vae = fc.hip_models(*fc.models(layers=1, single_layers=1), lib, "cpu")
        return [vae.encoder_plan(64, 96), vae.decoder_plan(8, 12)], vae
    raise ValueError(model)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("model", choices=("kontext", "klein") + tuple(VARIANTS))
    ap.add_argument("--variant", default=None, help="which build of a non-DiT entry (VARIANTS; default: its first)")
    ap.add_argument("--fp8", nargs="*", default=None, metavar="KIND", help="DiT: no kind: every block linear; else the kinds (FP8_ALL of the model)")
    ap.add_argument("--cached", action="store_true", help="Kontext: the three plans of the first-block cache")
    ap.add_argument("--size", nargs=3, type=int, default=(4, 6, 16), metavar=("H2", "W2", "T_TXT"), help="DiT: the step's size")
    ap.add_argument("--off", nargs="*", default=(), metavar="SWITCH", help="DiT: constructor switches to turn off (fused_quant, attn_q8, ...)")
    ap.add_argument("--digest", action="store_true", help="print the SHA-256 of the dump only")
    ap.add_argument("--weights", action="store_true", help="also print `weights <SHA-256>` over every weight tensor of the model")
    a = ap.parse_args(argv)
    fp8 = False if a.fp8 is None else (tuple(a.fp8) or True)
    plans, holder = toy_plan(a.model, simulator(), tuple(a.size), fp8, a.cached, variant=a.variant, **{k: False for k in a.off})
    lines = dump(plans, holder)
    print(digest(lines) if a.digest else "\n".join(lines))
    if a.weights:
        print("weights", weights_digest(holder))


if __name__ == "__main__":
    main()
