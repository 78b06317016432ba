"""Op stream of a DiT step as text: one line per recorded op, for diffing two builds of the same model.

    python tools/plan_dump.py kontext --fp8 --cached --size 4 6 16
    python tools/plan_dump.py klein --fp8 qkv --size 22 24 16

A line holds the op's label, kind and lane, every non-pointer field of its argument block (include/mtx_hip.h) and every pointer field as `0`
or `<buffer>+<byte offset>`.  A buffer is named by the ordinal of its first appearance in the dump plus its shape and dtype, never by its
address or its place in `plan._keep`: two builds that record the same ops over the same layout give the same text, whatever order they
allocated in.  Pointers are looked up in the buffers the plans keep alive (the head, body and skip plans of a cached build together) and in
the model's weights (`W`, `blocks`, `singles`); one that lies in none of them is an error.

The command line builds the toy networks of the test suite on the kernel simulator (tests/emu), so it needs no GPU."""
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


def dump(plan, model) -> list:
    """the lines of `plan` (with `.body` / `.skip` where it is the head of a cached build) of `model`"""
    plans = plan_family(plan)
    bufs = _Buffers(tensors_of([p._keep for p in plans]) + tensors_of([model.W, model.blocks, model.singles]))
    lines = []
    for part, p in zip(("head", "body", "skip"), plans):
        for i, (label, op) in enumerate(zip(p.labels, p.ops)):
            where = f"{part}[{i}] {label}"
            args = getattr(op.u, abi.UNION_FIELD[op.kind])
            lines.append(" ".join([part, label, _KIND_NAME.get(op.kind, str(op.kind)), f"lane={op.lane}"] + _fields(args, where, bufs)))
    return lines


def digest(lines) -> str:
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def simulator():
    import subprocess
    from mangatranslator_amd.hip.lib import _open_simulator_for_tests
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT / "mangatranslator_amd" / "csrc", check=True)
    return _open_simulator_for_tests(ROOT / "tests" / "emu" / "libmtx_emu.so")


def toy_plan(model: str, lib, size=(4, 6, 16), fp8=False, cached=False, net=None, **dit_kw):
    """(plan, dit) of one toy network of the test suite (tests/flux2_checks.py, tests/kontext_fp8_checks.py) on `lib`"""
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("model", choices=("kontext", "klein"))
    ap.add_argument("--fp8", nargs="*", default=None, metavar="KIND", help="no kind: every block linear; else the kinds (FP8_ALL of the model)")
    ap.add_argument("--cached", action="store_true", help="Kontext: the three plans of the first-block cache")
    ap.add_argument("--size", nargs=3, type=int, default=(4, 6, 16), metavar=("H2", "W2", "T_TXT"))
    ap.add_argument("--off", nargs="*", default=(), metavar="SWITCH", help="constructor switches to turn off (fused_quant, attn_q8, ...)")
    ap.add_argument("--digest", action="store_true", help="print the SHA-256 of the dump only")
    a = ap.parse_args(argv)
    fp8 = False if a.fp8 is None else (tuple(a.fp8) or True)
    plan, dit = toy_plan(a.model, simulator(), tuple(a.size), fp8, a.cached, **{k: False for k in a.off})
    lines = dump(plan, dit)
    print(digest(lines) if a.digest else "\n".join(lines))


if __name__ == "__main__":
    main()
