"""Lane hazards of the DiT step plans (FLUX.1-Kontext, FLUX.2-Klein): which launches may run at the same time, and that no two of them touch
the same bytes.

Three layers, shared by tests/test_lane_hazards_sim.py and tests/test_lane_hazards_gpu.py:
  * `check_footprints`  — the model of "what does an op touch" (tests/plan_footprints.py) held against the kernels on the simulator: every op
    runs alone twice, once on the in-order state and once with every byte outside its declared reads scrambled (NaN patterns included); the
    declared writes must come out equal, and nothing outside them may change.  A write region that is not also read was scrambled before the
    second run, so a region declared more coarsely than the kernel writes fails the first assertion too.
  * `check_no_hazards`  — the static analysis: every side / main pair `mtx_plan_run` leaves unordered has disjoint footprints.
  * `check_lanes_bit_equal` — hardware: the step built with lanes equals the step built on one lane, eagerly and as a hipGraph replay.
"""
import contextlib
import gc
import math

import numpy as np
import torch

from mangatranslator_amd.core.ml import dit_graph
from mangatranslator_amd.core.ml import flux as fx
from mangatranslator_amd.core.ml import flux2 as f2
from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.plan import PlanBuilder

import flux2_checks as f2c
import flux_checks as fc
import kontext_fp8_checks as kc
import plan_footprints as pf

GEOMETRIES = {"small": (16, 4, 6),        # the suite's own: t_txt, h2, w2
              "odd": (23, 5, 7)}          # T = 23 + 2 x 35 = 93 for both models: neither the text rows nor all rows are a multiple of 64, or of the 4 rows
                                          # whose scale words share 16 bytes, so the text / image cut of every scale plane falls inside such a group
KLEIN_F8 = dict(d=256, heads=2, axes_dim=(32, 32, 32, 32), layers=2, single_layers=1)      # 3 d % 256 == 0: the gated epilogue exists; head dim 128
KONTEXT_F8 = dict(layers=2, single_layers=1)               # the toy network, one single block less: every op form, a third less simulator time
VARIANTS = {
    "kontext": ("kontext", {}, {}),
    "kontext.cached": ("kontext", {}, {}),
    "kontext.fp8": ("kontext", dict(fp8=True), KONTEXT_F8),
    "kontext.fp8.no_act_epilogue": ("kontext", dict(fp8=True, act_epilogue=False), KONTEXT_F8),
    "klein": ("klein", {}, {}),
    "klein.fp8": ("klein", dict(fp8=True), KLEIN_F8),
    "klein.fp8.no_fused_quant": ("klein", dict(fp8=True, fused_quant=False), KLEIN_F8),
    "klein.fp8.no_glu_epilogue": ("klein", dict(fp8=True, glu_epilogue=False), KLEIN_F8),
    "klein.fp8.no_attn_q8": ("klein", dict(fp8=True, attn_q8=False), KLEIN_F8),
}
_models = {}


def _oracle_models(kind, model_kw):
    key = (kind, tuple(sorted(model_kw.items())))
    if key not in _models:
        _models[key] = (fc if kind == "kontext" else f2c).models(**model_kw)
    return _models[key]


def build_step(lib, device, variant, geometry="small", lanes=True):
    """-> (dit, [(name, plan)]) with the step's inputs filled; the cached Kontext form gives its three plans in the order they run"""
    kind, dit_kw, model_kw = VARIANTS[variant]
    t_txt, h2, w2 = GEOMETRIES[geometry] if isinstance(geometry, str) else geometry
    t, v = _oracle_models(kind, model_kw)
    if kind == "kontext":
        dit, _ = kc.hip_models(t, v, lib, device, text_stream_on_side_lane=lanes, **dit_kw)
        lat, pe, pooled = kc.step_inputs(t.cfg, h2, w2, t_txt)
        head = dit.plan_for(t_txt, h2, w2, 1, cached=variant.endswith(".cached"))
        head.mod.copy_(dit.modulation(0.7, 2.5, pooled.to(device, torch.bfloat16)))
        plans = [("head", head), ("body", head.body), ("skip", head.skip)] if variant.endswith(".cached") else [("step", head)]
    else:
        dit, _ = f2c.hip_models(t, v, lib, device, text_stream_on_side_lane=lanes, **dit_kw)
        for k in ("fused_quant", "glu_epilogue", "attn_q8"):
            assert getattr(dit, k) == dit_kw.get(k, True) or not dit_kw.get("fp8"), f"{variant}: the geometry does not allow {k}"
        lat, pe = f2c.step_inputs(t, h2, w2, h2, w2, t_txt)
        head = dit.plan_for(t_txt, h2, w2, h2, w2)
        head.mod.copy_(dit.modulation(0.7))
        plans = [("step", head)]
    head.ctx_in.copy_(pe.to(device, torch.bfloat16))
    head.lat.copy_(lat.to(device, torch.bfloat16))
    return dit, plans


def model_tensors(obj):
    """every tensor reachable from a DiT's weight tables (`W`, `blocks`, `singles`: tensors, tuples, dicts, dit_graph.Weight)"""
    out = []
    if torch.is_tensor(obj):
        return [obj]
    if isinstance(obj, dit_graph.Weight):
        return [t for t in (obj.w16, obj.q, obj.scale, obj.bias) if t is not None]
    if isinstance(obj, dict):
        obj = list(obj.values())
    if isinstance(obj, (list, tuple)):
        for o in obj:
            out += model_tensors(o)
    return out


def held_tensors(dit, plans):
    """everything the plans' kernels may touch: the buffers every plan of the step holds, and the model's weights"""
    ts = model_tensors([dit.W, dit.blocks, dit.singles])
    for _, p in plans:
        ts += [t.t if hasattr(t, "t") and torch.is_tensor(t.t) else t for t in p._keep]
    return [t for t in ts if torch.is_tensor(t)]


# ---- the A/B check of the footprint model (simulator) ---------------------------------------------------------------------------------------
_NAN = {torch.bfloat16: (np.uint16, 0x7FC0), torch.float16: (np.uint16, 0x7E00), torch.float32: (np.uint32, 0x7FC00000)}


class Arena:
    """the storages behind a list of CPU tensors as byte arrays (views of one storage are one entry)"""

    def __init__(self, tensors, seed=0):
        seen = {}
        for t in tensors:
            st = t.untyped_storage()
            if st.data_ptr() not in seen and st.nbytes() > 0:
                seen[st.data_ptr()] = (torch.empty(0, dtype=torch.uint8).set_(st).numpy(), t.dtype)
        self.base = sorted(seen)
        self.bytes = [seen[b][0] for b in self.base]
        rng = np.random.default_rng(seed)
        self.noise = []
        for b in self.base:
            arr, dt = seen[b]
            z = rng.integers(0, 256, arr.size, dtype=np.uint8)
            if dt in _NAN and arr.size % np.dtype(_NAN[dt][0]).itemsize == 0:      # 16-bit and fp32 buffers: every fifth element a NaN
                z.view(_NAN[dt][0])[::5] = _NAN[dt][1]
            self.noise.append(z)

    def snapshot(self):
        return [b.copy() for b in self.bytes]

    def restore(self, snap):
        for b, s in zip(self.bytes, snap):
            b[:] = s

    def mask(self, rects, what):
        """per storage, the bytes inside `rects`; a declared byte that lies in no held tensor is an error of the model (or an unknown tensor)"""
        ms = [np.zeros(b.size, dtype=bool) for b in self.bytes]
        for r in rects:
            found = 0
            for k, tb in enumerate(self.base):
                te = tb + self.bytes[k].size
                if r.base >= te or r.end <= tb:
                    continue
                for i in range(r.rows):
                    lo, hi = max(r.base + i * r.stride, tb), min(r.base + i * r.stride + r.row_bytes, te)
                    if hi > lo:
                        ms[k][lo - tb:hi - tb] = True
                        found += hi - lo
            assert found == r.rows * r.row_bytes, f"{what}: {r} declares {r.rows * r.row_bytes} bytes, {found} of them inside tensors the plan holds"
        return ms


def check_footprints(plans, tensors, stats=None, seed=0):
    """plans: [(name, plan)] run one after the other over shared buffers (simulator).  stats: dict kind-name -> ops checked (filled)."""
    arena = Arena(tensors, seed)
    for pname, plan in plans:
        for i, (op, label) in enumerate(zip(plan.ops, plan.labels)):
            what = f"{pname} op {i} '{label}'"
            reads, writes = pf.footprint(op)
            rmask, wmask = arena.mask(reads, what + " reads"), arena.mask(writes, what + " writes")
            before = arena.snapshot()
            plan.run_range(i, i)                                   # A
            after_a = arena.snapshot()
            arena.restore(before)
            for b, z, m in zip(arena.bytes, arena.noise, rmask):   # B: everything outside the declared reads is noise
                np.copyto(b, z, where=~m)
            scrambled = arena.snapshot()
            plan.run_range(i, i)
            for k, (a, b, s, m) in enumerate(zip(after_a, arena.bytes, scrambled, wmask)):
                bad = np.nonzero((a != b) & m)[0]
                assert bad.size == 0, (f"{what}: {bad.size} bytes of its declared writes depend on bytes outside its declared reads "
                                       f"(first at 0x{arena.base[k] + int(bad[0]):x}; reads {[str(r) for r in reads]})")
                bad = np.nonzero((b != s) & ~m)[0]
                assert bad.size == 0, (f"{what}: wrote {bad.size} bytes outside its declared writes "
                                       f"(first at 0x{arena.base[k] + int(bad[0]):x}; writes {[str(r) for r in writes]})")
            arena.restore(after_a)                                 # the in-order state goes on
            if stats is not None:
                key = op_kind_name(op)
                stats[key] = stats.get(key, 0) + 1


def check_footprints_long_forms(lib, device="cpu", stats=None):
    """the forms only long sequences and large problems reach, at the smallest shapes that reach them, as plans of a few ops:
    attention with sq 1024, sk 256, one head of 128 — 16-bit with its workspace, then with MX fp8 output, fp8 scores and fp8 P V (fed by the
    rotary kernel's e4m3 twin and the V^T kernel) — and the 256-tile GEMM with its K-slice workspace (1024 x 256 x 4096: one tile left over
    on the simulator's 3 CUs, cut into K slices), 16-bit and fp8."""
    g = torch.Generator().manual_seed(11)
    sq, sk, d = 1024, 256, 128
    pb = PlanBuilder(lib, device, abi.BF16)
    qkv = pb.buf((sq, 3 * d), torch.bfloat16)
    qkv.copy_(torch.randn(sq, 3 * d, generator=g).to(torch.bfloat16))
    o = pb.buf((sq, d), torch.bfloat16)
    cs = pb.buf((2, sq, 2, d // 2))
    ang = torch.rand(sq, d // 2, generator=g) * 6.283
    cs[0].copy_(torch.stack([ang.cos(), ang.sin()], 1))
    cs[1].copy_(cs[0] * (1.4426950408889634 / math.sqrt(d)))
    gamma = pb.buf((2 * d,))
    gamma.copy_(1.0 + 0.1 * torch.randn(2 * d, generator=g))
    qk8 = pb.buf((sq, 2 * d), torch.uint8, zero=True)
    o8, o8s = pb.buf((sq, d), torch.uint8), pb.buf((d // 128, sq), torch.int32, zero=True)
    from mangatranslator_amd.hip.plan import Act
    pb.qk_norm_rope(Act(qkv.view(1, 1, sq, 3 * d), 1, 1, sq, 2 * d), cs[0], sq * d, gamma, d, 1, y8=(qk8, 2 * d, 8.0), label="rope+y8")
    strides = ((0, 3 * d, d),) * 3 + ((0, d, d),)
    pb.attention(qkv, qkv, qkv, o, 1, 1, sq, sk, d, *strides, 1.0 / math.sqrt(d), k_off=d, v_off=2 * d, q_prescaled=True, label="attn.long")
    vt8 = pb.v_f8t(qkv, sk, 1, 3 * d, v_off=2 * d, label="v_f8t")
    pb.attention(qkv, qkv, qkv, None, 1, 1, sq, sk, d, *strides, 1.0 / math.sqrt(d), k_off=d, v_off=2 * d, q_prescaled=True,
                 q8=(o8, o8s, d, sq, 0), qk_f8=(qk8, 0, d, 2 * d, -3), pv_f8=vt8, label="attn.long.f8")
    plan = pb.build()
    assert all(op.u.attn.workspace for op in plan.ops if op.kind == abi.OP_ATTN)
    check_footprints([("attention", plan)], plan._keep, stats)

    m, n, k = 1024, 256, 4096
    pb = PlanBuilder(lib, device, abi.BF16)
    a, w = pb.buf((m, k), torch.bfloat16), pb.buf((n, k), torch.bfloat16)
    a.copy_(torch.randn(m, k, generator=g).to(torch.bfloat16)); w.copy_((torch.randn(n, k, generator=g) / 64).to(torch.bfloat16))
    res = pb.buf((m, n), torch.bfloat16)
    res.copy_(torch.randn(m, n, generator=g).to(torch.bfloat16))
    gate = pb.buf((2, n), torch.bfloat16)
    gate.copy_(torch.randn(2, n, generator=g).to(torch.bfloat16))
    pb.gemm(a, w, m, n, k, res=res, gate=gate, gate_rows_per=m // 2, flags=abi.GEMM_FORCE_TILE256, label="gemm256.kslice")
    _check_sliced_gemm(lib, pb.build(), stats)
    m, n, k = 1024, 256, 1024                                   # fp8: the same tile plane, 8 K iterations of 128, the left-over tile in 3 slices (MTX_GEMM_SLICES(3))
    pb = PlanBuilder(lib, device, abi.BF16)
    a, w = pb.buf((m, k), torch.bfloat16), pb.buf((n, k), torch.bfloat16)
    a.copy_(torch.randn(m, k, generator=g).to(torch.bfloat16)); w.copy_((torch.randn(n, k, generator=g) / 32).to(torch.bfloat16))
    aq, asc, lds_a = pb.quantize(a, m, k, label="quant.a")
    wq, wsc, lds_w = pb.quantize(w, n, k, label="quant.w")
    pb.gemm(aq, wq, m, n, k, f8=(asc, lds_a, wsc, lds_w, 0, 0), flags=abi.GEMM_FORCE_TILE256 | (3 << 8), label="gemm256.f8.kslice")
    _check_sliced_gemm(lib, pb.build(), stats)


def _check_sliced_gemm(lib, plan, stats):
    g = plan.ops[-1].u.gemm
    assert plan.ops[-1].kind == abi.OP_GEMM and g.workspace and g.workspace_bytes == abi.GEMM_WORKSPACE_BYTES
    check_footprints([("gemm", plan)], plan._keep, stats)
    split = lib.gemm_last_split()              # (whole tiles, K slices, tail pieces) of the last launch: the shape really took the K-slice tail
    assert split[1] >= 2 and split[2] >= 2, f"'{plan.labels[-1]}' did not slice K: {split}"


_EW_NAMES = {abi.EW_COPY: "copy", abi.EW_SUB: "sub", abi.EW_ADD: "add", abi.EW_SWIGLU: "swiglu", abi.EW_QK_NORM_ROPE: "qk_norm_rope",
             abi.EW_V_F8T: "v_f8t", abi.EW_RESIDUAL_DIST: "residual_dist"}


def op_kind_name(op):
    """kind and the options that change the footprint, for the per-kind tally of the experiments log"""
    if op.kind == abi.OP_GEMM:
        g = op.u.gemm
        return "gemm" + (".f8" if g.in_dtype == abi.F8 else "") + (".actq" if g.actq_q else "") + (".glu" if g.glu_q else "") + \
            (".gate" if g.gate else "") + (".res" if g.res else "") + (".f32out" if g.out_dtype == abi.F32 else "") + (".ws" if g.workspace else "")
    if op.kind == abi.OP_NORM:
        a = op.u.norm
        return "norm" + (".mod" if a.mod_scale else "") + (".q8" if a.q else "") + ("" if a.y else ".no_y")
    if op.kind == abi.OP_ATTN:
        a = op.u.attn
        return "attn" + (".q8" if a.q8 else "") + (".qk_f8" if a.q_f8 else "") + (".pv_f8" if a.v_f8t else "") + (".ws" if a.workspace else "")
    if op.kind == abi.OP_QUANT:
        a = op.u.quant
        return "quant" + (".swiglu" if a.op == abi.QUANT_SWIGLU else "") + (".y" if a.y else "")
    if op.kind == abi.OP_EW:
        return "ew." + _EW_NAMES.get(op.u.ew.kind, str(op.u.ew.kind)) + (".y8" if op.u.ew.y8 else "")
    return f"kind{op.kind}"


# ---- the static analysis ------------------------------------------------------------------------------------------------------------------
def check_no_hazards(plans):
    """-> {plan name: (ops, side runs, concurrent pairs)}; fails on the first overlap, naming both ops"""
    out = {}
    for pname, plan in plans:
        n_side = sum(1 for op in plan.ops if op.lane & abi.LANE_SIDE)
        pairs, found = pf.hazards(plan.ops, plan.labels)
        out[pname] = (len(plan.ops), pf.side_runs(plan.ops), pairs)
        print(f"lane hazards: {pname}: {len(plan.ops)} ops, {n_side} on the side lane in {pf.side_runs(plan.ops)} runs, {pairs} concurrent pairs examined, "
              f"{len(found)} overlaps")
        assert not found, f"{pname}: " + "; ".join(str(h) for h in found[:4])
        assert n_side or pname == "skip", f"{pname}: the plan has no side op"     # (the skip plan of the first-block cache has no double block)
        assert pairs > 0 or not n_side, f"{pname}: side ops but no concurrent pair examined"
    return out


# ---- plans at production width, built and analysed, never run -------------------------------------------------------------------------------
PROD_GEOMETRY = (512, 24, 32)             # t_txt, h2, w2; one reference image of the same size: T = 512 + 2 * 768 = 2048


@contextlib.contextmanager
def shape_only_weights():
    """A plan that is only analysed needs its weights' addresses and shapes, not their values: inside this context a DiT's fp8 weights are
    allocated (bytes and scale planes as `dit_graph.quantize_weight` lays them out) without running the quantiser."""
    def alloc(lib, device, dtype, w16, bias=None):
        n, k = w16.shape
        lds = (n + 63) // 64 * 64
        return dit_graph.Weight(q=torch.zeros((n, k), dtype=torch.uint8, device=device), scale=torch.zeros((k // 128, lds), dtype=torch.int32, device=device),
                                lds=lds, bias=bias)
    saved = (fx.quantize_weight, f2.quantize_weight)
    fx.quantize_weight = f2.quantize_weight = alloc
    try:
        yield
    finally:
        fx.quantize_weight, f2.quantize_weight = saved


def zeros_provider(shapes):
    """parameters of the right shapes whose pages are never touched (bf16 matrices, fp32 vectors, as `flux_checks.named_provider` types them)"""
    return lambda name: torch.zeros(shapes[name], dtype=torch.bfloat16 if len(shapes[name]) >= 2 else torch.float32)


def production_cfg(kind):
    cfg = dict(fx.KONTEXT_DIT_CFG if kind == "kontext" else f2.KLEIN_4B_DIT_CFG)
    cfg.update(layers=2, single_layers=1)
    return cfg


def build_production(lib, device, kind, provider=None, lanes=True, **dit_kw):
    """the three-block (2 double + 1 single) DiT at full width and its step plan at PROD_GEOMETRY; provider None = shape-only weights"""
    cfg = production_cfg(kind)
    mod = fx if kind == "kontext" else f2
    shapes = mod.dit_param_shapes(cfg)
    ctx = shape_only_weights() if provider is None else contextlib.nullcontext()
    with ctx:
        cls = fx.FluxDiTHip if kind == "kontext" else f2.Flux2DiTHip
        dit = cls(provider if provider is not None else zeros_provider(shapes), cfg, device, lib=lib, text_stream_on_side_lane=lanes, **dit_kw)
    t_txt, h2, w2 = PROD_GEOMETRY
    plan = dit.plan_for(t_txt, h2, w2, 1) if kind == "kontext" else dit.plan_for(t_txt, h2, w2, h2, w2)
    return dit, plan


def check_production_scratch(plan):
    """what only the production shapes attach: every attention has a workspace of its own, and a side-lane GEMM's K-slice workspace is never a
    main-lane GEMM's"""
    attn_ws = [op.u.attn.workspace for op in plan.ops if op.kind == abi.OP_ATTN]
    assert attn_ws and all(attn_ws) and len(set(attn_ws)) == len(attn_ws), "attention workspaces missing or shared"
    ws = {True: set(), False: set()}
    for op in plan.ops:
        if op.kind == abi.OP_GEMM and op.u.gemm.workspace:
            ws[bool(op.lane & abi.LANE_SIDE)].add(op.u.gemm.workspace)
    assert ws[False], "no main-lane GEMM carries a K-slice workspace at production shapes"
    assert not (ws[True] & ws[False]), "a side-lane GEMM shares its K-slice workspace with a main-lane GEMM"
    return len(attn_ws), len(ws[True]), len(ws[False])


# ---- authored plans: the analysis itself under test -------------------------------------------------------------------------------------------
def authored(lib, device, fault=None):
    """A small two-lane plan in the shape of a DiT block — side rows [0, MS), main rows [MS, MS + MM) of shared buffers, a quantiser pair, a
    GEMM pair with K-slice workspaces, a join, a joint op — built and never run.  fault: None (clean) or one of FAULTS.
    -> (plan, expected (side label, main label) or None)"""
    MS, MM, D = 24, 72, 128
    T = MS + MM
    pb = PlanBuilder(lib, device, abi.BF16)
    x, y, z = pb.buf((T, D), torch.bfloat16), pb.buf((T, D), torch.bfloat16), pb.buf((T, D), torch.bfloat16)
    w = [pb.buf((D, D), torch.bfloat16) for _ in range(5)]
    q8, sc = pb.buf((T, D), torch.uint8), pb.buf((D // 128, 128), torch.int32, zero=True)
    f = abi.GEMM_FORCE_TILE256                                 # both GEMMs of the first pair carry a K-slice workspace
    with pb.side():
        pb.quantize(x, MS, D, q=q8, scale=sc, row_off=0, lds=128, ldq=D, label="side.quant")
        if fault == "scale_row_off":                            # the scale plane cut one row too late: its last word is the main quantiser's first
            pb.ops[-1].u.quant.scale = pb.ops[-1].u.quant.scale + 4
        pb.gemm(x, w[0], MS + 1 if fault == "write_overlap" else MS, D, D, out=y, flags=f, label="side.gemm0")
        pb.gemm(y, w[2], MS + 1 if fault == "read_overlap" else MS, D, D, out=z, label="side.gemm1")      # the fault: a row of y that main.gemm0 writes
    pb.quantize(x, MM, D, x_off=MS * D, q=q8, scale=sc, row_off=MS, lds=128, ldq=D, label="main.quant")
    pb.gemm(x, w[1], MM, D, D, out=y, a_off=MS * D, c_off=MS * D, flags=f, label="main.gemm0")
    if fault == "shared_workspace":
        pb.ops[-1].u.gemm.workspace = pb.ops[1].u.gemm.workspace
    if fault != "late_join":
        pb.join()
    pb.gemm(y, w[3], T, D, D, out=x, label="main.joint")       # reads every row of y: the side lane's gemm0 must have landed
    if fault == "late_join":
        pb.join()
    pb.gemm(z, w[4], T, D, D, out=y, label="main.joint2")
    expect = {None: None, "write_overlap": ("side.gemm0", "main.gemm0"), "read_overlap": ("side.gemm1", "main.gemm0"),
              "shared_workspace": ("side.gemm0", "main.gemm0"), "late_join": ("side.gemm0", "main.joint"),
              "scale_row_off": ("side.quant", "main.quant")}[fault]
    return pb.build(), expect


FAULTS = ("write_overlap", "read_overlap", "shared_workspace", "late_join", "scale_row_off")


def check_authored(lib, device):
    plan, _ = authored(lib, device)
    pairs, found = pf.hazards(plan.ops, plan.labels)
    assert pairs > 0 and not found, [str(h) for h in found]
    for fault in FAULTS:
        plan, (s_label, m_label) = authored(lib, device, fault)
        pairs, found = pf.hazards(plan.ops, plan.labels)
        named = {(h.side_label, h.main_label) for h in found}
        print(f"authored hazard '{fault}': {pairs} pairs, reported {sorted(named)}")
        assert (s_label, m_label) in named, f"{fault}: expected {s_label} / {m_label}, reported {sorted(named)}"
        if fault != "late_join":       # (a late join leaves later pairs unordered as well; the other faults are one pair each)
            assert named == {(s_label, m_label)}, f"{fault}: reported {sorted(named)}"


# ---- hardware: lanes on == lanes off --------------------------------------------------------------------------------------------------------
def run_forms(plans, device, replays=3):
    """the step eagerly, then as hipGraph replays, `replays` times each -> [(vel, x)] per run"""
    outs = []
    cuda = torch.device(device).type == "cuda"
    sync = torch.cuda.synchronize if cuda else (lambda: None)
    # eager launches fork only from a real stream (mtx_plan_run keeps a plan on one lane on the legacy default stream)
    stream = torch.cuda.Stream(device) if cuda else None
    sync()
    for graph in (False, True):
        for _ in range(replays):
            with (torch.cuda.stream(stream) if cuda and not graph else contextlib.nullcontext()):
                for _, p in plans:
                    p.run(graph=graph)
            sync()
            outs.append((plans[0][1].vel.clone(), plans[0][1].x.clone()))
    return outs


def assert_same_runs(on, off, what):
    for k, ((v1, x1), (v0, x0)) in enumerate(zip(on, off)):
        assert torch.isfinite(v0).all() and float(v0.abs().mean()) > 0, f"{what}: the one-lane step is degenerate"
        assert torch.equal(v1, v0), f"{what}: run {k}: velocity differs between lanes on and off ({int((v1 != v0).sum())} values)"
        assert torch.equal(x1, x0), f"{what}: run {k}: token buffer differs between lanes on and off ({int((x1 != x0).sum())} values)"


def check_lanes_bit_equal(lib, device, variant, geometry="small"):
    outs = []
    gc.collect()                                               # plans that earlier tests left to the cycle collector go now, not in the middle of a run
    for lanes in (True, False):
        dit, plans = build_step(lib, device, variant, geometry, lanes=lanes)
        n_side = sum(1 for _, p in plans for op in p.ops if op.lane & abi.LANE_SIDE)
        assert (n_side > 0) == lanes, f"{variant}: lanes={lanes} but {n_side} side ops"
        if lanes:
            check_no_hazards(plans)                            # nothing the analysis flags is run
        outs.append(run_forms([p for p in plans if p[0] != "skip"], device))      # head + body is the computed step; one-plan forms have just "step"
        _retire(dit, plans)
        del dit, plans
    assert_same_runs(outs[0], outs[1], variant)


def _retire(dit, plans):
    """destroys the plans' graphs, side streams and events NOW: a DiT object sits in a reference cycle (its modulation cache holds a bound
    method), so without this its plans are destroyed whenever the cycle collector next runs, in the middle of a later build or run"""
    for _, p in plans:
        p.close()
    dit._plans.clear()
    gc.collect()


def production_inputs(plan, dit, kind, device, seed=4):
    g = torch.Generator().manual_seed(seed)
    plan.lat.copy_(torch.randn(plan.lat.shape, generator=g).to(device, torch.bfloat16))
    plan.ctx_in.copy_(torch.randn(plan.ctx_in.shape, generator=g).to(device, torch.bfloat16))
    if kind == "kontext":
        pooled = torch.randn(dit.cfg["pooled_dim"], generator=g).to(device, torch.bfloat16)
        plan.mod.copy_(dit.modulation(0.7, 2.5, pooled))
    else:
        plan.mod.copy_(dit.modulation(0.7))


def check_production_lanes_bit_equal(lib, device, kind, provider, **dit_kw):
    outs = []
    gc.collect()
    for lanes in (True, False):
        dit, plan = build_production(lib, device, kind, provider=provider, lanes=lanes, **dit_kw)
        assert plan.T >= 2048
        if lanes:
            check_no_hazards([("step", plan)])
            check_production_scratch(plan)
        production_inputs(plan, dit, kind, device)
        outs.append(run_forms([("step", plan)], device))
        _retire(dit, [("step", plan)])
        del dit, plan
    assert_same_runs(outs[0], outs[1], f"{kind} at production width")
