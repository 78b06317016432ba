"""CPU tier of the lane-hazard tests (tests/lane_hazard_checks.py): the footprint model against the kernels on the simulator, the static
hazard analysis of every DiT step plan, the production-width plans (built, analysed, never run) and the analysis under test itself."""
import ctypes as C

import numpy as np
import pytest

from mangatranslator_amd.hip import abi

import lane_hazard_checks as lh
import plan_footprints as pf

CASES = [(v, g) for v in lh.VARIANTS for g in lh.GEOMETRIES]
_built = {}


def _step(lib, variant, geometry):
    if (variant, geometry) not in _built:
        _built[(variant, geometry)] = lh.build_step(lib, "cpu", variant, geometry)
    return _built[(variant, geometry)]


# ---- the tools ------------------------------------------------------------------------------------------------------------------------------
def test_overlap_is_exact():
    """`rects_overlap` against a byte set, on rects that interleave by rows and columns inside one allocation (where bounding intervals always
    intersect), touch without sharing a byte, or differ in stride"""
    R = pf.Rect
    assert pf.rects_overlap(R(1000, 16, 64, 256), R(1064, 16, 64, 256)) is None              # column slices of the same rows
    assert pf.rects_overlap(R(1000, 16, 256, 256), R(1000 + 16 * 256, 40, 256, 256)) is None  # text rows, then image rows
    assert pf.rects_overlap(R(1000, 17, 256, 256), R(1000 + 16 * 256, 40, 256, 256)) == (1000 + 16 * 256, 256)
    assert pf.rects_overlap(R(1000, 4, 16 * 4, 64 * 4), R(1000 + 15 * 4, 4, 8, 64 * 4)) == (1060, 4)   # scale words: rows [0, 16) against [15, 17)
    rng = np.random.default_rng(0)
    hits = 0
    for _ in range(400):
        rs = []
        for _ in range(2):
            stride = int(rng.integers(8, 40))
            rs.append(R(int(rng.integers(0, 120)), int(rng.integers(1, 7)), int(rng.integers(1, stride + 1)), stride))
        sets = [{r.base + i * r.stride + b for i in range(r.rows) for b in range(r.row_bytes)} for r in rs]
        got, common = pf.rects_overlap(*rs), sets[0] & sets[1]
        assert (got is not None) == bool(common), (rs, got)
        if got:
            hits += 1
            assert set(range(got[0], got[0] + got[1])) <= common
    assert 50 < hits < 350


def _ops(lanes):
    ops = []
    for l in lanes:
        op = abi.Op()
        op.kind, op.lane = abi.OP_GEMM, {"m": 0, "s": abi.LANE_SIDE, "j": abi.LANE_JOIN}[l]
        ops.append(op)
    return ops


def test_ordering_rule():
    """the unordered pairs of small lane sequences, written out by hand from csrc/api.hip's fork / join edges"""
    assert pf.concurrent_pairs(_ops("mmm")) == []
    assert pf.concurrent_pairs(_ops("msmjm")) == [(1, 2)]                      # forked behind op 0, joined at op 3
    assert pf.concurrent_pairs(_ops("smsm")) == [(0, 1), (0, 3), (2, 3)]       # op 2 forks again behind op 1; nothing joins before the end
    assert pf.concurrent_pairs(_ops("ssmmjsm")) == [(0, 2), (0, 3), (1, 2), (1, 3), (5, 6)]
    assert pf.concurrent_pairs(_ops("sjm")) == [] and pf.concurrent_pairs(_ops("smmj")) == [(0, 1), (0, 2)]
    assert pf.side_runs(_ops("ssmmjsm")) == 2


def test_unknown_ops_are_refused(emu_lib):
    """no rule, no footprint: another op kind, another element-wise kind, an option outside the rules"""
    op = abi.Op()
    op.kind = abi.OP_CONV2D
    with pytest.raises(pf.UnknownOp):
        pf.footprint(op)
    plan, _ = lh.authored(emu_lib, "cpu")
    gemm = next(o for o in plan.ops if o.kind == abi.OP_GEMM)
    assert all(pf.footprint(gemm))
    for field, value in (("batch", 2), ("w_lo", 4096), ("dtype", abi.F32), ("flags", 1 << 20)):
        o = abi.Op()
        C.memmove(C.byref(o), C.byref(gemm), C.sizeof(o))
        setattr(o.u.gemm, field, value)
        with pytest.raises(pf.UnknownOp):
            pf.footprint(o)
    ew = abi.Op()
    ew.kind = abi.OP_EW
    ew.u.ew.kind, ew.u.ew.a, ew.u.ew.y, ew.u.ew.n, ew.u.ew.h, ew.u.ew.w, ew.u.ew.c = abi.EW_MAXPOOL, 4096, 8192, 1, 1, 4, 8
    with pytest.raises(pf.UnknownOp):
        pf.footprint(ew)


def test_authored_hazards_are_reported(emu_lib):
    """overlapping writes, a side read of rows the main lane writes, one workspace on both lanes, a join one op late, a scale plane cut on
    the wrong row: each reported with the right pair named; the clean plan passes"""
    lh.check_authored(emu_lib, "cpu")


# ---- the step plans -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,geometry", CASES)
def test_no_lane_hazards(emu_lib, variant, geometry):
    """every side / main pair the plan leaves unordered touches disjoint bytes; a plan with side ops examines at least one pair"""
    _, plans = _step(emu_lib, variant, geometry)
    lh.check_no_hazards(plans)


@pytest.mark.parametrize("variant,geometry", CASES)
def test_footprints_match_kernels(emu_lib, variant, geometry):
    """every op of the step, alone, on the in-order state and on the state scrambled outside its declared reads: same declared writes,
    nothing else written"""
    dit, plans = _step(emu_lib, variant, geometry)
    lh.check_no_hazards(plans)
    stats = {}
    lh.check_footprints(plans, lh.held_tensors(dit, plans), stats)
    print(f"footprints {variant} / {geometry}: " + ", ".join(f"{k} x{v}" for k, v in sorted(stats.items())))
    assert sum(stats.values()) == sum(len(p.ops) for _, p in plans)


def test_footprints_of_the_long_sequence_forms(emu_lib):
    stats = {}
    lh.check_footprints_long_forms(emu_lib, "cpu", stats)
    print("footprints, long forms: " + ", ".join(f"{k} x{v}" for k, v in sorted(stats.items())))
    assert {"attn.ws", "attn.q8.qk_f8.pv_f8.ws", "ew.v_f8t.y8", "ew.qk_norm_rope.y8", "gemm.gate.res.ws", "gemm.f8.ws"} <= set(stats)


@pytest.mark.parametrize("drop", ["read", "write"])
def test_the_ab_check_notices_a_footprint_that_declares_too_little(emu_lib, monkeypatch, drop):
    """the A/B check under test: with the gate rows left out of a GEMM's reads, or the scale plane left out of a quantiser's writes, it fails"""
    import torch
    from mangatranslator_amd.hip.plan import PlanBuilder
    g = torch.Generator().manual_seed(0)
    pb = PlanBuilder(emu_lib, "cpu", abi.BF16)
    x, w, gate = pb.buf((40, 128), torch.bfloat16), pb.buf((128, 128), torch.bfloat16), pb.buf((2, 128), torch.bfloat16)
    for t in (x, w, gate):
        t.copy_(torch.randn(t.shape, generator=g).to(torch.bfloat16))
    y = pb.gemm(x, w, 40, 128, 128, gate=gate, gate_rows_per=20, res=x, label="gemm")
    pb.quantize(y, 40, 128, label="quant")
    plan = pb.build()
    lh.check_footprints([("clean", plan)], plan._keep)
    real = pf.footprint

    def short(op):
        r, w_ = real(op)
        if drop == "read":
            return [q for q in r if q.name != "gate"], w_
        return r, [q for q in w_ if q.name != "scale"]
    monkeypatch.setattr(pf, "footprint", short)
    with pytest.raises(AssertionError, match="outside its declared reads" if drop == "read" else "outside its declared writes"):
        lh.check_footprints([("short", plan)], plan._keep)


@pytest.mark.parametrize("kind,fp8", [("kontext", False), ("kontext", True), ("klein", False), ("klein", True)])
def test_production_width_plans_have_no_hazards(emu_lib, kind, fp8):
    """d = 3072, 24 heads, 2 double + 1 single block, t_txt 512 + 2 x (24 x 32) tokens: the shapes at which the builder attaches K-slice and
    attention workspaces and the fp8 attention forms.  Built and analysed, never run (the weights are shapes only)."""
    dit, plan = lh.build_production(emu_lib, "cpu", kind, fp8=fp8)
    assert plan.T == 2048 and dit.cfg["d"] == 3072
    stats = lh.check_no_hazards([(f"{kind}{'.fp8' if fp8 else ''} at production width", plan)])
    n_attn, ws_side, ws_main = lh.check_production_scratch(plan)
    assert ws_side >= 1, "no side-lane GEMM carries a K-slice workspace at production shapes"
    if fp8:
        attn = [op.u.attn for op in plan.ops if op.kind == abi.OP_ATTN]
        assert all(a.q8 for a in attn), "the fp8 plan's attention does not write the next linear's operand"
    print(f"{kind} fp8={fp8}: {n_attn} attention workspaces, {ws_side} side / {ws_main} main K-slice workspaces, {stats}")


def test_klein_lane_switch_keeps_the_default_op_stream(emu_lib):
    """`text_stream_on_side_lane`: the default records the side lane as before; off records the same ops, in the same order, on one lane"""
    _, (( _, on),) = lh.build_step(emu_lib, "cpu", "klein", "small")
    _, (( _, off),) = lh.build_step(emu_lib, "cpu", "klein", "small", lanes=False)
    assert on.labels == off.labels and [o.kind for o in on.ops] == [o.kind for o in off.ops]
    side = [lb for lb, o in zip(on.labels, on.ops) if o.lane & abi.LANE_SIDE]
    assert side == [f"dbl{i}.{n}" for i in range(2) for n in ("qkv_ctx", "to_add_out", "ff_in_ctx", "ff_out_ctx")]
    assert not any(o.lane & abi.LANE_SIDE for o in off.ops)
