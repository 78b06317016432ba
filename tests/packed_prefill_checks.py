"""Checks of the packed fill of PaddleOCR-VL's decode slots (csrc/attention.hip: MTX_OP_SEG_ATTN; csrc/causal.hip: MTX_OP_CAUSAL_PREFILL_SLOTS;
`PaddleOcrVlHip(..., packed_prefill=True)`), written once and run on the simulator (tests/test_paddle_packed_sim.py) and on the product library
(tests/test_paddle_packed_gpu.py).

The reference of every kernel check is the single-sequence op on a copy of one segment's operands (mtx_attention through its short kernel,
mtx_causal_attention with rows = L at pos = 0), and the comparison is bit for bit: a segment's result may not depend on what shares its launch.
The one exception is a one-row prompt, where the single op takes its streaming kernel: that row is held to `causal_ref` under
`check_causal_random`'s bound.  The model checks hold a packed fill to itself (independence of companions, slot and rung: bit for bit) and to the
oracle (the bounds the one-crop path already has); against the one-crop path it is NOT bit-identical, the GEMMs run at another M."""
import ctypes as C

import pytest
import torch

import paddle_batch_checks as bc
import paddle_ocr_vl_checks as pc
from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.plan import PlanBuilder
from mangatranslator_amd.utils.exceptions import ModelError
from op_checks import TD, _dev, _sync
from paddle_ocr_vl_checks import D, GUARD, MANT, NAN_BITS, CausalRig, _bits, causal_ref

MTX_ERR_INVALID, MTX_ERR_UNSUPPORTED = -1, -3          # include/mtx_hip.h
SEGS = abi.SEGS_MAX
AT_KV, AT_QB = 64, abi.ATTN_QB                          # csrc/attention.hip
TQ, TK = abi.CAUSAL_TQ, abi.CAUSAL_TK
SEG_CAP = 1024
SEG_HEADS = 2
SEG_WIDTHS = [64, 72]
SEG_LENGTHS = [1, AT_KV - 1, AT_KV, AT_KV + 1, AT_QB - 1, AT_QB, AT_QB + 1, 200]      # both sides of a key tile and of a query block, one row
SEG_LENGTHS_EMPTY = [5, 0, 0, 130, 0, 64, 0, 1]                                      # empty segments at the front, middle and end of a run
MAX_LEN = bc.MAX_LEN                                                                 # 2 * 64 + 8
PREFILL_HEADS = [(4, 2), (16, 2)]
PREFILL_LENGTHS = [2, TK - 1, TK, TK + 1, TQ - 1, TQ, TQ + 1, 2 * TQ + 3]            # both sides of a key tile and of a query block
PREFILL_LENGTHS_EMPTY = [40, 0, 70, 0, 0, 0, 0, 2]
PREFILL_LENGTHS_ONE = [33, 1, 65, 0, 1, 2, 0, 70]                                    # L = 1 among longer segments
BYTE_PATTERN = 0x5A5A


def offsets(lengths, start=0):
    t = torch.zeros(SEGS + 1, dtype=torch.int32)
    t[0] = start
    t[1:] = start + torch.tensor(lengths, dtype=torch.int64).cumsum(0).to(torch.int32)
    return t


def damaged_tables(cap_rows, lengths):
    """a decreasing pair, a start below 0, an end above the capacity"""
    dec = offsets(lengths)
    dec[4] = dec[3] - 1
    neg = offsets(lengths)
    neg[0] = -1
    over = offsets(lengths)
    over[SEGS] = cap_rows + 1
    return {"a decreasing pair": dec, "seg[0] = -1": neg, "seg[8] = cap_rows + 1": over}


def _pattern(td, *shape, bits=NAN_BITS):
    return torch.full(shape, bits, dtype=torch.int16).view(td)


# ---- segment attention -------------------------------------------------------------------------------------------------------------------------
class SegRig:
    """one recorded MTX_OP_SEG_ATTN on packed [cap_rows, heads * d] buffers, and the single op (short kernel) per segment length on demand"""

    def __init__(self, lib, dtype, heads, d, cap_rows=SEG_CAP):
        self.lib, self.dev, self.td, self.dtype = lib, _dev(lib), TD[dtype], dtype
        self.heads, self.d, self.cap, self.w = heads, d, cap_rows, heads * d
        self.scale = d ** -0.5
        pb = PlanBuilder(lib, self.dev, dtype)
        self.q, self.k, self.v, self.o = (pb.buf((cap_rows, self.w), self.td, zero=True) for _ in range(4))
        self.seg = pb.buf((SEGS + 1,), torch.int32, zero=True)
        st = (self.w, d)
        pb.segment_attention(self.q, self.k, self.v, self.o, self.seg, heads, d, cap_rows, st, st, st, st, self.scale)
        self.pb, self.plan = pb, pb.build()

    def run(self, q, k, v, seg, o):
        self.q.copy_(q); self.k.copy_(k); self.v.copy_(v); self.seg.copy_(seg); self.o.copy_(o)
        self.plan.run()
        _sync(self.lib)
        return self.o.cpu()

    def single(self, q, k, v):
        """mtx_attention (batch 1, sq = sk = len, the packed buffers' strides) on a copy of one segment"""
        n = q.shape[0]
        pb = PlanBuilder(self.lib, self.dev, self.dtype)
        qt, kt, vt = pb.const(q.clone()), pb.const(k.clone()), pb.const(v.clone())
        o = pb.const(_pattern(self.td, n, self.w))
        st = (n * self.w, self.w, self.d)
        pb.attention(qt, kt, vt, o, 1, self.heads, n, n, self.d, st, st, st, st, self.scale)
        pb.build().run()
        _sync(self.lib)
        route = self.lib.attention_last_route()
        assert route[0] == (64 if self.d <= 64 else 96), f"the reference launch took kernel {route}, not the short kernel"
        return o.cpu()


def _seg_operands(rig, seed):
    g = torch.Generator().manual_seed(seed * 1000 + rig.d)
    return tuple((torch.randn(rig.cap, rig.w, generator=g) * 1.5).to(rig.td) for _ in range(3))


def _check_segments(rig, q, k, v, lengths, got, what):
    seg = offsets(lengths).tolist()
    for s, n in enumerate(lengths):
        if n == 0:
            continue
        a, b = seg[s], seg[s + 1]
        want = rig.single(q[a:b], k[a:b], v[a:b])
        assert bool(torch.isfinite(want.float()).all()), f"{what}: the reference launch left rows of segment {s} unwritten"
        bad = int((_bits(got[a:b]) != _bits(want)).sum())
        assert bad == 0, f"{what}: segment {s} (rows {a}..{b}): {bad} of {n * rig.w} elements differ from mtx_attention on the segment alone"
    tail = _bits(got[seg[SEGS]:])
    assert bool((tail == NAN_BITS).all()), f"{what}: rows at or beyond seg[8] were written"


def check_segment_attention(lib, dtype, d, lengths, seed=0):
    """tests 1 and 2: random operands, o pre-filled with the NaN pattern; every segment equals the single op bit for bit, the tail keeps the pattern"""
    rig = SegRig(lib, dtype, SEG_HEADS, d)
    q, k, v = _seg_operands(rig, seed)
    got = rig.run(q, k, v, offsets(lengths), _pattern(rig.td, rig.cap, rig.w))
    _check_segments(rig, q, k, v, lengths, got, f"segment attention d={d} lengths={lengths}")


def check_segment_isolation(lib, dtype, d, victim=3, seed=0):
    """test 3: segment `victim`'s q, k, v rows and the unused tail set to NaN: the other seven segments are bit-identical to the clean run"""
    lengths = SEG_LENGTHS
    rig = SegRig(lib, dtype, SEG_HEADS, d)
    q, k, v = _seg_operands(rig, seed)
    seg = offsets(lengths)
    clean = rig.run(q, k, v, seg, _pattern(rig.td, rig.cap, rig.w)).clone()
    a, b, end = int(seg[victim]), int(seg[victim + 1]), int(seg[SEGS])
    dirty = []
    for t in (q, k, v):
        t = t.clone()
        t.view(torch.int16)[a:b] = NAN_BITS
        t.view(torch.int16)[end:] = NAN_BITS
        dirty.append(t)
    got = rig.run(*dirty, seg, _pattern(rig.td, rig.cap, rig.w))
    for s in range(SEGS):
        if s == victim:
            continue
        x, y = int(seg[s]), int(seg[s + 1])
        assert torch.equal(_bits(got[x:y]), _bits(clean[x:y])), f"segment attention d={d}: segment {s} changed when segment {victim} and the tail became NaN"
        assert bool(torch.isfinite(got[x:y].float()).all())
    assert bool((_bits(got[end:]) == NAN_BITS).all())


def check_segment_damaged_tables(lib, dtype, d=64, seed=0):
    """test 4: return code 0 and o keeps every byte of its pattern"""
    rig = SegRig(lib, dtype, SEG_HEADS, d)
    q, k, v = _seg_operands(rig, seed)
    for name, table in damaged_tables(rig.cap, SEG_LENGTHS).items():
        got = rig.run(q, k, v, table, _pattern(rig.td, rig.cap, rig.w))          # (a refused launch would raise ModelError out of plan.run)
        assert bool((_bits(got) == NAN_BITS).all()), f"segment attention, {name}: o was written"


def check_segment_refusals(lib):
    """test 5: argument checks only — the launch function returns before any launch"""
    rig = SegRig(lib, abi.BF16, SEG_HEADS, 64, cap_rows=256)
    base = rig.pb.ops[-1].u.segattn

    def rc(**edit):
        a = abi.SegAttnArgs.from_buffer_copy(base)
        for key, val in edit.items():
            setattr(a, key, val)
        return lib.mtx_segment_attention(C.byref(a), C.c_void_p(0))
    assert rc(d=128) == MTX_ERR_UNSUPPORTED and rc(d=20) == MTX_ERR_UNSUPPORTED
    assert rc(q=base.q + 2) == MTX_ERR_INVALID and rc(o=base.o + 2) == MTX_ERR_INVALID
    for field in ("q", "k", "v", "o", "seg"):
        assert rc(**{field: None}) == MTX_ERR_INVALID, field
    assert rc(cap_rows=0) == MTX_ERR_INVALID and rc(q_ss=rig.w + 4) == MTX_ERR_INVALID and rc(dtype=abi.F32) == MTX_ERR_INVALID
    bad = PlanBuilder(lib, _dev(lib), abi.BF16)
    st = (rig.w, 128)
    bad.segment_attention(rig.q, rig.k, rig.v, rig.o, rig.seg, 1, 128, 256, st, st, st, st, 1.0)
    with pytest.raises(ModelError):
        bad.build().run()


# ---- packed causal prefill ---------------------------------------------------------------------------------------------------------------------
class PrefillRig:
    """one recorded MTX_OP_CAUSAL_PREFILL_SLOTS: eight slot caches with a guard band each, packed qkv and o with optional row padding"""

    def __init__(self, lib, dtype, heads, kv_heads, cap_rows, max_len=MAX_LEN, pad_qkv=0, pad_o=0, pad_cache=0):
        self.lib, self.dev, self.td, self.dtype = lib, _dev(lib), TD[dtype], dtype
        self.heads, self.kv, self.cap, self.max_len = heads, kv_heads, cap_rows, max_len
        self.w, self.wo = (heads + 2 * kv_heads) * D, heads * D
        self.ld_qkv, self.ld_o = self.w + pad_qkv, self.wo + pad_o
        self.crows = max_len + GUARD + pad_cache                    # rows of one slot's cache buffer: the stride is larger than the cache
        self.scale = D ** -0.5
        pb = PlanBuilder(lib, self.dev, dtype)
        self.qkv = pb.buf((cap_rows, self.ld_qkv), self.td, zero=True)
        self.kc = pb.buf((SEGS, self.crows, kv_heads * D), self.td, zero=True)
        self.vc = pb.buf((SEGS, self.crows, kv_heads * D), self.td, zero=True)
        self.seg = pb.buf((SEGS + 1,), torch.int32, zero=True)
        self.o = pb.buf((cap_rows, self.ld_o), self.td, zero=True)
        pb.causal_prefill_slots(self.qkv, self.kc, self.vc, self.seg, self.o, cap_rows, heads, kv_heads, D, max_len, self.scale,
                                cache_stride=self.crows * kv_heads * D, ld_qkv=self.ld_qkv, ld_o=self.ld_o)
        self.pb, self.plan = pb, pb.build()

    def run(self, qkv, kc, vc, seg, o):
        self.qkv.copy_(qkv); self.kc.copy_(kc); self.vc.copy_(vc); self.seg.copy_(seg); self.o.copy_(o)
        self.plan.run()
        _sync(self.lib)
        return self.o.cpu(), self.kc.cpu(), self.vc.cpu()

    def operands(self, seed, cache_bits=NAN_BITS):
        """random packed rows (NaN in the row padding), caches and o filled with a pattern"""
        g = torch.Generator().manual_seed(seed * 1000 + self.heads)
        qkv = _pattern(self.td, self.cap, self.ld_qkv)
        qkv[:, :self.w] = (torch.randn(self.cap, self.w, generator=g) * 1.5).to(self.td)
        kc = _pattern(self.td, SEGS, self.crows, self.kv * D, bits=cache_bits)
        vc = _pattern(self.td, SEGS, self.crows, self.kv * D, bits=cache_bits)
        return qkv, kc, vc, _pattern(self.td, self.cap, self.ld_o)

    def single(self, qkv_rows, kc, vc):
        """mtx_causal_attention(rows = L, pos = 0) on copies of one slot's operands -> (o rows, k cache, v cache)"""
        n = qkv_rows.shape[0]
        one = CausalRig(self.lib, self.dtype, n, self.heads, self.kv, self.max_len)
        one.o.copy_(_pattern(self.td, n, self.wo))
        o = one.run(qkv_rows[:, :self.w], kc[:self.max_len + GUARD], vc[:self.max_len + GUARD], 0)
        return o, one.kc.cpu(), one.vc.cpu()


def _check_slots(rig, qkv, kc, vc, o0, lengths, got, what, tile_only=()):
    """per slot with L >= 2: o rows and the whole cache equal the single op's; an empty slot's cache and every o row outside a segment keep every byte.
    Slots in `tile_only` (L == 1) are held to causal_ref and to the cache discipline instead."""
    go, gk, gv = got
    seg = offsets(lengths).tolist()
    n_guard = rig.max_len + GUARD
    written = torch.zeros(rig.cap, dtype=torch.bool)
    for s, n in enumerate(lengths):
        a, b = seg[s], seg[s + 1]
        if n == 0:
            assert torch.equal(_bits(gk[s]), _bits(kc[s])) and torch.equal(_bits(gv[s]), _bits(vc[s])), f"{what}: slot {s} is empty but its cache was written"
            continue
        written[a:b] = True
        assert torch.equal(_bits(gk[s, n_guard:]), _bits(kc[s, n_guard:])) and torch.equal(_bits(gv[s, n_guard:]), _bits(vc[s, n_guard:])), f"{what}: slot {s}: rows behind the guard band were written"
        assert torch.equal(_bits(go[a:b, rig.wo:]), _bits(o0[a:b, rig.wo:])), f"{what}: slot {s}: the padding of o was written"
        if s in tile_only:
            assert n == 1
            ref = causal_ref(qkv[a:b, :rig.w], kc[s], vc[s], 0, rig.heads, rig.kv, rig.scale)
            vmax = float(qkv[a:b, (rig.heads + rig.kv) * D:rig.w].double().abs().max())
            bound = ref.abs() * 2.0 ** -(MANT[rig.dtype] + 1) * (1 + 2.0 ** -6) + 300 * 2.0 ** -23 * vmax        # check_causal_random's
            ratio = float(((go[a:b, :rig.wo].double() - ref).abs() / bound).max())
            print(f"{what}: slot {s} (one row): error {ratio:.3f} x the bound")
            assert ratio <= 1.0, f"{what}: slot {s} (one row): error {ratio:.2f} x the bound (one rounding + fp32 softmax)"
            want_k, want_v = kc[s].clone(), vc[s].clone()
            want_k[0] = qkv[a, rig.heads * D:(rig.heads + rig.kv) * D]
            want_v[0] = qkv[a, (rig.heads + rig.kv) * D:rig.w]
            assert torch.equal(_bits(gk[s]), _bits(want_k)) and torch.equal(_bits(gv[s]), _bits(want_v)), f"{what}: slot {s} (one row): the cache holds other values"
            continue
        o1, k1, v1 = rig.single(qkv[a:b], kc[s], vc[s])
        assert bool(torch.isfinite(o1.float()).all()), f"{what}: the reference launch left rows of slot {s} unwritten"
        bad = int((_bits(go[a:b, :rig.wo]) != _bits(o1)).sum())
        assert bad == 0, f"{what}: slot {s} (L = {n}): {bad} of {n * rig.wo} elements of o differ from mtx_causal_attention(rows = L, pos = 0)"
        assert torch.equal(_bits(gk[s, :n_guard]), _bits(k1)) and torch.equal(_bits(gv[s, :n_guard]), _bits(v1)), f"{what}: slot {s} (L = {n}): the cache differs from the single op's"
    assert torch.equal(_bits(go[~written]), _bits(o0[~written])), f"{what}: o rows outside every segment were written"


def check_prefill_slots(lib, dtype, heads, kv, lengths, seed=0, tile_only=(), cache_bits=NAN_BITS, **pads):
    """tests 6, 7, 8 and 10: per slot equal to the single op, bit for bit; a second launch gives the same bytes"""
    cap = sum(lengths) + 37                                                     # an unused tail that is no multiple of a tile
    rig = PrefillRig(lib, dtype, heads, kv, cap, **pads)
    qkv, kc, vc, o0 = rig.operands(seed, cache_bits)
    what = f"packed prefill heads={heads}/{kv} lengths={lengths}"
    first = tuple(t.clone() for t in rig.run(qkv, kc, vc, offsets(lengths), o0))
    _check_slots(rig, qkv, kc, vc, o0, lengths, first, what, tile_only)
    rig.o.copy_(o0)
    rig.plan.run()
    _sync(lib)
    again = (rig.o.cpu(), rig.kc.cpu(), rig.vc.cpu())
    for x, y in zip(first, again):
        assert torch.equal(_bits(x), _bits(y)), f"{what}: the second launch gave other bytes"


def check_prefill_nothing_written(lib, dtype, heads=4, kv=2, seed=0):
    """test 9: one segment with L = max_len + 1, and the damaged tables: return code 0 and nothing is written anywhere"""
    lengths = [3, MAX_LEN + 1, 2, 0, 40, 0, 1, 5]
    cap = sum(lengths) + 11
    rig = PrefillRig(lib, dtype, heads, kv, cap)
    qkv, kc, vc, o0 = rig.operands(seed, BYTE_PATTERN)
    tables = {"a segment of max_len + 1 rows": offsets(lengths)}
    tables.update(damaged_tables(cap, [3, 20, 2, 0, 40, 0, 1, 5]))
    for name, table in tables.items():
        go, gk, gv = rig.run(qkv, kc, vc, table, o0)
        assert torch.equal(_bits(go), _bits(o0)), f"packed prefill, {name}: o was written"
        assert torch.equal(_bits(gk), _bits(kc)) and torch.equal(_bits(gv), _bits(vc)), f"packed prefill, {name}: a cache was written"


def check_prefill_refusals(lib):
    """test 11: argument checks only — the launch function returns before any launch"""
    rig = PrefillRig(lib, abi.BF16, 4, 2, 64, max_len=8)
    base = rig.pb.ops[-1].u.cprefs

    def rc(**edit):
        a = abi.CausalPrefillSlotsArgs.from_buffer_copy(base)
        for key, val in edit.items():
            setattr(a, key, val)
        return lib.mtx_causal_prefill_slots(C.byref(a), C.c_void_p(0))
    assert rc(cap_rows=0) == MTX_ERR_INVALID and rc(max_len=0) == MTX_ERR_INVALID
    for field in ("qkv", "k_cache", "v_cache", "seg", "o"):
        assert rc(**{field: None}) == MTX_ERR_INVALID, field
    assert rc(d=64) == MTX_ERR_UNSUPPORTED and rc(heads=3) == MTX_ERR_UNSUPPORTED
    assert rc(dtype=abi.F32) == MTX_ERR_INVALID and rc(cache_stride=8 * 2 * D - 8) == MTX_ERR_INVALID
    assert rc(ld_qkv=rig.w - 8) == MTX_ERR_INVALID and rc(ld_o=rig.wo + 4) == MTX_ERR_INVALID and rc(qkv=base.qkv + 8) == MTX_ERR_INVALID
    bad = PlanBuilder(lib, _dev(lib), abi.BF16)
    bad.causal_prefill_slots(rig.qkv, rig.kc, rig.vc, rig.seg, rig.o, 64, 3, 2, D, 8, 1.0)
    with pytest.raises(ModelError):
        bad.build().run()


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
def _item(seed, grid=(4, 6), **kw):
    ids, pix, thw = pc.make_inputs(seed, grid=grid, **kw)
    return dict(input_ids=ids, pixel_values=pix, image_grid_thw=thw)


def _empty(m):
    """every slot free again (the caches keep their bytes: a fill owns rows [0, T) of its slot only)"""
    m.slot_state.zero_()
    m.slot_state[abi.SLOT_DONE] = 1


def _snapshot(m, slot, T):
    """(first token, state lane, rows [0, T) of the slot's caches of every layer)"""
    _sync(m.lib)
    return (int(m.slot_out[slot, 0]), m.slot_state[:, slot].cpu().clone(),
            [(kc[slot, :T].cpu().clone(), vc[slot, :T].cpu().clone()) for kc, vc in m.slot_caches])


def _assert_same_fill(a, b, what):
    assert a[0] == b[0], f"{what}: first token {a[0]} != {b[0]}"
    assert torch.equal(a[1], b[1]), f"{what}: state lane {a[1].tolist()} != {b[1].tolist()}"
    for i, ((k1, v1), (k2, v2)) in enumerate(zip(a[2], b[2])):
        assert bool(torch.isfinite(k1.float()).all()) and bool(torch.isfinite(v1.float()).all())
        assert torch.equal(_bits(k1), _bits(k2)) and torch.equal(_bits(v1), _bits(v2)), f"{what}: cache rows of layer {i} differ"


def check_fill_is_independent(lib, m, item, companions, what):
    """tests 12 and 18: `item` filled alone in slot 0, then as the last of the pack behind `companions` in the last slot: first token, state lane
    and cache rows [0, T) of every layer are bit-identical.  -> the rungs of the two fills"""
    T = int(item["input_ids"].shape[1])
    assert m.fill_slots([(0, item)]) == [T]
    alone, rung_alone = _snapshot(m, 0, T), m.last_rungs
    assert alone[1].tolist()[:2] == [T, 1], f"{what}: the filled lane must stand at pos = T, n_out = 1, not {alone[1].tolist()}"
    _empty(m)
    slot = len(companions)
    m.fill_slots([(s, c) for s, c in enumerate(companions)] + [(slot, item)])
    together, rung_together = _snapshot(m, slot, T), m.last_rungs
    _assert_same_fill(alone, together, what)
    return rung_alone, rung_together


def check_independence_tiny(lib, dtype=abi.F16):
    m = pc.hip_model(lib, dtype, bc.SEED, sigma=pc.GREEDY_SIGMA, slots=3, packed_prefill=True)
    try:
        rungs = check_fill_is_independent(lib, m, _item(0, (4, 6)), [_item(1, (2, 8)), _item(2, (6, 4))], "tiny configuration")
    finally:
        m.close()
    print(f"rungs (patches, rows) alone / among three: {rungs}")
    return rungs


def _published_items():
    return [_item(k, grid) for k, grid in enumerate([(20, 28), (28, 40), (8, 12)])]


def check_independence_published(lib):
    """test 18: the wheel's default widths (vocabulary 8 192), f16: at these widths the linears would change kernel family with M if their route
    were not pinned; the two fills must land on different rungs"""
    items = _published_items()
    T = max(int(it["input_ids"].shape[1]) for it in items)
    m = pc.hip_model(lib, abi.F16, 0, real=True, max_new_tokens=16, max_prompt=T + 8, slots=3, packed_prefill=True)
    try:
        alone, together = check_fill_is_independent(lib, m, items[0], [items[1], items[2]], "published widths")
    finally:
        m.close()
    print(f"rungs (patches, rows) alone / among three: {alone} / {together}")
    assert alone[0] != together[0] and alone[1] != together[1], f"the two fills must take different rungs: {alone} / {together}"


def packed_teacher_forced(lib, dtype, seed, slot=1, sigma=pc.SIGMA):
    """test 13: the prompt's last-row distribution from the packed fill, then STEPS - 1 teacher-forced steps on the batched stepper: (max, rms)
    absolute log-prob error against the oracle over STEPS distributions"""
    toks, ref, _ = pc.oracle_greedy(seed, sigma=sigma)
    m = pc.hip_model(lib, dtype, seed, sigma=sigma, slots=3, packed_prefill=True)
    try:
        T, = m.fill_slots([(slot, _item(seed))])
        _sync(lib)
        assert m.slot_state[:3, slot].tolist() == [T, 1, 0]
        rows = [m.pk_logits[slot].float().cpu().clone()]
        for t in toks[:-1]:
            rows.append(m.slot_step_logits(slot, t))
    finally:
        m.close()
    assert len(rows) == ref.shape[0] and (sigma != pc.SIGMA or len(rows) == pc.STEPS)
    err = torch.log_softmax(torch.stack(rows), -1) - ref
    assert bool(torch.isfinite(err).all())
    return float(err.abs().max()), float(err.pow(2).mean().sqrt())


_GREEDY_RUNS = {}


def greedy_run(lib, seed, packed):
    """the tokens `generate_many` gives for the greedy tests' item of `seed` (f16, GREEDY_SIGMA, three slots) with or without the packed fill;
    computed once per library and shared, never modified"""
    key = (lib.is_simulator, seed, packed)
    if key not in _GREEDY_RUNS:
        item = _item(seed)
        T = item["input_ids"].shape[1]
        m = pc.hip_model(lib, abi.F16, seed, sigma=pc.GREEDY_SIGMA, slots=3, packed_prefill=packed)
        try:
            out, = m.generate_many([item], max_new_tokens=pc.STEPS)
        finally:
            m.close()
        assert out.dtype == torch.int64 and out.shape[0] == 1 and torch.equal(out[0, :T], item["input_ids"][0])
        _GREEDY_RUNS[key] = out[0, T:].tolist()
    return _GREEDY_RUNS[key]


def check_greedy_tokens_packed(lib, seed, delta):
    """test 14: the tokens of `generate_many` with the packed fill equal the oracle's over the seed's decided prefix; -> its length"""
    toks, n = pc.decided_prefix(seed, delta)
    got = greedy_run(lib, seed, True)
    assert got[:n] == toks[:n], f"seed {seed}: device {got[:n]} != oracle {toks[:n]} over the decided prefix of {n}"
    return n


def check_decided_prefix_packed_equals_unpacked(lib, seed, delta):
    """test 15, the items of test 14: with and without the option the tokens are equal over the decided prefix; -> whether they differ beyond it"""
    _, n = pc.decided_prefix(seed, delta)
    a, b = greedy_run(lib, seed, True), greedy_run(lib, seed, False)
    assert a[:n] == b[:n], f"seed {seed}: packed {a[:n]} != unpacked {b[:n]} over the decided prefix of {n}"
    return a != b


def check_packed_against_unpacked(lib, n=7, slots=3):
    """test 15: the same list through `generate_many` with and without the option: same order, same types, the prompts in place; how many
    sequences differ is printed, not asserted (the GEMMs of the two fills run at different M)"""
    items = bc.make_items(n)
    a, log_a = bc.many(lib, items, slots)
    b, log_b = bc.many(lib, items, slots, packed_prefill=True)
    assert len(a) == len(b) == n
    for k, (x, y, it) in enumerate(zip(a, b, items)):
        T = it["input_ids"].shape[1]
        assert isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.dtype == y.dtype == torch.int64 and y.shape[0] == 1, f"item {k}"
        assert torch.equal(y[0, :T], it["input_ids"][0]) and T < y.shape[1] <= T + bc.BUDGET, f"item {k}: {y}"
    assert sorted(i for i, _, _ in log_b) == list(range(n)) and [i for i, _, _ in log_b[:slots]] == list(range(slots))
    assert all(len(entry) == 3 for entry in log_b)
    differ = sum(not torch.equal(x, y) for x, y in zip(a, b))
    print(f"packed against unpacked: {differ} of {n} sequences differ")
    return differ


def check_refused_items_packed(lib):
    """test 16: a prompt longer than max_prompt, an odd grid and a prompt whose placeholders do not match its grid between good ones leave
    ModelErrors at their indices and take no slot; the good ones come back in place"""
    good = bc.make_items(3)
    long_ids, pix, thw = pc.make_inputs(0, extra=tuple(range(30, 30 + 60)))
    assert long_ids.shape[1] > 64
    odd = dict(input_ids=good[0]["input_ids"], pixel_values=torch.randn(3 * 4, 3, 14, 14), image_grid_thw=torch.tensor([[1, 3, 4]]))
    other = _item(1, (2, 8))
    mismatch = dict(input_ids=good[0]["input_ids"], pixel_values=other["pixel_values"], image_grid_thw=other["image_grid_thw"])      # 6 placeholders, a grid of 4
    items = [good[0], dict(input_ids=long_ids, pixel_values=pix, image_grid_thw=thw), good[1], odd, mismatch, good[2]]
    got, log = bc.many(lib, items, 2, packed_prefill=True)
    assert [isinstance(g, ModelError) for g in got] == [False, True, False, True, True, False], got
    for k in (0, 2, 5):
        T = items[k]["input_ids"].shape[1]
        assert got[k].dtype == torch.int64 and torch.equal(got[k][0, :T], items[k]["input_ids"][0]) and got[k].shape[1] > T
    assert [i for i, _, _ in log] == [0, 2, 5], log
    with pytest.raises(ModelError):
        bc.model(lib, 1, packed_prefill=True)
    with pytest.raises(ModelError):
        bc.model(lib, 2, packed_prefill=1)


def check_driver_packed(lib, tmp_path, monkeypatch):
    """test 16: the driver with paddle_ocr_vl_packed_prefill = True and three slots: one `generate_many` call for the page, the marker at the
    unreadable crop's index, texts elsewhere; with slots = 1 (or a non-bool) the loader raises ModelError"""
    from mangatranslator_amd.core.image import ocr_detection as od
    from mangatranslator_amd.core.ml import paddle_ocr_vl as pv
    from mangatranslator_amd.core.ml.model_manager import ModelType, get_model_manager
    mgr = get_model_manager()
    root = pc.stage_directory(tmp_path / "paddleocr-vl-1.6")
    monkeypatch.setitem(mgr.model_paths, ModelType.PADDLE_OCR_VL, root)
    monkeypatch.setitem(mgr.models, ModelType.PADDLE_OCR_VL, None)
    if lib.is_simulator:
        monkeypatch.setattr(pv, "get_library", lambda: lib)
        monkeypatch.setattr(mgr, "device", torch.device("cpu"))
    a, b, c = bc.images()
    crops = [a, None, b, c]
    real_load = pv.load_pair
    monkeypatch.setattr(pv, "load_pair", lambda *args, **kw: real_load(*args, **dict(kw, max_new_tokens=16)))
    real_many = pv.PaddleOcrVlHip.generate_many
    calls = []

    def counted_many(self, items, **kw):
        calls.append((len(items), self.packed))
        return real_many(self, items, **dict(kw, max_new_tokens=16))
    monkeypatch.setattr(pv.PaddleOcrVlHip, "generate_many", counted_many)
    try:
        monkeypatch.setattr(mgr, "paddle_ocr_vl_slots", 3, raising=False)
        monkeypatch.setattr(mgr, "paddle_ocr_vl_packed_prefill", True, raising=False)
        try:
            texts = od.extract_text_with_paddle_ocr_vl(crops)
            model = mgr.get_paddle_ocr_vl()[1].model
            assert model.packed and model.slots == 3 and len(model.fill_log) == 3
        finally:
            mgr.unload_ocr_models()
        assert calls == [(3, True)], f"generate_many calls: {calls}"
        assert len(texts) == 4 and texts[1] == od.OCR_FAILED and od.OCR_FAILED not in (texts[0], texts[2], texts[3]), texts
        for slots, flag in ((1, True), (3, "yes")):
            monkeypatch.setattr(mgr, "paddle_ocr_vl_slots", slots, raising=False)
            monkeypatch.setattr(mgr, "paddle_ocr_vl_packed_prefill", flag, raising=False)
            with pytest.raises(ModelError):
                mgr.get_paddle_ocr_vl()
    finally:
        mgr.unload_ocr_models()


NEVER = 509                                                      # an end-of-sequence token the tiny model does not produce in these runs (asserted)


def check_fill_leaves_live_slots_alone(lib):
    """test 17: two slots are decoding while a third is filled: the fill changes no byte of the live lanes of slot_state, of their slot_out rows
    or of their caches, and over the next 8 steps the two live slots' tokens are what they are without the fill"""
    items = bc.make_items(3)
    m = bc.model(lib, 3, packed_prefill=True, hp=dict(eos=[NEVER]))
    try:
        step = m._stepper_batch()
        m.fill_slots([(0, items[0]), (1, items[1])])
        for _ in range(3):
            step.run(graph=m._graph)
        _sync(lib)
        state, out = m.slot_state.cpu().clone(), m.slot_out.cpu().clone()
        caches = [(kc.cpu().clone(), vc.cpu().clone()) for kc, vc in m.slot_caches]
        assert state[abi.SLOT_NOUT, :2].tolist() == [4, 4] and state[abi.SLOT_DONE].tolist()[:3] == [0, 0, 1]
        for _ in range(8):
            step.run(graph=m._graph)
        _sync(lib)
        want = m.slot_out[:2, :12].cpu().clone()
        assert m.slot_state[abi.SLOT_NOUT, :2].tolist() == [12, 12], "precondition: both live slots decode through the 8 steps"
        # back to the state after step 3, then the same 8 steps with a fill of the third slot in front of them
        m.slot_state.copy_(state); m.slot_out.copy_(out)
        for (kc, vc), (k0, v0) in zip(m.slot_caches, caches):
            kc.copy_(k0); vc.copy_(v0)
        m.fill_slots([(2, items[2])])
        _sync(lib)
        after = m.slot_state.cpu()
        assert torch.equal(after[:, :2], state[:, :2]), "the fill wrote a live lane of slot_state"
        assert after[:3, 2].tolist() == [items[2]["input_ids"].shape[1], 1, 0]
        assert torch.equal(m.slot_out[:2].cpu(), out[:2]), "the fill wrote a live slot's output row"
        for i, ((kc, vc), (k0, v0)) in enumerate(zip(m.slot_caches, caches)):
            assert torch.equal(_bits(kc[:2].cpu()), _bits(k0[:2])) and torch.equal(_bits(vc[:2].cpu()), _bits(v0[:2])), f"the fill wrote a live slot's cache (layer {i})"
        for _ in range(8):
            step.run(graph=m._graph)
        _sync(lib)
        assert torch.equal(m.slot_out[:2, :12].cpu(), want), "the live slots' tokens changed when a third slot was filled beside them"
        assert int(m.slot_state[abi.SLOT_NOUT, 2]) == 9
    finally:
        m.close()


def packed_published_widths(lib, seed=0, steps=40, slot=1):
    """test 19: paddle_ocr_vl_checks.check_published_widths with the prompt through the packed fill and the steps on the batched stepper:
    (max, rms) absolute log-prob error over positions 0-9 and 30-39; then 16 tokens per item of the three published-width items decode"""
    _, model = pc.oracle(seed, real=True)
    g = torch.Generator().manual_seed(seed)
    teacher = torch.randint(3, 8000, (steps,), generator=g).tolist()
    ids, pix, thw = pc.make_inputs(seed, grid=(20, 28), extra=tuple(teacher[:-1]))
    T = ids.shape[1] - (steps - 1)
    ref = torch.log_softmax(pc.oracle_logits(model, ids, pix, thw)[T - 1:], -1)
    m = pc.hip_model(lib, abi.F16, seed, real=True, max_new_tokens=steps + 8, max_prompt=T + 8, slots=3, packed_prefill=True)
    try:
        assert m.fill_slots([(slot, dict(input_ids=ids[:, :T], pixel_values=pix, image_grid_thw=thw))]) == [T]
        _sync(lib)
        rows = [m.pk_logits[slot].float().cpu().clone()]
        for t in teacher[:-1]:
            rows.append(m.slot_step_logits(slot, t))
    finally:
        m.close()
    err = torch.log_softmax(torch.stack(rows), -1) - ref
    err = torch.cat([err[:10], err[30:40]])
    assert bool(torch.isfinite(err).all())
    items = _published_items()
    Tm = max(int(it["input_ids"].shape[1]) for it in items)
    m = pc.hip_model(lib, abi.F16, 0, real=True, max_new_tokens=16, max_prompt=Tm + 8, slots=3, packed_prefill=True)
    try:
        got = m.generate_many(items, max_new_tokens=16)
    finally:
        m.close()
    for k, (y, it) in enumerate(zip(got, items)):
        Tk = it["input_ids"].shape[1]
        assert isinstance(y, torch.Tensor) and torch.equal(y[0, :Tk], it["input_ids"][0]) and Tk < y.shape[1] <= Tk + 16, f"item {k}: {y}"
    return float(err.abs().max()), float(err.pow(2).mean().sqrt())
