"""Checks of the slot-batched decode step (csrc/causal.hip: MTX_OP_CAUSAL_STEP_BATCH, MTX_OP_GREEDY_BATCH) and of `PaddleOcrVlHip.generate_many`,
written once and run on the simulator (tests/test_paddle_batch_sim.py) and on the product library (tests/test_paddle_batch_gpu.py).

The reference of every kernel check is the single-sequence op on the same operands (mtx_causal_attention with rows = 1, mtx_greedy_pick), and the
comparison is bit for bit: a slot's result may not depend on which other slots shared its launch.  The model checks hold `generate_many` to
`generate` in the same way, token for token."""
import ctypes as C

import pytest
import torch

import paddle_ocr_vl_checks as pc
from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.plan import PlanBuilder
from mangatranslator_amd.utils.exceptions import ModelError
from op_checks import TD, _dev, _sync
from paddle_ocr_vl_checks import D, GUARD, HEADS, NAN_BITS, S, CausalRig, _bits  # noqa: F401  (HEADS is the test files' parameter list)

MTX_ERR_INVALID, MTX_ERR_UNSUPPORTED = -1, -3          # include/mtx_hip.h
MAX_LEN = 2 * S + 8                                     # three key splits; the last position sits in the third
POSITIONS = [0, 1, S - 1, S, S + 1, 2 * S + 5, MAX_LEN - 1]
# per-slot positions of one launch: both sides of a split boundary in every launch of two or more slots
SLOT_POSITIONS = {1: [2 * S + 5], 2: [S - 1, S], 3: [S + 1, 0, MAX_LEN - 1], 8: POSITIONS + [S]}
LANES = abi.SLOTS_MAX
WS_PATTERN = 0xA5


def make_state(pos, done=None, n_out=None, token=None, rope=None):
    """the int32 [SLOT_FIELDS][SLOTS_MAX] block; lanes beyond the given slots are empty (done = 1)"""
    st = torch.zeros(abi.SLOT_FIELDS, LANES, dtype=torch.int32)
    st[abi.SLOT_DONE] = 1
    n = len(pos)
    st[abi.SLOT_POS, :n] = torch.tensor(pos, dtype=torch.int32)
    st[abi.SLOT_DONE, :n] = torch.tensor(done if done is not None else [0] * n, dtype=torch.int32)
    for field, vals in ((abi.SLOT_NOUT, n_out), (abi.SLOT_TOKEN, token), (abi.SLOT_ROPE, rope)):
        if vals is not None:
            st[field, :n] = torch.tensor(vals, dtype=torch.int32)
    return st


class BatchRig:
    """one recorded MTX_OP_CAUSAL_STEP_BATCH: per-slot caches with a guard band each, the state block, a workspace the test can look into"""

    def __init__(self, lib, dtype, slots, heads, kv_heads, max_len=MAX_LEN):
        self.lib, self.dev, self.td = lib, _dev(lib), TD[dtype]
        self.slots, self.heads, self.kv, self.max_len = slots, heads, kv_heads, max_len
        self.w = (heads + 2 * kv_heads) * D
        self.ws_bytes = abi.causal_ws_bytes(heads, max_len)
        pb = PlanBuilder(lib, self.dev, dtype)
        self.qkv = pb.buf((slots, self.w), self.td, zero=True)
        self.kc = pb.buf((slots, max_len + GUARD, kv_heads * D), self.td, zero=True)
        self.vc = pb.buf((slots, max_len + GUARD, kv_heads * D), self.td, zero=True)
        self.state = pb.buf((abi.SLOT_FIELDS, LANES), torch.int32, zero=True)
        self.o = pb.buf((slots, heads * D), self.td, zero=True)
        self.ws = pb.buf((slots * self.ws_bytes,), torch.uint8, zero=True)
        self.scale = D ** -0.5
        pb.causal_step_batch(self.qkv, self.kc, self.vc, self.state, self.o, slots, heads, kv_heads, D, max_len, self.scale,
                             cache_stride=(max_len + GUARD) * kv_heads * D, ld_qkv=self.w, ld_o=heads * D, workspace=self.ws)
        self.pb, self.plan = pb, None

    def load(self, qkv, kc, vc, state, o=None):
        self.qkv.copy_(qkv); self.kc.copy_(kc); self.vc.copy_(vc); self.state.copy_(state)
        if o is not None:
            self.o.copy_(o)

    def run(self):
        if self.plan is None:
            self.plan = self.pb.build()
        self.plan.run()
        _sync(self.lib)
        return self.o.cpu()

    def counters(self):
        """the ticket words of every slot's workspace region, [slots, heads]"""
        return self.ws.cpu().view(self.slots, self.ws_bytes)[:, :self.heads * 4].contiguous().view(torch.int32)


def _poisoned(td, kv, pos, g, max_len=MAX_LEN):
    """random caches of one slot; everything from `pos` on (the launch's own position, the free tail, the guard band) is NaN"""
    n = max_len + GUARD
    kc = torch.randn(n, kv * D, generator=g).to(td)
    vc = torch.randn(n, kv * D, generator=g).to(td)
    for c in (kc, vc):
        c.view(torch.int16)[max(pos, 0):] = NAN_BITS
    return kc, vc


def _nan_rows(td, rows, width):
    return torch.full((rows, width), NAN_BITS, dtype=torch.int16).view(td)


def _single(single, qkv_row, kc, vc, pos):
    """mtx_causal_attention(rows = 1) on copies of one slot's operands -> (o row, k cache, v cache)"""
    single.o.zero_()
    o = single.run(qkv_row[None], kc, vc, pos)
    return o[0].clone(), single.kc.cpu().clone(), single.vc.cpu().clone()


def _compare_slot(rig, single, s, qkv, kc, vc, pos, got_o, what):
    o1, k1, v1 = _single(single, qkv[s], kc[s], vc[s], pos)
    assert torch.equal(_bits(got_o[s]), _bits(o1)), f"{what}: slot {s} (pos {pos}): o differs from the single step"
    assert torch.equal(_bits(rig.kc[s].cpu()), _bits(k1)) and torch.equal(_bits(rig.vc[s].cpu()), _bits(v1)), \
        f"{what}: slot {s} (pos {pos}): the cache differs from the single step's"


def check_batch_equals_single(lib, dtype, heads, kv, slots, seed=0):
    """item 1: random operands, poisoned caches; per slot o row and whole cache (guard band included) equal the single step's; a second launch
    on the same workspace gives the same bytes; every counter word is zero after each launch"""
    positions = SLOT_POSITIONS[slots]
    g = torch.Generator().manual_seed(seed * 1000 + slots * 31 + heads)
    rig = BatchRig(lib, dtype, slots, heads, kv)
    single = CausalRig(lib, dtype, 1, heads, kv, MAX_LEN)
    caches = [_poisoned(rig.td, kv, p, g) for p in positions]
    kc, vc = torch.stack([c[0] for c in caches]), torch.stack([c[1] for c in caches])
    qkv = (torch.randn(slots, rig.w, generator=g) * 1.5).to(rig.td)
    what = f"batched step slots={slots} heads={heads}/{kv}"
    rig.load(qkv, kc, vc, make_state(positions), o=_nan_rows(rig.td, slots, heads * D))
    first = rig.run().clone()
    assert int(rig.counters().abs().sum()) == 0, f"{what}: ticket counters are not zero after the launch"
    assert bool(torch.isfinite(first.float()).all()), f"{what}: non-finite output (a cache entry at or beyond pos was read, or a row was not written)"
    for s, p in enumerate(positions):
        _compare_slot(rig, single, s, qkv, kc, vc, p, first, what)
    k_after, v_after = rig.kc.cpu().clone(), rig.vc.cpu().clone()
    rig.o.copy_(_nan_rows(rig.td, slots, heads * D))
    second = rig.run()
    assert torch.equal(_bits(second), _bits(first)), f"{what}: the second launch on the same workspace gave other bytes"
    assert torch.equal(_bits(rig.kc.cpu()), _bits(k_after)) and torch.equal(_bits(rig.vc.cpu()), _bits(v_after))
    assert int(rig.counters().abs().sum()) == 0, f"{what}: ticket counters are not zero after the second launch"


def check_sitting_out(lib, dtype, heads, kv, seed=0):
    """item 2: a done slot between two live ones, a slot at pos == max_len and one at pos < 0: their caches, o rows (a NaN pattern) and
    workspace regions (a byte pattern, counters included) keep every byte; the live slots still equal the single step; with every slot done
    the launch succeeds and changes nothing"""
    positions = [S + 1, S, 2 * S + 5, MAX_LEN, -1]
    done = [0, 1, 0, 0, 0]
    live = [0, 2]
    slots = len(positions)
    g = torch.Generator().manual_seed(seed + heads)
    rig = BatchRig(lib, dtype, slots, heads, kv)
    single = CausalRig(lib, dtype, 1, heads, kv, MAX_LEN)
    caches = [_poisoned(rig.td, kv, p if s in live else MAX_LEN + GUARD, g) for s, p in enumerate(positions)]
    kc, vc = torch.stack([c[0] for c in caches]), torch.stack([c[1] for c in caches])
    qkv = (torch.randn(slots, rig.w, generator=g) * 1.5).to(rig.td)
    o0 = _nan_rows(rig.td, slots, heads * D)
    ws0 = torch.zeros(slots, rig.ws_bytes, dtype=torch.uint8)
    for s in range(slots):
        if s not in live:
            ws0[s] = WS_PATTERN
    what = f"batched step, slots that sit out, heads={heads}/{kv}"
    for all_done in (False, True):
        state = make_state(positions, [1] * slots if all_done else done)
        rig.load(qkv, kc, vc, state, o=o0)
        rig.ws.copy_(ws0.view(-1))
        got = rig.run()
        assert torch.equal(rig.state.cpu(), state), f"{what}: the state block was written"
        for s, p in enumerate(positions):
            if s in live and not all_done:
                _compare_slot(rig, single, s, qkv, kc, vc, p, got, what)
                continue
            assert torch.equal(_bits(got[s]), _bits(o0[s])), f"{what}: slot {s} sat out but its o row was written"
            assert torch.equal(_bits(rig.kc[s].cpu()), _bits(kc[s])) and torch.equal(_bits(rig.vc[s].cpu()), _bits(vc[s])), f"{what}: slot {s} sat out but its cache was written"
            assert torch.equal(rig.ws.cpu().view(slots, -1)[s], ws0[s]), f"{what}: slot {s} sat out but its workspace region was written"
        if not all_done:
            assert int(rig.counters()[live].abs().sum()) == 0


def _selection_case(td, pos, heads, kv, winner, g):
    """paddle_ocr_vl_checks.check_causal_selection's construction for ONE row at `pos` (scale 1): -> (qkv row, k cache, v cache, the chosen V row
    spread over the query heads).  One visible key scores 0, every other at most -120, the first key of the future would score more."""
    n = MAX_LEN + GUARD
    j = torch.arange(n)
    i_abs = torch.tensor([pos])
    w = None if winner == "own" else (pos if winner == "pos" else 0)
    phi = torch.zeros(n, D, dtype=torch.float64)
    phi[:, 0], phi[:, 1] = (j // 16).double(), (j % 16).double()
    phi[:, 2] = 1.0
    phi[:, 3] = 1.0
    if w is not None:
        phi[:, 4] = (j != w).double()
        phi[:, 5] = (j == w).double()
        phi[:, 6] = (j == w).double()
    psi = torch.zeros(1, D, dtype=torch.float64)
    hi, lo = pc._b16(i_abs)
    psi[:, 0], psi[:, 1], psi[:, 2], psi[:, 3] = 128.0 * 16, 128.0, -128.0 * hi, -128.0 * lo
    if w is not None:
        hi, lo = pc._b16(i_abs - w)
        psi[:, 4], psi[:, 5], psi[:, 6] = -120.0, 128.0 * hi, 128.0 * lo
    M = psi @ phi.t()
    for t in (phi, psi):
        assert torch.equal(t, t.to(td).double()), "the test's own premise: every feature is exact in the storage type"
    win = pos if w is None else w
    vis = M[0, :pos + 1]
    assert vis[win] == 0 and int((vis > -120).sum()) == 1 and M[0, pos + 1] == (128.0 if w is None else 8.0)
    keys = phi.to(td)[:, None, :].expand(n, kv, D).reshape(n, kv * D)
    vals = torch.randn(n, kv * D, generator=g).to(td)
    qkv = torch.cat([psi.to(td)[:, None, :].expand(1, heads, D).reshape(1, heads * D), keys[pos:pos + 1], vals[pos:pos + 1]], 1)[0]
    kc, vc = keys.clone(), vals.clone()
    for c in (kc, vc):
        cb = c.view(torch.int16)
        cb[pos:pos + 1] = NAN_BITS                   # the launch's own position is read from its row, not from the cache
        cb[pos + 2:] = NAN_BITS                      # cache[pos + 1] keeps the key of the future that would outscore the winner
    want = vals[win].view(kv, D).repeat_interleave(heads // kv, 0).reshape(heads * D)
    return qkv, kc, vc, want


def check_batch_selection(lib, dtype, heads, kv, seed=0):
    """item 3: a different winner (own, pos, zero) in each slot of one launch, the slots at different positions: every o row is the chosen V
    row bit for bit"""
    cases = [("own", S + 1), ("pos", 2 * S + 5), ("zero", S - 1), ("zero", S), ("own", 0), ("pos", 1)]
    slots = len(cases)
    g = torch.Generator().manual_seed(seed + heads)
    rig = BatchRig(lib, dtype, slots, heads, kv)
    rig.scale = 1.0
    rig.pb.ops[-1].u.cstepb.scale = 1.0
    built = [_selection_case(rig.td, pos, heads, kv, winner, g) for winner, pos in cases]
    qkv, kc, vc = (torch.stack([b[i] for b in built]) for i in range(3))
    rig.load(qkv, kc, vc, make_state([p for _, p in cases]), o=_nan_rows(rig.td, slots, heads * D))
    got = rig.run()
    for s, (winner, pos) in enumerate(cases):
        bad = int((_bits(got[s]) != _bits(built[s][3])).sum())
        assert bad == 0, f"batched step heads={heads}/{kv} slot {s} pos={pos} winner={winner}: {bad} of {heads * D} elements differ from the chosen V row"
        want_k, want_v = kc[s].clone(), vc[s].clone()
        want_k[pos] = qkv[s, heads * D:(heads + kv) * D]
        want_v[pos] = qkv[s, (heads + kv) * D:]
        assert torch.equal(_bits(rig.kc[s].cpu()), _bits(want_k)) and torch.equal(_bits(rig.vc[s].cpu()), _bits(want_v)), f"slot {s}: the cache changed elsewhere than at pos"


def _selection_case_per_head(td, pos, heads, kv, g):
    """paddle_ocr_vl_checks.per_head_selection for ONE row at `pos` (scale 1): query head h plays VARIANTS[h % 3] -> (qkv row, k cache, v cache,
    per query head the chosen row of ITS kv head's values)"""
    n = MAX_LEN + GUARD
    phi, psi, win = pc.per_head_selection(td, n, pos, 1, heads)
    keys = phi.to(td)[:, None, :].expand(n, kv, D).reshape(n, kv * D)
    vals = torch.randn(n, kv * D, generator=g).to(td)
    qkv = torch.cat([psi.to(td).reshape(1, heads * D), keys[pos:pos + 1], vals[pos:pos + 1]], 1)[0]
    kc, vc = keys.clone(), vals.clone()
    for c in (kc, vc):
        cb = c.view(torch.int16)
        cb[pos:pos + 1] = NAN_BITS                   # the launch's own position is read from its row, not from the cache
        cb[pos + 2:] = NAN_BITS                      # cache[pos + 1] keeps the key of the future that would outscore the winner
    want = vals.view(n, kv, D)[win[0], torch.arange(heads) // (heads // kv)].reshape(heads * D)
    return qkv, kc, vc, want


def check_batch_selection_per_head(lib, dtype, heads, kv, seed=0):
    """check_batch_selection with a winner per query head: every slot's head h returns its own chosen V row bit for bit (slot = blockIdx.z / nz,
    zc = blockIdx.z - slot * nz and h0 = kvh * gfull + zc * G all have to be right for that), and the ticket words are zero afterwards"""
    positions = [S + 1, 2 * S + 5, S - 1, S, 0, 1]
    slots = len(positions)
    g = torch.Generator().manual_seed(seed + heads)
    rig = BatchRig(lib, dtype, slots, heads, kv)
    rig.scale = 1.0
    rig.pb.ops[-1].u.cstepb.scale = 1.0
    built = [_selection_case_per_head(rig.td, pos, heads, kv, g) for pos in positions]
    qkv, kc, vc = (torch.stack([b[i] for b in built]) for i in range(3))
    rig.load(qkv, kc, vc, make_state(positions), o=_nan_rows(rig.td, slots, heads * D))
    got = rig.run()
    assert int(rig.counters().abs().sum()) == 0, f"batched step heads={heads}/{kv}: ticket counters are not zero after the launch"
    for s, pos in enumerate(positions):
        wrong = (_bits(got[s]) != _bits(built[s][3])).view(heads, D).any(-1).nonzero().flatten().tolist()
        assert not wrong, f"batched step heads={heads}/{kv} (G, nz) = {pc.step_layout(heads, kv)} slot {s} pos={pos}: query heads {wrong} differ from their own chosen V row"
        want_k, want_v = kc[s].clone(), vc[s].clone()
        want_k[pos] = qkv[s, heads * D:(heads + kv) * D]
        want_v[pos] = qkv[s, (heads + kv) * D:]
        assert torch.equal(_bits(rig.kc[s].cpu()), _bits(want_k)) and torch.equal(_bits(rig.vc[s].cpu()), _bits(want_v)), f"slot {s}: the cache changed elsewhere than at pos"


def check_batch_padded_strides(lib, dtype, heads=24, kv=2, seed=0):
    """ld_qkv = w + 24, ld_o = heads * D + 8 in the batched step: every slot's row equals the single step's, the padding of o keeps its sentinel and
    NaN patterns in the padding of qkv are not read"""
    pc.assert_layout(heads, kv)
    positions = SLOT_POSITIONS[3]
    slots = len(positions)
    g = torch.Generator().manual_seed(seed + heads)
    w = (heads + 2 * kv) * D
    td = TD[dtype]
    pb = PlanBuilder(lib, _dev(lib), dtype)
    qkv_b = pb.buf((slots, w + 24), td, zero=True)
    kc_b = pb.buf((slots, MAX_LEN + GUARD, kv * D), td, zero=True)
    vc_b = pb.buf((slots, MAX_LEN + GUARD, kv * D), td, zero=True)
    st_b = pb.buf((abi.SLOT_FIELDS, LANES), torch.int32, zero=True)
    o_b = pb.buf((slots, heads * D + 8), td, zero=True)
    pb.causal_step_batch(qkv_b, kc_b, vc_b, st_b, o_b, slots, heads, kv, D, MAX_LEN, D ** -0.5, cache_stride=(MAX_LEN + GUARD) * kv * D,
                         ld_qkv=w + 24, ld_o=heads * D + 8)
    single = CausalRig(lib, dtype, 1, heads, kv, MAX_LEN)
    caches = [_poisoned(td, kv, p, g) for p in positions]
    kc, vc = torch.stack([c[0] for c in caches]), torch.stack([c[1] for c in caches])
    qkv = (torch.randn(slots, w, generator=g) * 1.5).to(td)
    padded = _nan_rows(td, slots, w + 24)
    padded[:, :w] = qkv
    sentinel = torch.full((slots, heads * D + 8), 7.0).to(td)
    qkv_b.copy_(padded); kc_b.copy_(kc); vc_b.copy_(vc); st_b.copy_(make_state(positions)); o_b.copy_(sentinel)
    pb.build().run()
    _sync(lib)
    got = o_b.cpu()
    assert torch.equal(_bits(got[:, heads * D:]), _bits(sentinel[:, heads * D:])), "the padding of o was written"
    for s, p in enumerate(positions):
        o1, k1, v1 = _single(single, qkv[s], kc[s], vc[s], p)
        assert torch.equal(_bits(got[s, :heads * D]), _bits(o1)), f"padded strides, slot {s}: o differs from the single step"
        assert torch.equal(_bits(kc_b[s].cpu()), _bits(k1)) and torch.equal(_bits(vc_b[s].cpu()), _bits(v1)), f"padded strides, slot {s}: the cache differs"


# ---- greedy batch --------------------------------------------------------------------------------------------------------------------------
BATCH_VOCABS = [1, 255, 4097, 103424]
OUT_GUARD = 4
ROLES = ["max", "nan", "done", "tie", "last", "eos"]


def _greedy_batch(lib, logits, state, out, vocab, max_new, eos, advance, repeats=None):
    """one launch (or, with `repeats` = a list of logits blocks, one plan with a pick per block) -> (state [5, 8], out rows, the guard words)"""
    dev = _dev(lib)
    slots = out.shape[0]
    pb = PlanBuilder(lib, dev, abi.F16)
    st = pb.const(state.to(torch.int32).clone())               # (on the simulator `const` keeps the caller's storage: the launch must not write the test's own inputs)
    flat = pb.const(torch.cat([torch.full((OUT_GUARD,), -99, dtype=torch.int32), out.reshape(-1).to(torch.int32), torch.full((OUT_GUARD,), -99, dtype=torch.int32)]))
    rows = flat[OUT_GUARD:OUT_GUARD + slots * max_new]
    for lg in (repeats if repeats is not None else [logits]):
        pb.greedy_pick_batch(pb.const(lg.float().clone()), st, rows, slots, vocab, max_new, eos=eos, advance=advance, ld_logits=lg.shape[1])
    pb.build().run()
    _sync(lib)
    f = flat.cpu()
    return st.cpu(), f[OUT_GUARD:-OUT_GUARD].view(slots, max_new), torch.cat([f[:OUT_GUARD], f[-OUT_GUARD:]])


def check_greedy_batch(lib, vocab, slots, shift, seed=0):
    """item 4: slot s plays ROLES[(s + shift) % 6] — a plain maximum (in a chunk of its own where the vocabulary has several), all NaN, a done
    slot, two equal maxima, the last free output position, an end-of-sequence token; per slot the state lane and the out row equal the
    single op's, and the rotary row moves with pos"""
    max_new, advance, eos = 6, 1, [3, vocab - 1] if vocab > 4 else [vocab + 5]
    ld = vocab + 13
    g = torch.Generator().manual_seed(seed + vocab + 17 * slots + shift)
    logits = torch.randn(slots, ld, generator=g)
    logits[:, vocab:] = 50.0                                   # the padding behind each row would win if it were read
    state = make_state([10 + s for s in range(slots)], n_out=[2] * slots, token=[5] * slots, rope=[40 + 3 * s for s in range(slots)])
    out = torch.full((slots, max_new), -7, dtype=torch.int32)
    out[:, :2] = torch.tensor([11, 12], dtype=torch.int32)
    roles = [ROLES[(s + shift) % len(ROLES)] for s in range(slots)]
    for s, role in enumerate(roles):
        spot = (s * abi.GREEDY_CHUNK + 17 * s + 5) % vocab      # per-slot maxima in different chunks
        if role == "nan":
            logits[s, :vocab] = float("nan")
            continue
        logits[s, spot] = 9.0
        if role == "done":
            state[abi.SLOT_DONE, s] = 1
        elif role == "tie" and vocab > 1:
            logits[s, vocab - 1 if spot != vocab - 1 else 0] = 9.0
            if vocab > abi.GREEDY_CHUNK and spot + abi.GREEDY_CHUNK < vocab:
                logits[s, spot + abi.GREEDY_CHUNK] = 9.0       # an equal maximum one chunk on
        elif role == "last":
            state[abi.SLOT_NOUT, s] = max_new - 1
            out[s, 2:max_new - 1] = 13
        elif role == "eos":
            logits[s, spot] = 0.0
            logits[s, eos[-1] if eos[-1] < vocab else 0] = 9.0
    st, rows, guard = _greedy_batch(lib, logits, state, out, vocab, max_new, eos, advance)
    assert guard.tolist() == [-99] * (2 * OUT_GUARD), "the words around `out` were written"
    assert torch.equal(st[:, slots:], state[:, slots:]), "lanes beyond `slots` were written"
    for s, role in enumerate(roles):
        st1, out1 = pc._greedy(lib, logits[s, :vocab], state[:4, s].tolist(), max_new, eos, advance, out=out[s].clone())
        what = f"greedy batch vocab={vocab} slots={slots} slot {s} ({role})"
        assert st[:4, s].tolist() == st1 and rows[s].tolist() == out1, f"{what}: state {st[:, s].tolist()} out {rows[s].tolist()} != single {st1} {out1}"
        moved = st1[0] - int(state[abi.SLOT_POS, s])
        assert int(st[abi.SLOT_ROPE, s]) == int(state[abi.SLOT_ROPE, s]) + moved, f"{what}: the rotary row did not move with pos"
        if role == "nan":
            assert st1[3] == 0
        if role == "done":
            assert st1 == state[:4, s].tolist() and out1 == out[s].tolist()
        if role == "last":
            assert st1[1] == max_new and st1[2] == 1
        if role == "eos" and eos[-1] < vocab:
            assert st1[2] == 1 and st1[3] == eos[-1]
        if role in ("max", "tie") and vocab > 1:
            assert st1[3] == (s * abi.GREEDY_CHUNK + 17 * s + 5) % vocab


def check_greedy_batch_damaged_state(lib):
    """n_out outside 0 .. max_new - 1 sets done and writes nothing else (as the single op)"""
    vocab, max_new = 300, 4
    logits = torch.zeros(3, vocab); logits[:, 7] = 1.0
    state = make_state([5, 6, 7], n_out=[-1, max_new, 1], rope=[1, 2, 3])
    out = torch.full((3, max_new), -7, dtype=torch.int32)
    st, rows, guard = _greedy_batch(lib, logits, state, out, vocab, max_new, [], 1)
    assert guard.tolist() == [-99] * (2 * OUT_GUARD)
    assert st[:, 0].tolist() == [5, -1, 1, 0, 1] and st[:, 1].tolist() == [6, max_new, 1, 0, 2] and st[:, 2].tolist() == [8, 2, 0, 7, 4]
    assert rows.tolist() == [[-7] * 4, [-7] * 4, [-7, 7, -7, -7]]


def check_greedy_batch_65_chunks(lib):
    """paddle_ocr_vl_checks.greedy_65_cases in slot 1 of 2 (record run 2 * 1 * 65 on) with ld_logits = vocab + 3; slot 0 holds the next case.
    Three launches; the expected tokens come from the cases, not from the single op"""
    cases = pc.greedy_65_cases()
    vocab, max_new = pc.VOCAB_65, 4
    assert pc.greedy_chunks(vocab) == 65
    for k in range(len(cases)):
        pair = [cases[(k + 1) % len(cases)], cases[k]]
        logits = torch.full((2, vocab + 3), 50.0)              # the padding behind each row would win if it were read
        for s, (_, lg, _) in enumerate(pair):
            logits[s, :vocab] = lg
        state = make_state([10, 20], n_out=[1, 2], token=[-1, -1], rope=[40, 43])
        out = torch.full((2, max_new), -7, dtype=torch.int32)
        st, rows, guard = _greedy_batch(lib, logits, state, out, vocab, max_new, [], 1)
        assert guard.tolist() == [-99] * (2 * OUT_GUARD) and torch.equal(st[:, 2:], state[:, 2:])
        for s, (name, _, want) in enumerate(pair):
            n = 1 + s
            assert st[:, s].tolist() == [10 + 10 * s + 1, n + 1, 0, want, 40 + 3 * s + 1], f"65 chunks, slot {s}, {name}: state {st[:, s].tolist()}, expected token {want}"
            assert rows[s].tolist() == [-7] * n + [want] + [-7] * (max_new - n - 1)


def check_greedy_batch_run(lib):
    """a run of 5 batched picks in one plan equals 5 single picks per slot; slot 1 meets its end-of-sequence token at the third"""
    vocab, max_new, slots, eos = 255, 8, 3, [2]
    toks = [[5, 6, 7, 8, 9], [20, 21, 2, 22, 23], [30, 30, 31, 32, 33]]
    blocks = []
    for k in range(5):
        lg = torch.zeros(slots, vocab + 3)
        for s in range(slots):
            lg[s, toks[s][k]] = 1.0
        blocks.append(lg)
    state = make_state([30, 40, 50], token=[-1] * slots, rope=[3, 4, 5])
    out = torch.full((slots, max_new), -7, dtype=torch.int32)
    st, rows, guard = _greedy_batch(lib, None, state, out, vocab, max_new, eos, 1, repeats=blocks)
    assert guard.tolist() == [-99] * (2 * OUT_GUARD)
    dev = _dev(lib)
    for s in range(slots):
        pb = PlanBuilder(lib, dev, abi.F16)
        st1 = pb.const(state[:4, s].clone())
        ot1 = pb.const(out[s].clone())
        for k in range(5):
            pb.greedy_pick(pb.const(blocks[k][s, :vocab].clone()), st1, ot1, vocab, max_new, eos=eos, advance=1)
        pb.build().run()
        _sync(lib)
        assert st[:4, s].tolist() == st1.cpu().tolist() and rows[s].tolist() == ot1.cpu().tolist(), f"slot {s}: {st[:, s].tolist()} {rows[s].tolist()}"
        assert int(st[abi.SLOT_ROPE, s]) - int(state[abi.SLOT_ROPE, s]) == int(st[abi.SLOT_POS, s]) - int(state[abi.SLOT_POS, s])
    assert st[:, 1].tolist() == [43, 3, 1, 2, 7] and rows[1].tolist() == [20, 21, 2] + [-7] * 5


def check_batch_refusals(lib):
    """item 5: argument checks only — the launch functions return before any launch"""
    rig = BatchRig(lib, abi.BF16, 2, 4, 2, max_len=8)
    base = rig.pb.ops[-1].u.cstepb

    def rc(**edit):
        a = abi.CausalStepBatchArgs.from_buffer_copy(base)
        for k, v in edit.items():
            setattr(a, k, v)
        return lib.mtx_causal_step_batch(C.byref(a), C.c_void_p(0))
    assert rc(slots=0) == MTX_ERR_INVALID and rc(slots=abi.SLOTS_MAX + 1) == MTX_ERR_INVALID
    assert rc(state=None) == MTX_ERR_INVALID
    assert rc(workspace_bytes=2 * abi.causal_ws_bytes(4, 8) - 1) == MTX_ERR_INVALID and rc(workspace=None) == MTX_ERR_INVALID
    assert rc(d=64) == MTX_ERR_UNSUPPORTED and rc(heads=3) == MTX_ERR_UNSUPPORTED
    assert rc(dtype=abi.F32) == MTX_ERR_INVALID and rc(cache_stride=8 * 2 * D - 8) == MTX_ERR_INVALID
    pb = PlanBuilder(lib, _dev(lib), abi.F16)
    st, lg, ot = pb.buf((abi.SLOT_FIELDS, LANES), torch.int32, zero=True), pb.buf((2, 16)), pb.buf((2, 4), torch.int32, zero=True)
    pb.greedy_pick_batch(lg, st, ot, 2, 16, 4)
    gbase = pb.ops[-1].u.greedyb

    def grc(**edit):
        a = abi.GreedyBatchArgs.from_buffer_copy(gbase)
        for k, v in edit.items():
            setattr(a, k, v)
        return lib.mtx_greedy_pick_batch(C.byref(a), C.c_void_p(0))
    for edit in (dict(slots=0), dict(slots=abi.SLOTS_MAX + 1), dict(state=None), dict(vocab=0), dict(max_new=0), dict(n_eos=5), dict(ld_logits=15)):
        assert grc(**edit) == MTX_ERR_INVALID, edit
    bad = PlanBuilder(lib, _dev(lib), abi.BF16)
    bad.causal_step_batch(rig.qkv, rig.kc, rig.vc, rig.state, rig.o, abi.SLOTS_MAX + 1, 4, 2, D, 8, 1.0)
    with pytest.raises(ModelError):
        bad.build().run()


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
SEED = 0                                                         # ONE set of weights (GREEDY_SIGMA) for every model check
GRIDS = [(4, 6), (2, 8), (4, 4), (2, 2), (6, 4)]
BUDGET = 12


def make_items(n, first=0):
    """n prompts of different image seeds, grids and lengths"""
    items = []
    for k in range(first, first + n):
        ids, pix, thw = pc.make_inputs(k, grid=GRIDS[k % len(GRIDS)], before=(1, 10, 11) + tuple(range(12, 12 + k % 3)), after=(20, 21, 22)[:1 + k % 3])
        items.append(dict(input_ids=ids, pixel_values=pix, image_grid_thw=thw))
    return items


def model(lib, slots, **kw):
    return pc.hip_model(lib, abi.F16, SEED, sigma=pc.GREEDY_SIGMA, slots=slots, **kw)


def one_at_a_time(lib, items, budget=BUDGET, **kw):
    """`generate` per item on a fresh model"""
    m = model(lib, 1, **kw)
    try:
        return [m.generate(**it, max_new_tokens=budget) for it in items]
    finally:
        m.close()


def many(lib, items, slots, budget=BUDGET, check_every=None, **kw):
    m = model(lib, slots, **kw)
    try:
        return m.generate_many(items, max_new_tokens=budget, check_every=check_every), list(m.fill_log)
    finally:
        m.close()


# The end-of-sequence token of the model checks, chosen as check_device_loop does, among the free-running tokens of the 8 items (simulator, f16,
# budget 12; item 3 starts with it, items 4 and 6 meet it at steps 10 and 4, the others never):
#   0: 373 x 12                                   4: 270 327 119 270 x 6 45 45 45
#   1: 200 200 133 49 206 206 453 133 49 206 30 48  5: 133 160 414 112 414 49 30 106 0 184 184 511
#   2: 405 327 x 10 314                            6: 119 53 405 45 x 6 419 498 498
#   3: 45 365 x 11
# The checks assert what they need of it (their preconditions) on the library they run on.
STOP = 45
_REFERENCE = {}


def reference(lib):
    """computed once per library and shared, never modified: (items, what `generate` returns per item with STOP as the end-of-sequence token,
    generated lengths) for the 8 items of the model checks"""
    key = lib.is_simulator
    if key not in _REFERENCE:
        items = make_items(8)
        want = one_at_a_time(lib, items, hp=dict(eos=[STOP]))
        lens = [int(w.shape[1] - it["input_ids"].shape[1]) for w, it in zip(want, items)]
        print(f"generated lengths with end-of-sequence token {STOP}: {lens}")
        _REFERENCE[key] = (items, want, lens)
    return _REFERENCE[key]


def check_generate_many_equals_generate(lib, check_every, n=7, slots=3):
    """item 6.  The order of the items comes from the reference run alone: one that ends early by EOS goes first, beside two others, so that
    its slot is refilled while they are mid-sequence.  Asserts its own preconditions: two items end by EOS at different step counts, one runs
    to the budget, a slot is refilled while another is mid-sequence"""
    items, want, lens = reference(lib)
    items, want, lens = items[:n], want[:n], lens[:n]
    hp = dict(hp=dict(eos=[STOP]))
    ended = [int(w[0, -1]) == STOP for w in want]
    by_eos = sorted({n_ for n_, e in zip(lens, ended) if e and n_ < BUDGET})
    assert len(by_eos) >= 2, f"precondition: two items must end by EOS at different step counts, lengths {lens}"
    assert any(n_ == BUDGET and not e for n_, e in zip(lens, ended)), f"precondition: one item must run to the budget, lengths {lens}"
    first = min((k for k in range(n) if ended[k] and 1 < lens[k] < BUDGET), key=lambda k: lens[k])
    order = [first] + sorted((k for k in range(n) if k != first), key=lambda k: -lens[k])
    got, log = many(lib, [items[k] for k in order], slots, check_every=check_every, **hp)
    for k, a in zip(order, got):
        assert isinstance(a, torch.Tensor) and a.dtype == torch.int64 and torch.equal(a, want[k]), f"item {k} (check_every {check_every}): {a} != generate's {want[k]}"
    assert len(log) == n and sorted(i for i, _, _ in log) == list(range(n))
    assert any(1 < n_other < lens[order[other]] for _, _, others in log[slots:] for other, n_other in others), \
        f"precondition: a slot must be refilled while another is mid-sequence, fill log {log}, lengths {[lens[k] for k in order]}"
    rev, _ = many(lib, [items[k] for k in order[::-1]], slots, check_every=check_every, **hp)
    for k, a in zip(order[::-1], rev):
        assert torch.equal(a, want[k]), f"item {k} in reverse order: {a} != {want[k]}"
    return lens


def check_other_slot_counts(lib):
    """slots = 8 with 8 items, slots = 2 with 1 item"""
    items, want, _ = reference(lib)
    hp = dict(hp=dict(eos=[STOP]))
    got, _ = many(lib, items, 8, **hp)
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"slots = 8, item {k}: {a} != {b}"
    got, _ = many(lib, items[3:4], 2, **hp)
    assert len(got) == 1 and torch.equal(got[0], want[3])


def check_refused_items(lib):
    """item 7: a prompt longer than max_prompt and an odd grid between good ones leave ModelErrors at their indices; `generate` still refuses
    two rows of input_ids"""
    good = make_items(3)
    long_ids, pix, thw = pc.make_inputs(0, extra=tuple(range(30, 30 + 60)))
    assert long_ids.shape[1] > 64
    odd = dict(input_ids=good[0]["input_ids"], pixel_values=torch.randn(3 * 4, 3, 14, 14), image_grid_thw=torch.tensor([[1, 3, 4]]))
    items = [good[0], dict(input_ids=long_ids, pixel_values=pix, image_grid_thw=thw), good[1], odd, good[2]]
    want = one_at_a_time(lib, good)
    got, _ = many(lib, items, 2)
    assert isinstance(got[1], ModelError) and isinstance(got[3], ModelError), got
    assert all(torch.equal(got[k], w) for k, w in zip((0, 2, 4), want))
    got, _ = many(lib, items[1:4], 1)                          # slots = 1: the items go through `generate` one by one
    assert isinstance(got[0], ModelError) and isinstance(got[2], ModelError) and torch.equal(got[1], want[1])
    m = model(lib, 2)
    try:
        with pytest.raises(ModelError):
            m.generate(input_ids=torch.cat([good[0]["input_ids"]] * 2), pixel_values=good[0]["pixel_values"], image_grid_thw=good[0]["image_grid_thw"])
        with pytest.raises(ModelError):
            model(lib, abi.SLOTS_MAX + 1)
    finally:
        m.close()


def images():
    import numpy as np
    from PIL import Image
    out = []
    for a, b, h, w in ((7, 13, 50, 90), (11, 5, 64, 64), (3, 17, 90, 40)):
        yy, xx = np.mgrid[0:h, 0:w]
        out.append(Image.fromarray(((xx * a + yy * b) % 97 + 80).astype(np.uint8)).convert("RGB"))
    return out


def check_driver(lib, tmp_path, monkeypatch):
    """item 8: the driver with paddle_ocr_vl_slots = 3 returns what it returns with slots = 1, the marker at the unreadable crop's index; with
    generate_many raising, the same texts through the per-image loop"""
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
    a, b, c = images()
    crops = [a, None, b, c]
    # the driver asks for 1024 new tokens; the staged (seeded) model seldom meets its EOS, so the model is built for 16
    real_load = pv.load_pair
    monkeypatch.setattr(pv, "load_pair", lambda *args, **kw: real_load(*args, **dict(kw, max_new_tokens=16)))
    real_generate, real_many = pv.PaddleOcrVlHip.generate, pv.PaddleOcrVlHip.generate_many
    monkeypatch.setattr(pv.PaddleOcrVlHip, "generate", lambda self, **kw: real_generate(self, **dict(kw, max_new_tokens=16)))
    calls = []

    def counted_many(self, items, **kw):
        calls.append(len(items))
        return real_many(self, items, **dict(kw, max_new_tokens=16))
    monkeypatch.setattr(pv.PaddleOcrVlHip, "generate_many", counted_many)
    texts = {}
    try:
        for slots in (1, 3):
            monkeypatch.setattr(mgr, "paddle_ocr_vl_slots", slots, raising=False)
            try:
                texts[slots] = od.extract_text_with_paddle_ocr_vl(crops)
                assert mgr.get_paddle_ocr_vl()[1].slots == slots
            finally:
                mgr.unload_ocr_models()
        assert calls == [3], f"generate_many calls: {calls}"
        assert texts[1][1] == od.OCR_FAILED and od.OCR_FAILED not in (texts[1][0], texts[1][2], texts[1][3]) and len(set(texts[1])) >= 3, texts[1]
        assert texts[3] == texts[1], (texts[3], texts[1])

        def broken(self, items, **kw):
            raise RuntimeError("batch path down")
        monkeypatch.setattr(pv.PaddleOcrVlHip, "generate_many", broken)
        try:
            assert od.extract_text_with_paddle_ocr_vl(crops) == texts[1]
        finally:
            mgr.unload_ocr_models()
    finally:
        mgr.unload_ocr_models()


def check_published_widths(lib, slots=3, steps=16):
    """item 9 (GPU tier): the wheel's default sizes with the vocabulary cut to 8 192 — 16 query heads over 2 key-value heads, the G = 8
    instantiation — three grids, 16 tokens each: generate_many equals generate exactly"""
    items = []
    for k, grid in enumerate([(20, 28), (28, 40), (8, 12)]):
        ids, pix, thw = pc.make_inputs(k, grid=grid)
        items.append(dict(input_ids=ids, pixel_values=pix, image_grid_thw=thw))
    T = max(int(it["input_ids"].shape[1]) for it in items)
    kw = dict(real=True, max_new_tokens=steps, max_prompt=T + 8)
    m = pc.hip_model(lib, abi.F16, 0, **kw)
    try:
        want = [m.generate(**it, max_new_tokens=steps) for it in items]
    finally:
        m.close()
    m = pc.hip_model(lib, abi.F16, 0, slots=slots, **kw)
    try:
        got = m.generate_many(items, max_new_tokens=steps)
    finally:
        m.close()
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"published widths, item {k}: {a[0, -steps:].tolist()} != {b[0, -steps:].tolist()}"
