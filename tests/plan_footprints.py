"""What a recorded plan op reads and writes, and which ops of a plan may run at the same time — test infrastructure only.

`footprint(op)` is computed from the ctypes argument block the native library receives (`plan.ops[i]`) and nothing else: every rule below
restates include/mtx_hip.h, the way the other test modules restate dispatch rules.  A region is a list of `Rect`s — `rows` runs of
`row_bytes` bytes, `stride` bytes apart, from `base` — and `rects_overlap` is exact: the text and image streams of a DiT step interleave
by rows inside one allocation, so bounding intervals would flag everything.

`concurrent_pairs(ops)` restates the ordering `mtx_plan_run` creates (csrc/api.hip):
  * main ops are in order among themselves, and so are side ops (one stream each);
  * a side run — consecutive side ops — forks where it starts: its ops come after every main op recorded before its FIRST op;
  * a main op that carries MTX_LANE_JOIN waits for every side op recorded before it, and so does every main op after it;
  * the end of the plan joins.
A side op s and a main op m are therefore ordered iff m < start_of_run(s), or s < j <= m for some main op j with the join flag; every other
side / main pair is concurrent.  (Paths through several forks and joins add nothing: they only run forward in program order.)

`hazards(ops, labels)` reports every concurrent pair with write / write, write / read or read / write overlap."""
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from mangatranslator_amd.hip import abi

RESDIST_PARTS = 256                     # MTX_RESDIST_PARTS
_ES = {abi.BF16: 2, abi.F16: 2}         # element sizes of the 16-bit plans; anything else is refused where it matters


class UnknownOp(ValueError):
    """an op kind or option `footprint` has no rule for: never an empty footprint"""


@dataclass(frozen=True)
class Rect:
    base: int
    rows: int
    row_bytes: int
    stride: int
    name: str = ""

    @property
    def end(self) -> int:
        return self.base + (self.rows - 1) * self.stride + self.row_bytes

    def __str__(self):
        return f"{self.name}[0x{self.base:x} + {self.rows} x {self.row_bytes} B / {self.stride} B]"


def _rect(name, ptr, rows, row_bytes, stride) -> List[Rect]:
    """rows x row_bytes from ptr; nothing for a null pointer or an empty shape; rows that touch or overlap are merged into one run"""
    if not ptr or rows <= 0 or row_bytes <= 0:
        return []
    rows, row_bytes, stride = int(rows), int(row_bytes), int(stride)
    if rows > 1 and stride < row_bytes:
        raise UnknownOp(f"{name}: rows of {row_bytes} bytes overlap at a stride of {stride} bytes")
    if rows == 1 or stride == row_bytes:
        return [Rect(int(ptr), 1, rows * row_bytes, rows * row_bytes, name)]
    return [Rect(int(ptr), rows, row_bytes, stride, name)]


def _plane(name, ptr, planes, rows, lds) -> List[Rect]:
    """an MX scale plane: one uint32 per (row, 128 k) at scale[(k / 128) * lds + row]"""
    return _rect(name, ptr, planes, 4 * rows, 4 * lds)


def _es(dtype, what) -> int:
    if dtype not in _ES:
        raise UnknownOp(f"{what}: dtype {dtype} is not a 16-bit type")
    return _ES[dtype]


def _cdiv(a, b):
    return -(-int(a) // int(b))


# ---- per kind ---------------------------------------------------------------------------------------------------------------------------
def _gemm(g):
    es = _es(g.dtype, "gemm")
    if g.batch != 1:
        raise UnknownOp(f"gemm: batch {g.batch}")
    if g.w_lo:
        raise UnknownOp("gemm: weight pair (w_lo)")
    if g.out_dtype not in (g.dtype, abi.F32):
        raise UnknownOp(f"gemm: out_dtype {g.out_dtype}")
    if g.res_dtype not in (0, g.dtype, abi.F32):
        raise UnknownOp(f"gemm: res_dtype {g.res_dtype}")
    if g.flags & ~(abi.GEMM_FORCE_TILE256 | abi.GEMM_NO_SPLIT | 0xff00):
        raise UnknownOp(f"gemm: flags {g.flags:#x}")
    m, n, k = g.m, g.n, g.k
    r, w = [], []
    if g.in_dtype == abi.F8:
        if k % 128:
            raise UnknownOp("gemm: fp8 operands with K % 128 != 0")
        r += _rect("a", g.a, m, k, g.lda) + _rect("w", g.w, n, k, g.ldw)
        r += _plane("a_scale", g.a_scale, k // 128, m, g.lds_a) + _plane("w_scale", g.w_scale, k // 128, n, g.lds_w)
    elif g.in_dtype in (0, g.dtype):
        if g.a_scale or g.w_scale:
            raise UnknownOp("gemm: scale planes on 16-bit operands")
        r += _rect("a", g.a, m, k * es, g.lda * es) + _rect("w", g.w, n, k * es, g.ldw * es)
    else:
        raise UnknownOp(f"gemm: in_dtype {g.in_dtype}")
    r += _rect("bias", g.bias, 1, 4 * n, 4 * n)
    res_es = 4 if g.res_dtype == abi.F32 else es
    r += _rect("res", g.res, m, n * res_es, g.ldres * res_es)
    if g.gate:
        if g.gate_rows_per < 1:
            raise UnknownOp("gemm: gate without gate_rows_per")
        r += _rect("gate", g.gate, _cdiv(m, g.gate_rows_per), n * es, g.ldgate * es)
    out_es = 4 if g.out_dtype == abi.F32 else es
    if g.actq_q:
        if g.glu_q or g.in_dtype != abi.F8 or n % 128:
            raise UnknownOp("gemm: activation epilogue beside glu / 16-bit operands / ragged n")
        w += _rect("actq_q", g.actq_q, m, n, g.actq_ldq) + _plane("actq_scale", g.actq_scale, n // 128, m, g.actq_lds)
    elif g.glu_q:
        hid = (n - g.glu_col0) // 2
        if g.in_dtype != abi.F8 or g.glu_col0 < 0 or (n - g.glu_col0) % 256 or g.glu_col0 % 256:
            raise UnknownOp("gemm: gated epilogue with 16-bit operands or ragged spans")
        w += _rect("c", g.c, m, g.glu_col0 * out_es, g.ldc * out_es)
        w += _rect("glu_q", g.glu_q, m, hid, g.glu_ldq) + _plane("glu_scale", g.glu_scale, hid // 128, m, g.glu_lds)
    else:
        if not g.c:
            raise UnknownOp("gemm: no output")
        w += _rect("c", g.c, m, n * out_es, g.ldc * out_es)
    if g.workspace:
        ws = _rect("workspace", g.workspace, 1, g.workspace_bytes, g.workspace_bytes)
        r, w = r + ws, w + ws
    return r, w


def _norm(a):
    es = _es(a.dtype, "norm")
    if a.kind not in (0, 1):
        raise UnknownOp(f"norm: kind {a.kind}")
    rows, c = a.rows, a.c
    r = _rect("x", a.x, rows, c * es, a.ldx * es)
    r += _rect("gamma", a.gamma, 1, 4 * c, 4 * c) + _rect("beta", a.beta, 1, 4 * c, 4 * c)
    if a.mod_scale or a.mod_shift:
        if a.rows_per < 1:
            raise UnknownOp("norm: modulation without rows_per")
        nmod = _cdiv(rows, a.rows_per)
        r += _rect("mod_scale", a.mod_scale, nmod, c * es, max(a.ldmod, c) * es) + _rect("mod_shift", a.mod_shift, nmod, c * es, max(a.ldmod, c) * es)
    w = _rect("y", a.y, rows, c * es, a.ldy * es)
    if a.q:
        if c % 128:
            raise UnknownOp("norm: fp8 twin with C % 128 != 0")
        w += _rect("q", a.q, rows, c, a.ldq) + _plane("q_scale", a.q_scale, c // 128, rows, a.lds_q)
    if not w:
        raise UnknownOp("norm: no output")
    return r, w


def _heads(name, ptr, batch, heads, s, d_bytes, bs, ss, hs, es):
    """[batch, s, heads, d] through strides (elements): one rect per batch where the heads of a row lie side by side, else one per head"""
    out = []
    for b in range(batch):
        p = ptr + b * bs * es if ptr else ptr
        if hs * es == d_bytes or heads == 1:
            out += _rect(name, p, s, heads * d_bytes, ss * es)
        else:
            for h in range(heads):
                out += _rect(f"{name}.h{h}", p + h * hs * es if p else p, s, d_bytes, ss * es)
    return out


def _attn(a):
    es = _es(a.dtype, "attention")
    if a.flags & ~abi.ATTN_Q_PRESCALED:
        raise UnknownOp(f"attention: flags {a.flags:#x}")
    B, H, sq, sk, d = a.batch, a.heads, a.sq, a.sk, a.d
    fp8_any = a.q8 or a.q_f8 or a.k_f8 or a.v_f8t
    if fp8_any and (d != 128 or B != 1):
        raise UnknownOp("attention: fp8 forms need d = 128 and batch 1")
    if bool(a.q_f8) != bool(a.k_f8) or (a.v_f8t and not (a.q_f8 and a.q8)):
        raise UnknownOp("attention: incomplete fp8 operand set")
    r, w = [], []
    if a.q_f8:
        r += _rect("q_f8", a.q_f8, sq, H * 128, a.qf8_ss) + _rect("k_f8", a.k_f8, sk, H * 128, a.kf8_ss)
    else:
        r += _heads("q", a.q, B, H, sq, d * es, a.q_bs, a.q_ss, a.q_hs, es) + _heads("k", a.k, B, H, sk, d * es, a.k_bs, a.k_ss, a.k_hs, es)
    if a.v_f8t:
        r += _rect("v_f8t", a.v_f8t, H * 128, _cdiv(sk, 64) * 64, a.vf8_ld)
    else:
        r += _heads("v", a.v, B, H, sk, d * es, a.v_bs, a.v_ss, a.v_hs, es)
    w += _heads("o", a.o, B, H, sq, d * es, a.o_bs, a.o_ss, a.o_hs, es)
    if a.q8:
        w += _rect("q8", a.q8, sq, H * 128, a.ldq8) + _plane("q8_scale", a.q8_scale, H, sq, a.lds_q8)
    if not w:
        raise UnknownOp("attention: no output")
    if a.workspace:
        ws = _rect("workspace", a.workspace, 1, a.workspace_bytes, a.workspace_bytes)
        r, w = r + ws, w + ws
    return r, w


def _quant(a):
    es = _es(a.dtype, "quantize")
    if a.k % 128:
        raise UnknownOp("quantize: K % 128 != 0")
    rows, k = a.rows, a.k
    r = _rect("x", a.x, rows, k * es, a.ldx * es)
    w = _rect("q", a.q, rows, k, a.ldq) + _plane("scale", a.scale, k // 128, rows, a.lds)
    if a.op == abi.QUANT_SWIGLU:
        if not a.b:
            raise UnknownOp("quantize: SwiGLU without b")
        r += _rect("b", a.b, rows, k * es, a.ldb * es)
        w += _rect("y", a.y, rows, k * es, a.ldy * es)
    elif a.op != abi.QUANT_PLAIN:
        raise UnknownOp(f"quantize: op {a.op}")
    elif a.b or a.y:
        raise UnknownOp("quantize: b / y on a plain launch")
    return r, w


def _ew(e):
    es = _es(e.dtype, "elementwise")
    rows, c, k = e.n * e.h * e.w, e.c, e.kind
    if k in (abi.EW_COPY, abi.EW_SUB, abi.EW_ADD, abi.EW_SWIGLU):
        two = k != abi.EW_COPY
        if e.s or e.y8 or bool(e.b) != two:
            raise UnknownOp(f"elementwise kind {k}: unexpected operand set")
        r = _rect("a", e.a, rows, c * es, e.lda * es) + (_rect("b", e.b, rows, c * es, e.ldb * es) if two else [])
        return r, _rect("y", e.y, rows, c * es, e.ldy * es)
    if k == abi.EW_QK_NORM_ROPE:
        d, qh = e.i0, e.i1
        if d <= 0 or c % d or not e.b or not e.s or qh < 0:
            raise UnknownOp("qk_norm_rope: head width / table / gamma")
        heads = c // d
        r = _rect("a", e.a, rows, c * es, e.lda * es) + _rect("gamma", e.s, 1, 4 * d * (2 if qh > 0 else 1), 4 * d * 2)
        q_tab = qh > 0 and e.ldb > 0                     # the q heads read the copy ldb floats behind b
        if not q_tab or heads > qh:
            r += _rect("table", e.b, 1, 4 * d * rows, 4 * d * rows)
        if q_tab:
            r += _rect("table.q", e.b + 4 * e.ldb, 1, 4 * d * rows, 4 * d * rows)
        w = _rect("y", e.y, rows, c * es, e.ldy * es) + _rect("y8", e.y8, rows, c, e.ldy8)
        return r, w
    if k == abi.EW_V_F8T:
        if c % 128 or not e.y8 or e.y or e.b or e.s:
            raise UnknownOp("v_f8t: operand set")
        return _rect("a", e.a, rows, c * es, e.lda * es), _rect("y8", e.y8, c, _cdiv(rows, 64) * 64, e.ldy8)
    if k == abi.EW_RESIDUAL_DIST:
        if not (e.a and e.b and e.s and e.y):
            raise UnknownOp("residual_dist: operand set")
        r = _rect("a", e.a, rows, c * es, e.lda * es) + _rect("b", e.b, rows, c * es, e.ldb * es) + _rect("prev", e.s, rows, c * es, e.lds * es)
        return r, _rect("parts", e.y, 1, 8 * RESDIST_PARTS, 8 * RESDIST_PARTS)
    raise UnknownOp(f"elementwise kind {k}")


_KINDS = {abi.OP_GEMM: ("gemm", _gemm), abi.OP_NORM: ("norm", _norm), abi.OP_ATTN: ("attn", _attn), abi.OP_QUANT: ("quant", _quant),
          abi.OP_EW: ("ew", _ew)}


def footprint(op) -> Tuple[List[Rect], List[Rect]]:
    """(reads, writes) of one recorded abi.Op"""
    if op.kind not in _KINDS:
        raise UnknownOp(f"op kind {op.kind}")
    field, fn = _KINDS[op.kind]
    r, w = fn(getattr(op.u, field))
    if not w or not r:
        raise UnknownOp(f"op kind {op.kind}: empty footprint")
    return r, w


# ---- exact overlap ----------------------------------------------------------------------------------------------------------------------
def rects_overlap(p: Rect, q: Rect) -> Optional[Tuple[int, int]]:
    """first shared byte range (address, bytes) of two rects, or None.  Exact: every row of the shorter rect is intersected with the rows of
    the other by integer arithmetic, no bounding box beyond the first quick reject"""
    if p.base >= q.end or q.base >= p.end:
        return None
    if p.rows > q.rows:
        p, q = q, p
    lo = p.base + np.arange(p.rows, dtype=np.int64) * p.stride           # p's rows: [lo, hi)
    hi = lo + p.row_bytes
    # rows j of q with q.base + j * stride < hi  and  q.base + j * stride + row_bytes > lo
    j0 = np.maximum(-((q.base + q.row_bytes - lo - 1) // q.stride), 0)   # smallest j with q.base + j * stride + row_bytes > lo
    j1 = np.minimum((hi - 1 - q.base) // q.stride, q.rows - 1)           # largest j with q.base + j * stride < hi
    hit = np.nonzero(j0 <= j1)[0]
    if hit.size == 0:
        return None
    i, j = int(hit[0]), int(j0[hit[0]])
    a = max(int(lo[i]), q.base + j * q.stride)
    b = min(int(hi[i]), q.base + j * q.stride + q.row_bytes)
    assert b > a
    return a, b - a


def regions_overlap(ra: List[Rect], rb: List[Rect]):
    """(rect of ra, rect of rb, address, bytes) of the first overlap, or None"""
    for p in ra:
        for q in rb:
            o = rects_overlap(p, q)
            if o:
                return p, q, o[0], o[1]
    return None


# ---- ordering ---------------------------------------------------------------------------------------------------------------------------
def concurrent_pairs(ops) -> List[Tuple[int, int]]:
    """(side op index, main op index) of every pair `mtx_plan_run` leaves unordered"""
    lanes = [int(op.lane) for op in ops]
    side = [bool(l & abi.LANE_SIDE) for l in lanes]
    run_start, start = [None] * len(ops), None
    for i, s in enumerate(side):
        if s:
            if i == 0 or not side[i - 1]:
                start = i
            run_start[i] = start
    joins = [i for i, l in enumerate(lanes) if (l & abi.LANE_JOIN) and not side[i]]
    pairs = []
    for s in range(len(ops)):
        if not side[s]:
            continue
        nxt = next((j for j in joins if j > s), len(ops))     # the first join behind s; every main op from there on waits for s
        for m in range(run_start[s], nxt):                     # main ops at or behind the fork and before that join
            if not side[m]:
                pairs.append((s, m))
    return pairs


def side_runs(ops) -> int:
    side = [bool(op.lane & abi.LANE_SIDE) for op in ops]
    return sum(1 for i, s in enumerate(side) if s and (i == 0 or not side[i - 1]))


@dataclass
class Hazard:
    kind: str          # "write/write", "write/read" (side writes what main reads) or "read/write"
    side: int
    main: int
    side_label: str
    main_label: str
    side_rect: Rect
    main_rect: Rect
    address: int
    nbytes: int

    def __str__(self):
        return (f"{self.kind}: side op {self.side} '{self.side_label}' {self.side_rect} and main op {self.main} '{self.main_label}' {self.main_rect} "
                f"share {self.nbytes} bytes at 0x{self.address:x}")


def hazards(ops, labels) -> Tuple[int, List[Hazard]]:
    """-> (concurrent pairs examined, hazards found)"""
    fps = {}

    def fp(i):
        if i not in fps:
            fps[i] = footprint(ops[i])
        return fps[i]
    pairs, found = concurrent_pairs(ops), []
    for s, m in pairs:
        (sr, sw), (mr, mw) = fp(s), fp(m)
        for kind, x, y in (("write/write", sw, mw), ("write/read", sw, mr), ("read/write", sr, mw)):
            o = regions_overlap(x, y)
            if o:
                found.append(Hazard(kind, s, m, labels[s], labels[m], o[0], o[1], o[2], o[3]))
    return len(pairs), found
