"""Static-graph builder: Python describes a network once, libmtx_hip executes it natively.

A `PlanBuilder` allocates activation buffers as torch tensors (PyTorch is only the allocator /
stream owner here) and records ops as `mtx_op` structs; `build()` hands the array to
`mtx_plan_create`.  `Plan.run()` is then one C call that launches every kernel of the network on
the caller's HIP stream (optionally as a hipGraph replay) — no Python in the per-layer loop.
"""
import contextlib
import threading
import ctypes as C
from dataclasses import dataclass
from typing import List, Optional

import torch

from ..utils.exceptions import ModelError
from . import abi

_TORCH_DT = {abi.BF16: torch.bfloat16, abi.F16: torch.float16, abi.F32: torch.float32}


def _ptr(t, offset_elems: int = 0) -> Optional[int]:
    if t is None:
        return None
    if isinstance(t, Act):
        return t.ptr
    return t.data_ptr() + offset_elems * t.element_size()


@dataclass
class Act:
    """Channels-last activation view: channels [c0, c0+c) of a [N, H, W, LD] buffer."""
    t: torch.Tensor
    n: int
    h: int
    w: int
    c: int
    c0: int = 0

    @property
    def ld(self) -> int:
        return self.t.shape[-1]

    @property
    def ptr(self) -> int:
        return self.t.data_ptr() + self.c0 * self.t.element_size()

    def slice(self, c0: int, c: int) -> "Act":
        assert c0 % 8 == 0 and c % 8 == 0 and c0 + c <= self.c
        return Act(self.t, self.n, self.h, self.w, c, self.c0 + c0)

    def torch(self) -> torch.Tensor:
        return self.t[..., self.c0:self.c0 + self.c]


class Plan:
    def __init__(self, lib, handle, keep, n_ops):
        self.lib = lib
        self._h = C.c_void_p(handle)
        self._keep = keep
        self.n_ops = n_ops

    def _dev(self):
        """the plan's own device (the HIP device is per thread and defaults to 0 — a worker thread of rank k must not launch this
        plan on device 0's stream); None = the thread's current device (plans built before `device` existed, CPU simulator)"""
        d = getattr(self, "device", None)
        return d if d is not None and getattr(d, "type", None) == "cuda" else None

    def _stream(self, stream):
        if stream is not None:
            return C.c_void_p(stream)
        if torch.cuda.is_available() and not self.lib.is_simulator:
            return C.c_void_p(torch.cuda.current_stream(self._dev()).cuda_stream)
        return C.c_void_p(0)

    def run(self, stream=None, graph: bool = False) -> None:
        if not graph or self.lib.is_simulator:
            self.lib.check(self.lib.mtx_plan_run(self._h, self._stream(stream)), "mtx_plan_run")
            return
        # hipGraph capture/replay needs a non-default stream: use a side stream owned by the
        # plan, ordered after the caller's current stream and joined back into it.
        if stream is not None:
            self.lib.check(self.lib.mtx_plan_run_graph(self._h, C.c_void_p(stream)), "mtx_plan_run_graph")
            return
        cur = torch.cuda.current_stream(self._dev())
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=cur.device)
        self._side.wait_stream(cur)
        self.lib.check(self.lib.mtx_plan_run_graph(self._h, C.c_void_p(self._side.cuda_stream)), "mtx_plan_run_graph")
        cur.wait_stream(self._side)

    def run_range(self, first: int, last: int, stream=None) -> None:
        self.lib.check(self.lib.mtx_plan_run_range(self._h, first, last, self._stream(stream)), "mtx_plan_run_range")

    def time(self, iters: int, graph: bool = False, stream=None) -> float:
        ms = C.c_float(0.0)
        if graph and stream is None and not self.lib.is_simulator:
            torch.cuda.synchronize()
            if getattr(self, "_side", None) is None:
                self._side = torch.cuda.Stream(device=self._dev())
            stream = self._side.cuda_stream
        self.lib.check(self.lib.mtx_plan_time(self._h, self._stream(stream), iters, int(graph), C.byref(ms)), "mtx_plan_time")
        return float(ms.value)

    def time_range(self, first: int, last: int, iters: int, stream=None) -> float:
        ms = C.c_float(0.0)
        self.lib.check(self.lib.mtx_plan_time_range(self._h, first, last, self._stream(stream), iters, C.byref(ms)), "mtx_plan_time_range")
        return float(ms.value)

    def time_ops(self, op_indices, iters: int = 1, stream=None) -> float:
        """in-context duration (ms) of the listed ops summed over `iters` measurements: graph replay of the whole plan minus graph
        replay without them, or (MTX_TIME_OPS=stamp) device wall-clock stamps around them inside one replay (include/mtx_hip.h)"""
        idx = (C.c_int * len(op_indices))(*[int(i) for i in op_indices])
        ms = C.c_float(0.0)
        self.lib.check(self.lib.mtx_plan_time_ops(self._h, self._stream(stream), idx, len(op_indices), iters, C.byref(ms)), "mtx_plan_time_ops")
        return float(ms.value)

    def close(self):
        """Destroys the native plan (its hipGraph exec, lane side stream and events) and releases the activation buffers.  The last
        replay may still be in flight on the plan's side stream when a cache evicts the plan, so the streams the plan ran on are
        drained first — destroying a graph exec / stream under running work relies on the runtime deferring it."""
        if self._h:
            if not self.lib.is_simulator and torch.cuda.is_available():
                side = getattr(self, "_side", None)
                if side is not None:
                    side.synchronize()
                torch.cuda.current_stream().synchronize()
            self.lib.mtx_plan_destroy(self._h)
            self._h = None
            self._keep = None          # the activation buffers go back to the allocator

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PlanCache:
    """shape-keyed plans with a bound: every plan pins its own activation buffers, and bubble crops / intermediate upscale passes come in
    arbitrary sizes, so an unbounded dict grows device memory with every new size.  Least recently used plans are destroyed — where the owner
    gave `may_evict(key, value)`, only entries it releases: the cache stays over its bound while the others are in use."""

    def __init__(self, capacity: int = 8, may_evict=None):
        from collections import OrderedDict
        self.capacity, self.may_evict, self._d = max(1, int(capacity)), may_evict, OrderedDict()

    def __contains__(self, key):
        return key in self._d

    def __len__(self):
        return len(self._d)

    def __getitem__(self, key):
        self._d.move_to_end(key)
        return self._d[key]

    def __setitem__(self, key, value):
        self._d[key] = value
        self._d.move_to_end(key)
        for k in list(self._d)[:-1]:           # oldest first; never the entry that was just set
            if len(self._d) <= self.capacity:
                break
            if self.may_evict is None or self.may_evict(k, self._d[k]):
                self._close(self._d.pop(k))

    @staticmethod
    def _close(old):
        for p in (old if isinstance(old, (tuple, list)) else (old,)):
            if hasattr(p, "close"):
                p.close()

    def get(self, key, default=None):
        return self[key] if key in self._d else default

    def items(self):
        return self._d.items()

    def values(self):
        return self._d.values()

    def clear(self):
        while self._d:
            self._close(self._d.popitem(last=False)[1])


class PlanBuilder:
    def __init__(self, lib, device, dtype: int = abi.BF16, lanes: bool = True):
        self.lib = lib
        self._lanes = lanes                     # False: `with pb.side()` records on the main lane (one in-order stream)
        self.device = torch.device(device)
        self.dtype = dtype
        self.tdtype = _TORCH_DT[dtype]
        self.ops: List[abi.Op] = []
        self._side, self._join_next = False, False
        self.labels: List[str] = []
        self.keep: list = []
        self.conv1x1_as_gemm = True             # 1x1 convolutions of >= 1024 pixels go to the GEMM kernels (round 4: detector graphs -15 %); False = the conv kernel, for A/Bs

    # ---- memory ---------------------------------------------------------------------------
    def hold(self, t):
        self.keep.append(t)
        return t

    def act(self, n, h, w, c, ld=None, zero=False) -> Act:
        ld = c if ld is None else ld
        assert ld % 8 == 0, "pixel stride must be a multiple of 8 elements"
        t = (torch.zeros if zero else torch.empty)((n, h, w, ld), dtype=self.tdtype, device=self.device)
        self.keep.append(t)
        return Act(t, n, h, w, c)

    def buf(self, shape, dtype=torch.float32, zero=False):
        t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device)
        self.keep.append(t)
        return t

    def const(self, t: torch.Tensor, dtype=None):
        t = t.detach().to(device=self.device, dtype=dtype if dtype is not None else t.dtype).contiguous()
        self.keep.append(t)
        return t

    # ---- op recording ---------------------------------------------------------------------
    # ---- lanes (include/mtx_hip.h, MTX_LANE_*): ops recorded inside `with pb.side():` go to the plan's side stream and run beside the
    # main ops recorded after the block; `pb.join()` makes the next main op wait for them
    def side(self):
        pb = self

        class _Side:
            def __enter__(self_):
                pb._side = pb._lanes

            def __exit__(self_, *exc):
                pb._side = False
        return _Side()

    def join(self):
        self._join_next = True

    def _add(self, kind: int, args, label: str) -> int:
        op = abi.Op()
        op.kind = kind
        op.lane = (abi.LANE_SIDE if self._side else 0) | (abi.LANE_JOIN if (self._join_next and not self._side) else 0)
        if self._join_next and not self._side:
            self._join_next = False
        setattr(op.u, abi.UNION_FIELD[kind], args)
        self.ops.append(op)
        self.labels.append(label)
        return len(self.ops) - 1

    def conv2d(self, x: Act, w_packed, bias, cout: int, ksize: int = 3, stride: int = 1,
               act: int = abi.ACT_NONE, act_param: float = 0.0, res: Optional[Act] = None,
               res_scale: float = 1.0, out: Optional[Act] = None, pixel_shuffle: int = 0,
               chan_sum=None, res_broadcast: bool = False, pad_mode: int = 0, act_after_res: bool = False,
               label: str = "conv", valid_hw=None, out_scale=None) -> Act:
        pad_total = 1 if pad_mode == 1 else 2 * (ksize // 2)
        ho = (x.h + pad_total - ksize) // stride + 1
        wo = (x.w + pad_total - ksize) // stride + 1
        if out is None:
            if pixel_shuffle:
                out = self.act(x.n, ho * pixel_shuffle, wo * pixel_shuffle, cout // (pixel_shuffle ** 2))
            else:
                out = self.act(x.n, ho, wo, cout)
        if (self.conv1x1_as_gemm and ksize == 1 and stride == 1 and not pixel_shuffle and chan_sum is None and not res_broadcast and valid_hw is None
                and out_scale is None and not act_after_res and res_scale == 1.0 and pad_mode == 0 and act_param == 0.0 and x.c % 8 == 0 and cout % 8 == 0
                and x.n * x.h * x.w >= 1024):
            # a 1x1 convolution over NHWC pixels IS a GEMM of the pixel rows ([n h w, ld] with K = Cin) against the packed filter [Cout, Cin]: the
            # MFMA GEMM kernels (fused bias / act / residual, output into a channel slice through ldc) serve it 2-3x faster than the halo-tile
            # conv kernel at detector shapes — YOLO11m-seg @1600 7.16 -> 6.10 ms, YOLO12x @640 10.6 -> 8.8 ms, config 2 34.0 -> 35.7 pages/s on
            # one box (profiles/r04_visit_n_conv1x1_as_gemm_ab.log); parity tests unchanged
            self.gemm(x, w_packed, x.n * x.h * x.w, cout, x.c, lda=x.ld, ldw=int(w_packed.shape[-1]), out=out, ldc=out.ld, bias=bias, act=act,
                      res=res, ldres=(res.ld if res is not None else None), label=label)
            return out
        a = abi.ConvArgs()
        a.x, a.w, a.bias = x.ptr, _ptr(w_packed), _ptr(bias)
        a.res = res.ptr if res is not None else None
        a.y = out.ptr
        a.chan_sum = _ptr(chan_sum)
        a.n, a.h, a.w_in, a.cin, a.cout = x.n, x.h, x.w, x.c, cout
        a.ksize, a.stride = ksize, stride
        a.ldx, a.ldy, a.ldres = x.ld, out.ld, (res.ld if res is not None else 0)
        a.act, a.act_param, a.res_scale = act, act_param, res_scale
        a.pixel_shuffle, a.dtype = pixel_shuffle, self.dtype
        a.res_broadcast_n = 1 if res_broadcast else 0
        a.pad_mode = pad_mode
        a.act_after_res = 1 if act_after_res else 0
        a.valid_hw = _ptr(valid_hw)
        a.out_scale = _ptr(out_scale)        # device [n][cout] f32: y = out_scale * act(conv + bias) + res_scale * res
        self._add(abi.OP_CONV2D, a, label)
        return out

    def conv_tiles(self, x: Act, ksize=3, stride=1, cout=None, with_res=False, with_scale=False, act=abi.ACT_NONE, pixel_shuffle=0) -> int:
        """rows per image of the chan_sum buffer the conv with these arguments fills (which kernel runs — hence how many partial rows it
        writes — depends on the channel counts, on whether a residual or output factors come with the sums, on the activation and the store form:
        pass what the conv2d call will pass)"""
        a = abi.ConvArgs()
        a.n, a.h, a.w_in, a.cin, a.cout, a.ksize, a.stride = x.n, x.h, x.w, x.c, (cout if cout is not None else x.c), ksize, stride
        a.ldx, a.ldy, a.dtype = x.ld, (cout if cout is not None else x.c), self.dtype
        a.chan_sum = x.ptr                       # non-null markers: only their presence matters here
        a.res = x.ptr if with_res else None
        a.ldres = a.ldy
        a.out_scale = x.ptr if with_scale else None
        a.act, a.pixel_shuffle = act, pixel_shuffle
        t = self.lib.mtx_conv2d_tiles(C.byref(a))
        if t < 0:
            raise ModelError(f"mtx_conv2d_tiles: {self.lib.last_error()}")
        return t

    def gemm(self, a_t, w_t, m, n, k, lda=None, ldw=None, out=None, ldc=None, bias=None, act=abi.ACT_NONE,
             res=None, ldres=None, gate=None, ldgate=None, gate_rows_per=1, alpha=1.0, batch=1,
             a_bs=0, w_bs=0, c_bs=0, res_bs=0, out_f32=False, a_off=0, w_off=0, c_off=0, res_off=0,
             label="gemm", f8=None, flags=0, glu=None, w_lo=None, res_f32=False, actq=None):
        """w_lo: the low half of a weight pair W = w_t + w_lo (same layout as w_t; mtx_gemm_args.w_lo).  res_f32: `res` is an fp32 matrix
        (needs out_f32; the fp32 residual stream of SAM's precision "high").
        f8 = (a_scale, lds_a, w_scale, lds_w, a_scale_off, w_scale_off): a_t / w_t are e4m3 byte matrices from `quantize` (offsets in
        bytes), the epilogue operands and the output stay in the builder's 16-bit type (include/mtx_hip.h, in_dtype == MTX_F8).
        glu = (q, scale, ldq, lds, col0, row_off, q_col_off): the columns from col0 on are [32 a | 32 b] spans (`glu_interleave` order of
        w's rows) and land as the MX fp8 matrix silu(a) * b in rows [row_off, row_off + m) of q / scale from byte column q_col_off on
        (mtx_gemm_args.glu_*); with col0 == 0 no 16-bit output exists at all
        actq = (q, scale, ldq, lds, row_off, q_col_off): act(alpha * acc + bias) of EVERY column lands as an MX fp8 matrix in rows
        [row_off, row_off + m) of q / scale from byte column q_col_off on (mtx_gemm_args.actq_*); no 16-bit `out` is needed or written"""
        g = abi.GemmArgs()
        g.flags = flags
        if actq is not None:
            aq, asc, aldq, alds, arow, aqcol = actq
            assert f8 is not None and glu is None and out is None and aqcol % 128 == 0
            g.actq_q, g.actq_scale = aq.data_ptr() + arow * aldq + aqcol, asc.data_ptr() + 4 * (arow + (aqcol // 128) * alds)
            g.actq_ldq, g.actq_lds = aldq, alds
        if glu is not None:
            gq, gsc, gldq, glds, gcol0, grow, gqcol = glu
            assert f8 is not None and gqcol % 128 == 0 and gcol0 % 256 == 0
            g.glu_q, g.glu_scale = gq.data_ptr() + grow * gldq + gqcol, gsc.data_ptr() + 4 * (grow + (gqcol // 128) * glds)
            g.glu_ldq, g.glu_lds, g.glu_col0 = gldq, glds, gcol0
            if out is None and gcol0 == 0:
                out = self.buf((8,), self.tdtype)          # never written: every tile takes the gated epilogue
        if f8 is not None:
            a_sc, lds_a, w_sc, lds_w, a_sc_off, w_sc_off = f8
            g.a_scale, g.w_scale = a_sc.data_ptr() + 4 * a_sc_off, w_sc.data_ptr() + 4 * w_sc_off
            g.lds_a, g.lds_w, g.in_dtype = lds_a, lds_w, abi.F8
        if out is None and actq is None:
            out = self.buf((batch, m, n) if batch > 1 else (m, n), torch.float32 if out_f32 else self.tdtype)
        g.a, g.w, g.c = _ptr(a_t, a_off), _ptr(w_t, w_off), (_ptr(out, c_off) if out is not None else None)
        g.bias, g.res, g.gate = _ptr(bias), _ptr(res, res_off), _ptr(gate)
        g.m, g.n, g.k = m, n, k
        g.lda, g.ldw, g.ldc = (lda or k), (ldw or k), (ldc or n)
        g.ldres, g.ldgate = (ldres or n), (ldgate or n)
        g.batch, g.a_bstride, g.w_bstride, g.c_bstride = batch, a_bs, w_bs, c_bs
        g.res_bstride = res_bs
        g.gate_rows_per = gate_rows_per
        g.act, g.act_param, g.alpha = act, 0.0, alpha
        g.dtype, g.out_dtype = self.dtype, (abi.F32 if out_f32 else self.dtype)
        if w_lo is not None:
            g.w_lo = _ptr(w_lo, w_off)
        if res_f32:
            assert out_f32 and res is not None
            g.res_dtype = abi.F32
        whole_tiles = (flags & abi.GEMM_FORCE_TILE256) and (flags & abi.GEMM_NO_SPLIT)      # forced onto whole 256-tiles: the scratch would never be used
        if ((m >= 2048 and n >= 1024 and k >= 512) or (m >= 256 and k >= 8192) or (flags & abi.GEMM_FORCE_TILE256)) and batch == 1 and not out_f32 and not whole_tiles:
            # large problems: one shared scratch per plan for the K-slice tail of the 256-tile kernel (ops of a plan run in order)
            # (side-lane ops run beside main-lane ops: they get a scratch of their own)
            ws_name = "_gemm_ws_side" if self._side else "_gemm_ws"
            if getattr(self, ws_name, None) is None:
                setattr(self, ws_name, self.buf((abi.GEMM_WORKSPACE_BYTES,), torch.uint8, zero=True))      # the tickets in its last 4 KiB start at zero
            g.workspace, g.workspace_bytes = getattr(self, ws_name).data_ptr(), abi.GEMM_WORKSPACE_BYTES
        self._add(abi.OP_GEMM, g, label)
        return out

    def attention(self, q, k, v, o, batch, heads, sq, sk, d, q_str, k_str, v_str, o_str, scale,
                  q_off=0, k_off=0, v_off=0, o_off=0, label="attn", q_prescaled=False, q8=None, qk_f8=None, pv_f8=None):
        """q8 = (q bytes [sq, ldq], scale plane [ldq / 128, lds], ldq, lds, byte column offset): the rows leave as the MX fp8 operand of the
        next linear instead of (o None) or beside 16-bit values — long-sequence kernel only (mtx_attn_args.q8).
        qk_f8 = (e4m3 bytes [rows, ld], q byte column, k byte column, ld, exponent): the scores are 2^exponent * q_f8 k_f8^T on the fp8
        matrix instruction (mtx_attn_args.q_f8 / k_f8; the rotary kernel's y8) — pre-scaled q, long-sequence kernel only"""
        a = abi.AttnArgs()
        a.flags = abi.ATTN_Q_PRESCALED if q_prescaled else 0
        a.q, a.k, a.v, a.o = _ptr(q, q_off), _ptr(k, k_off), _ptr(v, v_off), (_ptr(o, o_off) if o is not None else None)
        if q8 is not None:
            q8q, q8s, ldq, lds8, col = q8
            assert col % 128 == 0 and o is None
            a.q8, a.q8_scale, a.ldq8, a.lds_q8 = q8q.data_ptr() + col, q8s.data_ptr() + 4 * (col // 128) * lds8, ldq, lds8
        if qk_f8 is not None:
            t8, qc, kc, ld8, ex = qk_f8
            assert q_prescaled and t8.dtype == torch.uint8
            a.q_f8, a.k_f8, a.qf8_ss, a.kf8_ss, a.qk_f8_exp = t8.data_ptr() + qc, t8.data_ptr() + kc, ld8, ld8, ex
        if pv_f8 is not None:            # (e4m3 V^T [heads * 128, ld] as `v_f8t` writes it, ld): P V on the fp8 instruction too (mtx_attn_args.v_f8t)
            vt8, ld_v = pv_f8
            assert qk_f8 is not None and q8 is not None and vt8.dtype == torch.uint8
            a.v_f8t, a.vf8_ld = vt8.data_ptr(), ld_v
        a.batch, a.heads, a.sq, a.sk, a.d = batch, heads, sq, sk, d
        a.q_bs, a.q_ss, a.q_hs = q_str
        a.k_bs, a.k_ss, a.k_hs = k_str
        a.v_bs, a.v_ss, a.v_hs = v_str
        a.o_bs, a.o_ss, a.o_hs = o_str
        a.scale, a.dtype = scale, self.dtype
        if d == 128 and sq >= 1024 and sk >= 256:      # long sequences: scratch for the key-split tail (include/mtx_hip.h)
            ws = self.buf((abi.ATTN_WORKSPACE_BYTES,), torch.uint8)
            a.workspace, a.workspace_bytes = ws.data_ptr(), abi.ATTN_WORKSPACE_BYTES
        self._add(abi.OP_ATTN, a, label)
        return o

    def decode_attention(self, qkv, k_cache, v_cache, pos, src, o, rows, slots, heads, d, max_len, scale, ld_qkv=None, ld_o=None,
                         label="decode_attn"):
        """MTX_OP_DECODE_ATTN: one query per (row, head) over the caches [max_len, slots, heads * d]; `pos` (int32 scalar) and `src` (int32
        [max_len, slots], the slot that holds row r's history at position j) live on the device, so the recorded op serves every step"""
        a = abi.DecodeAttnArgs()
        a.qkv, a.k_cache, a.v_cache, a.pos, a.src, a.o = _ptr(qkv), _ptr(k_cache), _ptr(v_cache), _ptr(pos), _ptr(src), _ptr(o)
        a.rows, a.slots, a.heads, a.d, a.max_len = rows, slots, heads, d, max_len
        a.ld_qkv, a.ld_o = (ld_qkv or 3 * heads * d), (ld_o or heads * d)
        a.scale, a.dtype = scale, self.dtype
        self._add(abi.OP_DECODE_ATTN, a, label)
        return o

    def causal_attention(self, qkv, k_cache, v_cache, pos, o, rows, heads, kv_heads, d, max_len, scale, ld_qkv=None, ld_o=None,
                         workspace=None, label="causal_attn"):
        """MTX_OP_CAUSAL_ATTN: causal grouped-query attention of `rows` new rows [q | k | v] that appends them to the caches [max_len,
        kv_heads * d]; `pos` (int32, positions already cached) lives on the device, so the recorded op serves every step.  The step (rows == 1)
        merges its key splits through a zeroed workspace, made here unless one is passed (layers of one plan may share it: they run in order)"""
        a = abi.CausalAttnArgs()
        a.qkv, a.k_cache, a.v_cache, a.pos, a.o = _ptr(qkv), _ptr(k_cache), _ptr(v_cache), _ptr(pos), _ptr(o)
        a.rows, a.heads, a.kv_heads, a.d, a.max_len = rows, heads, kv_heads, d, max_len
        a.ld_qkv, a.ld_o = (ld_qkv or (heads + 2 * kv_heads) * d), (ld_o or heads * d)
        a.scale, a.dtype = scale, self.dtype
        if rows == 1:
            need = abi.causal_ws_bytes(heads, max_len)
            if workspace is None:
                workspace = self.buf((need,), torch.uint8, zero=True)
            assert workspace.numel() * workspace.element_size() >= need
            a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
        self._add(abi.OP_CAUSAL_ATTN, a, label)
        return o

    def greedy_pick(self, logits, state, out, vocab, max_new, eos=(), advance=1, label="greedy_pick"):
        """MTX_OP_GREEDY: the device end of a greedy step on fp32 `logits` [vocab].  `state` (int32 [4] = pos, n_out, done, token) and `out`
        (int32 [max_new]) live on the device; unless done: out[n_out++] = token = arg max (lowest index among equals), pos += advance,
        done = token in eos or n_out == max_new"""
        eos = [int(e) for e in eos]
        assert len(eos) <= 4 and logits.dtype == torch.float32 and state.dtype == torch.int32 and out.dtype == torch.int32
        a = abi.GreedyArgs()
        scratch = self.buf((max(abi.greedy_scratch_bytes(vocab), 8),), torch.uint8)
        a.logits, a.state, a.out, a.scratch = _ptr(logits), _ptr(state), _ptr(out), scratch.data_ptr()
        a.vocab, a.max_new, a.n_eos, a.advance = vocab, max_new, len(eos), advance
        for i, e in enumerate(eos):
            a.eos[i] = e
        self._add(abi.OP_GREEDY, a, label)
        return state

    def causal_step_batch(self, qkv, k_cache, v_cache, state, o, slots, heads, kv_heads, d, max_len, scale, cache_stride=None, ld_qkv=None,
                          ld_o=None, workspace=None, label="causal_step_batch"):
        """MTX_OP_CAUSAL_STEP_BATCH: the rows == 1 step of `causal_attention` for `slots` sequences in one launch.  qkv [slots, ld_qkv],
        o [slots, ld_o], caches [slots, max_len, kv_heads * d] (slot stride `cache_stride` elements); `state` is the int32
        [SLOT_FIELDS, SLOTS_MAX] block: a slot with done != 0 or pos outside [0, max_len) sits out.  One zeroed workspace of
        slots * causal_ws_bytes, made here unless one is passed (layers of one plan may share it: they run in order)"""
        assert state.dtype == torch.int32 and state.numel() >= abi.SLOT_FIELDS * abi.SLOTS_MAX and state.is_contiguous()
        a = abi.CausalStepBatchArgs()
        a.qkv, a.k_cache, a.v_cache, a.state, a.o = _ptr(qkv), _ptr(k_cache), _ptr(v_cache), _ptr(state), _ptr(o)
        a.slots, a.heads, a.kv_heads, a.d, a.max_len = slots, heads, kv_heads, d, max_len
        a.ld_qkv, a.ld_o = (ld_qkv or (heads + 2 * kv_heads) * d), (ld_o or heads * d)
        a.cache_stride = cache_stride if cache_stride is not None else max_len * kv_heads * d
        a.scale, a.dtype = scale, self.dtype
        need = max(slots, 0) * abi.causal_ws_bytes(heads, max_len)
        if workspace is None:
            workspace = self.buf((max(need, 16),), torch.uint8, zero=True)
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
        self._add(abi.OP_CAUSAL_STEP_BATCH, a, label)
        return o

    def greedy_pick_batch(self, logits, state, out, slots, vocab, max_new, eos=(), advance=1, ld_logits=None, label="greedy_pick_batch"):
        """MTX_OP_GREEDY_BATCH: `greedy_pick` for `slots` rows of fp32 `logits` [slots, ld_logits] into `out` [slots, max_new] on the int32
        [SLOT_FIELDS, SLOTS_MAX] state block; a slot that advances also moves its rotary row by `advance`"""
        eos = [int(e) for e in eos]
        assert len(eos) <= 4 and logits.dtype == torch.float32 and state.dtype == torch.int32 and out.dtype == torch.int32
        a = abi.GreedyBatchArgs()
        scratch = self.buf((max(max(slots, 1) * abi.greedy_scratch_bytes(max(vocab, 1)), 8),), torch.uint8)
        a.logits, a.state, a.out, a.scratch = _ptr(logits), _ptr(state), _ptr(out), scratch.data_ptr()
        a.ld_logits = ld_logits if ld_logits is not None else vocab
        a.slots, a.vocab, a.max_new, a.n_eos, a.advance = slots, vocab, max_new, len(eos), advance
        for i, e in enumerate(eos):
            a.eos[i] = e
        self._add(abi.OP_GREEDY_BATCH, a, label)
        return state

    def segment_attention(self, q, k, v, o, seg, heads, d, cap_rows, q_str, k_str, v_str, o_str, scale, q_off=0, k_off=0, v_off=0, o_off=0,
                          label="seg_attn"):
        """MTX_OP_SEG_ATTN: non-causal attention over up to SEGS_MAX sequences packed row-wise into [cap_rows] rows; `seg` (int32
        [SEGS_MAX + 1] row offsets) lives on the device, so the recorded op serves every combination of lengths.  *_str = (row stride, head
        stride) in elements.  A segment's rows are bit for bit `attention`'s (batch 1, short kernel) on that segment alone"""
        assert seg.dtype == torch.int32 and seg.numel() >= abi.SEGS_MAX + 1 and seg.is_contiguous()
        a = abi.SegAttnArgs()
        a.q, a.k, a.v, a.o, a.seg = _ptr(q, q_off), _ptr(k, k_off), _ptr(v, v_off), _ptr(o, o_off), _ptr(seg)
        a.heads, a.d, a.cap_rows = heads, d, cap_rows
        a.q_ss, a.q_hs = q_str
        a.k_ss, a.k_hs = k_str
        a.v_ss, a.v_hs = v_str
        a.o_ss, a.o_hs = o_str
        a.scale, a.dtype = scale, self.dtype
        self._add(abi.OP_SEG_ATTN, a, label)
        return o

    def causal_prefill_slots(self, qkv, k_cache, v_cache, seg, o, cap_rows, heads, kv_heads, d, max_len, scale, cache_stride=None, ld_qkv=None,
                             ld_o=None, label="causal_prefill_slots"):
        """MTX_OP_CAUSAL_PREFILL_SLOTS: the rows > 1 path of `causal_attention` for up to SLOTS_MAX prompts packed into qkv [cap_rows, ld_qkv],
        prompt s = rows [seg[s], seg[s + 1]) into the EMPTY slot cache s of [slots, max_len, kv_heads * d] (slot stride `cache_stride`
        elements); `seg` (int32 [SLOTS_MAX + 1]) lives on the device.  An empty segment leaves its slot alone"""
        assert seg.dtype == torch.int32 and seg.numel() >= abi.SLOTS_MAX + 1 and seg.is_contiguous()
        a = abi.CausalPrefillSlotsArgs()
        a.qkv, a.k_cache, a.v_cache, a.seg, a.o = _ptr(qkv), _ptr(k_cache), _ptr(v_cache), _ptr(seg), _ptr(o)
        a.cap_rows, a.heads, a.kv_heads, a.d, a.max_len = cap_rows, heads, kv_heads, d, max_len
        a.ld_qkv, a.ld_o = (ld_qkv or (heads + 2 * kv_heads) * d), (ld_o or heads * d)
        a.cache_stride = cache_stride if cache_stride is not None else max_len * kv_heads * d
        a.scale, a.dtype = scale, self.dtype
        self._add(abi.OP_CAUSAL_PREFILL_SLOTS, a, label)
        return o

    def rel_attention(self, q, k, v, o, s, heads, kv_heads, d, q_str, k_str, v_str, o_str, scale, rel=None, ld_rel=None, n_keys=None,
                      q_off=0, k_off=0, v_off=0, o_off=0, label="rel_attn"):
        """MTX_OP_REL_ATTN: attention of `s` rows with the additive bias rel[h][j - i + s - 1] (fp32 [heads, ld_rel >= 2 s - 1]; an entry at or
        below abi.REL_MASKED masks the key; None = no bias) over the keys j < min(s, n_keys); `n_keys` (int32 scalar) lives on the device, so
        the recorded op serves every prompt length.  *_str = (row stride, head stride) in elements; k and v hold `kv_heads` heads"""
        a = abi.RelAttnArgs()
        a.q, a.k, a.v, a.o = _ptr(q, q_off), _ptr(k, k_off), _ptr(v, v_off), _ptr(o, o_off)
        if rel is not None:
            assert rel.dtype == torch.float32 and rel.dim() == 2 and rel.shape[0] == heads and rel.stride(1) == 1
            a.rel, a.ld_rel = _ptr(rel), (ld_rel if ld_rel is not None else rel.stride(0))
        if n_keys is not None:
            assert n_keys.dtype == torch.int32
            a.n_keys = _ptr(n_keys)
        a.heads, a.kv_heads, a.s, a.d = heads, kv_heads, s, d
        a.q_ss, a.q_hs = q_str
        a.k_ss, a.k_hs = k_str
        a.v_ss, a.v_hs = v_str
        a.o_ss, a.o_hs = o_str
        a.scale, a.dtype = scale, self.dtype
        self._add(abi.OP_REL_ATTN, a, label)
        return o

    def row_linear(self, a_t, w_t, rows, n, k, lda=None, ldw=None, out=None, ldc=None, bias=None, act=abi.ACT_NONE, res=None, ldres=None,
                   alpha=1.0, out_f32=False, label="rowlin"):
        """MTX_OP_ROWLIN: the skinny-row (rows <= 8) linear of a decode step, same epilogue and rounding contract as `gemm`"""
        if out is None:
            out = self.buf((rows, n), torch.float32 if out_f32 else self.tdtype)
        g = abi.RowLinArgs()
        g.a, g.w, g.bias, g.res, g.c = _ptr(a_t), _ptr(w_t), _ptr(bias), _ptr(res), _ptr(out)
        g.rows, g.n, g.k = rows, n, k
        g.lda, g.ldw, g.ldc, g.ldres = (lda or k), (ldw or k), (ldc or n), (ldres or n)
        g.act, g.act_param, g.alpha = act, 0.0, alpha
        g.dtype, g.out_dtype = self.dtype, (abi.F32 if out_f32 else self.dtype)
        self._add(abi.OP_ROWLIN, g, label)
        return out

    def row_linear_wide(self, a_t, w_t, rows, n, k, lda=None, ldw=None, out=None, ldc=None, bias=None, act=abi.ACT_NONE, res=None, ldres=None,
                        alpha=1.0, out_f32=False, label="rowlin_wide"):
        """MTX_OP_ROWLIN_WIDE: `row_linear` for up to 32 rows; the weights are read once per launch and every row is bit for bit the single
        op's"""
        if out is None:
            out = self.buf((rows, n), torch.float32 if out_f32 else self.tdtype)
        g = abi.RowLinArgs()
        g.a, g.w, g.bias, g.res, g.c = _ptr(a_t), _ptr(w_t), _ptr(bias), _ptr(res), _ptr(out)
        g.rows, g.n, g.k = rows, n, k
        g.lda, g.ldw, g.ldc, g.ldres = (lda or k), (ldw or k), (ldc or n), (ldres or n)
        g.act, g.act_param, g.alpha = act, 0.0, alpha
        g.dtype, g.out_dtype = self.dtype, (abi.F32 if out_f32 else self.dtype)
        self._add(abi.OP_ROWLIN_WIDE, g, label)
        return out

    def decode_attention_batch(self, qkv, k_cache, v_cache, state, o, groups, beams, heads, d, max_len, scale, cache_stride=None, src=None,
                               src_stride=None, state_stride=None, ld_qkv=None, ld_o=None, label="decode_attn_batch"):
        """MTX_OP_DECODE_ATTN_BATCH: `decode_attention` for `groups` groups of `beams` rows, each group at the position its state block
        holds.  qkv [groups * beams, ld_qkv], o [groups * beams, ld_o], caches [groups, max_len, beams, heads * d]; `state` is the int32
        [groups, state_stride] block of `beam_step` (a group with done != 0 or pos outside [0, max_len) sits out); the ancestry tables are
        the block's own unless `src` [groups, max_len, beams] is given"""
        assert state.dtype == torch.int32 and state.is_contiguous()
        words = abi.beam_state_words(beams, max_len)
        a = abi.DecodeAttnBatchArgs()
        a.qkv, a.k_cache, a.v_cache, a.state, a.o = _ptr(qkv), _ptr(k_cache), _ptr(v_cache), _ptr(state), _ptr(o)
        a.state_stride = state_stride if state_stride is not None else words
        if src is None:
            a.src, a.src_stride = state.data_ptr() + 4 * abi.beam_src(beams, max_len), a.state_stride
        else:
            assert src.dtype == torch.int32
            a.src, a.src_stride = _ptr(src), (src_stride if src_stride is not None else max_len * beams)
        a.groups, a.beams, a.heads, a.d, a.max_len = groups, beams, heads, d, max_len
        a.ld_qkv, a.ld_o = (ld_qkv or 3 * heads * d), (ld_o or heads * d)
        a.cache_stride = cache_stride if cache_stride is not None else max_len * beams * heads * d
        a.scale, a.dtype = scale, self.dtype
        self._add(abi.OP_DECODE_ATTN_BATCH, a, label)
        return o

    def beam_step(self, logits, state, tok_idx, pos_idx, len_pow, groups, beams, vocab, max_len, max_length, eos, ngram=0, early=False,
                  lp_positive=True, ld_logits=None, state_stride=None, label="beam_step"):
        """MTX_OP_BEAM_STEP: one iteration of `beam_search` (core/ml/manga_ocr.py) per group with done == 0, on fp32 `logits`
        [groups * beams, ld_logits] and the int32 [groups, state_stride] state block; writes the next token and position of every row to
        `tok_idx` / `pos_idx`.  `len_pow`: fp32 [max_len], float32(float(j) ** length_penalty) for j = 1 ..; early: False, True or "never"."""
        eos = [int(e) for e in eos]
        assert len(eos) <= 4 and logits.dtype == torch.float32 and state.dtype == torch.int32 and state.is_contiguous()
        assert tok_idx.dtype == torch.int32 and pos_idx.dtype == torch.int32 and len_pow.dtype == torch.float32
        a = abi.BeamStepArgs()
        keep = abi.beam_keep(beams, len(eos))
        scratch = self.buf((max(abi.beam_scratch_bytes(max(groups * beams, 1), max(vocab, 1), keep), 16),), torch.uint8)
        a.logits, a.state, a.tok_idx, a.pos_idx, a.len_pow, a.scratch = (_ptr(logits), _ptr(state), _ptr(tok_idx), _ptr(pos_idx), _ptr(len_pow),
                                                                           scratch.data_ptr())
        a.ld_logits = ld_logits if ld_logits is not None else vocab
        a.state_stride = state_stride if state_stride is not None else abi.beam_state_words(beams, max_len)
        a.groups, a.beams, a.vocab, a.max_len, a.max_length, a.n_eos, a.ngram = groups, beams, vocab, max_len, max_length, len(eos), ngram
        a.early = 2 if early == "never" else (1 if early is True or early == 1 else 0)
        a.lp_positive = 1 if lp_positive else 0
        for i, e in enumerate(eos):
            a.eos[i] = e
        self._add(abi.OP_BEAM_STEP, a, label)
        return state

    def v_f8t(self, v, rows, heads, ldv, v_off=0, out=None, label="v_f8t"):
        """MTX_EW_V_F8T: the value rows [rows, heads * 128] (16-bit, row stride ldv) as e4m3 V^T [heads * 128, ld] with ld = rows padded to 64, keys in
        accumulator order inside every 64-key tile — the operand of `attention(pv_f8=...)`.  -> (tensor, ld)"""
        ld = (rows + 63) // 64 * 64
        if out is None:
            out = self.buf((heads * 128, ld), torch.uint8, zero=True)
        self._ew_args(label, abi.EW_V_F8T, _ptr(v, v_off), None, (1, 1, rows, heads * 128), lda=ldv, y8=(out.data_ptr(), ld, 0.0))
        return out, ld

    def norm(self, x, y, rows, c, ldx=None, ldy=None, gamma=None, beta=None, eps=1e-6, kind=0,
             mod_scale=None, mod_shift=None, rows_per=0, ldmod=0, x_off=0, y_off=0, act=abi.ACT_NONE,
             label="norm", q8=None, q_row_off=0, lds_q=0, dtype=None, out_dtype=None):
        """out_dtype (dtype = abi.F32 only): the type y is written in — None = fp32, abi.BF16 / abi.F16 = rounded once to the next linear's operand type.
        q8 = (q bytes [R, c], scale plane [c / 128, lds_q]): also (or, with y None, only) the MX fp8 twin of the result, rows landing
        at q_row_off (include/mtx_hip.h mtx_norm_args.q)"""
        a = abi.NormArgs()
        a.x, a.y = _ptr(x, x_off), (_ptr(y, y_off) if y is not None else None)
        if q8 is not None:
            a.q, a.q_scale = q8[0].data_ptr() + q_row_off * c, q8[1].data_ptr() + 4 * q_row_off
            a.ldq, a.lds_q = c, lds_q
        a.gamma, a.beta = _ptr(gamma), _ptr(beta)
        a.mod_scale, a.mod_shift = _ptr(mod_scale), _ptr(mod_shift)
        a.rows, a.c, a.ldx, a.ldy = rows, c, (ldx or c), (ldy or c)
        a.rows_per, a.ldmod = rows_per, ldmod
        a.eps, a.kind, a.dtype, a.act = eps, kind, (self.dtype if dtype is None else dtype), act      # dtype = abi.F32: an fp32 op inside a 16-bit plan
        a.out_dtype = a.dtype if out_dtype is None else out_dtype
        self._add(abi.OP_NORM, a, label)
        return y

    def groupnorm(self, x: Act, gamma, beta, groups=32, eps=1e-6, act=abi.ACT_NONE, out=None, label="gn") -> Act:
        assert x.c == x.ld and x.c0 == 0, "groupnorm needs a dense NHWC tensor"
        if out is None:
            out = self.act(x.n, x.h, x.w, x.c)
        ws = self.buf((abi.groupnorm_ws_floats(x.n, x.h * x.w, x.c, groups),), torch.float32)
        a = abi.GroupNormArgs()
        a.x, a.y, a.gamma, a.beta, a.workspace = x.ptr, out.ptr, _ptr(gamma), _ptr(beta), _ptr(ws)
        a.n, a.hw, a.c, a.groups = x.n, x.h * x.w, x.c, groups
        a.eps, a.act, a.dtype = eps, act, self.dtype
        self._add(abi.OP_GROUPNORM, a, label)
        return out

    def _ew_args(self, label, kind, a, y, nhwc, b=None, s=None, lda=0, ldb=0, ldy=0, lds=0, act=0, act_param=0.0, i0=0, i1=0, dtype=None, y8=None):
        """one MTX_OP_EW op: the argument block (include/mtx_hip.h mtx_ew_args) filled from pointers and numbers; what is not given stays zero.
        dtype: None = the builder's; y8 = (pointer, ldy8, y8_mul)"""
        e = abi.EwArgs()
        e.a, e.b, e.s, e.y = a, b, s, y
        e.n, e.h, e.w, e.c = nhwc
        e.lda, e.ldb, e.ldy, e.lds = lda, ldb, ldy, lds
        e.kind, e.act, e.act_param, e.i0, e.i1, e.dtype = kind, act, act_param, i0, i1, (self.dtype if dtype is None else dtype)
        if y8 is not None:
            e.y8, e.ldy8, e.y8_mul = y8
        self._add(abi.OP_EW, e, label)

    def ew(self, kind, a_: Act, b: Optional[Act] = None, s=None, out: Optional[Act] = None, lds=0,
           act=abi.ACT_NONE, act_param=0.0, i0=0, i1=0, label="ew", dtype=None) -> Act:
        if out is None:
            if kind == abi.EW_UPSAMPLE2X:
                out = self.act(a_.n, a_.h * 2, a_.w * 2, a_.c)
            elif kind == abi.EW_AVGPOOL2:
                out = self.act(a_.n, (a_.h + 1) // 2, (a_.w + 1) // 2, a_.c)
            elif kind == abi.EW_MAXPOOL:
                pd = i0 // 2 if i0 % 2 else 0
                out = self.act(a_.n, (a_.h + 2 * pd - i0) // i1 + 1, (a_.w + 2 * pd - i0) // i1 + 1, a_.c)
            else:
                out = self.act(a_.n, a_.h, a_.w, a_.c)
        self._ew_args(label, kind, a_.ptr, out.ptr, (a_.n, a_.h, a_.w, a_.c), b=(b.ptr if b is not None else None), s=_ptr(s), lda=a_.ld,
                      ldb=(b.ld if b is not None else 0), ldy=out.ld, lds=lds, act=act, act_param=act_param, i0=i0, i1=i1, dtype=dtype)
        return out

    def qk_norm_rope(self, qk: Act, cs, ld_cs, gamma_qk, d, heads, eps=1e-6, y8=None, label="qk_norm_rope"):
        """MTX_EW_QK_NORM_ROPE in place over `qk`, the q | k column view ([rows, 2 * heads * d]) of some token rows: per-head RMSNorm (gamma_qk
        fp32 [2 d]: q's vector, then k's) and the rotary turn.  cs: fp32 [rows][2][d / 2] cos | sin rows of the same tokens; the q heads read
        the copy ld_cs floats behind it (pre-multiplied by softmax scale * log2(e), MTX_ATTN_Q_PRESCALED).
        y8 = (e4m3 bytes of the same rows, ldy8, q multiplier): also the plain e4m3 twin of the result (mtx_ew_args.y8; `attention(qk_f8=...)`)"""
        self._ew_args(label, abi.EW_QK_NORM_ROPE, qk.ptr, qk.ptr, (1, 1, qk.w, qk.c), b=_ptr(cs), s=_ptr(gamma_qk), lda=qk.ld, ldb=ld_cs, ldy=qk.ld,
                      act_param=eps, i0=d, i1=heads, y8=None if y8 is None else (_ptr(y8[0]), y8[1], y8[2]))

    def qk_rope(self, qk: Act, cs, d, q_heads=0, ld_cs=0, label="qk_rope"):
        """MTX_EW_QK_ROPE in place over `qk`, the q | k column view ([rows, 2 * heads * d]) of some token rows: the rotary turn on interleaved
        pairs, nothing else.  cs: fp32 [rows][2][d / 2] cos | sin rows of the same tokens; with ld_cs > 0 the first `q_heads` heads read the copy
        ld_cs floats behind it (pre-multiplied by softmax scale * log2(e): the attention then runs with `q_prescaled`)"""
        self._ew_args(label, abi.EW_QK_ROPE, qk.ptr, qk.ptr, (1, 1, qk.w, qk.c), b=_ptr(cs), lda=qk.ld, ldb=ld_cs, ldy=qk.ld, i0=d, i1=q_heads)

    def residual_dist(self, after, before, prev, rows, c, parts=None, after_off=0, before_off=0, ld=None, label="residual_dist"):
        """first-block cache probe (include/mtx_hip.h MTX_EW_RESIDUAL_DIST): r = after - before (rounded to the storage type) against `prev`;
        -> fp32 [RESDIST_PARTS, 2]: per part (sum |prev - r|, sum |prev|); `residual_distance(parts)` adds them in index order"""
        if parts is None:
            parts = self.buf((abi.RESDIST_PARTS, 2), torch.float32, zero=True)
        self._ew_args(label, abi.EW_RESIDUAL_DIST, _ptr(after, after_off), parts.data_ptr(), (1, 1, rows, c), b=_ptr(before, before_off), s=_ptr(prev),
                      lda=(ld or c), ldb=(ld or c), ldy=2, lds=c)
        return parts

    def dwconv(self, x: Act, w_taps, bias, ksize: int, act=abi.ACT_NONE, out: Optional[Act] = None, label="dwconv") -> Act:
        """depthwise k x k, stride 1 (include/mtx_hip.h MTX_EW_DWCONV): w_taps T [k*k, C], bias fp32 [C] or None"""
        if out is None:
            out = self.act(x.n, x.h, x.w, x.c)
        self._ew_args(label, abi.EW_DWCONV, x.ptr, out.ptr, (x.n, x.h, x.w, x.c), b=_ptr(bias), s=_ptr(w_taps), lda=x.ld, ldy=out.ld, act=act, i0=ksize)
        return out

    def channel_attention(self, chan_sum, w1, b1, w2, b2, s_out, n, tiles, c, cr, inv_hw, label="ca", inv_hw_dev=None,
                          before_conv=None, valid_hw=None, split=True):
        """before_conv = (t: Act, conv_w_packed, conv_bias): chan_sum holds the sums of t and the factors are those of
        mean(conv3x3(t) + bias) — available before that conv runs (include/mtx_hip.h, mtx_ca_args.t)"""
        a = abi.CaArgs()
        a.inv_hw_dev = _ptr(inv_hw_dev)
        a.chan_sum, a.w1, a.b1, a.w2, a.b2, a.s = (_ptr(chan_sum), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(s_out))
        a.n, a.tiles, a.c, a.cr, a.inv_hw = n, tiles, c, cr, inv_hw
        if before_conv is not None:
            t, cw, cb = before_conv
            a.t, a.conv_w, a.conv_b = t.ptr, _ptr(cw), _ptr(cb)
            a.h, a.w, a.ldt, a.dtype = t.h, t.w, t.ld, self.dtype
            a.valid_hw = _ptr(valid_hw)
            if split:
                # MTX_CA_SPLIT workgroups per image: partial records + arrival counters (zero once; every launch leaves them zero).
                # One scratch per builder and image count: the ops of a plan run one after the other.
                key = f"_ca_scratch_{n}"
                if getattr(self, key, None) is None:
                    setattr(self, key, self.buf((abi.ca_scratch_bytes(n) // 4,), torch.float32, zero=True))
                a.scratch = getattr(self, key).data_ptr()
        self._add(abi.OP_CA, a, label)
        return s_out

    def image_convert(self, kind, src, dst, n, h, w, c_pad, unshuffle=1, mul=1.0, add=(0.0, 0.0, 0.0), label="img", valid_hw=None):
        a = abi.ImgArgs()
        a.valid_hw = _ptr(valid_hw)
        a.src, a.dst = _ptr(src), _ptr(dst)
        a.n, a.h, a.w, a.c_pad, a.unshuffle, a.mul = n, h, w, c_pad, unshuffle, mul
        for i in range(3):
            a.add[i] = float(add[i])
        a.add[3] = 0.0
        a.kind, a.dtype = kind, self.dtype
        self._add(abi.OP_IMG, a, label)
        return dst

    def row_gather(self, src, dst, index_i32, rows, c, lda=None, ldy=None, label="row_gather", dtype=None):
        """dst[r, :c] = src[index[r], :c]  (token re-ordering between window layouts)"""
        self._ew_args(label, abi.EW_ROW_GATHER, _ptr(src), _ptr(dst), (1, 1, rows, c), s=_ptr(index_i32), lda=(lda or c), ldy=(ldy or c), dtype=dtype)
        return dst

    # ---- fp32 ops (csrc/f32ops.hip) --------------------------------------------------------------------------------------------------
    def cvt16(self, src_f32, dst16, rows, c, copies=1, lda=None, label="cvt16"):
        """dst16 [rows, >= copies * c] (this builder's 16-bit type) <- src_f32 [rows, c] rounded, written `copies` times side by side"""
        assert self.dtype in (abi.F16, abi.BF16) and src_f32.dtype == torch.float32 and dst16.dtype == self.tdtype
        self._ew_args(label, abi.EW_CVT_16, _ptr(src_f32), _ptr(dst16), (1, 1, rows, c), lda=(lda or c), ldy=dst16.shape[-1], i0=self.dtype, i1=copies, dtype=abi.F32)
        return dst16

    def cvt_f32(self, x: Act, src_dtype: int, label="cvt_f32", out: Optional[Act] = None) -> Act:
        """fp32 copy of a 16-bit activation (`src_dtype` = its abi dtype); `out`: an fp32 activation of the same shape to write into"""
        if out is None:
            out = self.act(x.n, x.h, x.w, x.c) if self.dtype == abi.F32 else Act(self.buf((x.n, x.h, x.w, x.c), torch.float32), x.n, x.h, x.w, x.c)
        self._ew_args(label, abi.EW_CVT_F32, x.ptr, out.ptr, (x.n, x.h, x.w, x.c), lda=x.ld, ldy=out.ld, i0=src_dtype, dtype=abi.F32)
        return out

    def shuffle2_add(self, cols, n, h, w, c, skip: Optional[Act] = None, skip_broadcast: bool = True, label="shuffle2_add") -> Act:
        """`cols` [n*h*w, 4c]: the four output pixels of every input pixel side by side (a ConvTranspose2d(k=2, s=2) computed as a GEMM) ->
        [n, 2h, 2w, c] plus an optional skip feature at output resolution (one image for every n when `skip_broadcast`)"""
        assert self.dtype == abi.F32
        out = self.act(n, 2 * h, 2 * w, c)
        self._ew_args(label, abi.EW_SHUFFLE2_ADD, _ptr(cols), out.ptr, (n, h, w, c), b=(skip.ptr if skip is not None else None), lda=4 * c,
                      ldb=(skip.ld if skip is not None else 0), ldy=out.ld, lds=0 if (skip is None or skip_broadcast) else 4 * h * w * skip.ld, dtype=abi.F32)
        return out

    def im2col(self, x: Act, dst, k, stride, ldy, row_map=None, label="im2col", pad=True):
        """pad: taps reach k / 2 pixels beyond the image (a padded convolution); False = MTX_EW_IM2COL_PATCH, patches inside the image only"""
        self._ew_args(label, abi.EW_IM2COL if pad else abi.EW_IM2COL_PATCH, x.ptr, _ptr(dst), (x.n, x.h, x.w, x.c), s=_ptr(row_map), lda=x.ld, ldy=ldy, i0=k, i1=stride)
        return dst

    def mask_select(self, logits, iou, counts, sel, n, pix, delta=0.05, thresh=0.98, label="mask_select"):
        a = abi.MaskSelectArgs()
        a.logits, a.iou, a.counts, a.sel = _ptr(logits), _ptr(iou), _ptr(counts), _ptr(sel)
        a.n, a.pix, a.delta, a.thresh = n, pix, delta, thresh
        self._add(abi.OP_MASK_SELECT, a, label)

    def preprocess(self, src_u8, dst: "Act", h, w, mean, std, label="preprocess"):
        a = abi.PreprocArgs()
        a.src, a.dst = _ptr(src_u8), dst.ptr
        a.h, a.w, a.oh, a.ow, a.c_pad = h, w, dst.h, dst.w, dst.ld
        for i in range(3):
            a.mean[i], a.std[i] = float(mean[i]), float(std[i])
        a.dtype = self.dtype
        self._add(abi.OP_PREPROC, a, label)
        return dst

    def resample_u8(self, src_u8, dst_u8, out_h, out_w, c, ld_src, ld_dst, bounds_i32, taps_i32, ksize, axis, coeff_bits=0, src_row0=0, label="resample"):
        """one axis of a fixed-point 8-bit resampling pass (mtx_tail_args, MTX_TAIL_RESAMPLE): Pillow's (coeff_bits 0 = 22) or ATen's"""
        a = abi.TailArgs()
        a.kind, a.src, a.dst = abi.TAIL_RESAMPLE, _ptr(src_u8), _ptr(dst_u8)
        a.out_h, a.out_w, a.c, a.ld_src, a.ld_dst = out_h, out_w, c, ld_src, ld_dst
        a.bounds, a.coeff, a.ksize, a.axis, a.src_row0, a.coeff_bits = _ptr(bounds_i32), _ptr(taps_i32), ksize, axis, src_row0, coeff_bits
        self._add(abi.OP_TAIL, a, label)
        return dst_u8

    def letterbox(self, src_u8, dst: "Act", h, w, new_h, new_w, pad_top, pad_left, pad_value=114.0, label="letterbox"):
        a = abi.PreprocArgs()
        a.src, a.dst = _ptr(src_u8), dst.ptr
        a.h, a.w, a.oh, a.ow, a.c_pad = h, w, dst.h, dst.w, dst.ld
        for i in range(3):
            a.mean[i], a.std[i] = 0.0, 1.0
        a.dtype, a.mode = self.dtype, 1
        a.new_h, a.new_w, a.pad_top, a.pad_left, a.pad_value = new_h, new_w, pad_top, pad_left, pad_value
        self._add(abi.OP_PREPROC, a, label)
        return dst

    def yolo_decode(self, levels, strides, nc, nm, reg_max, out, cls_off=0, mc_off=0, label="yolo_decode", box_f32=None, image=0):
        """box_f32: per level an fp32 [n * h * w, 4 * reg_max] matrix of DFL logits (mtx_yolo_decode_args.box_f32) read instead of the level's box channels;
        image: which image of a batched head [n, h, w, ld] this launch decodes (one launch per image)"""
        a = abi.YoloDecodeArgs()
        for i, (lv, st) in enumerate(zip(levels, strides)):
            a.level[i], a.lh[i], a.lw[i], a.lld[i], a.lstride[i] = lv.ptr + image * lv.h * lv.w * lv.ld * lv.t.element_size(), lv.h, lv.w, lv.ld, st
            if box_f32 is not None:
                a.box_f32[i] = _ptr(box_f32[i]) + image * lv.h * lv.w * 4 * reg_max * 4
        a.n_levels, a.nc, a.nm, a.reg_max, a.out, a.dtype = len(levels), nc, nm, reg_max, _ptr(out), self.dtype
        a.cls_off, a.mc_off = cls_off, mc_off
        self._add(abi.OP_YOLO_DECODE, a, label)
        return out

    def detector_tail(self, decoded, nc, nm, anchors=None, ld=None, max_keep=abi.DET_TAIL_MAX_KEEP, label="detector_tail"):
        """MTX_OP_DET_TAIL: score filter, class-aware NMS and the rescale to page coordinates of one image's `decoded` rows (fp32
        [anchors, ld], the output of `yolo_decode`; a slot of a batched plan's [B, anchors, ld] is passed as it is).  Thresholds, max_det and
        the letterbox figures are read from `params` (int32 [DET_TAIL_PARAM_WORDS], fp32 fields in the same words), which the caller
        rewrites before a run: one recorded op serves every call.  -> namespace of the buffers: params, out (the whole result block, int32
        words), state (= out[:4]: kept, candidates, overflow), boxes [max_keep, 4], conf, cls (fp32 views of out), rows (int32 view), coef
        ([max_keep, nm] in the builder's 16-bit type; None for a detect-only head)"""
        from types import SimpleNamespace
        anchors = int(decoded.shape[0]) if anchors is None else anchors
        ld = int(decoded.stride(0)) if ld is None else ld
        params = self.buf((abi.DET_TAIL_PARAM_WORDS,), torch.int32, zero=True)
        out = self.buf((abi.det_tail_out_words(max_keep),), torch.int32, zero=True)
        coef = self.buf((max_keep, nm), self.tdtype, zero=True) if nm > 0 else None
        ws = self.buf((abi.DET_TAIL_WS_BYTES,), torch.uint8, zero=True)          # the op needs its counter word zero at first and leaves it so
        a = abi.DetTailArgs()
        a.decoded, a.params, a.out, a.coef, a.workspace = _ptr(decoded), _ptr(params), _ptr(out), _ptr(coef), _ptr(ws)
        a.ld, a.workspace_bytes = ld, abi.DET_TAIL_WS_BYTES
        a.anchors, a.nc, a.nm, a.max_keep, a.dtype = anchors, nc, nm, max_keep, self.dtype
        self._add(abi.OP_DET_TAIL, a, label)
        f = out.view(torch.float32)
        c0, l0, r0 = abi.det_tail_conf(max_keep), abi.det_tail_cls(max_keep), abi.det_tail_rows(max_keep)
        return SimpleNamespace(params=params, out=out, state=out[:abi.DET_TAIL_BOXES], boxes=f[abi.DET_TAIL_BOXES:c0].view(max_keep, 4),
                               conf=f[c0:l0], cls=f[l0:r0], rows=out[r0:r0 + max_keep], coef=coef, max_keep=max_keep)

    def resize_threshold(self, src, dst, n, hs, ws, hd, wd, thresh=0.0, src_dtype=abi.F32, pix_stride=1,
                         sel=None, batch_stride=-1, roi=None, crop_xyxy=None, label="resize_thresh"):
        a = abi.ResizeThreshArgs()
        a.src, a.dst = _ptr(src), _ptr(dst)
        a.pix_stride, a.sel = pix_stride, _ptr(sel)
        a.batch_stride = batch_stride
        if roi is not None:
            a.roi_y, a.roi_x, a.roi_h, a.roi_w = roi
        a.crop_xyxy = _ptr(crop_xyxy)
        a.n, a.hs, a.ws, a.hd, a.wd, a.thresh, a.dtype = n, hs, ws, hd, wd, thresh, src_dtype
        self._add(abi.OP_RESIZE_THRESH, a, label)
        return dst

    def deform_attention(self, value, off, aw, ref_f32, out, rows, heads, d, level_shapes, points, offset_scale,
                         ld_value=None, ld_off=None, ld_aw=None, ld_out=None, label="deform_attn"):
        """RT-DETR multi-scale deformable attention (include/mtx_hip.h mtx_detr_args kind 0)"""
        a = abi.DetrArgs()
        a.value, a.off, a.aw, a.ref, a.out = _ptr(value), _ptr(off), _ptr(aw), _ptr(ref_f32), _ptr(out)
        a.kind, a.rows, a.heads, a.d, a.levels, a.points = 0, rows, heads, d, len(level_shapes), points
        start = 0
        for i, (h, w) in enumerate(level_shapes):
            a.lh[i], a.lw[i], a.lstart[i] = h, w, start
            start += h * w
        lp = len(level_shapes) * points
        a.ld_value, a.ld_out = ld_value or heads * d, ld_out or heads * d
        a.ld_off, a.ld_aw = ld_off or heads * lp * 2, ld_aw or heads * lp
        a.offset_scale, a.dtype = offset_scale, self.dtype
        self._add(abi.OP_DETR, a, label)
        return out

    def box_refine(self, ref_in_f32, ref_out_f32, ref_t, rows, delta=None, ld_delta=8, label="box_refine"):
        """ref_out = sigmoid(delta + logit(ref_in)) (delta given) or sigmoid(ref_in) (logits in); ref_t = T copy [rows, 8]"""
        a = abi.DetrArgs()
        a.ref, a.ref_out, a.ref_t, a.delta = _ptr(ref_in_f32), _ptr(ref_out_f32), _ptr(ref_t), _ptr(delta)
        a.kind, a.rows, a.ld_delta, a.dtype = (1 if delta is not None else 2), rows, ld_delta, self.dtype
        self._add(abi.OP_DETR, a, label)

    def quantize(self, x, rows, k, ldx=None, x_off=0, q=None, scale=None, row_off=0, lds=None, label="quantize_mx",
                 ldq=None, q_col_off=0, swiglu_b=None, b_off=0, ldb=None, y=None, y_off=0, ldy=None):
        """MX fp8 copy of rows [0, rows) of a 16-bit [*, ldx] matrix starting x_off elements in; with `q` / `scale` given the result
        lands in rows [row_off, row_off + rows) of those buffers (q [R, ldq] bytes from column q_col_off on, scale [K / 128, lds] uint32
        from plane q_col_off / 128 on).  swiglu_b: the quantised matrix is silu(x) * swiglu_b (MTX_QUANT_SWIGLU; y: its 16-bit copy).
        -> (q, scale, lds)"""
        if q is None:
            lds = (rows + 63) // 64 * 64
            q = self.buf((rows, k), torch.uint8)
            scale = self.buf((k // 128, lds), torch.int32, zero=True)
        ldq = ldq or k
        assert q_col_off % 128 == 0
        a = abi.QuantArgs()
        a.x, a.q, a.scale = _ptr(x, x_off), q.data_ptr() + row_off * ldq + q_col_off, scale.data_ptr() + 4 * (row_off + (q_col_off // 128) * lds)
        a.rows, a.k, a.ldx, a.ldq, a.lds, a.dtype = rows, k, (ldx or k), ldq, lds, self.dtype
        if swiglu_b is not None:
            a.op, a.b, a.ldb = abi.QUANT_SWIGLU, _ptr(swiglu_b, b_off), (ldb or ldx or k)
            if y is not None:
                a.y, a.ldy = _ptr(y, y_off), (ldy or k)
        self._add(abi.OP_QUANT, a, label)
        return q, scale, lds

    def memset(self, t, value=0, label="memset"):
        a = abi.MemsetArgs()
        a.ptr, a.bytes, a.value = _ptr(t), t.numel() * t.element_size(), value
        self._add(abi.OP_MEMSET, a, label)

    # ---- finish ---------------------------------------------------------------------------
    def build(self) -> Plan:
        n = len(self.ops)
        arr = (abi.Op * max(n, 1))(*self.ops)
        handle = C.c_void_p()
        self.lib.check(self.lib.mtx_plan_create(arr, n, C.byref(handle)), "mtx_plan_create")
        plan = Plan(self.lib, handle.value, list(self.keep), n)
        plan.device = self.device          # where its buffers live: `run` takes streams of THIS device, whatever the calling thread's current device is
        plan.labels = list(self.labels)
        plan.ops = list(self.ops)          # the recorded argument blocks (benchmarks group launches by kernel and shape)
        return plan


def residual_distance(parts: torch.Tensor) -> float:
    """mean |prev - r| / mean |prev| from the parts a `residual_dist` op left (added in index order, in double: the same bytes give the same
    verdict on every run); inf when `prev` is all zero"""
    p = parts.detach().to("cpu", torch.float64)
    d, m = float(p[:, 0].sum()), float(p[:, 1].sum())
    return d / m if m > 0.0 else float("inf")


def glu_interleave(col0: int, hid: int) -> torch.Tensor:
    """Row order of a fused [col0 + 2 * hid, K] projection for the gated epilogue of the fp8 GEMM (mtx_gemm_args.glu_*): rows below col0
    stay, then runs of 32 "a" rows (col0 + 32 u ..) each followed by the 32 "b" rows of the same outputs (col0 + hid + 32 u ..).
    `w[glu_interleave(col0, hid)]` is the weight to hand to the kernel."""
    assert hid % 32 == 0
    u = torch.arange(hid // 32)[:, None, None] * 32 + torch.arange(32)[None, None, :]                # [U, 1, 32]
    pair = torch.cat([col0 + u, col0 + hid + u], 1).reshape(-1)                                      # a-run, b-run per u
    return torch.cat([torch.arange(col0), pair])


class AsyncLane:
    """One model's private HIP stream for `submit` / `collect` style calls.

    The reference runs a page's detectors one after the other, each call returning finished results (`model(img, conf=...)`,
    core/image/detection.py:1337-1351, 1401-1407; core/image/ocr_detection.py:425-431).  On an MI355X the 640-pixel networks are far
    too small to fill 256 CUs, and every call ends in a synchronising read — four detectors cost the SUM of their GPU times plus
    their host post-processing.  With a lane per model, `submit` enqueues the upload and the graph replay on the model's own stream
    and returns at once; the caller submits every detector of the page, then collects: the graphs run side by side on the chip and one
    model's post-processing overlaps the others' kernels.  `__call__` = `collect(submit(...))` keeps the reference's call shape.

    The lane also owns the model's busy lock: a model's plan has ONE set of buffers, so a second submit waits until the first was
    collected.  On the CPU simulator (no streams) everything degenerates to an in-line call."""

    def __init__(self, device, simulator: bool):
        self.on = (not simulator) and torch.cuda.is_available() and torch.device(device).type == "cuda"
        self.device = torch.device(device)
        self._stream = None
        self.busy = threading.Lock()

    @property
    def stream(self):
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=self.device)
        return self._stream

    def enter(self):
        """context for the enqueue half: the lane's stream, ordered after everything the caller has queued so far"""
        if not self.on:
            return contextlib.nullcontext()
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        return torch.cuda.stream(self.stream)

    def resume(self):
        """context for the collect half (reads the results on the lane's stream)"""
        return torch.cuda.stream(self.stream) if self.on else contextlib.nullcontext()

    def adopt(self, *tensors):
        """device tensors the CALLER allocated and the lane's kernels read (a page uploaded once for several detectors): the allocator
        must not hand their blocks out again while the lane still reads them, whatever the caller does with them after `submit`"""
        if self.on:
            for t in tensors:
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(self.stream)

    def hand_over(self, *tensors):
        """the caller's stream may touch what the lane produced; `tensors` = results allocated on the lane's stream that leave with the
        caller (their blocks return to the lane's pool when the caller drops them: recorded on the caller's stream so that the lane does
        not reuse them under kernels of the caller that still read them — ADVICE r03)"""
        if self.on:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_stream(self.stream)
            for t in tensors:
                if torch.is_tensor(t) and t.is_cuda:
                    t.record_stream(cur)

    ACQUIRE_TIMEOUT_S = 120.0      # far beyond any graph of this package; a wait this long is a ticket that was never closed

    def acquire(self):
        """waits for the model's previous ticket to be closed.  A ticket kept alive by a traceback / frame / reference cycle, or a caller that
        re-submits to the same model inside the `except` of a failed collect, never releases the lane by itself (the finaliser only runs when
        the ticket is collected): instead of hanging the thread for good, say so"""
        if not self.busy.acquire(timeout=self.ACQUIRE_TIMEOUT_S):
            raise RuntimeError(f"model lane busy for {self.ACQUIRE_TIMEOUT_S:.0f} s: a ticket of an earlier submit() was neither collected nor closed "
                               "(close tickets in try / finally, or use `with ticket:`)")

    def release(self):
        """idempotent: a ticket may be closed by `collect` and again by its finaliser"""
        try:
            self.busy.release()
        except RuntimeError:
            pass


def result_tensors(obj, _depth=0):
    """the CUDA tensors reachable from a result object (lists / tuples / dicts / namespaces / small result classes, three levels deep):
    what `AsyncLane.hand_over` records on the consumer's stream"""
    if torch.is_tensor(obj):
        return [obj] if obj.is_cuda else []
    if _depth >= 3 or obj is None or isinstance(obj, (str, bytes, int, float, bool)):
        return []
    if isinstance(obj, dict):
        items = obj.values()
    elif isinstance(obj, (list, tuple)):
        items = obj
    elif hasattr(obj, "__dict__"):
        items = vars(obj).values()
    else:
        return []
    out = []
    for v in items:
        out += result_tensors(v, _depth + 1)
    return out


class LaneTicket(dict):
    """What a model's `submit` returns: the arguments of its `collect` half, plus the duty to free the model's lane.  `collect` closes it;
    a ticket that is DROPPED (an exception between submit and collect in the caller) releases the lane when it is garbage-collected, so a
    failed page cannot leave a model busy for good.  The lane's stream is in order, so a later submit that reuses the
    model's buffers still runs behind whatever the dropped ticket had queued."""

    def __init__(self, lane: "AsyncLane", **fields):
        super().__init__(**fields)
        self._lane, self._open = lane, True

    def close(self):
        if self._open:
            self._open = False
            self._lane.release()

    def __enter__(self):
        return self

    def __exit__(self, *exc):          # `with model.submit(...) as ticket:` — the lane is free again however the block ends
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001 — interpreter shutdown
            pass
