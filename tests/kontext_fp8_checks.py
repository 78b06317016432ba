"""FLUX.1-Kontext with its block linears on the MX-fp8 matrix path (FluxDiTHip(fp8=...)): the activation + MX-fp8 epilogue of the fp8 GEMM
(mtx_gemm_args.actq_*) against the two launches it replaces, its argument validation, and the fp8 graph against the fp32 oracle
(oracle/flux_ref.py) and against the bf16 graph of the same weights.

Written once, run twice like op_checks.py / flux_checks.py: on the kernel simulator (tests/test_kontext_fp8_sim.py) and on gfx950
(tests/test_kontext_fp8_gpu.py)."""
import ctypes as C
import math

import numpy as np
import torch

from mangatranslator_amd.core.ml import flux as fx
from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.plan import PlanBuilder
from oracle import flux_ref as fr

import flux_checks as fc
from flux_checks import PSNR_MIN_DB, assert_repeats, rel
from op_checks import TD, _dev, _run, _sync

FP8_STEP_TOL = 0.12          # the project's fp8 step bound for a toy network against the fp32 oracle (flux2_checks.check_dit_step)
HD128 = dict(heads=1, axes_dim=(16, 56, 56))      # the toy network with ONE head of 128: the geometry the long-sequence attention kernel serves


def psnr(a, b):
    mse = ((a.float().cpu() - b.float().cpu()) ** 2).mean().item()
    return 99.0 if mse == 0 else 10 * math.log10(1.0 / mse)


# ---- the epilogue -----------------------------------------------------------------------------------------------------------------------
def check_gemm_f8_actq(lib, dtype, m, n, k, act=abi.ACT_NONE, with_bias=False, seed=0, row_off=0, q_col_off=0, spread=1.0, zero_row=None):
    """The activation + MX-fp8 epilogue of the fp8 GEMM against the two launches it replaces — fp8 GEMM with bias and activation into a
    16-bit [m, n] matrix (whole tiles: FORCE_TILE256 | NO_SPLIT, the K order of the fused kernel), then mtx_quantize_mx — on the same
    operands: the e4m3 bytes and the E8M0 scale words must be IDENTICAL, and nothing outside rows [row_off, row_off + m) x byte columns
    [q_col_off, q_col_off + n) of a larger twin buffer may be written.  zero_row: that row of A is all zero and there is no bias, so
    its blocks take the zero-block rule (scale byte 127, bytes 0)."""
    g = torch.Generator().manual_seed(seed)
    dev, td = _dev(lib), TD[dtype]
    a = (torch.randn(m, k, generator=g) * torch.exp(spread * torch.randn(m, k // 32, generator=g)).repeat_interleave(32, 1)).to(td)
    if zero_row is not None:
        assert not with_bias
        a[zero_row] = 0
    w = (torch.randn(n, k, generator=g) / math.sqrt(k) * 1.5).to(td)
    b = torch.randn(n, generator=g) if with_bias else None
    R, QW = row_off + m + 3, q_col_off + n + 128          # three spare rows below, one spare 128-byte group to the right
    lds = (R + 63) // 64 * 64
    outs = []
    for fused in (False, True):
        pb = PlanBuilder(lib, dev, dtype)
        aq, asc, lds_a = pb.quantize(pb.const(a), m, k)
        wq, wsc, lds_w = pb.quantize(pb.const(w), n, k)
        bias = pb.const(b) if b is not None else None
        q8 = pb.buf((R, QW), torch.uint8, zero=True)
        sc = pb.buf((QW // 128, lds), torch.int32, zero=True)
        if fused:
            c = pb.gemm(aq, wq, m, n, k, bias=bias, act=act, f8=(asc, lds_a, wsc, lds_w, 0, 0), actq=(q8, sc, QW, lds, row_off, q_col_off))
            assert c is None, "the fused launch must not need a 16-bit output buffer"
        else:
            c = pb.gemm(aq, wq, m, n, k, bias=bias, act=act, f8=(asc, lds_a, wsc, lds_w, 0, 0), flags=abi.GEMM_FORCE_TILE256 | abi.GEMM_NO_SPLIT)
            pb.quantize(c, m, n, q=q8, scale=sc, row_off=row_off, lds=lds, ldq=QW, q_col_off=q_col_off)
        _run(pb)
        outs.append((q8.cpu().numpy().copy(), sc.cpu().numpy().copy()))
    (q0, s0), (q1, s1) = outs
    assert q0.any() and s0.any()
    assert np.array_equal(q0, q1), f"activation epilogue: {(q0 != q1).sum()} of {q0.size} e4m3 bytes differ"
    assert np.array_equal(s0, s1), f"activation epilogue: {(s0 != s1).sum()} scale words differ"
    win = np.zeros_like(q1, dtype=bool)
    win[row_off:row_off + m, q_col_off:q_col_off + n] = True
    assert not q1[~win].any(), "e4m3 bytes outside the target window were written"
    swin = np.zeros_like(s1, dtype=bool)
    swin[q_col_off // 128:(q_col_off + n) // 128, row_off:row_off + m] = True
    assert not s1[~swin].any(), "scale words outside the target window were written"
    if zero_row is not None:
        assert not q1[row_off + zero_row].any() and (s1[swin.any(1)][:, row_off + zero_row] == 0x7f7f7f7f).all(), "zero-block rule: bytes 0, scale byte 127"


def check_actq_cases(lib):
    """ragged M, one and several K tiles, both 32-column spans of a wave, several column tiles, a row and a column offset, every compiled activation"""
    check_gemm_f8_actq(lib, abi.BF16, 300, 256, 128, act=abi.ACT_GELU_TANH, with_bias=True)
    check_gemm_f8_actq(lib, abi.F16, 260, 512, 256, act=abi.ACT_SILU, with_bias=True, row_off=5, q_col_off=128, spread=1.5, seed=1)
    check_gemm_f8_actq(lib, abi.BF16, 256, 256, 384, zero_row=77, seed=2)


def check_actq_validation(lib):
    """every combination include/mtx_hip.h refuses for the activation + MX-fp8 epilogue returns MTX_ERR_INVALID with a message and launches
    nothing; the arguments they are derived from are a valid launch over real buffers"""
    dev, td = _dev(lib), torch.bfloat16
    m, n, k = 64, 256, 128
    pb = PlanBuilder(lib, dev, abi.BF16)
    a16 = pb.const((torch.randn(m, k, generator=torch.Generator().manual_seed(0))).to(td))
    w16 = pb.const((torch.randn(n + 8, k, generator=torch.Generator().manual_seed(1)) / 8).to(td))
    aq, asc, lds_a = pb.quantize(a16, m, k)
    wq, wsc, lds_w = pb.quantize(w16, n, k)
    _run(pb)
    q8 = torch.zeros((m, n + 64), dtype=torch.uint8, device=dev)
    sc = torch.zeros((n // 128, 64), dtype=torch.int32, device=dev)
    c16 = torch.zeros((m, n), dtype=td, device=dev)
    row = torch.zeros((1, n), dtype=td, device=dev)

    def base():
        g = abi.GemmArgs()
        g.a, g.w, g.m, g.n, g.k, g.lda, g.ldw, g.ldc, g.ldres, g.ldgate = aq.data_ptr(), wq.data_ptr(), m, n, k, k, k, n, n, n
        g.batch, g.gate_rows_per, g.alpha, g.dtype, g.out_dtype, g.act = 1, 1, 1.0, abi.BF16, abi.BF16, abi.ACT_GELU_TANH
        g.a_scale, g.w_scale, g.lds_a, g.lds_w, g.in_dtype = asc.data_ptr(), wsc.data_ptr(), lds_a, lds_w, abi.F8
        g.actq_q, g.actq_scale, g.actq_ldq, g.actq_lds = q8.data_ptr(), sc.data_ptr(), n + 64, 64
        return g

    def call(g):
        rc = lib.mtx_gemm(C.byref(g), C.c_void_p(0) if lib.is_simulator else C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _sync(lib)
        return rc, lib.last_error()

    rc, msg = call(base())
    assert rc == 0, f"the valid launch was refused: {msg}"
    assert q8[:, :n].any() and not q8[:, n:].any()

    def non_fp8(g):
        g.a, g.w, g.in_dtype, g.c = a16.data_ptr(), w16.data_ptr(), 0, c16.data_ptr()

    def f32_operands(g):
        non_fp8(g)
        g.dtype = g.out_dtype = abi.F32

    def ragged_n(g):
        g.n, g.ldc = n - 8, n - 8

    def with_gate(g):
        g.gate, g.c = row.data_ptr(), c16.data_ptr()

    def with_res(g):
        g.res, g.c = c16.data_ptr(), c16.data_ptr()

    def with_glu(g):
        g.glu_q, g.glu_scale, g.glu_ldq, g.glu_lds, g.glu_col0, g.c, g.act = q8.data_ptr(), sc.data_ptr(), n + 64, 64, 0, c16.data_ptr(), abi.ACT_NONE

    def misaligned(g):
        g.actq_q = q8.data_ptr() + 8

    def bad_ldq(g):
        g.actq_ldq = n + 8

    def short_lds(g):
        g.actq_lds = m - 1

    def no_scale(g):
        g.actq_scale = None

    before = (q8.clone(), sc.clone())
    for bad in (non_fp8, f32_operands, ragged_n, with_gate, with_res, with_glu, misaligned, bad_ldq, short_lds, no_scale):
        g = base()
        bad(g)
        rc, msg = call(g)
        assert rc == -1 and msg, f"{bad.__name__}: expected MTX_ERR_INVALID with a message, got {rc} {msg!r}"
    assert torch.equal(q8, before[0]) and torch.equal(sc, before[1]), "a refused launch wrote something"


# ---- the graph --------------------------------------------------------------------------------------------------------------------------
def hip_models(t, v, lib, device, fp8=False, **dit_kw):
    tsd, vsd = t.state_dict(), v.state_dict()
    c = t.cfg
    dcfg = dict(d=c["d"], heads=c["heads"], layers=c["layers"], single_layers=c["single_layers"], in_channels=c["in_channels"],
                joint_dim=c["joint_dim"], pooled_dim=c["pooled_dim"], axes_dim=tuple(c["axes_dim"]))
    vcfg = dict(ch=tuple(v.cfg["ch"]), groups=v.cfg["groups"], scaling_factor=v.cfg["scaling_factor"], shift_factor=v.cfg["shift_factor"])
    dit = fx.FluxDiTHip(lambda n: tsd[n], dcfg, device, lib=lib, fp8=fp8, **dit_kw)
    vae = fx.FluxVAEHip(lambda n: vsd[n], vcfg, device, lib=lib)
    return dit, vae


def step_inputs(cfg, h2, w2, t_txt, seed=3):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(2 * h2 * w2, 64, generator=g).to(torch.bfloat16).float()
    pe = torch.randn(t_txt, cfg["joint_dim"], generator=g).to(torch.bfloat16).float()
    pooled = torch.randn(cfg["pooled_dim"], generator=g).to(torch.bfloat16).float()
    return lat, pe, pooled


def run_step(dit, lat, pe, pooled, h2, w2, device):
    plan = dit.plan_for(pe.shape[0], h2, w2, 1)
    plan.ctx_in.copy_(pe.to(device, torch.bfloat16))
    plan.lat.copy_(lat.to(device, torch.bfloat16))
    plan.mod.copy_(dit.modulation(0.7, 2.5, pooled.to(device, torch.bfloat16)))
    plan.run()
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    return plan.vel.float().cpu().clone(), plan


def gemm_ops(plan):
    return [(lb, o.u.gemm) for lb, o in zip(plan.labels, plan.ops) if o.kind == abi.OP_GEMM]


def block_gemms(plan):
    return [(lb, g) for lb, g in gemm_ops(plan) if lb.startswith(("dbl", "sgl"))]


def check_dit_step_fp8(lib, device, h2=4, w2=6, t_txt=16, tol=FP8_STEP_TOL, **kw):
    """One toy Kontext step with every block linear on the MX fp8 kernel against the fp32 oracle, then the step again eagerly and as graph
    replays.  Bound: the project's fp8 step bound for a toy network, 0.12; the simulator measures 0.0329 on the default network (2 + 2 blocks, d = 128)."""
    t, v = fc.models(**kw)
    dit, _ = hip_models(t, v, lib, device, fp8=True)
    lat, pe, pooled = step_inputs(t.cfg, h2, w2, t_txt)
    ids = torch.cat([fr.image_ids(h2, w2, 0), fr.image_ids(h2, w2, 1)])
    with torch.no_grad():
        ref = t(lat, 0.7, 2.5, pooled, pe, torch.zeros(t_txt, 3), ids)[: h2 * w2]
    vel, plan = run_step(dit, lat, pe, pooled, h2, w2, device)
    e = rel(vel, ref)
    print(f"Kontext DiT step, fp8 block linears ({t.cfg['layers']}+{t.cfg['single_layers']} blocks, d={t.cfg['d']}, T={plan.T}): velocity rel err {e:.4f}")
    blk = block_gemms(plan)
    assert blk and all(g.in_dtype == abi.F8 for _, g in blk), "a block linear was left on the 16-bit kernel"
    assert any(g.actq_q for _, g in blk), "no GEMM of the step uses the activation + MX-fp8 epilogue"
    assert e < tol
    assert_repeats(plan, device)
    return e


def check_fusions_change_nothing(lib, device, h2=22, w2=24, t_txt=16, **kw):
    """An fp8 step long enough for the long-sequence attention (T >= 1024, head dim 128) with all three producer fusions — norms, the
    activation epilogue of ff1 / ff1_ctx / proj_mlp, attention with MX fp8 output — against the same step with a quantiser launch behind
    every producer: IDENTICAL velocity, no mtx_quantize_mx launch in the fused plan, some in the other"""
    kw = {**HD128, **kw}
    t, v = fc.models(**kw)
    lat, pe, pooled = step_inputs(t.cfg, h2, w2, t_txt)
    vels, nq = [], []
    for on in (False, True):
        dit, _ = hip_models(t, v, lib, device, fp8=True, fused_quant=on, act_epilogue=on, attn_q8=on)
        assert dit.act_epilogue == on and dit.attn_q8 == on, "the geometry does not allow the fusions"
        vel, plan = run_step(dit, lat, pe, pooled, h2, w2, device)
        assert plan.T >= 1024
        vels.append(vel)
        nq.append(sum(1 for o in plan.ops if o.kind == abi.OP_QUANT))
        assert any(g.actq_q for _, g in block_gemms(plan)) == on
    assert nq[0] > 0 and nq[1] == 0, nq
    assert torch.isfinite(vels[1]).all() and torch.equal(vels[0], vels[1]), f"the fusions change the step: rel {rel(vels[1], vels[0]):.3e}"
    return nq


def check_off_means_off(lib, device, h2=4, w2=6, t_txt=16, **kw):
    """fp8=False: no op of the plan takes fp8 operands or writes an fp8 twin, and no quantiser launch exists"""
    t, v = fc.models(**kw)
    dit, _ = hip_models(t, v, lib, device, fp8=False)
    assert dit.fp8 == ()
    for cached in (False, True):
        head = dit.plan_for(t_txt, h2, w2, 1, cached=cached)
        for plan in (head,) + ((head.body, head.skip) if cached else ()):
            assert not any(o.kind == abi.OP_QUANT for o in plan.ops)
            assert all(g.in_dtype != abi.F8 and not g.actq_q and not g.glu_q for _, g in gemm_ops(plan))
            assert not any(o.kind == abi.OP_NORM and o.u.norm.q for o in plan.ops) and not any(o.kind == abi.OP_ATTN and o.u.attn.q8 for o in plan.ops)


def check_first_block_cache_fp8(lib, device, h=64, w=96, t_txt=16, steps=3, **kw):
    """the three-plan form of the first-block cache with fp8 block linears: threshold 0 (the one-plan graph) and a threshold nothing
    passes (head + body every step) give the same bytes; a threshold everything passes skips every step but the first"""
    t, v = fc.models(**kw)
    dit, vae = hip_models(t, v, lib, device, fp8=True)
    img, pe, pooled, noise = fc.inputs(t, h, w, t_txt)
    pipe = fx.FluxKontextHip(dit, vae)
    call = lambda **k: pipe(image=img, width=w, height=h, num_inference_steps=steps, guidance_scale=2.5, prompt_embeds=pe[None],
                            pooled_prompt_embeds=pooled[None], latents=noise, **k).images[0].clone()
    base = call()
    assert pipe.last["skipped_steps"] == 0
    never = call(residual_diff_threshold=1e-12)
    assert pipe.last["skipped_steps"] == 0 and torch.equal(never, base), "fp8: head + body differs from the one-plan step"
    head = dit.plan_for(t_txt, h // 16, w // 16, 1, cached=True)
    assert all(g.in_dtype == abi.F8 for p in (head, head.body) for _, g in block_gemms(p))
    always = call(residual_diff_threshold=1e9)
    assert pipe.last["skipped_steps"] == steps - 1 and torch.isfinite(always).all()


def kontext_images(lib, device, modes, h=64, w=96, t_txt=16, steps=4, **kw):
    t, v = fc.models(**kw)
    img, pe, pooled, noise = fc.inputs(t, h, w, t_txt)
    outs = []
    for mode in modes:
        dit, vae = hip_models(t, v, lib, device, fp8=mode)
        pipe = fx.FluxKontextHip(dit, vae)
        outs.append(pipe(image=img, width=w, height=h, num_inference_steps=steps, guidance_scale=2.5, prompt_embeds=pe[None],
                         pooled_prompt_embeds=pooled[None], latents=noise).images[0].cpu())
    return outs


def check_kontext_fp8_vs_bf16(lib, device, h=64, w=96, t_txt=16, steps=4, **kw):
    """the bar of the fp8 path: image PSNR of the fp8 pipeline (fp8=True: the default set of kinds) against the bf16 pipeline of the same weights"""
    bf16, f8 = kontext_images(lib, device, (False, True), h, w, t_txt, steps, **kw)
    p = psnr(f8, bf16)
    print(f"Kontext {steps} steps {w}x{h}: fp8 block linears vs bf16 image PSNR {p:.1f} dB")
    assert p >= PSNR_MIN_DB
    return p
