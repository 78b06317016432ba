"""GPU micro-benchmarks of the MFMA-bound kernels at FLUX shapes (HIP-event timing via mtx_plan_time).
usage: python tools/bench_kernels.py [attn T [heads]] [gemm M N K] [gemm8 M N K] [quant ROWS K] [conv H W] [actq M N K] [kontext H2 W2 [LAYERS SINGLES]] [sam3 [LAYERS]] [mangaocr [DEC_LAYERS]] [mangaocr_batch] [paddleocr] [textenc [WHEEL_LAYERS]] [dettail] ..."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mangatranslator_amd.hip import abi
from mangatranslator_amd.hip.lib import get_library
from mangatranslator_amd.hip.plan import PlanBuilder

lib = get_library(); lib.init(0)
dev = torch.device("cuda:0")


def _time(plan, iters):
    plan.run(); torch.cuda.synchronize()
    plan.time(5)
    return min(plan.time(iters) for _ in range(3))


def attn(T, heads=24, d=128, iters=10):
    pb = PlanBuilder(lib, dev, abi.BF16)
    D = heads * d
    qkv = pb.buf((T, 3 * D), torch.bfloat16); qkv.normal_()
    o = pb.buf((T, D), torch.bfloat16)
    qkv[:, :D] *= d ** -0.5 * 1.4426950408889634         # the FLUX graphs' form: q pre-multiplied by scale * log2(e)
    pb.attention(qkv, qkv, qkv, o, 1, heads, T, T, d, (0, 3 * D, d), (0, 3 * D, d), (0, 3 * D, d), (0, D, d), d ** -0.5, k_off=D, v_off=2 * D,
                 q_prescaled=True)
    ms = _time(pb.build(), iters)
    print(f"attn T={T} heads={heads}: {ms:.3f} ms  {4 * T * T * D / ms / 1e9:.0f} TFLOP/s", flush=True)
    return ms


def attn_q8(T, heads=24, d=128, iters=10, fused=True):
    """FLUX.2 form: the rows leave as the MX fp8 operand of the next linear (fused: mtx_attn_args.q8; else attention + quantiser launch)"""
    pb = PlanBuilder(lib, dev, abi.BF16)
    D = heads * d
    qkv = pb.buf((T, 3 * D), torch.bfloat16); qkv.normal_()
    qkv[:, :D] *= d ** -0.5 * 1.4426950408889634
    lds = (T + 63) // 64 * 64
    q8 = pb.buf((T, D), torch.uint8, zero=True)
    sc = pb.buf((D // 128, lds), torch.int32, zero=True)
    strides = ((0, 3 * D, d), (0, 3 * D, d), (0, 3 * D, d), (0, D, d))
    if fused:
        pb.attention(qkv, qkv, qkv, None, 1, heads, T, T, d, *strides, d ** -0.5, k_off=D, v_off=2 * D, q_prescaled=True, q8=(q8, sc, D, lds, 0))
    else:
        o = pb.buf((T, D), torch.bfloat16)
        pb.attention(qkv, qkv, qkv, o, 1, heads, T, T, d, *strides, d ** -0.5, k_off=D, v_off=2 * D, q_prescaled=True)
        pb.quantize(o, T, D, q=q8, scale=sc, lds=lds, ldq=D)
    ms = _time(pb.build(), iters)
    print(f"attn -> MX fp8 T={T} heads={heads} [{'fused epilogue' if fused else 'attention + quantiser launch'}]: {ms:.3f} ms  {4 * T * T * D / ms / 1e9:.0f} TFLOP/s", flush=True)


def attn_f8_pv(T, heads=24, d=128, iters=10):
    """fp8 scores + fp8 P V (mtx_attn_args.v_f8t), MX fp8 rows out; the V^T producer launch (MTX_EW_V_F8T) timed with it and alone"""
    D = heads * d
    lds = (T + 63) // 64 * 64
    def build(with_attn, with_prod):
        pb = PlanBuilder(lib, dev, abi.BF16)
        qkv = pb.buf((T, 3 * D), torch.bfloat16); qkv.normal_()
        qk8 = pb.buf((T, 2 * D), torch.uint8)
        qk8.copy_(qkv[:, :2 * D].float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))
        q8 = pb.buf((T, D), torch.uint8, zero=True)
        sc = pb.buf((D // 128, lds), torch.int32, zero=True)
        vt8 = pb.buf((D, lds), torch.uint8, zero=True)
        if with_prod:
            pb.v_f8t(qkv, T, heads, 3 * D, v_off=2 * D, out=vt8)
        if with_attn:
            pb.attention(qkv, qkv, qkv, None, 1, heads, T, T, d, (0, 3 * D, d), (0, 3 * D, d), (0, 3 * D, d), (0, D, d), d ** -0.5, k_off=D, v_off=2 * D,
                         q_prescaled=True, q8=(q8, sc, D, lds, 0), qk_f8=(qk8, 0, D, 2 * D, -3), pv_f8=(vt8, lds))
        return pb.build()
    both, prod = _time(build(True, True), iters), _time(build(False, True), iters)
    print(f"attn, fp8 scores + fp8 P V T={T} heads={heads} [MX fp8 rows out]: {both - prod:.3f} ms  {4 * T * T * D / (both - prod) / 1e9:.0f} TFLOP/s; "
          f"with the V^T producer launch {both:.3f} ms (producer alone {prod * 1e3:.1f} us)", flush=True)


def attn_f8_scores(T, heads=24, d=128, iters=10, out8=True):
    """the fp8-score form (mtx_attn_args.q_f8 / k_f8): q and k as plain e4m3 rows; out8: rows leave as MX fp8 (the Klein graph's form), else 16-bit"""
    pb = PlanBuilder(lib, dev, abi.BF16)
    D = heads * d
    qkv = pb.buf((T, 3 * D), torch.bfloat16); qkv.normal_()
    qk8 = pb.buf((T, 2 * D), torch.uint8)
    qk8.copy_(qkv[:, :2 * D].float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))
    lds = (T + 63) // 64 * 64
    q8 = pb.buf((T, D), torch.uint8, zero=True)
    sc = pb.buf((D // 128, lds), torch.int32, zero=True)
    o = None if out8 else pb.buf((T, D), torch.bfloat16)
    pb.attention(qkv, qkv, qkv, o, 1, heads, T, T, d, (0, 3 * D, d), (0, 3 * D, d), (0, 3 * D, d), (0, D, d), d ** -0.5, k_off=D, v_off=2 * D,
                 q_prescaled=True, q8=(q8, sc, D, lds, 0) if out8 else None, qk_f8=(qk8, 0, D, 2 * D, -3))
    ms = _time(pb.build(), iters)
    print(f"attn, fp8 scores T={T} heads={heads} [{'MX fp8 rows out' if out8 else '16-bit rows out'}]: {ms:.3f} ms  {4 * T * T * D / ms / 1e9:.0f} TFLOP/s", flush=True)


def gemm8_glu(M, hid, K, col0=0, iters=20, fused=True):
    """FLUX.2 MLP-in: fp8 GEMM [M, col0 + 2 hid] whose gated half leaves as silu(a) * b in MX fp8 (fused: mtx_gemm_args.glu_*; else GEMM + SwiGLU quantiser)"""
    from mangatranslator_amd.hip.plan import glu_interleave
    pb = PlanBuilder(lib, dev, abi.BF16)
    N = col0 + 2 * hid
    a = pb.buf((M, K), torch.bfloat16); a.normal_()
    w = pb.buf((N, K), torch.bfloat16); w.normal_(0, K ** -0.5)
    if fused:
        w.copy_(w[glu_interleave(col0, hid).to(dev)].clone())
    q = PlanBuilder(lib, dev, abi.BF16)
    aq, asc, la = q.quantize(a, M, K)
    wq, wsc, lw = q.quantize(w, N, K)
    q.build().run(); torch.cuda.synchronize()
    pb.keep += [aq, asc, wq, wsc]
    lds = (M + 63) // 64 * 64
    q8 = pb.buf((M, hid), torch.uint8, zero=True)
    sc = pb.buf((hid // 128, lds), torch.int32, zero=True)
    if fused:
        pb.gemm(aq, wq, M, N, K, out=pb.buf((M, N), torch.bfloat16) if col0 else None, f8=(asc, la, wsc, lw, 0, 0), glu=(q8, sc, hid, lds, col0, 0, 0))
    else:
        c = pb.gemm(aq, wq, M, N, K, f8=(asc, la, wsc, lw, 0, 0))
        pb.quantize(c, M, hid, ldx=N, x_off=col0, q=q8, scale=sc, lds=lds, ldq=hid, swiglu_b=c, b_off=col0 + hid, ldb=N)
    ms = _time(pb.build(), iters)
    print(f"gemm8 + SwiGLU -> MX fp8 M={M} N={N} K={K} [{'gated epilogue' if fused else 'GEMM + SwiGLU quantiser launch'}]: {ms:.3f} ms  {2 * M * N * K / ms / 1e9:.0f} TFLOP/s", flush=True)


def gemm8_actq(M, N, K, iters=20, fused=True, plan_only=False):
    """FLUX.1-Kontext MLP-in: fp8 GEMM + bias + tanh-GELU whose result leaves as the MX fp8 operand of the next linear (fused: mtx_gemm_args.actq_*;
    else GEMM into 16 bits + quantiser launch)"""
    pb = PlanBuilder(lib, dev, abi.BF16)
    g = torch.Generator(device=dev).manual_seed(5)
    a = pb.buf((M, K), torch.bfloat16); a.normal_(generator=g)
    w = pb.buf((N, K), torch.bfloat16); w.normal_(0, K ** -0.5, generator=g)
    bias = pb.buf((N,), torch.float32); bias.normal_(generator=g)
    q = PlanBuilder(lib, dev, abi.BF16)
    aq, asc, la = q.quantize(a, M, K)
    wq, wsc, lw = q.quantize(w, N, K)
    q.build().run(); torch.cuda.synchronize()
    pb.keep += [aq, asc, wq, wsc]
    lds = (M + 63) // 64 * 64
    q8 = pb.buf((M, N), torch.uint8, zero=True)
    sc = pb.buf((N // 128, lds), torch.int32, zero=True)
    kw = dict(bias=bias, act=abi.ACT_GELU_TANH, f8=(asc, la, wsc, lw, 0, 0))
    if fused:
        pb.gemm(aq, wq, M, N, K, actq=(q8, sc, N, lds, 0, 0), **kw)
    else:
        c = pb.gemm(aq, wq, M, N, K, **kw)
        pb.quantize(c, M, N, q=q8, scale=sc, lds=lds, ldq=N)
    plan = pb.build()
    plan.q8, plan.sc = q8, sc
    if plan_only:
        return plan
    ms = _time(plan, iters)
    print(f"gemm8 + bias + tanh-GELU -> MX fp8 M={M} N={N} K={K} [{'activation epilogue' if fused else 'GEMM + quantiser launch'}]: {ms:.3f} ms  {2 * M * N * K / ms / 1e9:.0f} TFLOP/s", flush=True)
    return ms


def gemm8_actq_ab(M, N, K, reps=3, iters=20):
    """fused against unfused, alternating in one process; the operand bytes must be the same when the unfused GEMM runs whole tiles"""
    plans = {f: gemm8_actq(M, N, K, fused=f, plan_only=True) for f in (True, False)}
    best = {}
    for _ in range(reps):
        for f, plan in plans.items():
            best[f] = min(best.get(f, 1e9), _time(plan, iters))
    same = torch.equal(plans[True].q8, plans[False].q8) and torch.equal(plans[True].sc, plans[False].sc)
    split = lib.gemm_last_split()
    print(f"gemm8 + bias + tanh-GELU -> MX fp8 M={M} N={N} K={K}: activation epilogue {best[True]:.4f} ms ({2 * M * N * K / best[True] / 1e9:.0f} TF), "
          f"GEMM + quantiser launch {best[False]:.4f} ms ({2 * M * N * K / best[False] / 1e9:.0f} TF); same bytes: {same} "
          f"(the unfused GEMM's whole tiles, K slices, pieces = {split})", flush=True)


def _kontext_dits(layers, singles, modes, seed=11):
    from mangatranslator_amd.core.ml import flux as fx
    cfg = dict(fx.KONTEXT_DIT_CFG, layers=layers, single_layers=singles)
    shapes = fx.dit_param_shapes(cfg)
    # the same seeded weights for every mode: the provider is re-created per graph (it draws tensor by tensor from one generator, in load order)
    return cfg, {m: fx.FluxDiTHip(fx.synthetic_provider(shapes, dev, seed), cfg, dev, lib=lib, fp8=m) for m in modes}


def kontext_step_ab(h2, w2, layers=19, singles=38, t_txt=512, reps=3, iters=3):
    """One FLUX.1-Kontext denoising step, bf16 against fp8 block linears on the same seeded weights, graph replays alternating in one process;
    the block linears' share of each (plan.time_ops) and the fp8 linears' rate against the 5 PF MX-fp8 peak"""
    cfg, dits = _kontext_dits(layers, singles, (False, True))
    g = torch.Generator(device=dev).manual_seed(3)
    plans, groups = {}, {}
    for m, dit in dits.items():
        plan = dit.plan_for(t_txt, h2, w2, 1)
        plan.ctx_in.normal_(generator=g); plan.lat.normal_(generator=g)
        plan.mod.copy_(dit.modulation(0.7, 2.5, torch.zeros(cfg["pooled_dim"], device=dev, dtype=torch.bfloat16)))
        plans[m] = plan
        groups[m] = [i for i, (lb, o) in enumerate(zip(plan.labels, plan.ops)) if o.kind == abi.OP_GEMM and lb.startswith(("dbl", "sgl"))]
    step, gemms = {}, {}
    for _ in range(reps):
        for m, plan in plans.items():
            plan.run(graph=True); torch.cuda.synchronize()
            step[m] = min(step.get(m, 1e9), plan.time(iters, graph=True))
            gemms[m] = min(gemms.get(m, 1e9), plan.time_ops(groups[m], iters) / iters)
    fl = dits[True].flops_per_step(t_txt, h2, w2, 1)["gemm"]
    nq = sum(1 for o in plans[True].ops if o.kind == abi.OP_QUANT)
    print(f"Kontext step {layers}+{singles} blocks T={plans[True].T}: bf16 {step[False]:.2f} ms (block linears {gemms[False]:.2f} ms, {fl / gemms[False] / 1e9:.0f} TF), "
          f"fp8 {step[True]:.2f} ms (block linears {gemms[True]:.2f} ms, {fl / gemms[True] / 1e9:.0f} TF = {fl / gemms[True] / 1e9 / 5000:.2f} of the 5 PF fp8 peak); "
          f"quantiser launches left in the fp8 step: {nq}", flush=True)


def kontext_psnr(h, w, layers=4, singles=8, steps=4, t_txt=512):
    """4-step image PSNR of the fp8 Kontext pipeline against the bf16 one on the same seeded full-width weights (reduced depth)"""
    import math
    import numpy as np
    from mangatranslator_amd.core.ml import flux as fx
    cfg, dits = _kontext_dits(layers, singles, (False, True))
    vshapes = fx.vae_param_shapes(fx.KONTEXT_VAE_CFG)
    g = torch.Generator().manual_seed(1)
    img = (torch.rand(h, w, 3, generator=g) * 255).to(torch.uint8).numpy()
    pe = torch.randn(t_txt, cfg["joint_dim"], generator=g)
    pooled = torch.randn(cfg["pooled_dim"], generator=g)
    noise = torch.randn(1, 16, h // 8, w // 8, generator=g)
    outs = {}
    for m, dit in dits.items():
        vae = fx.FluxVAEHip(fx.synthetic_provider(vshapes, dev, 12), dict(fx.KONTEXT_VAE_CFG), dev, lib=lib)
        pipe = fx.FluxKontextHip(dit, vae)
        outs[m] = pipe(image=img, width=w, height=h, num_inference_steps=steps, guidance_scale=2.5, prompt_embeds=pe[None],
                       pooled_prompt_embeds=pooled[None], latents=noise).images[0].float().cpu()
    mse = ((outs[True] - outs[False]) ** 2).mean().item()
    T = t_txt + 2 * (h // 16) * (w // 16)
    print(f"Kontext {steps} steps {w}x{h} (T={T}, {layers}+{singles} blocks, d=3072, seeded weights): fp8 block linears vs bf16 image PSNR "
          f"{99.0 if mse == 0 else 10 * math.log10(1.0 / mse):.1f} dB", flush=True)


def gemm(M, N, K, iters=20, f8=False, pad=0, flags=0, act=0):
    """pad > 0: rows of A and W are `pad` elements apart more than K (leading-dimension padding, an address-interleave probe)"""
    pb = PlanBuilder(lib, dev, abi.BF16)
    a = pb.buf((M, K + pad), torch.bfloat16); a.normal_()
    w = pb.buf((N, K + pad), torch.bfloat16); w.normal_(0, K ** -0.5)
    if f8:
        q = PlanBuilder(lib, dev, abi.BF16)
        aq, asc, la = q.quantize(a, M, K)
        wq, wsc, lw = q.quantize(w, N, K)
        q.build().run(); torch.cuda.synchronize()
        pb.keep += [aq, asc, wq, wsc]
        pb.gemm(aq, wq, M, N, K, f8=(asc, la, wsc, lw, 0, 0), flags=flags)
    else:
        pb.gemm(a, w, M, N, K, lda=K + pad, ldw=K + pad, flags=flags, act=act, bias=(pb.buf((N,), torch.float32, zero=True) if act else None))
    ms = _time(pb.build(), iters)
    split = lib.gemm_last_split()
    tag = " [whole tiles only]" if flags & abi.GEMM_NO_SPLIT else f" [whole tiles, K slices, pieces = {split}]"
    if act:
        tag += " [bias + tanh-GELU epilogue]"
    print(f"gemm{'8' if f8 else ''} M={M} N={N} K={K}{f' ld+{pad}' if pad else ''}{tag}: {ms:.3f} ms  {2 * M * N * K / ms / 1e9:.0f} TFLOP/s", flush=True)


def gemm_epi(M, N, K, kind, f8=False, reps=3, iters=20):
    """The 256-tile kernels with the epilogue a FLUX linear really has — kind "b": bias; "g": bias + tanh-GELU; "r": bias + gate + residual
    (attention / MLP output projections).  (Round 5 compared the batched epilogue with the one-at-a-time form here: profiles/r05_visit_q_*.log.)"""
    pb = PlanBuilder(lib, dev, abi.BF16)
    g = torch.Generator(device=dev).manual_seed(5)
    a = pb.buf((M, K), torch.bfloat16); a.normal_(generator=g)
    w = pb.buf((N, K), torch.bfloat16); w.normal_(0, K ** -0.5, generator=g)
    bias = pb.buf((N,), torch.float32); bias.normal_(generator=g)
    gate = res = None
    if kind == "r":
        gate = pb.buf((2, N), torch.bfloat16); gate.normal_(generator=g)
        res = pb.buf((M, N), torch.bfloat16); res.normal_(generator=g)
    kw = dict(bias=bias, act=abi.ACT_GELU_TANH if kind == "g" else 0, res=res, gate=gate, gate_rows_per=(M + 1) // 2)
    if f8:
        q = PlanBuilder(lib, dev, abi.BF16)
        aq, asc, la = q.quantize(a, M, K)
        wq, wsc, lw = q.quantize(w, N, K)
        q.build().run(); torch.cuda.synchronize()
        pb.keep += [aq, asc, wq, wsc]
        pb.gemm(aq, wq, M, N, K, f8=(asc, la, wsc, lw, 0, 0), **kw)
    else:
        pb.gemm(a, w, M, N, K, **kw)
    plan = pb.build()
    best = min(_time(plan, iters) for _ in range(reps))
    what = {"b": "bias", "g": "bias + tanh-GELU", "r": "bias + gate + residual"}[kind]
    print(f"gemm{'8' if f8 else ''} M={M} N={N} K={K} [{what}]: {best:.3f} ms ({2 * M * N * K / best / 1e9:.0f} TFLOP/s)", flush=True)


def gemm_strips(M, N, K, f8=False, reps=3, iters=20, kind="b"):
    """Round 6: the workgroup -> tile map of the 256-tile kernels with 1 (rounds 1-5), 2, 4, 8 column strips and the launcher's own choice (0),
    alternating in one process (the launcher reads MTX_GEMM_STRIPS per launch); the outputs must be the same bytes."""
    pb = PlanBuilder(lib, dev, abi.BF16)
    g = torch.Generator(device=dev).manual_seed(5)
    a = pb.buf((M, K), torch.bfloat16); a.normal_(generator=g)
    w = pb.buf((N, K), torch.bfloat16); w.normal_(0, K ** -0.5, generator=g)
    bias = pb.buf((N,), torch.float32); bias.normal_(generator=g)
    kw = dict(bias=bias, act=abi.ACT_GELU_TANH if kind == "g" else 0)
    if f8:
        q = PlanBuilder(lib, dev, abi.BF16)
        aq, asc, la = q.quantize(a, M, K)
        wq, wsc, lw = q.quantize(w, N, K)
        q.build().run(); torch.cuda.synchronize()
        pb.keep += [aq, asc, wq, wsc]
        out = pb.gemm(aq, wq, M, N, K, f8=(asc, la, wsc, lw, 0, 0), **kw)
    else:
        out = pb.gemm(a, w, M, N, K, **kw)
    plan = pb.build()
    variants = (1, 2, 4, 0)                    # strips; 0 = the launcher's choice
    best, ref, same = {}, None, True
    for _ in range(reps):
        for st in variants:
            os.environ["MTX_GEMM_STRIPS"] = str(st)
            out.zero_()
            ms = _time(plan, iters)
            best[st] = min(best.get(st, 1e9), ms)
            if ref is None:
                ref = out.clone()
            same = same and torch.equal(out, ref)
    os.environ.pop("MTX_GEMM_STRIPS", None)
    print(f"gemm{'8' if f8 else ''} M={M} N={N} K={K} strips -> ms: " + "  ".join(f"{'auto' if st == 0 else st}: {best[st]:.4f} ({2 * M * N * K / best[st] / 1e9:.0f} TF)" for st in variants)
          + f"  same bytes: {same}", flush=True)


def quant(rows, K, iters=20):
    pb = PlanBuilder(lib, dev, abi.BF16)
    a = pb.buf((rows, K), torch.bfloat16); a.normal_()
    pb.quantize(a, rows, K)
    ms = _time(pb.build(), iters)
    print(f"quantize_mx rows={rows} K={K}: {ms * 1e3:.1f} us  {rows * K * (3 + 1 / 32) / ms / 1e6:.0f} GB/s", flush=True)


def conv(H, W, iters=20):
    """RCAN body conv 64 -> 64 (f16) at page resolution"""
    pb = PlanBuilder(lib, dev, abi.F16)
    x = pb.act(1, H, W, 64); x.t.normal_()
    w = pb.buf((64, 9, 64), torch.float16); w.normal_(0, 0.04)
    b = pb.buf((64,), torch.float32, zero=True)
    pb.conv2d(x, w, b, 64, act=abi.ACT_RELU)
    ms = _time(pb.build(), iters)
    byts = 2 * 64 * H * W * 2 + 9 * 64 * 64 * 2
    print(f"conv3x3 64->64 {W}x{H}: {ms * 1e3:.1f} us  {byts / ms / 1e6:.0f} GB/s  {2 * 9 * 64 * 64 * H * W / ms / 1e9:.0f} TFLOP/s", flush=True)


def norm(rows, c, reps=3, iters=50, q8=False):
    """adaLN LayerNorm rows of a FLUX block (no affine, modulation rows per stream); q8: the FLUX.2 form (MX fp8 twin from the registers, no
    16-bit store).  (Round 5 compared four kernel forms here: profiles/r05_visit_o / _p logs.)"""
    pb = PlanBuilder(lib, dev, abi.BF16)
    x = pb.buf((rows, c), torch.bfloat16); x.normal_()
    ms_, mh_ = pb.buf((2, c), torch.bfloat16), pb.buf((2, c), torch.bfloat16)
    ms_.normal_(); mh_.normal_()
    rows_per = (rows + 1) // 2
    lds = (rows + 63) // 64 * 64
    if q8:
        q, sc = pb.buf((rows, c), torch.uint8, zero=True), pb.buf((c // 128, lds), torch.int32, zero=True)
        pb.norm(x, None, rows, c, eps=1e-6, kind=0, mod_scale=ms_, mod_shift=mh_, rows_per=rows_per, ldmod=c, q8=(q, sc), lds_q=lds)
    else:
        y = pb.buf((rows, c), torch.bfloat16)
        pb.norm(x, y, rows, c, eps=1e-6, kind=0, mod_scale=ms_, mod_shift=mh_, rows_per=rows_per, ldmod=c)
    plan = pb.build()
    t_ms = min(_time(plan, iters) for _ in range(reps))
    byts = rows * c * (2 + (1 if q8 else 2))
    print(f"norm {rows}x{c} {'-> MX fp8' if q8 else 'bf16'}: {t_ms * 1e3:.1f} us  {byts / t_ms / 1e6:.0f} GB/s", flush=True)


def sam3(layers=32, boxes=8, iters=5):
    """SAM 3 (seeded weights, the shipped widths at 1008 x 1008; `layers` < 32 for a quick look): encoder ms at "fast" and "high", decoder ms per
    `boxes` boxes, and where the encoder's time goes — per group of launches, each group timed in context (`Plan.time_ops`: a replay of the
    whole plan minus a replay without the group)"""
    from transformers import Sam3TrackerConfig, Sam3TrackerModel
    from mangatranslator_amd.core.ml.sam3 import Sam3Hip
    cfg = Sam3TrackerConfig()
    bb = cfg.vision_config.backbone_config
    bb.num_hidden_layers = layers
    bb.global_attn_indexes = [i for i in bb.global_attn_indexes if i < layers]
    torch.manual_seed(0)
    sd = Sam3TrackerModel(cfg).state_dict()
    T, C, M, d = 72 * 72, bb.hidden_size, bb.intermediate_size, bb.hidden_size // bb.num_attention_heads
    nglob = len(bb.global_attn_indexes)
    lin = 2 * T * layers * (4 * C * C + 2 * C * M)
    att = 4 * C * ((layers - nglob) * T * bb.window_size ** 2 + nglob * T * T)
    print(f"sam3 work per page, {layers} layers: linears 2 T L (4 C^2 + 2 C M) = {lin / 1e12:.2f} TFLOP, attention 4 C (Lw T w^2 + Lg T^2) = {att / 1e12:.2f} TFLOP "
          f"(T = {T}, C = {C}, M = {M}, w^2 = {bb.window_size ** 2}, Lg = {nglob})", flush=True)
    for precision in ("fast", "high"):
        hipm = Sam3Hip(sd, cfg, device=dev, lib=lib, dtype=abi.F16, precision=precision)
        pre, enc, dec, post = hipm.plans(boxes, 1536, 1024)
        enc.img.t.normal_(); dec.tok0.normal_()
        enc.run(graph=True); dec.run(graph=True); torch.cuda.synchronize()
        enc.time(2, graph=True); dec.time(2, graph=True)
        e_ms = min(enc.time(iters, graph=True) for _ in range(3))
        d_ms = min(dec.time(iters, graph=True) for _ in range(3))
        print(f"sam3 {precision!r} f16, 1008 x 1008, {layers} layers: encoder {e_ms:.2f} ms ({len(enc.labels)} launches, {(lin * (2 if precision == 'high' else 1) + att) / e_ms / 1e9:.0f} TFLOP/s issued), "
              f"decoder {d_ms:.2f} ms per {boxes} boxes, pre {pre.time(iters):.3f} ms, post {post.time(iters):.3f} ms", flush=True)
        globs = {f"layer{i}" for i in bb.global_attn_indexes}
        groups = {}
        for i, lb in enumerate(enc.labels):
            head, _, tail = lb.partition(".")
            if head.startswith("layer"):
                key = tail if tail != "attn" else ("attn.global" if head in globs else "attn.window")
            else:
                key = head if head.startswith("neck") else lb
            groups.setdefault(key, []).append(i)
        parts = {k: enc.time_ops(v, iters) / iters for k, v in groups.items()}
        print("  per group, ms (launches): " + "  ".join(f"{k} {ms:.3f} ({len(groups[k])})" for k, ms in sorted(parts.items(), key=lambda kv: -kv[1])), flush=True)
        del hipm


def mangaocr(dec_layers=2, beams=4, reps=3, iters=20):
    """manga-ocr at the published widths (ViT-B/16 at 224 px, BERT decoder 768 / 12 heads, vocabulary 6144; seeded weights; the shipped decoder
    depth is not known: `dec_layers`): encoder ms, ms per decode step with every linear on the skinny-row kernel, on the tile GEMM, and with ONE
    shape moved to the GEMM — the step graphs built side by side in one process and timed in alternation (whole-graph replays) — and wall ms per
    crop at 10 and at 300 tokens (encoder + steps with their upload / download, no search)."""
    import time
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import manga_ocr_checks as mc
    from mangatranslator_amd.core.ml import manga_ocr as mo
    dims = dict(mc.REAL, d=dict(mc.REAL["d"], num_hidden_layers=dec_layers))
    mc.REAL.update(dims)
    model, pixels = mc.oracle(0, real=True)
    C, M, V = 768, 3072, 6144
    shapes = {"qkv": (3 * C, C), "proj": (C, C), "fc1": (M, C), "fc2": (C, M), "head": (V, C)}
    routes = {"rowlin": lambda r, n, k: "rowlin", "gemm": lambda r, n, k: "gemm"}
    for name, nk in shapes.items():
        routes[f"rowlin, {name} on gemm"] = (lambda r, n, k, nk=nk: "gemm" if (n, k) == nk else "rowlin")
    routes["shipped"] = mo.linear_route
    models = {k: mc.hip_model(lib, model, abi.F16, rows=beams, gen=dict(max_length=300, num_beams=beams), route=f) for k, f in routes.items()}
    first = next(iter(models.values()))
    first.encode_pixels(pixels[0]); torch.cuda.synchronize()
    enc = first._encoder()
    enc.time(3, graph=True)
    print(f"mangaocr f16, {dec_layers} decoder layers, {beams} rows: encoder {min(enc.time(iters, graph=True) for _ in range(reps)):.3f} ms ({len(enc.labels) if hasattr(enc, 'labels') else enc.n_ops} launches)", flush=True)
    best = {k: 1e9 for k in models}
    for k, m in models.items():
        m.encode_pixels(pixels[0])
        m.step(mo.BeamStep(0, [2] * beams, list(range(beams))))
        m._stepper().ctl[0] = 150                                  # a mid-length history for the attention
        m._stepper().time(3, graph=True)
    for _ in range(reps):                                          # alternate the graphs: same process, same clocks
        for k, m in models.items():
            best[k] = min(best[k], m._stepper().time(iters, graph=True))
    for k, ms in best.items():
        print(f"  step graph, linears on {k}: {ms:.4f} ms per step ({models[k]._stepper().n_ops} launches)", flush=True)
    m = models["shipped"]
    for tokens in (10, 300):
        walls = []
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            m.encode_pixels(pixels[0])
            for i in range(tokens - 1):
                m.step(mo.BeamStep(i, [2 + i % 7] * beams, list(range(beams))))
            walls.append((time.perf_counter() - t0) * 1e3)
        print(f"  per crop at {tokens} tokens ({beams} beams): {min(walls):.1f} ms wall (encoder + {tokens - 1} steps with upload / download)", flush=True)


def paddleocr(reps=3, iters=20):
    """PaddleOCR-VL at the wheel's default widths with the vocabulary cut to 8 192 (seeded weights): prefill ms at T = 300 / 1 300, ms per decode
    step at a cache of 300 / 2 300 positions with the step's linears on the skinny-row kernel and on the tile GEMM, tokens/s of the shipped route"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import paddle_ocr_vl_checks as pc
    routes = {"rowlin": lambda r, n, k: "rowlin", "gemm": lambda r, n, k: "gemm"}
    models = {k: pc.hip_model(lib, abi.F16, 0, real=True, max_new_tokens=1024, max_prompt=1344, route=f) for k, f in routes.items()}
    m = models["rowlin"]
    for T, grid in ((300, (28, 40)), (1300, (64, 80))):
        n_img = grid[0] * grid[1] // 4
        pre = m._prefill(T, 4, n_img)
        m.state.zero_(); pre.run(); torch.cuda.synchronize()
        best = 1e9
        for _ in range(reps):
            m.state.zero_()
            best = min(best, pre.time(1))
        print(f"paddleocr f16: prefill T = {T}: {best:.3f} ms ({pre.n_ops} launches)", flush=True)
    for k, mm in models.items():
        step = mm._stepper()
        for cache in (300, 2300):
            best = 1e9
            for _ in range(reps):
                mm.state.copy_(torch.tensor([cache, 0, 0, 5], dtype=torch.int32)); step.run(graph=True); torch.cuda.synchronize()
                mm.state.copy_(torch.tensor([cache, 0, 1, 5], dtype=torch.int32))          # done: the state stands still while the graph is timed
                best = min(best, step.time(iters, graph=True))
            print(f"  step graph, linears on {k}, cache {cache}: {best:.4f} ms per step = {1e3 / best:.0f} tokens/s ({step.n_ops} launches)", flush=True)


def paddleocr_batch(reps=3, windows=4, iters=60):
    """the slot-batched step graph (`PaddleOcrVlHip(slots=B)._stepper_batch()`) at B = 1, 2, 4, 8 beside the single-sequence step graph, same
    widths as `paddleocr`, caches of 300 and 2 300 positions.  Finished slots skip attention, so nothing is timed at done = 1: every window is a
    run of `iters` LIVE steps from the same start position, the state reset before it; a repetition is the mean of `windows` windows, the graphs
    alternate inside a repetition, the figure is the best repetition and the spread (max - min over the repetitions) is printed beside it."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import paddle_ocr_vl_checks as pc
    kw = dict(real=True, max_new_tokens=1024, max_prompt=1344)
    single = pc.hip_model(lib, abi.F16, 0, **kw)
    batched = {}
    for B in (1, 2, 4, 8):
        batched[B] = pc.hip_model(lib, abi.F16, 0, slots=max(B, 2), **kw)
        batched[B].slots = B                                       # (B = 1: the batched plan on one row of a two-slot model's buffers)

    def reset(m, B, cache):
        if B == 0:
            m.state.copy_(torch.tensor([cache, 0, 0, 5], dtype=torch.int32))
            return
        st = torch.zeros(abi.SLOT_FIELDS, abi.SLOTS_MAX, dtype=torch.int32)
        st[abi.SLOT_DONE] = 1
        st[abi.SLOT_POS, :B], st[abi.SLOT_DONE, :B], st[abi.SLOT_ROPE, :B] = cache, 0, cache
        st[abi.SLOT_TOKEN, :B] = 5 + torch.arange(B, dtype=torch.int32)
        m.slot_state.copy_(st)

    plans = {0: (single, single._stepper())}
    plans.update({B: (m, m._stepper_batch()) for B, m in batched.items()})
    for cache in (300, 2300):
        assert cache + iters < single.max_len
        for B, (m, plan) in plans.items():                         # warm every graph at this start position
            reset(m, B, cache)
            for _ in range(3):
                plan.run(graph=True)
            torch.cuda.synchronize()
        runs = {B: [] for B in plans}
        for _ in range(reps):
            for B, (m, plan) in plans.items():
                ms = []
                for _ in range(windows):
                    reset(m, B, cache); torch.cuda.synchronize()
                    ms.append(plan.time(iters, graph=True))
                runs[B].append(sum(ms) / len(ms))
        base = min(runs[0])
        for B, (m, plan) in plans.items():
            best, spread, n = min(runs[B]), max(runs[B]) - min(runs[B]), max(B, 1)
            name = "single step graph" if B == 0 else f"batched step graph B = {B}"
            print(f"  {name}, cache {cache}: {best:.4f} ms per step (spread {spread:.4f} over {reps} repetitions) = {n * 1e3 / best:.0f} tokens/s aggregate, "
                  f"{n * base / best:.2f} x the single step ({plan.n_ops} launches)", flush=True)


def paddleocr_fill(reps=3):
    """what feeds PaddleOCR-VL's decode slots, per crop against packed (`PaddleOcrVlHip(slots=8, packed_prefill=True)`): f16, the widths of
    `paddleocr`, eight items with the grids of the published-width checks, cycled.  Wall ms, each figure ending in a synchronise, the two
    paths alternating inside a repetition, best of `reps` with the spread (max - min) beside it: the per-crop fill of 8 slots with its plans
    warm, the same with eight DISTINCT grids (the page case: the bounded plan caches rebuild, plan builds included), the packed fill of 8;
    one per-crop fill against a packed fill of 1 (the steady-state refill).  Then the plans alone: vision per crop, the packed plans."""
    import time
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import paddle_ocr_vl_checks as pc

    def items_of(grids):
        out = []
        for k, grid in enumerate(grids):
            ids, pix, thw = pc.make_inputs(k, grid=grid)
            out.append(dict(input_ids=ids, pixel_values=pix, image_grid_thw=thw))
        return out
    cycle = [(20, 28), (28, 40), (8, 12)]
    warm_items = items_of([cycle[k % 3] for k in range(8)])
    page_items = items_of([(20, 28), (28, 40), (8, 12), (16, 20), (12, 24), (24, 24), (10, 30), (18, 22)])
    kw = dict(real=True, max_new_tokens=1024, max_prompt=1344, slots=8)
    per_crop, packed = pc.hip_model(lib, abi.F16, 0, **kw), pc.hip_model(lib, abi.F16, 0, packed_prefill=True, **kw)

    def empty(m):
        m.slot_state.zero_(); m.slot_state[abi.SLOT_DONE] = 1

    def wall(f):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    runs = {
        "per-crop fill of 8, plans warm": lambda: [per_crop._fill_slot(s, it) for s, it in enumerate(warm_items)],
        "per-crop fill of 8, eight distinct grids (plan builds included)": lambda: [per_crop._fill_slot(s, it) for s, it in enumerate(page_items)],
        "packed fill of 8": lambda: packed.fill_slots(list(enumerate(warm_items))),
        "packed fill of 8, eight distinct grids": lambda: packed.fill_slots(list(enumerate(page_items))),
        "one per-crop fill (20 x 28)": lambda: per_crop._fill_slot(0, warm_items[0]),
        "packed fill of 1 (20 x 28)": lambda: packed.fill_slots([(0, warm_items[0])]),
    }
    for name in ("per-crop fill of 8, plans warm", "packed fill of 8", "packed fill of 8, eight distinct grids", "packed fill of 1 (20 x 28)"):      # warm: plans, graphs
        for _ in range(2):
            empty(packed); runs[name]()
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    page, page_packed = "per-crop fill of 8, eight distinct grids (plan builds included)", "packed fill of 8, eight distinct grids"
    for _ in range(reps):
        for name in (page, page_packed, None, "per-crop fill of 8, plans warm", "packed fill of 8", "one per-crop fill (20 x 28)", "packed fill of 1 (20 x 28)"):
            empty(packed); empty(per_crop)
            if name is None:                                       # the page case has turned the bounded plan caches over: warm them again, untimed
                runs["per-crop fill of 8, plans warm"]()
                continue
            ms[name].append(wall(runs[name]))
    print(f"paddleocr_fill f16, 8 slots, max_prompt 1344; packed ladders {packed.pk_vis_ladder} patches / {packed.pk_txt_ladder} rows", flush=True)
    for name, v in ms.items():
        print(f"  {name}: {min(v):.2f} ms (spread {max(v) - min(v):.2f} over {reps} repetitions)", flush=True)
    a, b = min(ms["per-crop fill of 8, plans warm"]), min(ms["packed fill of 8"])
    c, d = min(ms["one per-crop fill (20 x 28)"]), min(ms["packed fill of 1 (20 x 28)"])
    print(f"  packed 8 against per-crop 8 (warm): {a / b:.2f} x; the page case: {min(ms[page]) / min(ms[page_packed]):.2f} x; "
          f"packed 1 against one per-crop fill: {c / d:.2f} x", flush=True)
    # the plans alone (event-timed replays)
    for grid in cycle:
        vis = per_crop._vision(*grid)
        vis.time(2)
        print(f"  vision plan per crop, grid {grid[0]} x {grid[1]} ({grid[0] * grid[1]} patches): {min(vis.time(5) for _ in range(reps)):.3f} ms eager ({vis.n_ops} launches)", flush=True)
    empty(packed); packed.fill_slots(list(enumerate(warm_items)))
    for what, plans in (("vision", packed._pk_vis), ("text", packed._pk_txt)):
        for cap, plan in sorted(plans.items()):
            plan.time(2, graph=True)
            print(f"  packed {what} plan, capacity {cap}: {min(plan.time(5, graph=True) for _ in range(reps)):.3f} ms per replay ({plan.n_ops} launches)", flush=True)
    per_crop.close(); packed.close()


def mangaocr_batch(reps=3, iters=40, crops=16):
    """manga-ocr's batched step graph (`MangaOcrHip(slots=S)._stepper_batch()`: wide row linears, group-batched attention, the beam search on the
    device) at S = 1, 2, 4, 8 beside today's 4-row step graph: published widths, f16, 4 beams, a 300-position cache.  Whole-graph replays; the
    batched graph advances its own positions, so every window is `iters` LIVE steps from position 150 with the state reset before it (no group
    at done = 1; the count of groups still searching after the window is printed), every window is warmed, the graphs alternate inside a
    repetition, the figure is the best repetition with the spread beside it.  Then `crops` synthetic crops by the wall, `recognise_many` at
    S = 8 against a loop of `__call__`, alternating, each ending in a synchronise, at max_length 32 and 300 (seeded weights never end a
    hypothesis early, so a crop costs max_length - 1 steps)."""
    import ctypes as C
    import time
    import numpy as np
    from PIL import Image
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import manga_ocr_checks as mc
    model, pixels = mc.oracle(0, real=True)
    B, START = 4, 150
    gen = dict(mc.GEN, max_length=300, num_beams=B)
    single = mc.hip_model(lib, model, abi.F16, rows=B, gen=gen)
    batched = {S: mc.hip_model(lib, model, abi.F16, rows=B, gen=gen, slots=S) for S in (1, 2, 4, 8)}
    single.encode_pixels(pixels[0])
    single.step(mc.mo.BeamStep(0, [2] * B, list(range(B))))
    single._stepper().ctl[0] = START
    plans = {0: single._stepper()}
    for S, m in batched.items():
        plan = m._stepper_batch()
        m.encode_pixels(pixels[0])
        for s in range(S):
            m._reset_group(plan, s)
        st = plan.state[0].clone()
        L = m.max_len
        run = abi.beam_running(B, L)
        st[run:run + B * L] = 5
        st[abi.BEAM_POS] = START
        st.view(torch.float32)[abi.BEAM_RSCORE:abi.BEAM_RSCORE + B] = torch.tensor([-10.0, -11.0, -12.0, -13.0], device=st.device)
        plan.start_state = st[None].expand(S, -1).contiguous()
        plan.idx[1] = START
        plans[S] = plan

    def reset(S):
        if S:
            plans[S].state.copy_(plans[S].start_state)
        torch.cuda.synchronize()

    for S, plan in plans.items():
        reset(S)
        plan.time(3, graph=True)
    runs, alive = {S: [] for S in plans}, {}
    for _ in range(reps):
        for S, plan in plans.items():
            reset(S)
            plan.time(3, graph=True)                               # warm this window
            reset(S)
            runs[S].append(plan.time(iters, graph=True))
            if S:
                alive[S] = int((plan.state[:, abi.BEAM_DONE] == 0).sum())
    base = min(runs[0])
    for S, plan in plans.items():
        best, spread, n = min(runs[S]), max(runs[S]) - min(runs[S]), max(S, 1)
        name = "single 4-row step graph (no search)" if S == 0 else f"batched step graph S = {S} ({alive[S]} of {S} groups still searching)"
        print(f"  {name}: {best:.4f} ms per step (spread {spread:.4f} over {reps} repetitions) = {n * 1e3 / best:.0f} groups x tokens/s, "
              f"{n * base / best:.2f} x the single step ({plan.n_ops} launches)", flush=True)
    p8 = plans[8]
    idx = [p8.beam_op]
    ms = C.c_float(0.0)
    reset(8)
    lib.check(lib.mtx_plan_time_ops(p8._h, None, (C.c_int * 1)(*idx), 1, 20, C.byref(ms)), "mtx_plan_time_ops")
    print(f"  beam step inside the S = 8 graph (graph with minus graph without): {ms.value / 20:.4f} ms", flush=True)
    enc = single._encoder()
    enc.time(3, graph=True)
    enc_ms = min(enc.time(10, graph=True) for _ in range(reps))
    print(f"  encoder: {enc_ms:.3f} ms per crop", flush=True)
    for m in [single, *batched.values()]:
        m.close()
    imgs = []
    for i in range(crops):
        h, w = 40 + 13 * (i % 5), 48 + 17 * (i % 7)
        yy, xx = np.mgrid[0:h, 0:w]
        imgs.append(Image.fromarray(((xx * (3 + i) + yy * (5 + 2 * i)) % 97 + 80).astype(np.uint8)).convert("RGB"))
    for max_length in (32, 300):
        g = dict(mc.GEN, max_length=max_length, num_beams=B)
        one, many = mc.hip_model(lib, model, abi.F16, rows=B, gen=g), mc.hip_model(lib, model, abi.F16, rows=B, gen=g, slots=8)
        want = [one(im) for im in imgs[:2]]
        got = many.recognise_many(imgs)                            # warms both paths (plans, graphs, pre-processing plans)
        for im in imgs[2:]:
            one(im)
        walls = {"loop": [], "many": []}
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            a = [one(im) for im in imgs]
            torch.cuda.synchronize(); walls["loop"].append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            b = many.recognise_many(imgs)
            torch.cuda.synchronize(); walls["many"].append((time.perf_counter() - t0) * 1e3)
        same = sum(x == y for x, y in zip(a, b))
        lo, mo_ = walls["loop"], walls["many"]
        print(f"  {crops} crops, max_length {max_length}: loop of __call__ {min(lo):.1f} ms (spread {max(lo) - min(lo):.1f}), recognise_many S = 8 "
              f"{min(mo_):.1f} ms (spread {max(mo_) - min(mo_):.1f}) = {min(lo) / min(mo_):.2f} x; encoder share of the batched page "
              f"{crops * enc_ms / min(mo_) * 100:.0f} %; {same} of {crops} texts equal", flush=True)
        one.close(); many.close()


def textenc(wheel_layers=2, reps=3, S=512):
    """FLUX's prompt encoders (core/ml/text_encoders.py) at the published widths, seeded bf16 weights made on the device, S = 512: Qwen3 at
    Klein-4B's widths (27 of 36 layers run) and T5-XXL (24 blocks) — ms per encode as the plan's HIP-event time and as the wall of `encode_ids`
    (host gather, upload, plan, synchronise).  Beside each the wall of the wheel's class on THIS box's CPU in bf16 for `wheel_layers` layers;
    the whole-model wheel figure printed from it is an extrapolation (layers x per-layer), not a measurement."""
    import time
    from transformers import Qwen3Config, Qwen3ForCausalLM, T5Config, T5EncoderModel
    from mangatranslator_amd.core.ml import text_encoders as te
    g = torch.Generator(device=dev).manual_seed(0)
    W = lambda *shape, sc=0.02: (torch.randn(*shape, device=dev, generator=g) * sc).to(torch.bfloat16)
    G = lambda n: (torch.rand(n, device=dev, generator=g) + 0.5).to(torch.bfloat16)
    ids = torch.randint(0, 1024, (S,), generator=torch.Generator().manual_seed(0))

    def report(name, enc, layers, run, wheel, wheel_run):
        plan = enc._plan(S)
        run()
        ms = _time(plan, 5)
        walls = []
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            run()
            walls.append((time.perf_counter() - t0) * 1e3)
        enc.close()
        wheel_run(); t = []
        for _ in range(2):
            t0 = time.perf_counter(); wheel_run(); t.append((time.perf_counter() - t0) * 1e3)
        per = min(t) / wheel_layers
        print(f"textenc {name}: {layers} layers, S = {S}: plan {ms:.3f} ms ({plan.n_ops} launches), encode_ids wall {min(walls):.2f} ms (spread "
              f"{max(walls) - min(walls):.2f}); wheel on this box's CPU, bf16, {wheel_layers} layers: {min(t):.0f} ms = {per:.0f} ms per layer, "
              f"{layers} layers EXTRAPOLATED (not measured) {per * layers / 1e3:.1f} s", flush=True)

    C, H, KV, I, L = 2560, 32, 8, 9728, 27
    sd = {"model.embed_tokens.weight": W(1024, C, sc=0.1).cpu()}
    for i in range(L):
        p = f"model.layers.{i}."
        sd.update({p + "input_layernorm.weight": G(C), p + "post_attention_layernorm.weight": G(C), p + "self_attn.q_norm.weight": G(128),
                   p + "self_attn.k_norm.weight": G(128), p + "self_attn.q_proj.weight": W(H * 128, C), p + "self_attn.k_proj.weight": W(KV * 128, C),
                   p + "self_attn.v_proj.weight": W(KV * 128, C), p + "self_attn.o_proj.weight": W(C, H * 128), p + "mlp.gate_proj.weight": W(I, C),
                   p + "mlp.up_proj.weight": W(I, C), p + "mlp.down_proj.weight": W(C, I)})
    cfg = dict(hidden_size=C, num_attention_heads=H, num_key_value_heads=KV, head_dim=128, intermediate_size=I, num_hidden_layers=36, rms_norm_eps=1e-6,
               rope_theta=1e6)
    enc = te.Qwen3EncoderHip(sd, cfg, taps=(9, 18, 27), device=dev, lib=lib)
    del sd
    wheel = Qwen3ForCausalLM(Qwen3Config(hidden_size=C, num_attention_heads=H, num_key_value_heads=KV, head_dim=128, intermediate_size=I,
                                         num_hidden_layers=wheel_layers, vocab_size=1024)).to(torch.bfloat16).eval()
    with torch.no_grad():
        report("Qwen3 (Klein-4B widths)", enc, L, lambda: enc.encode_ids(ids, 40), wheel,
               lambda: wheel(input_ids=ids[None], attention_mask=(torch.arange(S) < 40).long()[None], output_hidden_states=True, use_cache=False))
    del enc, wheel
    torch.cuda.empty_cache()

    C, H, F, L = 4096, 64, 10240, 24
    sd = {"shared.weight": W(1024, C, sc=1.0).cpu(), "encoder.final_layer_norm.weight": G(C),
          "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": W(32, H, sc=2.0)}
    for i in range(L):
        p = f"encoder.block.{i}.layer."
        sd.update({p + "0.layer_norm.weight": G(C), p + "1.layer_norm.weight": G(C), p + "0.SelfAttention.q.weight": W(C, C, sc=0.015),
                   p + "0.SelfAttention.k.weight": W(C, C, sc=0.015), p + "0.SelfAttention.v.weight": W(C, C, sc=0.015),
                   p + "0.SelfAttention.o.weight": W(C, C, sc=0.015), p + "1.DenseReluDense.wi_0.weight": W(F, C, sc=0.015),
                   p + "1.DenseReluDense.wi_1.weight": W(F, C, sc=0.015), p + "1.DenseReluDense.wo.weight": W(C, F, sc=0.015)})
    cfg = dict(d_model=C, num_heads=H, d_kv=64, d_ff=F, num_layers=L, feed_forward_proj="gated-gelu")
    enc = te.T5EncoderHip(sd, cfg, device=dev, lib=lib)
    del sd
    wheel = T5EncoderModel(T5Config(d_model=C, num_heads=H, d_kv=64, d_ff=F, num_layers=wheel_layers, vocab_size=1024,
                                    feed_forward_proj="gated-gelu")).to(torch.bfloat16).eval()
    with torch.no_grad():
        report("T5-XXL", enc, L, lambda: enc.encode_ids(ids), wheel, lambda: wheel(input_ids=ids[None]))


def _soft_head(net):
    """a seeded detection head saturates (every score 0 or 1): damp the last class / box convolutions as the page tests do"""
    head = net.model[-1]
    with torch.no_grad():
        for l in range(3):
            head.cv3[l][2].weight.mul_(0.05); head.cv3[l][2].bias.fill_(-1.0)
            head.cv2[l][2].weight.mul_(0.1)
    return net


def _dettail_detectors(reps, calls, candidates):
    """`tail="host"` against `tail="device"` on one state dict and the same synthetic pages, alternated in one process: medians over `reps`
    rounds of the wall and the process-CPU milliseconds per `model(page)` (every call ends in its own blocking read)"""
    import statistics
    import time
    import numpy as np
    from oracle import yolo11_ref as yr, yolo_ref
    from mangatranslator_amd.core.ml.yolo import YoloSegHip
    from mangatranslator_amd.core.ml.yolo11 import Yolo11Hip
    from mangatranslator_amd.utils.synthetic_pages import make_page
    pages = [np.ascontiguousarray(make_page(40 + i, 1024, 1536, bubbles=8)[0][..., ::-1]) for i in range(4)]
    specs = [("bubble detector (YOLOv8m-seg) @1600", lambda: yolo_ref.make_model("m", 1, seed=3), YoloSegHip, 1600),
             ("YOLO11-L detect-only @640", lambda: yr.make_model("11", "l", 1, False, seed=1), Yolo11Hip, 640),
             ("YOLO12x detect-only @640", lambda: yr.make_model("12", "x", 1, False, seed=2), Yolo11Hip, 640)]
    for name, make, cls, imgsz in specs:
        # a seeded network's features die out with depth and its head saturates: condition every convolution on a page (oracle/yolo11_ref.py,
        # `calibrate`, as the parity checks do; at 640 px, the conditioning is not the thing measured), which leaves unit-spread logits
        sd = yr.calibrate(make(), yolo_ref.letterbox(pages[0], 640)[0]).state_dict()
        models = {t: cls(sd, device=dev, lib=lib, tail=t) for t in ("host", "device")}
        # seeded scores are arbitrary: each page's threshold is put where `candidates` of its rows pass, a trained detector's count on a page of 8 bubbles
        confs, counts = [], []
        for pg in pages:
            models["host"](pg, conf=0.0, imgsz=imgsz, max_det=1)
            plan0, _ = next(iter(models["host"]._plans.values()))
            sc = plan0.decoded[:, 4].float().sort(descending=True).values
            confs.append(float(sc[min(candidates, len(sc) - 1)]))
        for pg, conf in zip(pages, confs):                # warm every plan of both models, and hold the two to the same bytes
            h, d = models["host"](pg, conf=conf, imgsz=imgsz)[0], models["device"](pg, conf=conf, imgsz=imgsz)[0]
            assert (h.boxes is None) == (d.boxes is None)
            if h.boxes is not None:
                assert all(torch.equal(getattr(h.boxes, f), getattr(d.boxes, f)) for f in ("xyxy", "conf", "cls")), f"{name}: tails differ"
                assert h.masks is None or torch.equal(h.masks.data, d.masks.data), f"{name}: masks differ"
            tp = next(iter(models["device"]._tail_plans.values()))
            counts.append(tuple(tp.bufs.state.tolist()[:3]))
        wall, cpu = {t: [] for t in models}, {t: [] for t in models}
        for r in range(reps):
            for t, m in list(models.items())[::1 if r % 2 == 0 else -1]:          # the order alternates: neither tail always runs second
                torch.cuda.synchronize()
                w0, c0 = time.perf_counter(), time.process_time()
                for i in range(calls):
                    m(pages[i % len(pages)], conf=confs[i % len(pages)], imgsz=imgsz)
                torch.cuda.synchronize()
                wall[t].append((time.perf_counter() - w0) * 1e3 / calls); cpu[t].append((time.process_time() - c0) * 1e3 / calls)
        print(f"dettail {name}, conf {', '.join(f'{c:.4f}' for c in confs)}, (kept, candidates, overflow) per page {counts}: same bytes from both tails", flush=True)
        for t in models:
            print(f"  tail={t:6s}  wall {statistics.median(wall[t]):.3f} ms / call (rounds {', '.join(f'{v:.3f}' for v in wall[t])})   "
                  f"process CPU {statistics.median(cpu[t]):.3f} ms / call ({', '.join(f'{v:.3f}' for v in cpu[t])})", flush=True)
        del models
        torch.cuda.empty_cache()


def _dettail_op(iters):
    """the op alone on synthetic rows of the bubble detector's row count (35 700 x 37): graph replays, HIP events"""
    import numpy as np
    rng = np.random.default_rng(5)
    A, nm = 35700, 32

    def rows(n, centres, size):
        r = np.zeros((A, 5 + nm), np.float32)
        r[:, :4] = rng.uniform(0, 1500, (A, 4)); r[:, 4] = rng.uniform(0, 0.1, A); r[:, 5:] = rng.normal(0, 1, (A, nm))
        c = rng.uniform(100, 1400, (centres, 2))[np.arange(n) % centres] + rng.uniform(-3, 3, (n, 2))
        r[rng.choice(A, n, replace=False), :5] = np.concatenate([c - size / 2, c + size / 2, rng.permutation(np.linspace(0.3, 0.99, n))[:, None]], 1)
        return torch.from_numpy(r).to(dev)

    cases = [("typical: 64 candidates around 8 bubbles", 64, 8, 120.0), ("typical: 200 candidates around 8 bubbles", 200, 8, 120.0),
             ("capacity: 1024 candidates around 40 centres", abi.DET_TAIL_CAP, 40, 60.0), ("capacity: 1024 candidates, none overlapping", abi.DET_TAIL_CAP, abi.DET_TAIL_CAP, 1.0)]
    for name, n, centres, size in cases:
        pb = PlanBuilder(lib, dev, abi.F16)
        bufs = pb.detector_tail(rows(n, centres, size), nc=1, nm=nm)
        plan = pb.build()
        p = np.zeros(abi.DET_TAIL_PARAM_WORDS, np.int32)
        f = p.view(np.float32)
        f[abi.DET_TAIL_P_CONF], f[abi.DET_TAIL_P_IOU], p[abi.DET_TAIL_P_MAX_DET] = 0.25, 0.7, 300
        f[abi.DET_TAIL_P_GAIN], p[abi.DET_TAIL_P_W0], p[abi.DET_TAIL_P_H0] = 1.0417, 1024, 1536
        bufs.params.copy_(torch.from_numpy(p))
        plan.time(5, graph=True)
        ms = [plan.time(iters, graph=True) for _ in range(3)]
        print(f"dettail op, {name}: {min(ms) * 1e3:.1f} us per replay (rounds {', '.join(f'{v * 1e3:.1f}' for v in ms)}), state {bufs.state.tolist()[:3]}", flush=True)


def _dettail_pages(n_pages, reps):
    """`n_pages` synthetic pages through `core.pipeline.process_page_vision_front` (bubble detector, RT-DETR, SAM 2.1 — seeded tiny graphs, so the
    share of the tails is as large as it gets) with `ModelManager.detector_tail` "host" and "device", alternated: pages / s and process-CPU s / page"""
    import statistics
    import time
    import types
    import numpy as np
    from PIL import Image
    from oracle import rtdetr_ref, sam2_ref, yolo_ref
    from mangatranslator_amd.core import pipeline
    from mangatranslator_amd.core.ml import model_manager as mm
    from mangatranslator_amd.core.ml.rtdetr import RTDetrHip
    from mangatranslator_amd.core.ml.sam2 import Sam2Hip
    from mangatranslator_amd.utils.synthetic_pages import make_page
    mgr = mm.get_model_manager(); mgr.device = dev
    ysd = _soft_head(yolo_ref.make_model("n", 1, seed=3)).state_dict()
    rmodel, rcfg = rtdetr_ref.make_model("tiny_test", seed=5)
    smodel, scfg = sam2_ref.make_model("tiny_test", seed=2)
    mgr.models[mm.ModelType.RTDETR_CONJOINED_BUBBLE] = RTDetrHip(rmodel.state_dict(), rcfg, device=dev, lib=lib, names={0: "bubble", 1: "text_bubble", 2: "text_free"})
    sam = Sam2Hip(smodel.state_dict(), scfg, device=dev, lib=lib)
    mgr.sam_precision = sam.precision                      # (the loader rebuilds a model whose arithmetic is not the one asked for)
    mgr.models[mm.ModelType.SAM2] = (mm._Sam2ProcessorShim(), mm._Sam2ModelShim(sam, torch.bfloat16))
    yolos = {}
    for t in ("host", "device"):
        mgr.detector_tail = t                              # the public switch: the factory hands it to the model
        yolos[t] = mgr._detector_from_state_dict(ysd, default_names={0: "speech_bubble"})
        assert yolos[t].tail == t
    mgr.detector_tail = "host"
    pages = [Image.fromarray(make_page(60 + i, 1024, 1536, bubbles=8)[0]).convert("RGBA") for i in range(8)]
    bgr = np.ascontiguousarray(np.asarray(pages[0].convert("RGB"))[..., ::-1])
    yolos["host"](bgr, conf=0.0, imgsz=640, max_det=1)
    sc = next(iter(yolos["host"]._plans.values()))[0].decoded[:, 4].float().sort(descending=True).values
    conf = float(sc[min(48, len(sc) - 1)])
    ns = types.SimpleNamespace
    cfg = ns(device=dev, yolo_model_path=None, upscaling_only=False, request_coordinator=None, verbose=False, preprocessing=ns(auto_scale=True),
             detection=ns(confidence=conf, seg_model="sam2", conjoined_detection=True, conjoined_confidence=0.35, use_osb_text_verification=False,
                          bubble_detector_model="yolo_1"),
             cleaning=ns(thresholding_value=200, use_otsu_threshold=False, roi_shrink_px=5, inpaint_colored_bubbles=False),
             outside_text=ns(enabled=False, enable_page_number_filtering=False, min_area_ignore_ratio=0.0, seed=1, huggingface_token="",
                             inpainting_method="flux_kontext", flux_backend="sdnq", flux_low_vram=False, flux_num_inference_steps=2,
                             flux_group_regions=False, flux_residual_diff_threshold=0.15, osb_confidence=0.5, osb_text_free_only=False,
                             bbox_expansion_percent_width=0.1, bbox_expansion_percent_height=0.1, osb_render_expansion_narrow_multiplier=1.0,
                             osb_render_expansion_tiny_multiplier=1.0, text_box_proximity_ratio=0.02),
             output=ns(upscale_final_image=False, image_upscale_factor=1.0, image_upscale_model="model_lite", output_format="png", jpeg_quality=95, png_compression=2))
    rate, cpu = {t: [] for t in yolos}, {t: [] for t in yolos}
    for r in range(reps + 1):                              # round 0 warms both
        for t, y in list(yolos.items())[::1 if r % 2 == 0 else -1]:
            mgr.models[mm.ModelType.YOLO_SPEECH_BUBBLE] = y
            torch.cuda.synchronize()
            w0, c0 = time.perf_counter(), time.process_time()
            for i in range(n_pages if r else len(pages)):
                pipeline.process_page_vision_front(pages[i % len(pages)], cfg, f"p{i}.png", "PNG", False)
            torch.cuda.synchronize()
            if r:
                rate[t].append(n_pages / (time.perf_counter() - w0)); cpu[t].append((time.process_time() - c0) / n_pages)
    for t in yolos:
        print(f"dettail pages, {n_pages} pages through process_page_vision_front, detector_tail={t:6s}: {statistics.median(rate[t]):.1f} pages/s "
              f"(rounds {', '.join(f'{v:.1f}' for v in rate[t])}), process CPU {statistics.median(cpu[t]) * 1e3:.2f} ms / page", flush=True)


def dettail(reps=4, calls=40, pages=64):
    _dettail_op(200)
    _dettail_detectors(reps, calls, 64)
    _dettail_pages(pages, reps)


if __name__ == "__main__":
    args = sys.argv[1:]
    while args:
        if args[0] == "dettail":                      # the detector tail: the op alone, three detectors host against device, 64 pages through the front half
            dettail(); args = args[1:]
            continue
        if args[0] == "textenc":                      # textenc [WHEEL_LAYERS]
            n = int(args[1]) if len(args) > 1 and args[1].isdigit() else 2
            textenc(n); args = args[2 if len(args) > 1 and args[1].isdigit() else 1:]
            continue
        if args[0] == "mangaocr_batch":
            mangaocr_batch(); args = args[1:]
            continue
        if args[0] == "paddleocr_fill":
            paddleocr_fill(); args = args[1:]
            continue
        if args[0] == "paddleocr":
            paddleocr(); paddleocr_batch(); args = args[1:]
            continue
        if args[0] == "mangaocr":                     # mangaocr [DEC_LAYERS]
            n = int(args[1]) if len(args) > 1 and args[1].isdigit() else 2
            mangaocr(n); args = args[2 if len(args) > 1 and args[1].isdigit() else 1:]
            continue
        if args[0] == "attn":
            attn(int(args[1])); args = args[2:]
        elif args[0] == "attn88":                       # fp8 scores + fp8 P V
            attn_f8_pv(int(args[1])); args = args[2:]
        elif args[0] in ("attn8", "attn8w"):          # fp8 scores: MX fp8 rows out / 16-bit rows out
            attn_f8_scores(int(args[1]), out8=args[0] == "attn8"); args = args[2:]
        elif args[0] in ("attnq", "attnqs"):          # attention with MX fp8 output: fused epilogue / separate quantiser
            attn_q8(int(args[1]), fused=args[0] != "attnqs"); args = args[2:]
        elif args[0] in ("glu", "glus"):              # glu M hid K col0
            gemm8_glu(int(args[1]), int(args[2]), int(args[3]), int(args[4]), fused=args[0] == "glu"); args = args[5:]
        elif args[0] in ("actq", "actqs", "actqab"):  # actq M N K: fp8 GEMM + bias + GELU -> MX fp8: fused epilogue / separate quantiser / both, alternating
            if args[0] == "actqab":
                gemm8_actq_ab(int(args[1]), int(args[2]), int(args[3]))
            else:
                gemm8_actq(int(args[1]), int(args[2]), int(args[3]), fused=args[0] == "actq")
            args = args[4:]
        elif args[0] == "kontext":                    # kontext H2 W2 LAYERS SINGLES: one step, bf16 against fp8 block linears
            kontext_step_ab(int(args[1]), int(args[2]), int(args[3]), int(args[4])); args = args[5:]
        elif args[0] == "kontextpsnr":                # kontextpsnr H W LAYERS SINGLES: 4-step image PSNR, fp8 against bf16
            kontext_psnr(int(args[1]), int(args[2]), int(args[3]), int(args[4])); args = args[5:]
        elif args[0] in ("norm", "normq"):              # norm ROWS C: every norm kernel form in turn
            norm(int(args[1]), int(args[2]), q8=args[0] == "normq"); args = args[3:]
        elif args[0] == "sam3":                       # sam3 [LAYERS]
            n = int(args[1]) if len(args) > 1 and args[1].isdigit() else 32
            sam3(n); args = args[2 if len(args) > 1 and args[1].isdigit() else 1:]
        elif args[0] == "quant":
            quant(int(args[1]), int(args[2])); args = args[3:]
        elif args[0] == "conv":
            conv(int(args[1]), int(args[2])); args = args[3:]
        elif args[0] in ("gemmeb", "gemmeg", "gemmer", "gemm8eb", "gemm8er"):      # gemmeK M N K: with a real epilogue (K = b / g / r), fp8 with gemm8eK
            gemm_epi(int(args[1]), int(args[2]), int(args[3]), args[0][-1], f8=args[0].startswith("gemm8")); args = args[4:]
        elif args[0] in ("gemmst", "gemm8st", "gemmgst"):     # strip-count A/B of the 256-tile kernels' tile map
            gemm_strips(int(args[1]), int(args[2]), int(args[3]), f8=args[0] == "gemm8st", kind="g" if args[0] == "gemmgst" else "b"); args = args[4:]
        elif args[0] == "gemmg":                       # bf16 GEMM with the bias + tanh-GELU epilogue (FLUX ff1 / proj_mlp)
            gemm(int(args[1]), int(args[2]), int(args[3]), act=abi.ACT_GELU_TANH); args = args[4:]
        elif args[0] == "gemmp":
            gemm(int(args[1]), int(args[2]), int(args[3]), pad=int(args[4])); args = args[5:]
        elif args[0].rstrip("0123456789") in ("gemm", "gemm8", "gemmn", "gemm8n", "gemms", "gemm8s", "gemmfs", "gemm8fs"):
            # ...n: no split at all, ...sN: exactly N K slices (e.g. gemms4, gemm8s2)
            name = args[0].rstrip("0123456789")
            fl = abi.GEMM_NO_SPLIT if name.endswith("n") else 0
            if name.endswith("s"):
                fl = int(args[0][len(name):]) << 8
            if name.endswith("fs"):                    # gemmfsN: N slices also where the launcher would not slice (K shorter than 64 iterations)
                fl |= abi.GEMM_FORCE_TILE256
            gemm(int(args[1]), int(args[2]), int(args[3]), f8=args[0].startswith("gemm8"), flags=fl); args = args[4:]
        else:
            raise SystemExit(f"unknown benchmark {args[0]}")
