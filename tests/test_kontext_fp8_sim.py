"""CPU tier: FLUX.1-Kontext with MX-fp8 block linears (FluxDiTHip(fp8=...), ModelManager.flux_kontext_fp8) and the activation + MX-fp8 epilogue
of the fp8 GEMM (mtx_gemm_args.actq_*), executed by the kernel simulator."""
import json

import numpy as np
import pytest
import torch
from PIL import Image
from safetensors.torch import save_file

import flux_checks as fc
import kontext_fp8_checks as kc


def test_gemm_f8_actq_epilogue(emu_lib):
    """bytes and scale words of the fused epilogue = fp8 GEMM (bias, activation) -> mtx_quantize_mx, nothing outside the window"""
    kc.check_actq_cases(emu_lib)


def test_gemm_f8_actq_validation(emu_lib):
    kc.check_actq_validation(emu_lib)


def test_kontext_dit_step_fp8(emu_lib):
    kc.check_dit_step_fp8(emu_lib, "cpu")


def test_kontext_fp8_fusions_change_nothing(emu_lib):
    """T = 1072, one head of 128: norms, MLP-in GEMMs and the joint attention write the fp8 operands themselves — same velocity bits as with a
    quantiser launch behind each of them, and no quantiser launch left"""
    kc.check_fusions_change_nothing(emu_lib, "cpu", layers=1, single_layers=1)


def test_kontext_fp8_off_means_off(emu_lib):
    kc.check_off_means_off(emu_lib, "cpu")


def test_kontext_fp8_first_block_cache(emu_lib):
    kc.check_first_block_cache_fp8(emu_lib, "cpu")


def test_kontext_fp8_vs_bf16_psnr(emu_lib):
    kc.check_kontext_fp8_vs_bf16(emu_lib, "cpu")


def test_kontext_fp8_geometry(emu_lib):
    """d % 128 != 0 refuses fp8 itself; a kind outside FP8_ALL is refused; a subset of kinds keeps the others on the 16-bit kernel and a
    geometry or subset that does not allow a fusion falls back to the separate launch"""
    from mangatranslator_amd.core.ml import flux as fx
    from mangatranslator_amd.hip import abi
    from mangatranslator_amd.utils.exceptions import ModelError
    t, v = fc.models(d=192, heads=3, axes_dim=(8, 28, 28), layers=1, single_layers=1)
    kc.hip_models(t, v, emu_lib, "cpu", fp8=False)
    with pytest.raises(ModelError):
        kc.hip_models(t, v, emu_lib, "cpu", fp8=True)
    t, v = fc.models(layers=1, single_layers=1)
    with pytest.raises(ModelError):
        kc.hip_models(t, v, emu_lib, "cpu", fp8=("qkv", "ff_in"))
    dit, _ = kc.hip_models(t, v, emu_lib, "cpu", fp8=("ff1", "proj_mlp", "proj_out"))      # ff2 stays 16-bit: ff1 must write 16 bits, proj_mlp need not
    lat, pe, pooled = kc.step_inputs(t.cfg, 4, 6, 16)
    vel, plan = kc.run_step(dit, lat, pe, pooled, 4, 6, "cpu")
    assert torch.isfinite(vel).all()
    by = {lb: g for lb, g in kc.block_gemms(plan)}
    assert by["dbl0.ff1.f8"].in_dtype == abi.F8 and not by["dbl0.ff1.f8"].actq_q and by["dbl0.ff2"].in_dtype != abi.F8
    assert by["sgl0.proj_mlp.f8"].actq_q and by["sgl0.proj_out.f8"].in_dtype == abi.F8 and by["sgl0.qkv"].in_dtype != abi.F8
    assert sum(1 for o in plan.ops if o.kind == abi.OP_QUANT) == 1          # the attention half of cat8 (T < 1024: the attention cannot write it)


def test_plan_dump_names_every_pointer_and_repeats(emu_lib):
    """tools/plan_dump.py on the three plans of a cached fp8 build: every pointer of every op lies in a buffer of the plans or in a weight of
    the model (the dump raises otherwise), and a second, independent build of the same model gives the same text"""
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    import plan_dump as pd
    dumps = []
    for _ in range(2):
        plan, dit = pd.toy_plan("kontext", emu_lib, (4, 6, 16), fp8=True, cached=True)
        dumps.append(pd.dump(plan, dit))
        assert len(dumps[-1]) == len(plan.ops) + len(plan.body.ops) + len(plan.skip.ops)
    assert dumps[0] == dumps[1]
    heads = {ln.split()[0] for ln in dumps[0]}
    assert heads == {"head", "body", "skip"} and any(" q=b" in ln for ln in dumps[0]) and "0x" not in "".join(dumps[0])
    # an op that points outside every known buffer is an error, not a line
    stray = torch.zeros(64, dtype=torch.bfloat16)
    plan.ops[0].u.gemm.bias = stray.data_ptr()
    with pytest.raises(LookupError):
        pd.dump(plan, dit)


def test_plan_dump_of_a_model_that_is_no_dit(emu_lib):
    """the same for manga-ocr (f16), with the model object itself as the weight holder: two independent builds give the same text and the same
    weights digest, a stray pointer raises, and the weights digest moves when one weight element does"""
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    import plan_dump as pd
    built = [pd.toy_plan("manga-ocr", emu_lib, variant="f16") for _ in range(2)]
    dumps = [pd.dump(plans, model) for plans, model in built]
    plans, model = built[0]
    assert dumps[0] == dumps[1] and len(dumps[0]) == sum(len(p.ops) for p in plans)
    assert {ln.split()[0] for ln in dumps[0]} == {"p0", "p1", "p2"} and "0x" not in "".join(dumps[0])
    assert any(" w=b" in ln and "patch_embed" in ln for ln in dumps[0])                      # a weight of the model, named as a buffer
    want = pd.weights_digest(model)
    assert want == pd.weights_digest(built[1][1])
    w = model.e_layers[1]["fc2"][0]
    w[3, 5] = w[3, 5] + 1
    assert pd.weights_digest(model) != want
    stray = torch.zeros(64, dtype=torch.float16)
    plans[1].ops[0].u.ew.s = stray.data_ptr()
    with pytest.raises(LookupError):
        pd.dump(plans, model)


@pytest.fixture()
def manager(emu_lib, tmp_path, monkeypatch):
    import mangatranslator_amd.hip.lib as libmod
    from mangatranslator_amd.core.ml import model_manager as mm
    monkeypatch.setattr(libmod, "_lib", emu_lib)
    monkeypatch.setattr(mm, "_model_manager", None)
    monkeypatch.setattr(mm.ModelManager, "_instance", None)
    m = mm.get_model_manager()
    for k in list(m.model_paths):
        rel = m.model_paths[k].relative_to(m.model_paths[k].parents[1])
        m.model_paths[k] = tmp_path / rel
    yield m
    monkeypatch.setattr(mm.ModelManager, "_instance", None)


@pytest.mark.parametrize("fp8", [False, True])
def test_manager_flag_reaches_the_dit_and_the_memo_key(manager, fp8):
    """ModelManager.flux_kontext_fp8 -> load_flux_kontext_sdnq -> FluxDiTHip(fp8=): the inpainter runs, and its stage-memo key carries the
    arithmetic only when the flag is on (off: the key the package made before the flag existed)"""
    from mangatranslator_amd.core.image.inpainting import FluxKontextInpainter
    from mangatranslator_amd.core.ml.dit_graph import Weight
    from mangatranslator_amd.core.ml.model_manager import ModelManager, ModelType
    assert ModelManager.flux_kontext_fp8 is False                 # the default stays bf16
    t, v = fc.models(seed=4)
    root = manager.model_paths[ModelType.FLUX_KONTEXT_SDNQ_PIPELINE]
    (root / "transformer").mkdir(parents=True); (root / "vae").mkdir()
    save_file({k: x.to(torch.bfloat16).contiguous() for k, x in t.state_dict().items()}, str(root / "transformer" / "diffusion_pytorch_model.safetensors"))
    save_file({k: x.contiguous() for k, x in v.state_dict().items()}, str(root / "vae" / "diffusion_pytorch_model.safetensors"))
    c = t.cfg
    (root / "transformer" / "config.json").write_text(json.dumps(dict(
        num_attention_heads=c["heads"], attention_head_dim=c["d"] // c["heads"], num_layers=c["layers"], num_single_layers=c["single_layers"],
        in_channels=64, joint_attention_dim=c["joint_dim"], pooled_projection_dim=c["pooled_dim"], axes_dims_rope=list(c["axes_dim"]))))
    (root / "vae" / "config.json").write_text(json.dumps(dict(block_out_channels=list(v.cfg["ch"]), norm_num_groups=v.cfg["groups"],
                                                            scaling_factor=v.cfg["scaling_factor"], shift_factor=v.cfg["shift_factor"])))
    g = torch.Generator().manual_seed(9)
    save_file({"prompt_embeds": torch.randn(8, c["joint_dim"], generator=g), "pooled_prompt_embeds": torch.randn(c["pooled_dim"], generator=g)},
              str(root / "prompt_embeds.safetensors"))
    manager.flux_kontext_fp8 = fp8
    pipe = manager.load_flux_kontext_sdnq()
    assert pipe is not None and manager.load_flux_models()[2] is pipe
    dit = pipe.transformer
    assert bool(dit.fp8) == fp8 and dit.blocks[0]["qkv"].fp8 == fp8 and dit.singles[0]["out"].fp8 == fp8 and isinstance(dit.blocks[0]["qkv"], Weight)
    assert dit.W["proj_out"][0].dtype == torch.bfloat16           # the output layer stays 16-bit either way
    inp = FluxKontextInpainter(num_inference_steps=1, backend="sdnq")
    inp.PREFERED_KONTEXT_RESOLUTIONS = [(48, 32), (32, 48), (32, 32)]
    page = Image.fromarray((np.random.default_rng(0).random((96, 128, 3)) * 255).astype(np.uint8))
    mask = np.zeros((96, 128), bool); mask[30:50, 40:80] = True
    out = inp.inpaint_mask(page, mask, seed=1)
    a, b = np.asarray(page).astype(int), np.asarray(out).astype(int)
    assert out.size == page.size and (a != b).any() and pipe.completed == 1
    # the memo key: with the flag off exactly the key built from the reference's parts; with it on, the same parts plus the arithmetic
    crop, mcrop = page.crop((30, 20, 90, 60)), mask[20:60, 30:90]
    key = inp._memo_key(crop, mcrop, 1, (30, 20, 60, 40), 8, 3, None, False, None)
    sig = (torch.nn.functional.interpolate(torch.from_numpy(mcrop.astype(np.float32))[None, None], size=(40, 60), mode="bilinear", align_corners=False) > 0.5).numpy().astype(np.uint8)[0, 0]
    params = {"bbox": (30, 20, 60, 40), "padding": 8, "blur": 3, "backend": "sdnq"}
    plain = inp.cache.get_inpaint_cache_key(crop, sig, 1, 1, inp.residual_diff_threshold, inp.guidance_scale, inp.prompt, dict(params))
    if fp8:
        assert key != plain and key == inp.cache.get_inpaint_cache_key(crop, sig, 1, 1, inp.residual_diff_threshold, inp.guidance_scale, inp.prompt,
                                                                       dict(params, arithmetic="fp8"))
    else:
        assert key == plain
    manager.unload_flux_kontext_sdnq_models()
