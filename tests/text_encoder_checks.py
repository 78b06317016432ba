"""Checks of FLUX's prompt encoders on the HIP path (core/ml/text_encoders.py: Qwen3EncoderHip, T5EncoderHip, ClipTextHip) and of their wiring
(core/ml/prompt_embeds.py `backend="hip"`, the pipelines' `set_text_encoder`), written once and run on the simulator
(tests/test_text_encoders_sim.py) and on the product library (tests/test_text_encoders_gpu.py).

The oracle is the wheel's own class (Qwen3ForCausalLM, T5EncoderModel, CLIPTextModel) in fp32 on the CPU, built from a tiny config with redrawn
weights.  The measure is the relative L2 error of the whole output.  The bound is not a fixed number: per seed the FLOOR is the error of the same
wheel model with every parameter rounded to bf16 against the fp32 one — what bf16 storage costs before any activation is rounded.  The floor must
lie in [0.2 %, 2 %] (so the inputs cannot drift into a regime where the bound means nothing) and the product's error must stay within 4 x floor:
PaddleOCR-VL measured 2.2 - 2.3 x its weights-only floor (docs/experiments.md), the product also rounds activations at four points per layer,
and a real defect (a wrong tap, a missing bias, a wrong key limit, an un-permuted gain) moves the output by tens of percent.

Weight recipes (they keep the floor small while the thing under test still matters):
  Qwen3   matrices N(0, 0.1), gains U(0.5, 1.5)
  T5      matrices N(0, 0.06), embeddings N(0, 1), gains U(0.5, 1.5), bias table N(0, 2)   (zeroing the bias moves the output by ~40 %)
  CLIP    matrices N(0, 0.1)"""
import copy
import functools
import json

import torch

from mangatranslator_amd.core.ml import text_encoders as te
from mangatranslator_amd.hip import abi
from op_checks import _dev

SEEDS = (0, 1, 2)
FLOOR_RANGE = (0.002, 0.02)
FACTOR = 4.0
QWEN_S, QWEN_VALID = 96, (1, 41, 96)
T5_S = (33, 150)
CLIP_S, CLIP_EOT_AT = 77, 9


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def redraw(model, seed, matrices, embeddings=None, gains=False, table=None):
    """the recipes of the module docstring, in the order of `named_parameters` from one generator"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if table is not None and "relative_attention_bias" in name:
                p.copy_(torch.randn(p.shape, generator=g) * table)
            elif embeddings is not None and ("shared" in name or "embed_tokens" in name):
                p.copy_(torch.randn(p.shape, generator=g) * embeddings)
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) * matrices)
            elif gains and p.dim() == 1 and "bias" not in name:
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
    return model.float().eval()


def rounded_twin(model):
    """the same wheel model with every parameter rounded to bf16 (kept in fp32 arithmetic)"""
    twin = copy.deepcopy(model)
    with torch.no_grad():
        for p in twin.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    return twin


def judge(what, got, ref, floor_out):
    """-> (error, floor, error / floor); prints them before it asserts"""
    floor, err = rel_l2(floor_out, ref), rel_l2(got.float().cpu(), ref)
    print(f"{what}: floor {100 * floor:.3f} %  error {100 * err:.3f} %  ratio {err / floor:.2f}")
    assert FLOOR_RANGE[0] <= floor <= FLOOR_RANGE[1], f"{what}: the floor {100 * floor:.3f} % left [0.2 %, 2 %]"
    assert err <= FACTOR * floor, f"{what}: error {100 * err:.3f} % is {err / floor:.2f} x the floor {100 * floor:.3f} % (bound 4 x)"
    return err, floor, err / floor


# ---- Qwen3 ----------------------------------------------------------------------------------------------------------------------------------------
def qwen_config(hidden=256, layers=4, heads=4, kv=2, mlp=384, vocab=512):
    from transformers import Qwen3Config
    return Qwen3Config(hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, num_key_value_heads=kv, head_dim=128,
                       intermediate_size=mlp, vocab_size=vocab, max_position_embeddings=1024, tie_word_embeddings=False)


@functools.lru_cache(maxsize=None)
def qwen_oracle(seed):
    from transformers import Qwen3ForCausalLM
    return redraw(Qwen3ForCausalLM(qwen_config()), seed, 0.1, gains=True)


def qwen_wheel(model, ids, n_valid, taps):
    S = ids.numel()
    mask = (torch.arange(S) < n_valid).long()[None]
    with torch.no_grad():
        hs = model(input_ids=ids[None], attention_mask=mask, output_hidden_states=True, use_cache=False).hidden_states
    return torch.cat([hs[k][0] for k in taps], 1)


def qwen_ids(seed, S=QWEN_S, vocab=512):
    return torch.randint(0, vocab, (S,), generator=torch.Generator().manual_seed(100 + seed))


def check_qwen3(lib, seed, taps=(1, 2, 3)):
    model = qwen_oracle(seed)
    twin = rounded_twin(model)
    ids = qwen_ids(seed)
    enc = te.Qwen3EncoderHip(model.state_dict(), model.config, taps=taps, device=_dev(lib), lib=lib)
    ratios = []
    try:
        assert len(enc.W) == max(taps), "only max(taps) layers are packed"
        for n in QWEN_VALID:
            got = enc.encode_ids(ids, n)
            assert got.dtype == torch.bfloat16 and tuple(got.shape) == (QWEN_S, len(taps) * 256)
            ratios.append(judge(f"Qwen3 seed {seed} n_valid {n}", got, qwen_wheel(model, ids, n, taps), qwen_wheel(twin, ids, n, taps))[2])
        assert len(enc._plans) == 1, "one plan per sequence length serves every n_valid"
    finally:
        enc.close()
    return ratios


def check_qwen3_padding(lib, seed=0, n=41, taps=(1, 2, 3)):
    """rows < n_valid do not depend on the tail at all; padding row i depends on its own id only"""
    model = qwen_oracle(seed)
    ids = qwen_ids(seed)
    enc = te.Qwen3EncoderHip(model.state_dict(), model.config, taps=taps, device=_dev(lib), lib=lib)
    try:
        base = enc.encode_ids(ids, n).cpu().view(torch.int16)
        other = ids.clone()
        other[n:] = (other[n:] + 7) % 512
        i = n + 5
        other[i] = ids[i]
        got = enc.encode_ids(other, n).cpu().view(torch.int16)
        assert torch.equal(got[:n], base[:n]), "rows below n_valid changed with the padding ids"
        assert torch.equal(got[i], base[i]), "a padding row changed with the OTHER padding ids"
        assert not torch.equal(got[i + 1], base[i + 1]), "the test's own premise: a padding row follows its own id"
    finally:
        enc.close()


# ---- T5 -------------------------------------------------------------------------------------------------------------------------------------------
def t5_config(d_model=128, heads=2, d_ff=256, layers=3, vocab=512):
    from transformers import T5Config
    return T5Config(d_model=d_model, d_kv=64, num_heads=heads, d_ff=d_ff, num_layers=layers, vocab_size=vocab, feed_forward_proj="gated-gelu",
                    dropout_rate=0.0)


@functools.lru_cache(maxsize=None)
def t5_oracle(seed):
    from transformers import T5EncoderModel
    return redraw(T5EncoderModel(t5_config()), seed, 0.06, embeddings=1.0, gains=True, table=2.0)


def t5_wheel(model, ids):
    with torch.no_grad():
        return model(input_ids=ids[None])[0][0]


def check_t5(lib, seed, S):
    model = t5_oracle(seed)
    ids = torch.randint(0, 512, (S,), generator=torch.Generator().manual_seed(200 + seed + S))
    ref = t5_wheel(model, ids)
    nobias = copy.deepcopy(model)
    with torch.no_grad():
        nobias.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight.zero_()
    moved = rel_l2(t5_wheel(nobias, ids), ref)
    assert moved > 0.2, f"the test's own premise: zeroing the bias table moves the output by {100 * moved:.1f} %"
    enc = te.T5EncoderHip(model.state_dict(), model.config, device=_dev(lib), lib=lib)
    try:
        got = enc.encode_ids(ids)
        assert got.dtype == torch.bfloat16 and tuple(got.shape) == (S, 128)
    finally:
        enc.close()
    return judge(f"T5 seed {seed} S {S}", got, ref, t5_wheel(rounded_twin(model), ids))[2]


def check_t5_table():
    """t5_relative_table against the wheel's own compute_bias, at a length beyond max_distance"""
    model = t5_oracle(0)
    att = model.encoder.block[0].layer[0].SelfAttention
    S = 150
    with torch.no_grad():
        want = att.compute_bias(S, S)[0]                                 # [heads, S, S]
    table = te.t5_relative_table(att.relative_attention_bias.weight.detach(), S)
    i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
    assert tuple(table.shape) == (2, 2 * S - 1) and torch.equal(table[:, j - i + S - 1], want)


def check_t5_refuses_f16(lib):
    import pytest
    from mangatranslator_amd.utils.exceptions import ModelError
    model = t5_oracle(0)
    with pytest.raises(ModelError):
        te.T5EncoderHip(model.state_dict(), model.config, device=_dev(lib), lib=lib, dtype=abi.F16)


# ---- CLIP -----------------------------------------------------------------------------------------------------------------------------------------
def clip_config(eos, hidden=128, heads=2, mlp=256, layers=3, vocab=512):
    from transformers import CLIPTextConfig
    return CLIPTextConfig(hidden_size=hidden, num_attention_heads=heads, intermediate_size=mlp, num_hidden_layers=layers, max_position_embeddings=77,
                          vocab_size=vocab, eos_token_id=eos, bos_token_id=0, pad_token_id=1, hidden_act="quick_gelu")


@functools.lru_cache(maxsize=None)
def clip_oracle(seed, eos):
    from transformers import CLIPTextModel
    return redraw(CLIPTextModel(clip_config(eos)), seed, 0.1)


def clip_ids(seed, eot):
    """random tokens below every end-of-text id in use, the end-of-text token at CLIP_EOT_AT and repeated to the end"""
    ids = torch.randint(3, 290, (CLIP_S,), generator=torch.Generator().manual_seed(300 + seed))
    ids[CLIP_EOT_AT:] = eot
    return ids


def check_clip(lib, seed, eos, eot=None):
    """eos = the config's eos_token_id (2: the legacy arg-max rule; else the first position holding it); eot = the token the prompt ends with"""
    eot = (511 if eos == 2 else eos) if eot is None else eot
    model = clip_oracle(seed, eos)
    ids = clip_ids(seed, eot)
    if eos != 2 and eot != 511:
        ids[3] = 511                                                     # the arg-max rule would pool row 3
    with torch.no_grad():
        out = model(input_ids=ids[None])
        twin = rounded_twin(model)(input_ids=ids[None])
    ref, pooled = out.last_hidden_state[0], out.pooler_output[0]
    assert torch.equal(pooled, ref[CLIP_EOT_AT]), "the test's own premise: the wheel pools the first end-of-text row"
    enc = te.ClipTextHip(model.state_dict(), model.config, device=_dev(lib), lib=lib)
    try:
        got = enc.encode_ids(ids)
        p = enc.pooled(ids)
        assert enc.pool_index(ids) == CLIP_EOT_AT
        assert p.dtype == torch.bfloat16 and tuple(p.shape) == (128,)
        assert torch.equal(p.cpu().view(torch.int16), got[CLIP_EOT_AT].cpu().view(torch.int16))
    finally:
        enc.close()
    return judge(f"CLIP seed {seed} eos_token_id {eos}", got, ref, twin.last_hidden_state[0])[2]


# ---- one layer at the published widths (GPU tier) --------------------------------------------------------------------------------------------------
def _judge_wide(what, got, ref, floor_out):
    floor, err = rel_l2(floor_out, ref), rel_l2(got.float().cpu(), ref)
    print(f"{what}: floor {100 * floor:.3f} %  error {100 * err:.3f} %  ratio {err / floor:.2f}")
    assert err <= FACTOR * floor, f"{what}: error {100 * err:.3f} % is {err / floor:.2f} x the floor {100 * floor:.3f} %"
    return err / floor


def check_published_qwen3(lib, seed=0, S=512):
    """Qwen3-4B's widths (2560, 32 heads over 8 of 128, MLP 9728): the stream after ONE layer, half of the rows padding"""
    from transformers import Qwen3ForCausalLM
    model = redraw(Qwen3ForCausalLM(qwen_config(2560, 2, 32, 8, 9728)), seed, 0.02, gains=True)
    ids = qwen_ids(seed, S)
    enc = te.Qwen3EncoderHip(model.state_dict(), model.config, taps=(1,), device=_dev(lib), lib=lib)
    try:
        got = enc.encode_ids(ids, S // 2 + 3)
    finally:
        enc.close()
    return _judge_wide("Qwen3-4B widths, one layer", got, qwen_wheel(model, ids, S // 2 + 3, (1,)), qwen_wheel(rounded_twin(model), ids, S // 2 + 3, (1,)))


def check_published_t5(lib, seed=0, S=512):
    """T5-XXL's widths (4096, 64 heads of 64, d_ff 10240): one block and the final norm"""
    from transformers import T5EncoderModel
    model = redraw(T5EncoderModel(t5_config(4096, 64, 10240, 1)), seed, 0.015, embeddings=1.0, gains=True, table=2.0)
    ids = torch.randint(0, 512, (S,), generator=torch.Generator().manual_seed(seed))
    enc = te.T5EncoderHip(model.state_dict(), model.config, device=_dev(lib), lib=lib)
    try:
        got = enc.encode_ids(ids)
    finally:
        enc.close()
    return _judge_wide("T5-XXL widths, one block", got, t5_wheel(model, ids), t5_wheel(rounded_twin(model), ids))


def check_published_clip(lib, seed=0):
    """CLIP-L's widths (768, 12 heads, MLP 3072) at 77 rows: one layer and the final LayerNorm"""
    from transformers import CLIPTextModel
    model = redraw(CLIPTextModel(clip_config(2, 768, 12, 3072, 1)), seed, 0.03)
    ids = clip_ids(seed, 511)
    with torch.no_grad():
        ref = model(input_ids=ids[None]).last_hidden_state[0]
        floor = rounded_twin(model)(input_ids=ids[None]).last_hidden_state[0]
    enc = te.ClipTextHip(model.state_dict(), model.config, device=_dev(lib), lib=lib)
    try:
        got = enc.encode_ids(ids)
    finally:
        enc.close()
    return _judge_wide("CLIP-L widths, one layer", got, ref, floor)


# ---- wiring: prompt_embeds.py backend "hip", the pipelines' set_text_encoder -------------------------------------------------------------------------
WORDS = ["<pad>", "</s>", "<unk>", "remove", "all", "text", ".", "<s>", "keep", "the", "line", "art", "another", "prompt", ",", "<eot>"]
STORED, OTHER = "remove all text .", "another prompt , keep the line art"
KLEIN_TAPS = (1, 2, 3)


def _tokenizer(folder, max_length, eos="</s>", template=None):
    """a word-level tokenizer built with the `tokenizers` package and saved the way a snapshot holds it; nothing is downloaded"""
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    tk = Tokenizer(models.WordLevel({w: i for i, w in enumerate(WORDS)}, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.Whitespace()
    kw = {} if template is None else {"chat_template": template}
    PreTrainedTokenizerFast(tokenizer_object=tk, pad_token="<pad>", eos_token=eos, unk_token="<unk>", bos_token="<s>", model_max_length=max_length,
                            padding_side="right", **kw).save_pretrained(str(folder))


def stage_klein(root, seed=0):
    """text_encoder/ (a tiny Qwen3, the Qwen3 recipe) + tokenizer/ with a chat template; -> the fp32 wheel model"""
    from transformers import Qwen3ForCausalLM
    model = redraw(Qwen3ForCausalLM(qwen_config(vocab=len(WORDS))), seed, 0.1, gains=True)
    model.save_pretrained(str(root / "text_encoder"))
    _tokenizer(root / "tokenizer", 512, template="{% for m in messages %}<s> {{ m['content'] }} </s>{% endfor %}")
    return model


def stage_kontext(root, seed=0):
    """text_encoder/ (CLIP) + text_encoder_2/ (T5) + their tokenizers (CLIP's ends with the highest id, as the published one does)"""
    from transformers import CLIPTextConfig, CLIPTextModel, T5EncoderModel
    clip = redraw(CLIPTextModel(CLIPTextConfig(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2, max_position_embeddings=77,
                                               vocab_size=len(WORDS), eos_token_id=2, bos_token_id=7, pad_token_id=15, hidden_act="quick_gelu")), seed, 0.1)
    t5 = redraw(T5EncoderModel(t5_config(layers=2, vocab=len(WORDS))), seed, 0.06, embeddings=1.0, gains=True, table=2.0)
    clip.save_pretrained(str(root / "text_encoder"))
    t5.save_pretrained(str(root / "text_encoder_2"))
    from tokenizers import Tokenizer, models, pre_tokenizers, processors
    from transformers import PreTrainedTokenizerFast
    tk = Tokenizer(models.WordLevel({w: i for i, w in enumerate(WORDS)}, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.Whitespace()
    tk.post_processor = processors.TemplateProcessing(single="<s> $A <eot>", special_tokens=[("<s>", 7), ("<eot>", 15)])
    PreTrainedTokenizerFast(tokenizer_object=tk, pad_token="<eot>", eos_token="<eot>", unk_token="<unk>", bos_token="<s>", model_max_length=77,
                            padding_side="right").save_pretrained(str(root / "tokenizer"))
    _tokenizer(root / "tokenizer_2", 512)
    return clip, t5


def _read(path):
    from safetensors import safe_open
    with safe_open(str(path), framework="pt") as f:
        return {k: f.get_tensor(k) for k in f.keys()}, dict(f.metadata() or {})


def _bytes(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _stub_dit(lib):
    """what a pipeline's constructor and `encode_prompt` read of its DiT"""
    from types import SimpleNamespace
    return SimpleNamespace(device=_dev(lib), lib=lib, side_lane=True, _plans={})


def check_klein_wiring(lib, tmp_path, monkeypatch):
    from mangatranslator_amd.core.ml import prompt_embeds as pe
    from mangatranslator_amd.core.ml.flux2 import Flux2KleinHip
    from mangatranslator_amd.core.ml.model_manager import ModelManager
    monkeypatch.setattr(pe, "QWEN3_LAYERS", KLEIN_TAPS)
    hip_root, wheel_root = tmp_path / "hip", tmp_path / "wheel"
    for r in (hip_root, wheel_root):
        r.mkdir()
        model = stage_klein(r)
    dev = _dev(lib)
    # 1. backend "hip" writes the file export_klein writes: keys, shape, dtype, metadata; the tensor within the model bound
    assert pe.ensure_prompt_embeds(hip_root, "klein", device=dev, backend="hip", lib=lib, log=print) is True
    assert pe.ensure_prompt_embeds(wheel_root, "klein", device="cpu", log=print) is True
    (got, gmd), (want, wmd) = _read(hip_root / "prompt_embeds.safetensors"), _read(wheel_root / "prompt_embeds.safetensors")
    assert gmd == wmd and set(got) == set(want) == {"prompt_embeds"} and gmd["prompt"]
    g, w = got["prompt_embeds"], want["prompt_embeds"]
    assert g.dtype == w.dtype == torch.bfloat16 and tuple(g.shape) == tuple(w.shape) == (512, 3 * 256)
    from transformers import AutoTokenizer
    tok = AutoTokenizer.from_pretrained(str(hip_root / "tokenizer"))
    text = tok.apply_chat_template([{"role": "user", "content": gmd["prompt"]}], tokenize=False, add_generation_prompt=True, enable_thinking=False)
    t = tok([text], padding="max_length", max_length=512, truncation=True, return_tensors="pt")
    n = int(t.attention_mask.sum())
    ref = qwen_wheel(model, t.input_ids[0], n, KLEIN_TAPS)
    floor = rel_l2(qwen_wheel(rounded_twin(model), t.input_ids[0], n, KLEIN_TAPS), ref)
    err = rel_l2(g.float(), w.float())
    print(f"Klein export, hip vs wheel (bf16): {100 * err:.3f} %  floor {100 * floor:.3f} %  ratio {err / floor:.2f}")
    assert err <= FACTOR * floor, f"backend hip differs from export_klein by {100 * err:.3f} %, {err / floor:.2f} x the floor"
    assert rel_l2(g.float(), ref) <= FACTOR * floor
    # 2. the pipeline hook
    pipe = Flux2KleinHip(_stub_dit(lib), None)
    pipe.set_prompt_embeds(g.to(dev), prompt=gmd["prompt"])
    stored = _bytes(pipe.encode_prompt(prompt=None)[0][0])
    assert torch.equal(_bytes(pipe.encode_prompt(prompt=OTHER)[0][0]), stored), "without an encoder a foreign prompt returns the stored bytes, as before"
    calls = []
    pipe.set_text_encoder(lambda prompt: (calls.append(prompt), pe.encode_klein_hip(hip_root, prompt, dev, lib))[1])
    assert torch.equal(_bytes(pipe.encode_prompt(prompt=None)[0][0]), stored) and torch.equal(_bytes(pipe.encode_prompt(prompt=gmd["prompt"])[0][0]), stored)
    assert calls == []
    other, ids = pipe.encode_prompt(prompt=OTHER)
    assert tuple(other.shape) == (1, 512, 3 * 256) and tuple(ids.shape) == (1, 512, 4)
    assert not torch.equal(_bytes(other[0]), stored), "another prompt gives the stored embeddings"
    assert torch.equal(_bytes(other[0]), _bytes(pe.encode_klein_hip(hip_root, OTHER, dev, lib))), "encode_prompt(other) is not encode_klein_hip(other)"
    pipe.encode_prompt(prompt=OTHER)
    assert calls == [OTHER], "an encoded prompt is kept"
    # 3. the manager's switch
    mgr = ModelManager.__new__(ModelManager)
    mgr.device, probe = dev, Flux2KleinHip(_stub_dit(lib), None)
    mgr.flux_prompt_encoder = "wheel"
    mgr._attach_prompt_encoder(probe, hip_root, "klein")
    assert probe._text_encoder is None
    mgr.flux_prompt_encoder = "hip"
    mgr._attach_prompt_encoder(probe, tmp_path / "nothing-staged", "klein")
    assert probe._text_encoder is None
    mgr._attach_prompt_encoder(probe, hip_root, "klein")
    assert probe._text_encoder is not None


def check_kontext_wiring(lib, tmp_path):
    from mangatranslator_amd.core.ml import prompt_embeds as pe
    from mangatranslator_amd.core.ml.flux import FluxKontextHip
    hip_root, wheel_root = tmp_path / "hip", tmp_path / "wheel"
    for r in (hip_root, wheel_root):
        r.mkdir()
        clip, t5 = stage_kontext(r)
    dev = _dev(lib)
    assert pe.ensure_prompt_embeds(hip_root, "kontext", device=dev, backend="hip", lib=lib, log=print) is True
    assert pe.ensure_prompt_embeds(wheel_root, "kontext", device="cpu", log=print) is True
    (got, gmd), (want, wmd) = _read(hip_root / "prompt_embeds.safetensors"), _read(wheel_root / "prompt_embeds.safetensors")
    assert gmd == wmd and set(got) == set(want) == {"prompt_embeds", "pooled_prompt_embeds"} and gmd["prompt"] == pe.KONTEXT_PROMPT
    for key, shape in (("prompt_embeds", (512, 128)), ("pooled_prompt_embeds", (128,))):
        assert got[key].dtype == want[key].dtype == torch.bfloat16 and tuple(got[key].shape) == tuple(want[key].shape) == shape
    from transformers import AutoTokenizer
    tok, tok2 = AutoTokenizer.from_pretrained(str(hip_root / "tokenizer")), AutoTokenizer.from_pretrained(str(hip_root / "tokenizer_2"))
    ids = tok([gmd["prompt"]], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    ids2 = tok2([gmd["prompt"]], padding="max_length", max_length=512, truncation=True, return_tensors="pt").input_ids
    with torch.no_grad():
        for what, key, ref, twin in (("T5 sequence", "prompt_embeds", t5_wheel(t5, ids2[0]), t5_wheel(rounded_twin(t5), ids2[0])),
                                     ("CLIP pooled", "pooled_prompt_embeds", clip(input_ids=ids).pooler_output[0], rounded_twin(clip)(input_ids=ids).pooler_output[0])):
            floor, err = rel_l2(twin, ref), rel_l2(got[key].float(), want[key].float())
            print(f"Kontext export, {what}, hip vs wheel (bf16): {100 * err:.3f} %  floor {100 * floor:.3f} %  ratio {err / floor:.2f}")
            assert err <= FACTOR * floor and rel_l2(got[key].float(), ref) <= FACTOR * floor, f"{what}: backend hip differs from export_kontext by {err / floor:.2f} x the floor"
    pipe = FluxKontextHip(_stub_dit(lib), None)
    pipe.set_prompt_embeds(got["prompt_embeds"].to(dev), got["pooled_prompt_embeds"].to(dev), prompt=gmd["prompt"])
    seq0, pooled0, _ = pipe.encode_prompt(prompt=None)
    seq1, pooled1, _ = pipe.encode_prompt(prompt=OTHER, prompt_2=None)
    assert torch.equal(_bytes(seq1), _bytes(seq0)) and torch.equal(_bytes(pooled1), _bytes(pooled0)), "without an encoder a foreign prompt returns the stored bytes"
    pipe.set_text_encoder(lambda prompt: pe.encode_kontext_hip(hip_root, prompt, dev, lib))
    for p in (None, gmd["prompt"]):
        s, q, _ = pipe.encode_prompt(prompt=p)
        assert torch.equal(_bytes(s), _bytes(seq0)) and torch.equal(_bytes(q), _bytes(pooled0))
    s, q, _ = pipe.encode_prompt(prompt=OTHER)
    assert tuple(s.shape) == (1, 512, 128) and tuple(q.shape) == (1, 128)
    assert not torch.equal(_bytes(s), _bytes(seq0)) and not torch.equal(_bytes(q), _bytes(pooled0)), "another prompt gives the stored embeddings"
    ws, wq = pe.encode_kontext_hip(hip_root, OTHER, dev, lib)
    assert torch.equal(_bytes(s[0]), _bytes(ws)) and torch.equal(_bytes(q[0]), _bytes(wq))
