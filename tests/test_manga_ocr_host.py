"""Host logic of manga-ocr (core/ml/manga_ocr.py), exact, on the CPU: the beam search against transformers' `generate`, the text rules as a table
of known answers, the checkpoint reader's refusals."""
import pytest
import torch

import manga_ocr_checks as mc
from mangatranslator_amd.core.ml import manga_ocr as mo
from mangatranslator_amd.utils.exceptions import ModelError

# scripted, step-dependent bonus on the EOS score (the seeded tiny models never emit EOS by themselves): hypotheses finish at different lengths,
# all at once, never
EOS_SCRIPTS = {"staggered": lambda n: 1.1 * n - 4.0, "at_once": lambda n: 1.0e4 if n >= 10 else 0.0, "never": lambda n: 0.0}


def _generate(seed, script, **gen):
    from transformers import LogitsProcessor, LogitsProcessorList
    model, pixels = mc.oracle(seed)

    class EosBonus(LogitsProcessor):
        def __call__(self, input_ids, scores):
            scores = scores.clone()
            scores[:, mc.EOS] += EOS_SCRIPTS[script](input_ids.shape[-1])
            return scores
    with torch.no_grad():
        out = model.generate(pixels, logits_processor=LogitsProcessorList([EosBonus()]), do_sample=False, **gen)
    return out[0].tolist()


def _search(seed, script, **gen):
    model, pixels = mc.oracle(seed)
    cfg = mo.hparams_from_config(mc.config_dict(model, gen))["gen"]
    lengths = []

    def step_fn(st):
        logp = mc.oracle_logp(model, pixels, st.sequences)[:, -1].clone()
        logp[:, mc.EOS] += EOS_SCRIPTS[script](len(st.sequences[0]))
        lengths.append(st.pos)
        return logp
    return mo.beam_search(step_fn, cfg), lengths


@pytest.mark.parametrize("script", list(EOS_SCRIPTS))
@pytest.mark.parametrize("seed", range(8))
def test_beam_search_equals_generate(seed, script):
    want = _generate(seed, script, **mc.GEN)
    got, steps = _search(seed, script, **mc.GEN)
    assert got == want, f"seed {seed}, EOS script {script}: beam_search {got} != generate {want}"
    assert steps == list(range(len(steps)))
    if script == "never":
        assert len(got) == mc.GEN["max_length"] and mc.EOS not in got
    if script == "at_once":
        assert got[-1] == mc.EOS and len(got) < mc.GEN["max_length"]


@pytest.mark.parametrize("script", list(EOS_SCRIPTS))
@pytest.mark.parametrize("seed", range(8))
def test_greedy_equals_generate(seed, script):
    gen = dict(num_beams=1, no_repeat_ngram_size=3, max_length=24)
    want = _generate(seed, script, **gen)
    got, _ = _search(seed, script, **gen)
    assert got == want, f"seed {seed}, EOS script {script}: greedy {got} != generate {want}"


def test_eos_scripts_make_hypotheses_finish_at_different_lengths():
    """the property the scripts are there for, from the oracle alone: over the seeds the staggered script ends sequences at several lengths"""
    assert len({len(_generate(s, "staggered", **mc.GEN)) for s in range(8)}) >= 3


TEXT_CASES = [("1 2", "１２"), ("p.3", "ｐ．３"), ("…", "．．．"), ("・・・", "．．．"), ("ｶﾞ", "ガ"), ("ﾊﾟﾊﾞﾊ", "パバハ"), ("ｱ ｲ\n\tｳ", "アイウ"),
              ("A-z!", "Ａ－ｚ！"), ("あ。・い", "あ。・い"), ("ｳﾞｧ", "ヴァ"), ("a..b", "ａ．．ｂ"), ("a.b", "ａ．ｂ")]


@pytest.mark.parametrize("raw,want", TEXT_CASES)
def test_post_process_known_answers(raw, want):
    assert mo.post_process(raw) == want


def test_dot_rules_run_before_the_full_width_pass():
    """upstream's order: the ellipsis and the runs become ASCII dots first, the full-width pass then widens them"""
    assert mo.dot_rules("・・・") == "..." and mo.dot_rules("…") == "..." and mo.dot_rules("・") == "・" and mo.dot_rules("・.・.") == "...."
    assert mo.h2z("...") == "．．．"


def test_tokens_to_text_drops_special_tokens_and_glues_pieces():
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "あ", "##い", "1", "2"]
    assert mo.tokens_to_text([2, 5, 6, 7, 0, 8, 3, 4, 1], vocab) == "あい 1 2"
    assert mo.post_process(mo.tokens_to_text([2, 7, 8, 3], vocab)) == "１２"


def test_refused_configurations_are_named():
    model, _ = mc.oracle(0)
    base = mc.config_dict(model)

    def hp(**over):
        c = {k: (dict(v) if isinstance(v, dict) else v) for k, v in base.items()}
        for k, v in over.items():
            if "." in k:
                a, b = k.split(".")
                c[a][b] = v
            else:
                c[k] = v
        return mo.hparams_from_config(c)
    for over, word in [({"do_sample": True}, "sampling"), ({"num_beams": 9}, "beams"), ({"decoder.num_attention_heads": 4}, "head width"),
                       ({"encoder.num_attention_heads": 1}, "head width"), ({"decoder.hidden_size": 256, "decoder.num_attention_heads": 4}, "enc_to_dec_proj"),
                       ({"decoder.hidden_act": "relu"}, "activation"), ({"max_length": 65}, "positions")]:
        with pytest.raises(ModelError, match=word):
            hp(**over)
    good = hp(**mc.GEN)
    sd = dict(model.state_dict())
    mo.normalise_state_dict(sd, good)
    with pytest.raises(ModelError, match="missing keys"):
        mo.normalise_state_dict({k: v for k, v in sd.items() if k != "encoder.layernorm.bias"}, good)
    with pytest.raises(ModelError, match="unexpected keys"):
        mo.normalise_state_dict(dict(sd, extra=torch.zeros(1)), good)
    with pytest.raises(ModelError, match="enc_to_dec_proj"):
        mo.normalise_state_dict({**sd, "enc_to_dec_proj.weight": torch.zeros(1)}, good)
