"""manga-ocr on the HIP path: the recogniser behind `ModelManager.get_manga_ocr()` (reference core/ml/model_manager.py:835-904, where it is
the `manga_ocr.MangaOcr` wrapper around a transformers `VisionEncoderDecoderModel`: ViT encoder, BERT decoder with cross-attention).

    MangaOcrHip(state_dict, config, vocab)(pil_image) -> str

  * every hyper-parameter comes from the checkpoint's `config.json` / `generation_config.json` (`read_checkpoint`); what this build does not
    serve raises ModelError by name: sampling, a head width other than 64, more than 8 beams, an `enc_to_dec_proj`, another activation;
  * encoder plan, once per image: MTX_EW_IM2COL_PATCH + patch GEMM (bias and position table in its epilogue), class token, pre-LN blocks on the
    GEMM / attention / norm kernels, final LayerNorm, then the cross-attention K | V of every decoder layer;
  * step plan, ONE graph replayed per token with R = num_beams rows: embedding gathers + LayerNorm; per layer QKV, decode attention over the
    device-resident cache (MTX_OP_DECODE_ATTN: length and beam ancestry live in device memory, a reorder moves no cache data), output
    projection, cross attention, MLP (BERT is post-LN); head transform -> fp32 vocabulary logits.  Between steps the host uploads token ids,
    position and the ancestry table in one small copy and downloads the logits;
  * storage: f16 by default (like the detectors), bf16 selectable — weights and the linears' operands in that type, every residual sum and
    LayerNorm input fp32 — or abi.F32 ("high": weights, activations and caches fp32 on the fp32 kernels of csrc/f32ops.hip and the fp32 forms of
    the two decode kernels) for a decoder whose log-probs must follow the fp32 model's to 1e-3 whatever its conditioning;
  * the linears of the step run on the skinny-row kernel (MTX_OP_ROWLIN) or the tile GEMM, per shape: `linear_route` (docs/experiments.md,
    "manga-ocr on the HIP path", holds the A/B);
  * the search is on the host: `beam_search` restates transformers' beam search (top 2 * beams candidates, finished hypotheses scored by
    sum / len ** length_penalty, n-gram ban, early stopping, final pick) as a pure function of a `step_fn`; num_beams == 1 is plain greedy
    through the same code.

PARITY UNPINNED (nothing on the build machine can pin them; DESIGN.md's oracle table says the same):
  * pre-processing: `img.convert("L").convert("RGB")`, then the antialiased bilinear resize and normalisation exactly as `SamHipBase._pre_plan`
    does them (ATen's uint8 kernel) — the wheel's processor is torchvision-backed and torchvision is absent here;
  * the hub checkpoint's key layout (both the historical names and transformers 5's are accepted; only `save_pretrained` output was seen) and
    the shipped decoder depth;
  * manga-ocr's text post-processing, restated from its published behaviour, and in it the ASCII punctuation of `jaconv.h2z` (H2Z_PUNCT)."""
import json
import math
import re
import threading
from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from ...hip import abi
from ...hip.lib import get_library
from ...hip.plan import Act, PlanBuilder, PlanCache
from ...utils.exceptions import ModelError
from . import packing, vit_common

MAX_BEAMS = abi.DECODE_MAX_ROWS
HEAD_DIM = 64
MAX_BATCH_ROWS = abi.WIDE_ROWS_MAX
# crops `ModelManager.get_manga_ocr()` reads together unless `manga_ocr_slots` says otherwise: decided by the page measurement of
# tools/bench_kernels.py mangaocr_batch (docs/experiments.md, "manga-ocr: a page's crops together")
DEFAULT_SLOTS = 8


# ---- generation settings and the host-side search ----------------------------------------------------------------------------------------------
@dataclass
class GenerationSettings:
    decoder_start_token_id: int
    eos_token_id: Sequence[int]
    pad_token_id: Optional[int] = None
    max_length: int = 20
    num_beams: int = 1
    no_repeat_ngram_size: int = 0
    length_penalty: float = 1.0
    early_stopping: object = False          # False, True or "never", as in transformers


@dataclass
class BeamStep:
    """what `step_fn` is asked: the log-probs [rows, vocab] of the next token for every row.  `pos` positions are already cached (the token fed
    is the one at index pos); row r continues the row `parents[r]` of the previous step and feeds `tokens[r]`; `sequences[r]` is its whole
    history (for a step_fn that recomputes instead of caching)."""
    pos: int
    tokens: List[int]
    parents: List[int]
    sequences: List[List[int]] = field(default_factory=list)


def _banned_ngram_tokens(seq: List[int], n: int) -> List[int]:
    """tokens that would repeat an n-gram of `seq` (transformers' NoRepeatNGramLogitsProcessor)"""
    if n <= 0 or len(seq) + 1 < n:
        return []
    prefix = tuple(seq[len(seq) + 1 - n:]) if n > 1 else ()
    return [seq[i + n - 1] for i in range(len(seq) - n + 1) if tuple(seq[i:i + n - 1]) == prefix]


def beam_search(step_fn: Callable[[BeamStep], torch.Tensor], cfg: GenerationSettings) -> List[int]:
    """transformers' beam search (generation/utils.py `_beam_search`, batch 1, one returned sequence) restated over a step function; the float32
    arithmetic and the `topk` calls are its own, so ties fall the same way.  Returns the chosen hypothesis, start token included."""
    B = int(cfg.num_beams)
    eos = set(int(t) for t in cfg.eos_token_id)
    early = cfg.early_stopping if B > 1 else True          # one beam: stop at its first finished hypothesis = greedy decoding
    lp, max_length = float(cfg.length_penalty), int(cfg.max_length)
    keep = max(2, 1 + len(eos)) * B
    top_mask = torch.tensor([True] * B + [False] * (keep - B))
    running = [[int(cfg.decoder_start_token_id)] for _ in range(B)]
    running_scores = torch.zeros(1, B)
    running_scores[:, 1:] = -1e9                            # the B rows start identical: only the first may seed candidates
    fin = [list(running[0]) for _ in range(B)]
    fin_scores = torch.full((1, B), -1e9)
    fin_done = torch.zeros(1, B, dtype=torch.bool)
    unsatisfied = torch.ones(1, 1, dtype=torch.bool)
    parents, cur_len = list(range(B)), 1
    if max_length <= 1:
        return running[0]
    while True:
        logp = torch.as_tensor(step_fn(BeamStep(cur_len - 1, [s[-1] for s in running], parents, running)), dtype=torch.float32).clone()
        V = logp.shape[-1]
        for b in range(B):
            banned = _banned_ngram_tokens(running[b], int(cfg.no_repeat_ngram_size))
            if banned:
                logp[b, banned] = -float("inf")
        acc = (logp.view(1, B, V) + running_scores[:, :, None]).reshape(1, B * V)
        top_lp, top_idx = torch.topk(acc, k=keep)
        beam_idx, tok = (top_idx // V)[0].tolist(), (top_idx % V)[0].tolist()
        cand = [running[b] + [t] for b, t in zip(beam_idx, tok)]
        hits = torch.tensor([[t in eos or cur_len + 1 >= max_length for t in tok]])
        # the running beams of the next step: the best candidates that did not stop
        masked = top_lp + hits.to(torch.float32) * -1.0e9
        nxt = torch.topk(masked, k=B)[1]
        running = [cand[i] for i in nxt[0].tolist()]
        running_scores = torch.gather(masked, 1, nxt)
        parents = [beam_idx[i] for i in nxt[0].tolist()]
        # the finished hypotheses: only a candidate among the top B may enter
        just = hits & top_mask[None, :]
        sc = top_lp / ((cur_len + 1 - 1) ** lp)
        full = torch.all(fin_done, dim=-1, keepdim=True) & (early is True)
        sc = sc + full.to(torch.float32) * -1.0e9
        sc = sc + (~unsatisfied).to(torch.float32) * -1.0e9
        sc = sc + (~just) * -1.0e9
        merged = fin + cand
        merged_scores = torch.cat((fin_scores, sc), dim=1)
        merged_done = torch.cat((fin_done, just), dim=1)
        pick = torch.topk(merged_scores, k=B)[1]
        fin = [merged[i] for i in pick[0].tolist()]
        fin_scores, fin_done = torch.gather(merged_scores, 1, pick), torch.gather(merged_done, 1, pick)
        cur_len += 1
        # can a running beam still beat the worst finished one?
        best_len = (max_length - 1) if (early == "never" and lp > 0.0) else (cur_len - 1)
        best_running = running_scores[:, :1] / (best_len ** lp)
        worst_fin = torch.where(fin_done, torch.min(fin_scores, dim=1, keepdim=True)[0], torch.tensor(-1.0e9))
        unsatisfied = unsatisfied & torch.any(best_running > worst_fin, dim=-1, keepdim=True)
        go_on = bool(torch.any(unsatisfied)) and not (bool(torch.all(fin_done)) and early is True) and not bool(torch.all(hits))
        if not go_on:
            return fin[0]


# ---- text ---------------------------------------------------------------------------------------------------------------------------------------
SPECIAL_TOKENS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")

# PARITY UNPINNED: jaconv.h2z(ascii=True) maps most of ASCII to the Unicode fullwidth block (code point + 0xFEE0); these are the characters whose
# fullwidth form is NOT that block's in the jaconv tables this was restated from, and the ones that differ between jaconv versions.
H2Z_PUNCT = {'"': "”", "'": "’", "\\": "￥", "`": "‘", " ": "　"}

_HW_KANA = "ｦｧｨｩｪｫｬｭｮｯｰｱｲｳｴｵｶｷｸｹｺｻｼｽｾｿﾀﾁﾂﾃﾄﾅﾆﾇﾈﾉﾊﾋﾌﾍﾎﾏﾐﾑﾒﾓﾔﾕﾖﾗﾘﾙﾚﾛﾜﾝﾞﾟ｡｢｣､･"
_FW_KANA = "ヲァィゥェォャュョッーアイウエオカキクケコサシスセソタチツテトナニヌネノハヒフヘホマミムメモヤユヨラリルレロワン゛゜。「」、・"
_KANA = dict(zip(_HW_KANA, _FW_KANA))
_VOICED = dict(zip("ｶｷｸｹｺｻｼｽｾｿﾀﾁﾂﾃﾄﾊﾋﾌﾍﾎｳ", "ガギグゲゴザジズゼゾダヂヅデドバビブベボヴ"))
_SEMI_VOICED = dict(zip("ﾊﾋﾌﾍﾎ", "パピプペポ"))


def h2z(text: str) -> str:
    """jaconv.h2z(text, kana=True, ascii=True, digit=True): half-width katakana (voiced marks folded into the letter before them), ASCII
    letters, digits and punctuation to their full-width forms"""
    out, i = [], 0
    while i < len(text):
        ch, nx = text[i], text[i + 1] if i + 1 < len(text) else ""
        if nx == "ﾞ" and ch in _VOICED:
            out.append(_VOICED[ch]); i += 2; continue
        if nx == "ﾟ" and ch in _SEMI_VOICED:
            out.append(_SEMI_VOICED[ch]); i += 2; continue
        if ch in _KANA:
            out.append(_KANA[ch])
        elif ch in H2Z_PUNCT:
            out.append(H2Z_PUNCT[ch])
        elif "!" <= ch <= "~":
            out.append(chr(ord(ch) + 0xFEE0))
        else:
            out.append(ch)
        i += 1
    return "".join(out)


def dot_rules(text: str) -> str:
    """the ellipsis character spelt out, runs of two or more of `・` / `.` as that many dots"""
    text = text.replace("…", "...")
    return re.sub("[・.]{2,}", lambda m: (m.end() - m.start()) * ".", text)


def post_process(text: str) -> str:
    """manga-ocr's clean-up of the decoded string, in its order: whitespace out, dot rules, then the full-width pass (so the dots a run was
    turned into leave full-width).  PARITY UNPINNED: restated, the package is not on the build machine."""
    return h2z(dot_rules("".join(text.split())))


def tokens_to_text(ids: Sequence[int], vocab: Sequence[str]) -> str:
    """BertTokenizer.decode(ids, skip_special_tokens=True): special tokens dropped, pieces joined by spaces, ` ##` continuations glued"""
    pieces = [vocab[i] if 0 <= i < len(vocab) else "[UNK]" for i in ids]
    return " ".join(p for p in pieces if p not in SPECIAL_TOKENS).replace(" ##", "").strip()


# ---- checkpoint ---------------------------------------------------------------------------------------------------------------------------------
def _rename_historical(key: str) -> str:
    """the hub's historical ViT names (transformers 4: encoder.encoder.layer.N.attention.attention.query ...) -> transformers 5's"""
    m = re.match(r"encoder\.encoder\.layer\.(\d+)\.(.+)$", key)
    if not m:
        return key
    n, rest = m.group(1), m.group(2)
    table = {"attention.attention.query": "attention.q_proj", "attention.attention.key": "attention.k_proj", "attention.attention.value": "attention.v_proj",
             "attention.output.dense": "attention.o_proj", "intermediate.dense": "mlp.fc1", "output.dense": "mlp.fc2",
             "layernorm_before": "layernorm_before", "layernorm_after": "layernorm_after"}
    for old, new in table.items():
        if rest.startswith(old + "."):
            return f"encoder.layers.{n}.{new}.{rest[len(old) + 1:]}"
    return key


# tensors a checkpoint may carry that the forward pass never reads: the ViT pooler, BERT's index buffers, the tied copy of the output bias
IGNORED_KEYS = ("encoder.pooler.", "decoder.bert.embeddings.position_ids", "decoder.bert.embeddings.token_type_ids", "decoder.bert.pooler.")


def hparams_from_config(config: dict, generation: Optional[dict] = None) -> dict:
    """every size the graphs need, from `config.json` (+ `generation_config.json`); ModelError names what is not served"""
    enc, dec = config.get("encoder"), config.get("decoder")
    if not isinstance(enc, dict) or not isinstance(dec, dict):
        raise ModelError("manga-ocr: config.json must hold an `encoder` and a `decoder` section (VisionEncoderDecoderConfig)")
    if enc.get("model_type", "vit") != "vit" or dec.get("model_type", "bert") != "bert":
        raise ModelError(f"manga-ocr: only a ViT encoder with a BERT decoder is built, not {enc.get('model_type')} / {dec.get('model_type')}")
    gen = dict(generation or {})

    def g(name, default=None):
        for src in (gen, config, dec):
            if src.get(name) is not None:
                return src[name]
        return default
    hp = dict(e_dim=int(enc["hidden_size"]), e_layers=int(enc["num_hidden_layers"]), e_heads=int(enc["num_attention_heads"]),
              e_mlp=int(enc["intermediate_size"]), patch=int(enc["patch_size"]), image=enc["image_size"], e_eps=float(enc.get("layer_norm_eps", 1e-12)),
              e_act=enc.get("hidden_act", "gelu"), channels=int(enc.get("num_channels", 3)),
              d_dim=int(dec["hidden_size"]), d_layers=int(dec["num_hidden_layers"]), d_heads=int(dec["num_attention_heads"]),
              d_mlp=int(dec["intermediate_size"]), vocab=int(dec["vocab_size"]), positions=int(dec["max_position_embeddings"]),
              d_eps=float(dec.get("layer_norm_eps", 1e-12)), d_act=dec.get("hidden_act", "gelu"))
    if isinstance(hp["image"], (list, tuple)):
        if len(set(hp["image"])) != 1:
            raise ModelError("manga-ocr: a non-square encoder input is not built")
        hp["image"] = hp["image"][0]
    hp["image"] = int(hp["image"])
    if hp["channels"] != 3 or hp["image"] % hp["patch"]:
        raise ModelError("manga-ocr: the encoder must take 3 channels and an image size that its patches tile")
    for side, dim, heads in (("encoder", hp["e_dim"], hp["e_heads"]), ("decoder", hp["d_dim"], hp["d_heads"])):
        if dim % heads or dim // heads != HEAD_DIM:
            raise ModelError(f"manga-ocr: {side} head width {dim / heads:g} is not built (only {HEAD_DIM})")
    if hp["e_act"] != "gelu" or hp["d_act"] != "gelu":
        raise ModelError(f"manga-ocr: activation {hp['e_act']!r} / {hp['d_act']!r} is not built (only erf-GELU)")
    if dec.get("position_embedding_type", "absolute") != "absolute":
        raise ModelError("manga-ocr: only absolute position embeddings are built")
    if not dec.get("add_cross_attention", True) or not dec.get("is_decoder", True):
        raise ModelError("manga-ocr: the decoder must be a BERT decoder with cross-attention")
    if hp["e_dim"] != hp["d_dim"] and not dec.get("cross_attention_hidden_size"):
        raise ModelError("manga-ocr: encoder and decoder widths differ, which needs an `enc_to_dec_proj`: not built")
    if g("do_sample", False):
        raise ModelError("manga-ocr: sampling (do_sample) is not built; the search is greedy / beam")
    if int(g("num_beam_groups", 1) or 1) != 1:
        raise ModelError("manga-ocr: grouped beam search is not built")
    beams = int(g("num_beams", 1) or 1)
    if not 1 <= beams <= MAX_BEAMS:
        raise ModelError(f"manga-ocr: {beams} beams are not built (1 .. {MAX_BEAMS})")
    start = g("decoder_start_token_id")
    eos = g("eos_token_id")
    if start is None or eos is None:
        raise ModelError("manga-ocr: config.json must give decoder_start_token_id and eos_token_id")
    max_length = int(g("max_length", 20))
    if max_length > hp["positions"]:
        raise ModelError(f"manga-ocr: max_length {max_length} exceeds the decoder's {hp['positions']} positions")
    hp["gen"] = GenerationSettings(decoder_start_token_id=int(start), eos_token_id=[int(e) for e in (eos if isinstance(eos, (list, tuple)) else [eos])],
                                   pad_token_id=g("pad_token_id"), max_length=max_length, num_beams=beams,
                                   no_repeat_ngram_size=int(g("no_repeat_ngram_size", 0) or 0), length_penalty=float(g("length_penalty", 1.0)),
                                   early_stopping=g("early_stopping", False))
    return hp


def expected_keys(hp: dict) -> List[str]:
    keys = ["encoder.embeddings.cls_token", "encoder.embeddings.position_embeddings"]

    def wb(prefix):
        keys.extend([prefix + ".weight", prefix + ".bias"])
    wb("encoder.embeddings.patch_embeddings.projection")
    for i in range(hp["e_layers"]):
        for n in ("attention.q_proj", "attention.k_proj", "attention.v_proj", "attention.o_proj", "layernorm_before", "layernorm_after", "mlp.fc1", "mlp.fc2"):
            wb(f"encoder.layers.{i}.{n}")
    wb("encoder.layernorm")
    e = "decoder.bert.embeddings."
    keys.extend([e + "word_embeddings.weight", e + "position_embeddings.weight", e + "token_type_embeddings.weight"])
    wb(e + "LayerNorm")
    for i in range(hp["d_layers"]):
        p = f"decoder.bert.encoder.layer.{i}."
        for a in ("attention", "crossattention"):
            for n in ("self.query", "self.key", "self.value", "output.dense", "output.LayerNorm"):
                wb(p + f"{a}.{n}")
        for n in ("intermediate.dense", "output.dense", "output.LayerNorm"):
            wb(p + n)
    c = "decoder.cls.predictions."
    wb(c + "transform.dense"); wb(c + "transform.LayerNorm")
    keys.extend([c + "bias", c + "decoder.weight", c + "decoder.bias"])
    return keys


def normalise_state_dict(sd: Dict[str, torch.Tensor], hp: dict) -> Dict[str, torch.Tensor]:
    """both key layouts -> transformers 5's names; the tied head tensors filled in; every missing or unexpected key is a ModelError"""
    out = {}
    for k, v in sd.items():
        if k.startswith(IGNORED_KEYS):
            continue
        if k.startswith("enc_to_dec_proj"):
            raise ModelError("manga-ocr: the checkpoint carries an `enc_to_dec_proj`, which is not built")
        out[_rename_historical(k)] = v
    c = "decoder.cls.predictions."
    if c + "decoder.weight" not in out and "decoder.bert.embeddings.word_embeddings.weight" in out:      # tied, and safetensors stores one copy
        out[c + "decoder.weight"] = out["decoder.bert.embeddings.word_embeddings.weight"]
    if c + "decoder.bias" not in out and c + "bias" in out:
        out[c + "decoder.bias"] = out[c + "bias"]
    if c + "bias" not in out and c + "decoder.bias" in out:
        out[c + "bias"] = out[c + "decoder.bias"]
    want = set(expected_keys(hp))
    missing, unexpected = sorted(want - set(out)), sorted(set(out) - want)
    if missing or unexpected:
        raise ModelError(f"manga-ocr checkpoint: missing keys {missing[:6]}{' ...' if len(missing) > 6 else ''}, "
                         f"unexpected keys {unexpected[:6]}{' ...' if len(unexpected) > 6 else ''}")
    return out


def read_checkpoint(root) -> dict:
    """a staged `manga-ocr-base` directory -> dict(hp, state_dict, vocab, mean, std)"""
    root = Path(root)
    if not (root / "config.json").is_file():
        raise ModelError(f"manga-ocr is not staged: {root / 'config.json'} not found")
    config = json.loads((root / "config.json").read_text())
    gen_path = root / "generation_config.json"
    hp = hparams_from_config(config, json.loads(gen_path.read_text()) if gen_path.is_file() else None)
    if (root / "model.safetensors").is_file():
        from safetensors.torch import load_file
        sd = load_file(str(root / "model.safetensors"))
    elif (root / "pytorch_model.bin").is_file():
        sd = torch.load(str(root / "pytorch_model.bin"), map_location="cpu", weights_only=True)
    else:
        raise ModelError(f"manga-ocr is not staged: neither model.safetensors nor pytorch_model.bin in {root}")
    if not (root / "vocab.txt").is_file():
        raise ModelError(f"manga-ocr is not staged: {root / 'vocab.txt'} not found")
    vocab = (root / "vocab.txt").read_text(encoding="utf-8").split("\n")
    if vocab and vocab[-1] == "":
        vocab.pop()
    mean = std = (0.5, 0.5, 0.5)
    pre_path = root / "preprocessor_config.json"
    if pre_path.is_file():
        pre = json.loads(pre_path.read_text())
        mean, std = tuple(pre.get("image_mean", mean)), tuple(pre.get("image_std", std))
    return dict(hp=hp, state_dict=normalise_state_dict(sd, hp), vocab=vocab, mean=mean, std=std)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
def linear_route(rows: int, n: int, k: int) -> str:
    """which kernel a linear of the decode step runs on: "rowlin" (MTX_OP_ROWLIN) or "gemm".  The step moves weights — 19 MB per decoder layer and
    9.4 MB for the 6144 x 768 head at the published widths, against at most 8 activation rows — and the 128-tile GEMM puts a 768-column linear on
    6 workgroups; the A/B of the whole step graph (tools/bench_kernels.py mangaocr; docs/experiments.md) decides per shape."""
    return "rowlin"


class MangaOcrHip:
    def __init__(self, state_dict: dict, hp: dict, vocab: Sequence[str], device="cuda", lib=None, dtype: int = abi.F16, graph: bool = True,
                 mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), rows: Optional[int] = None, route: Optional[Callable[[int, int, int], str]] = None,
                 slots: int = 1):
        """hp: `hparams_from_config`; state_dict: `normalise_state_dict`'s names.  Storage is f16 by default, like the detectors; abi.BF16 is
        selectable.  rows: rows of the step graph (default: num_beams).  route: overrides `linear_route` (benchmarks).  slots: crops that
        `generate_many` decodes together, each with num_beams rows of ONE step graph whose search runs on the device (1: nothing new is built)."""
        if dtype not in (abi.BF16, abi.F16, abi.F32):
            raise ModelError("manga-ocr: storage dtype must be bf16, f16 or f32")
        self.lib = lib if lib is not None else get_library()
        self.device = torch.device(device)
        self.hp, self.gen, self.vocab = hp, hp["gen"], list(vocab)
        self.dtype, self.tdt = dtype, {abi.BF16: torch.bfloat16, abi.F16: torch.float16, abi.F32: torch.float32}[dtype]
        self.f32 = dtype == abi.F32
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.rows = int(rows) if rows is not None else self.gen.num_beams
        if not 1 <= self.rows <= MAX_BEAMS:
            raise ModelError(f"manga-ocr: {self.rows} rows per step are not built (1 .. {MAX_BEAMS})")
        self.slots = int(slots)
        if not 1 <= self.slots <= abi.SLOTS_MAX or self.slots * self.gen.num_beams > MAX_BATCH_ROWS:
            raise ModelError(f"manga-ocr: {self.slots} slots of {self.gen.num_beams} beams are not built (1 .. {abi.SLOTS_MAX} slots, "
                             f"slots * num_beams <= {MAX_BATCH_ROWS})")
        if self.slots > 1 and not 1 <= len(self.gen.eos_token_id) <= 4:
            raise ModelError("manga-ocr: the device search takes 1 .. 4 eos_token_id")
        self._batch = None
        self.route = route or linear_route
        self._graph = graph and not self.lib.is_simulator
        self._lock = threading.Lock()
        self._pre = PlanCache(6)
        self._enc = self._step = None
        self.max_len = min(hp["positions"], max(self.gen.max_length, 1))
        self._pack({k: v.detach().float().cpu() for k, v in state_dict.items()})

    @classmethod
    def from_directory(cls, root, **kw):
        ck = read_checkpoint(root)
        if kw.get("slots") is None:                               # the default, lowered to what the checkpoint's beams allow
            kw["slots"] = max(1, min(DEFAULT_SLOTS, MAX_BATCH_ROWS // ck["hp"]["gen"].num_beams))
        return cls(ck["state_dict"], ck["hp"], ck["vocab"], mean=ck["mean"], std=ck["std"], **kw)

    # ------------------------------------------------------------------------------------------
    def _c(self, t, dtype=None):
        return packing.on_device(t, self.device, dtype if dtype is not None else self.tdt)

    def _pack(self, sd):
        """every linear as the triple (W, None, bias) of core/ml/packing.py `linear` (no hi + lo weights here), every LayerNorm as (gamma, beta)"""
        hp = self.hp
        f32 = torch.float32

        def ln(key):
            return packing.layer_norm(sd, key, self.device)

        def lin(*keys):
            return packing.linear(sd, *keys, device=self.device, dtype=self.tdt)

        C, pk = hp["e_dim"], hp["patch"]
        g = hp["image"] // pk
        W = {}
        W["pe"] = (self._c(packing.patch_embed_rows(sd["encoder.embeddings.patch_embeddings.projection.weight"])), None,       # [C, 3, p, p]
                   self._c(sd["encoder.embeddings.patch_embeddings.projection.bias"], f32))
        pos = sd["encoder.embeddings.position_embeddings"].reshape(-1, C)
        if pos.shape[0] != g * g + 1:
            raise ModelError("manga-ocr: the encoder's position table does not match its image and patch size")
        W["e_pos"] = self._c(pos[1:], f32)
        W["e_cls"] = self._c((sd["encoder.embeddings.cls_token"].reshape(C) + pos[0]).reshape(1, C), f32)
        self.e_layers = []
        for i in range(hp["e_layers"]):
            p = f"encoder.layers.{i}."
            self.e_layers.append(dict(ln1=ln(p + "layernorm_before"), ln2=ln(p + "layernorm_after"),
                                      qkv=lin(p + "attention.q_proj", p + "attention.k_proj", p + "attention.v_proj"), proj=lin(p + "attention.o_proj"),
                                      fc1=lin(p + "mlp.fc1"), fc2=lin(p + "mlp.fc2")))
        W["e_ln"] = ln("encoder.layernorm")
        e = "decoder.bert.embeddings."
        if sd[e + "word_embeddings.weight"].shape[0] != hp["vocab"] or sd[e + "position_embeddings.weight"].shape[0] != hp["positions"]:
            raise ModelError("manga-ocr: the decoder's embedding tables do not match vocab_size / max_position_embeddings")
        W["tok32"] = self._c(sd[e + "word_embeddings.weight"], f32)
        W["d_pos"] = self._c(sd[e + "position_embeddings.weight"] + sd[e + "token_type_embeddings.weight"][0], f32)      # every token has type 0
        W["d_ln"] = ln(e + "LayerNorm")
        self.d_layers = []
        for i in range(hp["d_layers"]):
            p = f"decoder.bert.encoder.layer.{i}."
            s, c = p + "attention.", p + "crossattention."
            self.d_layers.append(dict(qkv=lin(s + "self.query", s + "self.key", s + "self.value"), so=lin(s + "output.dense"), sln=ln(s + "output.LayerNorm"),
                                      cq=lin(c + "self.query"), ckv=lin(c + "self.key", c + "self.value"), co=lin(c + "output.dense"),
                                      cln=ln(c + "output.LayerNorm"), fc1=lin(p + "intermediate.dense"), fc2=lin(p + "output.dense"),
                                      oln=ln(p + "output.LayerNorm")))
        h = "decoder.cls.predictions."
        W["h_t"] = lin(h + "transform.dense")
        W["h_ln"] = ln(h + "transform.LayerNorm")
        W["h_out"] = lin(h + "decoder")
        self.W = W

    # ---- encoder ---------------------------------------------------------------------------------
    def _encoder(self):
        if self._enc is not None:
            return self._enc
        hp, W = self.hp, self.W
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        S, pk, C, heads = hp["image"], hp["patch"], hp["e_dim"], hp["e_heads"]
        g = S // pk
        P, T, K, d = g * g, g * g + 1, pk * pk * 8, HEAD_DIM
        eps = hp["e_eps"]
        img = pb.act(1, S, S, 8, zero=True)
        cols = pb.buf((P, K), self.tdt)
        if self.f32:        # the fp32 kernels have no im2col; with stride == kernel size it is a gather of pixel rows ([S * S, 8] -> [P * p * p, 8])
            py, px, ky, kx = torch.meshgrid(torch.arange(g), torch.arange(g), torch.arange(pk), torch.arange(pk), indexing="ij")
            pix = pb.hold(((py * pk + ky) * S + px * pk + kx).reshape(-1).to(torch.int32).to(self.device))
            pb.row_gather(img.t, cols, pix, P * pk * pk, 8, label="patch_gather")
        else:
            pb.im2col(img, cols, pk, pk, K, pad=False, label="patch_im2col")
        # the residual stream stays fp32 from the patch embedding to the final LayerNorm (SAM's "stream32", core/ml/vit_common.py)
        layer_norm, linear, close_branch = vit_common.trunk_helpers(pb, eps, self.tdt, self.dtype, stream32=True)
        x = pb.buf((T, C), torch.float32)
        x[0].copy_(W["e_cls"][0])                                 # class token + its position: written once, the patch GEMM fills rows 1 ..
        close_branch(cols, W["pe"], P, C, K, W["e_pos"], "patch_embed", out=x, c_off=C)
        for i, L in enumerate(self.e_layers):
            tag = f"enc{i}"
            qkv = linear(layer_norm(x, T, C, L["ln1"], tag + ".ln1"), L["qkv"], T, 3 * C, C, tag + ".qkv")
            o = pb.buf((T, C), self.tdt)
            st = (T * 3 * C, 3 * C, d)
            pb.attention(qkv, qkv, qkv, o, 1, heads, T, T, d, st, st, st, (T * C, C, d), 1.0 / math.sqrt(d), k_off=C, v_off=2 * C, label=tag + ".attn")
            x1 = close_branch(o, L["proj"], T, C, C, x, tag + ".proj")
            h = linear(layer_norm(x1, T, C, L["ln2"], tag + ".ln2"), L["fc1"], T, hp["e_mlp"], C, tag + ".fc1", act=abi.ACT_GELU)
            x = close_branch(h, L["fc2"], T, C, hp["e_mlp"], x1, tag + ".fc2")
        mem = layer_norm(x, T, C, W["e_ln"], "enc.ln")
        cross = [linear(mem, L["ckv"], T, 2 * hp["d_dim"], C, f"dec{i}.cross_kv") for i, L in enumerate(self.d_layers)]
        plan = pb.build()
        plan.img, plan.mem, plan.cross, plan.tokens = img, mem, cross, T
        self._enc = plan
        return plan

    def _pre_plan(self, h, w):
        """uint8 page -> the encoder's input (ATen's antialiased uint8 resize, then rescale + normalise), as SAM's: core/ml/vit_common.py"""
        if (h, w) not in self._pre:
            self._pre[(h, w)] = vit_common.resize_normalise_plan(self.lib, self.device, self.dtype, h, w, self._encoder().img, self.mean, self.std,
                                                                 widen_f16=self.f32)
        return self._pre[(h, w)]

    # ---- decode step -----------------------------------------------------------------------------
    def _stepper(self):
        if self._step is not None:
            return self._step
        hp, W = self.hp, self.W
        enc = self._encoder()
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        R, C, heads, d, L_max, T = self.rows, hp["d_dim"], hp["d_heads"], HEAD_DIM, self.max_len, enc.tokens
        eps = hp["d_eps"]
        # control block, uploaded in one copy per step: [pos | position index per row | token id per row | ancestry table [max_len][R]]
        ctl = pb.buf((1 + 2 * R + L_max * R,), torch.int32, zero=True)
        pos, pos_idx, tok_idx, src = ctl[0:1], ctl[1:1 + R], ctl[1 + R:1 + 2 * R], ctl[1 + 2 * R:]

        def lin(a, wb, n, k, label, act=abi.ACT_NONE, res=None, out_f32=False):
            if self.route(R, n, k) == "rowlin":
                return pb.row_linear(a, wb[0], R, n, k, bias=wb[2], act=act, res=res, out_f32=out_f32, label=label)
            return pb.gemm(a, wb[0], R, n, k, bias=wb[2], act=act, res=res, out_f32=out_f32, label=label)

        def norm(t, wb, label):
            """BERT is post-LN: the branch's sum arrives in fp32 (fp32-output linear + 16-bit residual) and is rounded once, after the norm"""
            return pb.norm(t, pb.buf((R, C), self.tdt), R, C, gamma=wb[0], beta=wb[1], eps=eps, dtype=abi.F32, out_dtype=self.dtype, label=label)

        f32 = torch.float32
        e_tok = pb.row_gather(W["tok32"], pb.buf((R, C), f32), tok_idx, R, C, label="embed.token", dtype=abi.F32)
        e_pos = pb.row_gather(W["d_pos"], pb.buf((R, C), f32), pos_idx, R, C, label="embed.position", dtype=abi.F32)
        e_sum = pb.ew(abi.EW_ADD, Act(e_tok.view(1, 1, R, C), 1, 1, R, C), Act(e_pos.view(1, 1, R, C), 1, 1, R, C),
                      out=Act(pb.buf((1, 1, R, C), f32), 1, 1, R, C), label="embed.add", dtype=abi.F32).t.view(R, C)
        x = norm(e_sum, W["d_ln"], "embed.ln")
        caches = []
        for i, L in enumerate(self.d_layers):
            tag = f"dec{i}"
            kc, vc = pb.buf((L_max, R, C), self.tdt, zero=True), pb.buf((L_max, R, C), self.tdt, zero=True)
            caches.append((kc, vc))
            qkv = lin(x, L["qkv"], 3 * C, C, tag + ".qkv")
            o = pb.decode_attention(qkv, kc, vc, pos, src, pb.buf((R, C), self.tdt), R, R, heads, d, L_max, 1.0 / math.sqrt(d), label=tag + ".self_attn")
            x1 = norm(lin(o, L["so"], C, C, tag + ".self_out", res=x, out_f32=True), L["sln"], tag + ".self_ln")
            cq = lin(x1, L["cq"], C, C, tag + ".cross_q")
            o2 = pb.buf((R, C), self.tdt)
            kv = enc.cross[i]
            pb.attention(cq, kv, kv, o2, 1, heads, R, T, d, (R * C, C, d), (T * 2 * C, 2 * C, d), (T * 2 * C, 2 * C, d), (R * C, C, d), 1.0 / math.sqrt(d),
                         v_off=C, label=tag + ".cross_attn")
            x2 = norm(lin(o2, L["co"], C, C, tag + ".cross_out", res=x1, out_f32=True), L["cln"], tag + ".cross_ln")
            h = lin(x2, L["fc1"], hp["d_mlp"], C, tag + ".fc1", act=abi.ACT_GELU)
            x = norm(lin(h, L["fc2"], C, hp["d_mlp"], tag + ".fc2", res=x2, out_f32=True), L["oln"], tag + ".out_ln")
        t = norm(lin(x, W["h_t"], C, C, "head.transform", act=abi.ACT_GELU, out_f32=True), W["h_ln"], "head.ln")
        logits = lin(t, W["h_out"], hp["vocab"], C, "head.logits", out_f32=True)
        plan = pb.build()
        plan.ctl, plan.logits, plan.caches = ctl, logits, caches
        plan.host = torch.zeros(ctl.shape, dtype=torch.int32, pin_memory=(self.device.type == "cuda"))
        plan.host_src = plan.host[1 + 2 * R:].view(L_max, R)
        self._step = plan
        return plan

    # ---- running ---------------------------------------------------------------------------------
    def encode(self, rgb_u8) -> None:
        """uint8 [H, W, 3] RGB -> the encoder memory and every decoder layer's cross K | V (kept in the plans' buffers)"""
        page = torch.from_numpy(np.array(rgb_u8, dtype=np.uint8, order="C"))
        h, w = int(page.shape[0]), int(page.shape[1])
        pre, enc = self._pre_plan(h, w), self._encoder()
        pre.page.copy_(page.to(self.device))
        pre.run()
        enc.run(graph=self._graph)

    def encode_pixels(self, pixel_values: torch.Tensor) -> None:
        """normalised pixel values [3, S, S] (what the HF processor would hand to the model) instead of a page: parity tests"""
        enc = self._encoder()
        enc.img.t[0, :, :, :3] = pixel_values.permute(1, 2, 0).to(self.device, self.tdt)
        enc.run(graph=self._graph)

    def step(self, st: BeamStep) -> torch.Tensor:
        """one replay of the step graph: fp32 log-probs [rows, vocab] on the host"""
        plan, R = self._stepper(), self.rows
        if not 0 <= st.pos < self.max_len or len(st.tokens) != R or len(st.parents) != R:
            raise ModelError("manga-ocr: decode step outside the cache, or with another row count than the graph's")
        host, hs = plan.host, plan.host_src
        if st.pos > 0:                                         # src'[j][r] = src[j][parent[r]] for j < pos; the position fed now is each row's own
            hs[:st.pos] = hs[:st.pos][:, list(st.parents)]
        hs[st.pos] = torch.arange(R, dtype=torch.int32)
        host[0] = st.pos
        host[1:1 + R] = st.pos
        host[1 + R:1 + 2 * R] = torch.tensor(st.tokens, dtype=torch.int32)
        plan.ctl.copy_(host, non_blocking=True)
        plan.run(graph=self._graph)
        return torch.log_softmax(plan.logits.float().cpu(), dim=-1)

    def generate(self) -> List[int]:
        """the configured search over the image last encoded"""
        return beam_search(self.step, self.gen)

    def __call__(self, img) -> str:
        """PIL image -> text, as `manga_ocr.MangaOcr.__call__`"""
        rgb = np.asarray(img.convert("L").convert("RGB"))
        with self._lock:
            self.encode(rgb)
            ids = self.generate()
        return post_process(tokens_to_text(ids, self.vocab))

    # ---- a page's crops together ------------------------------------------------------------------
    def _stepper_batch(self):
        """ONE plan at rows = slots * num_beams: the gathers read the index vectors the search wrote, every linear runs on MTX_OP_ROWLIN_WIDE,
        self attention on MTX_OP_DECODE_ATTN_BATCH (each group at its own position), cross attention on MTX_OP_ATTN with batch = slots over
        per-slot K | V, and MTX_OP_BEAM_STEP ends the step: no host upload or download inside it"""
        if self._batch is not None:
            return self._batch
        hp, W, gen = self.hp, self.W, self.gen
        enc = self._encoder()
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        S, B, C, heads, d, L_max, T = self.slots, gen.num_beams, hp["d_dim"], hp["d_heads"], HEAD_DIM, self.max_len, enc.tokens
        R, eps = S * B, hp["d_eps"]
        words = abi.beam_state_words(B, L_max)
        state = pb.buf((S, words), torch.int32, zero=True)
        state[:, abi.BEAM_DONE] = 1                              # every slot starts empty
        idx = pb.buf((2, R), torch.int32, zero=True)
        tok_idx, pos_idx = idx[0], idx[1]
        lp = float(gen.length_penalty)
        len_pow = pb.hold(torch.tensor([float(j) ** lp for j in range(1, L_max + 1)], dtype=torch.float64).to(torch.float32).to(self.device))

        def lin(a, wb, n, k, label, act=abi.ACT_NONE, res=None, out_f32=False):
            return pb.row_linear_wide(a, wb[0], R, n, k, bias=wb[2], act=act, res=res, out_f32=out_f32, label=label)

        def norm(t, wb, label):
            return pb.norm(t, pb.buf((R, C), self.tdt), R, C, gamma=wb[0], beta=wb[1], eps=eps, dtype=abi.F32, out_dtype=self.dtype, label=label)

        f32 = torch.float32
        e_tok = pb.row_gather(W["tok32"], pb.buf((R, C), f32), tok_idx, R, C, label="embed.token", dtype=abi.F32)
        e_pos = pb.row_gather(W["d_pos"], pb.buf((R, C), f32), pos_idx, R, C, label="embed.position", dtype=abi.F32)
        e_sum = pb.ew(abi.EW_ADD, Act(e_tok.view(1, 1, R, C), 1, 1, R, C), Act(e_pos.view(1, 1, R, C), 1, 1, R, C),
                      out=Act(pb.buf((1, 1, R, C), f32), 1, 1, R, C), label="embed.add", dtype=abi.F32).t.view(R, C)
        x = norm(e_sum, W["d_ln"], "embed.ln")
        caches, cross = [], []
        for i, L in enumerate(self.d_layers):
            tag = f"dec{i}"
            kc, vc = pb.buf((S, L_max, B, C), self.tdt, zero=True), pb.buf((S, L_max, B, C), self.tdt, zero=True)
            caches.append((kc, vc))
            kv = pb.buf((S, T, 2 * C), self.tdt, zero=True)
            cross.append(kv)
            qkv = lin(x, L["qkv"], 3 * C, C, tag + ".qkv")
            o = pb.decode_attention_batch(qkv, kc, vc, state, pb.buf((R, C), self.tdt), S, B, heads, d, L_max, 1.0 / math.sqrt(d),
                                          label=tag + ".self_attn")
            x1 = norm(lin(o, L["so"], C, C, tag + ".self_out", res=x, out_f32=True), L["sln"], tag + ".self_ln")
            cq = lin(x1, L["cq"], C, C, tag + ".cross_q")
            o2 = pb.buf((R, C), self.tdt)
            pb.attention(cq, kv, kv, o2, S, heads, B, T, d, (B * C, C, d), (T * 2 * C, 2 * C, d), (T * 2 * C, 2 * C, d), (B * C, C, d), 1.0 / math.sqrt(d),
                         v_off=C, label=tag + ".cross_attn")
            x2 = norm(lin(o2, L["co"], C, C, tag + ".cross_out", res=x1, out_f32=True), L["cln"], tag + ".cross_ln")
            h = lin(x2, L["fc1"], hp["d_mlp"], C, tag + ".fc1", act=abi.ACT_GELU)
            x = norm(lin(h, L["fc2"], C, hp["d_mlp"], tag + ".fc2", res=x2, out_f32=True), L["oln"], tag + ".out_ln")
        t = norm(lin(x, W["h_t"], C, C, "head.transform", act=abi.ACT_GELU, out_f32=True), W["h_ln"], "head.ln")
        logits = lin(t, W["h_out"], hp["vocab"], C, "head.logits", out_f32=True)
        early = gen.early_stopping if B > 1 else True           # one beam: greedy, as `beam_search`
        pb.beam_step(logits, state, tok_idx, pos_idx, len_pow, S, B, hp["vocab"], L_max, max(int(gen.max_length), 2), gen.eos_token_id,
                     ngram=int(gen.no_repeat_ngram_size), early=early, lp_positive=lp > 0.0, label="beam_step")
        plan = pb.build()
        plan.state, plan.idx, plan.logits, plan.caches, plan.cross, plan.words = state, idx, logits, caches, cross, words
        plan.beam_op = len(pb.ops) - 1
        self._batch = plan
        return plan

    def _reset_group(self, plan, s: int) -> None:
        """slot s takes the image last encoded: its cross K | V move device to device into the slot's region (same stream as the encoder), and
        its state becomes `beam_search`'s start: B identical rows of which only the first may seed candidates"""
        B, L_max, gen = self.gen.num_beams, self.max_len, self.gen
        for kv, mine in zip(plan.cross, self._encoder().cross):
            kv[s].copy_(mine)
        st = torch.zeros(plan.words, dtype=torch.int32)
        stf = st.view(torch.float32)
        start = int(gen.decoder_start_token_id)
        st[abi.BEAM_UNSAT] = 1
        stf[abi.BEAM_RSCORE:abi.BEAM_RSCORE + abi.BEAM_MAX] = -1e9
        stf[abi.BEAM_RSCORE] = 0.0
        stf[abi.BEAM_FSCORE:abi.BEAM_FSCORE + abi.BEAM_MAX] = -1e9
        st[abi.BEAM_FLEN:abi.BEAM_FLEN + abi.BEAM_MAX] = 1
        run, fin = abi.beam_running(B, L_max), abi.beam_fin(B, L_max)
        st[run:run + B * L_max:L_max] = start
        st[fin:fin + B * L_max:L_max] = start
        plan.state[s].copy_(st)
        plan.idx[0, s * B:(s + 1) * B] = start
        plan.idx[1, s * B:(s + 1) * B] = 0

    def generate_many(self, images, check_every: int = 4) -> list:
        """uint8 RGB arrays [H, W, 3] -> one token list per image (start token included, as `generate`), in input order.  The slots are kept
        full from the list: a crop is encoded into a free slot, the step graph is replayed `check_every` times, the head of the state block
        comes down, finished groups hand over their hypothesis and the slots refill.  An image that cannot be prepared, or whose search
        failed on the device (a logits row without a finite value), leaves a ModelError in its place and does not disturb the others.  With
        slots == 1 the images go one by one through `encode` + `generate`."""
        with self._lock:
            return self._generate_many(list(images), max(1, int(check_every)))

    def _generate_many(self, images, check_every):
        n = len(images)
        results: list = [None] * n
        if self.slots == 1 or self.gen.max_length <= 1:
            for i, img in enumerate(images):
                try:
                    self.encode(img)
                    results[i] = self.generate()
                except Exception as e:
                    results[i] = e if isinstance(e, ModelError) else ModelError(f"manga-ocr: image {i}: {e}")
            return results
        plan, S, L_max = self._stepper_batch(), self.slots, self.max_len
        head = abi.BEAM_OUT + L_max
        owner: List[Optional[int]] = [None] * S
        plan.state[:, abi.BEAM_DONE] = 1
        nxt = 0
        while True:
            for s in range(S):
                while owner[s] is None and nxt < n:
                    i, nxt = nxt, nxt + 1
                    try:
                        if isinstance(images[i], Exception):
                            raise images[i]
                        self.encode(images[i])
                        self._reset_group(plan, s)
                        owner[s] = i
                    except Exception as e:
                        results[i] = e if isinstance(e, ModelError) else ModelError(f"manga-ocr: image {i} could not be prepared: {e}")
            if all(o is None for o in owner):
                return results
            for _ in range(check_every):
                plan.run(graph=self._graph)
            st = plan.state[:, :head].cpu()
            for s in range(S):
                i = owner[s]
                if i is None or int(st[s, abi.BEAM_DONE]) == 0:
                    continue
                owner[s] = None
                n_out = int(st[s, abi.BEAM_OUT_LEN])
                if int(st[s, abi.BEAM_DONE]) == 1 and 1 <= n_out <= L_max:
                    results[i] = [int(t) for t in st[s, abi.BEAM_OUT:abi.BEAM_OUT + n_out]]
                else:
                    results[i] = ModelError(f"manga-ocr: the search of image {i} failed on the device (no finite logit, or a damaged state)")

    def recognise_many(self, pil_images) -> list:
        """PIL images -> texts, as `__call__` on each, read together through `generate_many`; an image that could not be read holds its
        ModelError instead of a string"""
        rgbs = []
        for img in pil_images:
            try:
                rgbs.append(np.asarray(img.convert("L").convert("RGB")))
            except Exception as e:
                rgbs.append(ModelError(f"manga-ocr: unreadable image: {e}"))
        ids = self.generate_many(rgbs)
        return [r if isinstance(r, Exception) else post_process(tokens_to_text(r, self.vocab)) for r in ids]

    def close(self):
        for p in [self._enc, self._step, self._batch, *self._pre.values()]:
            if p is not None:
                p.close()
        self._enc = self._step = self._batch = None
        self._pre.clear()
