"""PaddleOCR-VL on the HIP path: the (processor, model) pair behind `ModelManager.get_paddle_ocr_vl()` (reference core/ml/model_manager.py:927-980,
driven by core/image/ocr_detection.py:886-962 as `model.generate(**inputs, max_new_tokens=1024)`), after transformers'
`PaddleOCRVLForConditionalGeneration`: a SigLIP-like vision tower with a 2-D rotary turn, a 2 x 2 merging projector and a grouped-query text
decoder with multimodal rotary positions.

    PaddleOcrVlHip(state_dict, hp).generate(input_ids=, pixel_values=, image_grid_thw=, max_new_tokens=) -> int64 [1, T + n]
    PaddleOcrVlHip(state_dict, hp, slots=B).generate_many([dict(input_ids=, pixel_values=, image_grid_thw=), ...]) -> [int64 [1, T + n] | ModelError]

  * every size comes from the checkpoint's `config.json` / `generation_config.json` (`read_checkpoint`); what this build does not serve raises
    ModelError by name: a rope type other than "default", sliding-window layers, sampling, beams, a repetition penalty, video, several images;
    `generate` itself stays batch 1;
  * rotary turns without a new kernel: the wheel turns the pairs (i, i + d/2) (`rotate_half`), MTX_EW_QK_ROPE turns interleaved pairs, so the
    output rows of every q_proj / k_proj (and their biases) are permuted per head at load so that pair (i, i + d/2) lands on (2i, 2i + 1) — the
    same permutation on q and k leaves q . k unchanged, v and the output projection never see it.  The cos | sin rows are built on the host:
    from (row, col) for the vision tower, from the 3-D position ids with the `mrope_section` selection for the text decoder;
  * vision plan per (gh, gw), eager: patch rows (K zero-padded 588 -> 592) through the patch GEMM with the bias and the bilinearly resampled
    position table in its epilogue, pre-LN blocks (rotary at head width 72, full attention), post LayerNorm, the projector's LayerNorm, the
    2 x 2 merge as ONE row gather with a host-built index, Linear + erf-GELU + Linear into the fp32 image rows;
  * prefill plan per (T, image span), eager: embedding gather, the image rows copied over the placeholder rows, per layer RMSNorm -> fused
    q | k | v GEMM -> rotary -> MTX_OP_CAUSAL_ATTN (appends to the cache) -> o_proj + residual -> RMSNorm -> gate | up GEMM -> SwiGLU -> down +
    residual; final RMSNorm and the tied head on the LAST row only, fp32 logits, MTX_OP_GREEDY with advance = T;
  * ONE step plan, captured once and replayed per token: the same layer on one row (`linear_route`: skinny-row kernel or tile GEMM per shape),
    MTX_OP_CAUSAL_ATTN with rows = 1, MTX_OP_GREEDY with advance = 1.  Token, cache length and the rotary row all come from the 16-byte device
    state {pos, n_out, done, token}: the host replays `check_every` steps, then downloads the state and stops at `done`;
  * `slots = B` (2 .. 8): a page's crops decode together.  Each slot has its own key / value caches, its lane of the int32 [5][8] state
    block (pos | n_out | done | token | rope_row, include/mtx_hip.h) and its row of `out`; ONE batched step plan on B rows, captured once:
    token and rotary row gathered over token[0 .. B) and rope_row[0 .. B), the same layers with every linear on B rows (the skinny-row
    kernel reads the weights once for all of them), MTX_OP_CAUSAL_STEP_BATCH, the head on B rows, MTX_OP_GREEDY_BATCH.  Finished and empty
    slots ride along in the linears (rows are independent); attention and the pick skip them.  Vision and prefill stay per sequence on the
    plans and the staging set above (the plan caches stay as bounded as they are); device copies then move cache rows [0, T) and the state
    into the slot.  `generate_many` keeps the slots full from its list ("in-flight batching") and returns, item by item, exactly the tokens
    `generate` returns: every op of the step is per row, and the two batched ops are bit-identical per slot to the single ones.
    Memory per slot: t_layers * 2 * (max_prompt + max_new_tokens) * t_kv * 128 * 2 bytes of cache + 4 * vocab of logits + 4 * max_new_tokens
    of output + (heads * 4 rounded up to 256) + heads * ceil(max_len / 64) * 528 bytes of attention workspace — at the wheel's default sizes
    (18 layers, 16 / 2 heads, vocabulary 103 424) and the default 1 344 + 1 024 positions 43.6 MB + 0.4 MB + 0.3 MB = 44.4 MB per slot;
  * `packed_prefill=True` (needs slots > 1; off by default): what feeds the slots is ONE packed vision pass and ONE packed prompt pass for
    all the free slots at once instead of a vision and a prefill plan per crop.  The plans have a fixed shape — a patch capacity, a row
    capacity — and run a packed batch of variable-length sequences whose boundaries (an int32 [9] offset table) and whose per-grid tables
    (resampled position rows, 2-D rotary rows, the 2 x 2 merge gather indices; token ids, rotary rows, the source row of every stream row)
    are per-launch DATA the host writes for each pack, so one captured plan serves every combination of crop sizes: MTX_OP_SEG_ATTN in the
    tower, MTX_OP_CAUSAL_PREFILL_SLOTS (table index = slot, straight into the slot caches) in the decoder, every other op the existing one
    on more rows.  The fp32 stream is one row gather over [token embeddings | image rows].  Each segment's last row is gathered, the final
    norm, the head and MTX_OP_GREEDY_BATCH run on `slots` rows against a STAGING state block in which only the slots being filled have
    done = 0; the filled lanes are then copied into the slot state, so a slot that is decoding is never touched.  A crop's first token,
    state lane and cache rows do not depend on its companions, its slot, its place in the pack or the rung: row-wise kernels and the two
    segment kernels give that by construction, and the linears are pinned to a route that does not depend on M (`PACKED_GEMM_FLAGS`:
    16-bit outputs on whole 256-tiles without the K-slice tail wherever the shape admits that kernel, fp32 outputs on the 128-tile family).
    Capacities: a ladder of four rungs per plan, a factor of four apart, the top one serving `slots` prompts of `max_prompt`; a rung is
    built on first use and captured.  The packed plans reuse one set of activation buffers for all layers.  Memory per rung at the wheel's
    default widths, f16: 37.7 KB per patch of capacity for the vision plan, 46.6 KB per row for the text plan — with slots = 8 and the
    default max_prompt the rungs are 672 / 2 688 / 10 752 / 43 008 patches = 25 / 101 / 406 MB / 1.6 GB and 168 / 672 / 2 688 / 10 752 rows
    = 8 / 31 / 125 / 501 MB — plus, once, the fp32 [token embeddings | image rows] buffer (2 * slots * max_prompt rows of t_dim: 88 MB) and a
    staging row of logits and of output per slot;
  * storage: f16 by default, bf16 selectable — weights and the linears' operands in that type, the residual stream and every norm input fp32.

PARITY UNPINNED (nothing on the build machine can pin them; DESIGN.md's oracle table says the same):
  * pre-processing: the pair carries the wheel's own processor, with the PIL image processor where torchvision is absent — PIL's bicubic
    resize against torchvision's;
  * the hub checkpoint's key layout (the wheel's own renaming table and what its `save_pretrained` writes are both accepted; no hub file was
    seen) and its `generation_config.json`;
  * the 1.6 repository's actual sizes (the wheel's defaults were used to size the work)."""
import json
import math
import threading
from pathlib import Path
from typing import Callable, Dict, List, Optional

import torch

from ...hip import abi
from ...hip.lib import get_library
from ...hip.plan import Act, PlanBuilder, PlanCache
from ...utils.exceptions import ModelError
from . import packing, vit_common

HEAD_DIM = 128                      # the text decoder's head width MTX_OP_CAUSAL_ATTN is built for
WHAT = "PaddleOCR-VL"
# the linears of the packed plans: which kernel family runs, and how, must not depend on M (a crop's rows may not depend on its companions).
# With these flags a 16-bit-output linear takes the 256-tile kernel whenever its shape admits it (K % 64 == 0, 16-byte rows — nothing of M)
# and never the K-slice tail; fp32-output linears take the 128-tile family whatever M is (csrc/gemm.hip, gemm_route)
PACKED_GEMM_FLAGS = abi.GEMM_FORCE_TILE256 | abi.GEMM_NO_SPLIT
PACKED_RUNGS = 4                    # capacities per packed plan, a factor of PACKED_RUNG_RATIO apart
PACKED_RUNG_RATIO = 4


def packed_ladder(top: int) -> List[int]:
    """the capacities of a packed plan, ascending, multiples of 8, the last one `top`"""
    top = (int(top) + 7) // 8 * 8
    rungs = sorted({max(8, (top // PACKED_RUNG_RATIO ** k + 7) // 8 * 8) for k in range(PACKED_RUNGS)})
    return rungs


# ---- checkpoint ---------------------------------------------------------------------------------------------------------------------------------
def hparams_from_config(config: dict, generation: Optional[dict] = None) -> dict:
    """every size the graphs need, from `config.json` (+ `generation_config.json`); ModelError names what is not served"""
    vis, txt = config.get("vision_config"), config.get("text_config")
    if not isinstance(vis, dict) or not isinstance(txt, dict):
        raise ModelError(f"{WHAT}: config.json must hold a `vision_config` and a `text_config` section")
    rope = txt.get("rope_parameters") or txt.get("rope_scaling") or {}
    if rope.get("rope_type", rope.get("type", "default")) != "default":
        raise ModelError(f"{WHAT}: rope_type {rope.get('rope_type', rope.get('type'))!r} is not built (only 'default')")
    if any(t != "full_attention" for t in (txt.get("layer_types") or [])) or txt.get("use_sliding_window"):
        raise ModelError(f"{WHAT}: sliding-window layers are not built")
    gen = dict(generation or {})
    if gen.get("do_sample"):
        raise ModelError(f"{WHAT}: sampling (do_sample) is not built; decoding is greedy")
    if int(gen.get("num_beams") or 1) > 1:
        raise ModelError(f"{WHAT}: beam search (num_beams > 1) is not built; decoding is greedy")
    if float(gen.get("repetition_penalty") or 1.0) != 1.0:
        raise ModelError(f"{WHAT}: a repetition penalty is not built")
    hp = dict(v_dim=int(vis["hidden_size"]), v_layers=int(vis["num_hidden_layers"]), v_heads=int(vis["num_attention_heads"]),
              v_mlp=int(vis["intermediate_size"]), patch=int(vis.get("patch_size", 14)), image=int(vis.get("image_size", 384)),
              v_eps=float(vis.get("layer_norm_eps", 1e-6)), v_act=vis.get("hidden_act", "gelu_pytorch_tanh"), merge=int(vis.get("spatial_merge_size", 2)),
              channels=int(vis.get("num_channels", 3)),
              t_dim=int(txt["hidden_size"]), t_layers=int(txt["num_hidden_layers"]), t_heads=int(txt["num_attention_heads"]),
              t_kv=int(txt.get("num_key_value_heads") or txt["num_attention_heads"]), t_mlp=int(txt["intermediate_size"]), vocab=int(txt["vocab_size"]),
              t_eps=float(txt.get("rms_norm_eps", 1e-5)), t_act=txt.get("hidden_act", "silu"), theta=float(rope.get("rope_theta", txt.get("rope_theta", 10000.0))),
              image_token=int(config["image_token_id"]), tied=bool(config.get("tie_word_embeddings", txt.get("tie_word_embeddings", True))))
    hp["t_hd"] = int(txt.get("head_dim") or hp["t_dim"] // hp["t_heads"])
    section = rope.get("mrope_section")
    if not section or len(section) != 3 or sum(section) != hp["t_hd"] // 2:
        raise ModelError(f"{WHAT}: rope_parameters.mrope_section must hold three sizes that add up to head_dim / 2")
    hp["mrope"] = [int(s) for s in section]
    if hp["t_hd"] != HEAD_DIM or hp["t_heads"] % hp["t_kv"]:
        raise ModelError(f"{WHAT}: text head width {hp['t_hd']} / {hp['t_heads']} query heads over {hp['t_kv']} key-value heads is not built "
                         f"(head width {HEAD_DIM}, query heads a multiple of the key-value heads)")
    if txt.get("use_bias"):
        raise ModelError(f"{WHAT}: a text decoder with biased linears is not built")
    if hp["v_dim"] % hp["v_heads"] or (hp["v_dim"] // hp["v_heads"]) % 8 or hp["v_dim"] // hp["v_heads"] > 128 or (hp["v_dim"] // hp["v_heads"]) % 4:
        raise ModelError(f"{WHAT}: vision head width {hp['v_dim'] / hp['v_heads']:g} is not built (a multiple of 8 up to 128)")
    if hp["v_act"] not in ("gelu_pytorch_tanh", "gelu") or hp["t_act"] != "silu":
        raise ModelError(f"{WHAT}: activation {hp['v_act']!r} / {hp['t_act']!r} is not built")
    if hp["channels"] != 3 or hp["merge"] != 2 or hp["image"] < hp["patch"]:          # (the wheel's 384 / 14 leaves a remainder: the learned grid is 27 x 27)
        raise ModelError(f"{WHAT}: the vision tower must take 3 channels and merge 2 x 2")
    eos = gen.get("eos_token_id", txt.get("eos_token_id", config.get("eos_token_id")))
    if eos is None:
        raise ModelError(f"{WHAT}: neither generation_config.json nor config.json gives eos_token_id")
    hp["eos"] = [int(e) for e in (eos if isinstance(eos, (list, tuple)) else [eos])]
    if not 1 <= len(hp["eos"]) <= 4:
        raise ModelError(f"{WHAT}: {len(hp['eos'])} end-of-sequence tokens are not built (1 .. 4)")
    return hp


V, P, L = "model.visual.vision_model.", "model.projector.", "model.language_model."


def expected_keys(hp: dict) -> List[str]:
    keys = []

    def wb(prefix):
        keys.extend([prefix + ".weight", prefix + ".bias"])
    wb(V + "embeddings.patch_embedding")
    keys.append(V + "embeddings.position_embedding.weight")
    for i in range(hp["v_layers"]):
        for n in ("layer_norm1", "layer_norm2", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2"):
            wb(f"{V}encoder.layers.{i}.{n}")
    wb(V + "post_layernorm")
    for n in ("pre_norm", "linear_1", "linear_2"):
        wb(P + n)
    keys.append(L + "embed_tokens.weight")
    for i in range(hp["t_layers"]):
        for n in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj",
                  "input_layernorm", "post_attention_layernorm"):
            keys.append(f"{L}layers.{i}.{n}.weight")
    keys.extend([L + "norm.weight", "lm_head.weight"])
    return keys


# tensors a hub checkpoint carries that the wheel itself drops on load (`_keys_to_ignore_on_load_unexpected`)
IGNORED_KEYS = ("packing_position_embedding", "vision_model.head")


def _rename_hub(key: str) -> str:
    """the hub file's names -> `state_dict()`'s, as the wheel's conversion mapping for "paddleocr_vl" renames them on load (and back in
    `save_pretrained`): mlp_AR.* -> model.projector.*, visual.* -> model.visual.*, model.<rest> -> model.language_model.<rest>"""
    if key.startswith("mlp_AR"):
        return "model.projector" + key[len("mlp_AR"):]
    if key.startswith("visual"):
        return "model." + key
    if key.startswith("model") and not key.startswith(("model.visual", "model.projector", "model.language_model")):
        return "model.language_model" + key[len("model"):]
    return key


def normalise_state_dict(sd: Dict[str, torch.Tensor], hp: dict) -> Dict[str, torch.Tensor]:
    """both key layouts -> `state_dict()`'s names; a tied `lm_head.weight` that the file leaves out is filled in; every missing or unexpected
    key is a ModelError"""
    out = {_rename_hub(k): v for k, v in sd.items() if not any(skip in k for skip in IGNORED_KEYS)}
    if "lm_head.weight" not in out and hp["tied"] and L + "embed_tokens.weight" in out:
        out["lm_head.weight"] = out[L + "embed_tokens.weight"]
    want = set(expected_keys(hp))
    missing, unexpected = sorted(want - set(out)), sorted(set(out) - want)
    if missing or unexpected:
        raise ModelError(f"{WHAT} checkpoint: missing keys {missing[:6]}{' ...' if len(missing) > 6 else ''}, "
                         f"unexpected keys {unexpected[:6]}{' ...' if len(unexpected) > 6 else ''}")
    return out


def read_checkpoint(root) -> dict:
    """a staged `paddleocr-vl-1.6` directory -> dict(hp, state_dict): config.json + model.safetensors (or the shards its index names) +
    generation_config.json"""
    root = Path(root)
    if not (root / "config.json").is_file():
        raise ModelError(f"{WHAT} is not staged: {root / 'config.json'} not found")
    config = json.loads((root / "config.json").read_text())
    gen_path = root / "generation_config.json"
    hp = hparams_from_config(config, json.loads(gen_path.read_text()) if gen_path.is_file() else None)
    from safetensors.torch import load_file
    if (root / "model.safetensors").is_file():
        files = ["model.safetensors"]
    elif (root / "model.safetensors.index.json").is_file():
        files = sorted(set(json.loads((root / "model.safetensors.index.json").read_text())["weight_map"].values()))
    else:
        raise ModelError(f"{WHAT} is not staged: neither model.safetensors nor model.safetensors.index.json in {root}")
    sd = {}
    for f in files:
        if not (root / f).is_file():
            raise ModelError(f"{WHAT} is not staged: shard {root / f} not found")
        sd.update(load_file(str(root / f)))
    return dict(hp=hp, state_dict=normalise_state_dict(sd, hp))


def interleave_rows(w: torch.Tensor, heads: int, d: int) -> torch.Tensor:
    """rows (or entries) of a q / k projection [heads * d, ...] permuted per head so that the wheel's rotary pair (i, i + d/2) lands on the
    interleaved pair (2i, 2i + 1) the kernel turns"""
    idx = torch.stack([torch.arange(d // 2), torch.arange(d // 2) + d // 2], 1).reshape(-1)
    return w.reshape(heads, d, *w.shape[1:])[:, idx].reshape(w.shape)


def linear_route(rows: int, n: int, k: int) -> str:
    """which kernel a linear of the decode step runs on: "rowlin" (MTX_OP_ROWLIN) or "gemm".  One activation row against 2 - 6 MB of weights per
    linear (212 MB for the 103 424-row head at the published widths): weight streaming, as manga-ocr's step; the A/B of the whole step graph
    (tools/bench_kernels.py paddleocr; docs/experiments.md) decides per shape."""
    return "rowlin"


# ---- host-side tables ---------------------------------------------------------------------------------------------------------------------------
def vision_rope_table(gh: int, gw: int, d: int) -> torch.Tensor:
    """fp32 [gh * gw][2][d / 2] cos | sin: the first d / 4 frequencies turn with the row, the next d / 4 with the column (wheel :627-638, :845-856)"""
    q = d // 4
    inv = 1.0 / (10000.0 ** (torch.arange(0, d // 2, 2, dtype=torch.float) / (d // 2)))
    assert inv.numel() == q
    rows, cols = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
    ang = torch.cat([rows.reshape(-1, 1).float() * inv, cols.reshape(-1, 1).float() * inv], 1)          # [N, d / 2]
    return torch.stack([ang.cos(), ang.sin()], 1).contiguous()


def rope_positions(token_is_image: torch.Tensor, gh: int, gw: int, merge: int) -> torch.Tensor:
    """the 3-D position ids [3, T] of one prompt with one image (wheel get_rope_index / get_vision_position_ids): text tokens carry three
    equal indices, image tokens (start, start + row, start + col) on the merged grid, text after the image starts at the running maximum + 1"""
    T = int(token_is_image.numel())
    img = token_is_image.nonzero().reshape(-1)
    mh, mw = gh // merge, gw // merge
    if img.numel() != mh * mw or (img.numel() and int(img[-1] - img[0]) + 1 != img.numel()):
        raise ModelError(f"{WHAT}: the prompt's image placeholders ({img.numel()}) must be one run of {mh * mw} tokens")
    start = int(img[0])
    pos = torch.zeros(3, T, dtype=torch.long)
    pos[:, :start] = torch.arange(start)
    r, c = torch.meshgrid(torch.arange(mh), torch.arange(mw), indexing="ij")
    pos[0, start:start + mh * mw] = start
    pos[1, start:start + mh * mw] = start + r.reshape(-1)
    pos[2, start:start + mh * mw] = start + c.reshape(-1)
    after = start + max(mh, mw)
    n_after = T - start - mh * mw
    pos[:, start + mh * mw:] = after + torch.arange(n_after)
    return pos


def text_rope_table(pos3: torch.Tensor, section: List[int], theta: float, d: int) -> torch.Tensor:
    """fp32 [T][2][d / 2] cos | sin from 3-D ids [3, T]: frequency i takes the axis its `mrope_section` names (wheel :239-281)"""
    inv = 1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.float) / d))
    axis = torch.repeat_interleave(torch.arange(3), torch.tensor(section))                              # [d / 2]
    p = pos3.float()[axis, :].t()                                                                        # [T, d / 2]
    ang = p * inv
    return torch.stack([ang.cos(), ang.sin()], 1).contiguous()


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
class PaddleOcrVlHip:
    def __init__(self, state_dict: dict, hp: dict, device="cuda", lib=None, dtype: int = abi.F16, graph: bool = True, max_new_tokens: int = 1024,
                 max_prompt: int = 1280 + 64, check_every: int = 8, route: Optional[Callable[[int, int, int], str]] = None, slots: int = 1,
                 packed_prefill: bool = False):
        """hp: `hparams_from_config`; state_dict: `normalise_state_dict`'s names.  max_prompt: the longest prompt served (the processor's
        max_pixels bound gives at most 1 280 image tokens; the chat template adds a few tens); the cache holds max_prompt + max_new_tokens.
        slots: how many sequences `generate_many` decodes together (1 .. 8; 1 allocates nothing new), 2 * t_layers * max_len * t_kv * 128
        elements of cache per slot plus a row of logits and of output (the module docstring has the sum).
        packed_prefill: `generate_many` fills all free slots from one packed vision pass and one packed prompt pass (needs slots > 1)."""
        if dtype not in (abi.BF16, abi.F16):
            raise ModelError(f"{WHAT}: storage dtype must be f16 or bf16")
        if not 1 <= int(slots) <= abi.SLOTS_MAX:
            raise ModelError(f"{WHAT}: slots must be 1 .. {abi.SLOTS_MAX}, not {slots!r}")
        self.slots = int(slots)
        if not isinstance(packed_prefill, bool):
            raise ModelError(f"{WHAT}: packed_prefill must be a bool, not {packed_prefill!r}")
        if packed_prefill and self.slots < 2:
            raise ModelError(f"{WHAT}: packed_prefill fills decode slots and needs slots > 1")
        self.packed = packed_prefill
        self.lib = lib if lib is not None else get_library()
        self.device = torch.device(device)
        self.hp, self.dtype, self.tdt = hp, dtype, {abi.BF16: torch.bfloat16, abi.F16: torch.float16}[dtype]
        self.max_new, self.max_prompt, self.check_every = int(max_new_tokens), int(max_prompt), max(1, int(check_every))
        self.max_len = self.max_prompt + self.max_new
        self.route = route or linear_route
        self._graph = graph and not self.lib.is_simulator
        self._lock = threading.Lock()
        self._vis, self._pre = PlanCache(4), PlanCache(6)
        self._step = self._step_b = None
        self.fill_log = []                                           # (item, slot, [(item, n_out) of the other live slots]) per fill of the last generate_many
        self._pack({k: v.detach().float().cpu() for k, v in state_dict.items()})
        f32, i32 = torch.float32, torch.int32
        C, kvw = hp["t_dim"], hp["t_kv"] * HEAD_DIM
        z = lambda *s, dt=f32: torch.zeros(*s, dtype=dt, device=self.device)
        self.caches = [(z(self.max_len, kvw, dt=self.tdt), z(self.max_len, kvw, dt=self.tdt)) for _ in range(hp["t_layers"])]
        self.state = z(4, dt=i32)                                    # {pos, n_out, done, token}
        self.out = z(self.max_new, dt=i32)
        self.img_rows = z(max(self.max_prompt, 8), C)                # the projector's output, read by the prefill plans
        self.step_rope = z(self.max_len, HEAD_DIM)                   # cos | sin row of the token fed at cache position p (set per prompt)
        self.logits = z(1, hp["vocab"])
        if self.slots > 1:
            B = self.slots
            self.slot_caches = [(z(B, self.max_len, kvw, dt=self.tdt), z(B, self.max_len, kvw, dt=self.tdt)) for _ in range(hp["t_layers"])]
            self.slot_state = z(abi.SLOT_FIELDS, abi.SLOTS_MAX, dt=i32)          # pos | n_out | done | token | rope_row, one lane per slot
            self.slot_state[abi.SLOT_DONE] = 1                       # empty slots sit out
            self.slot_out = z(B, self.max_new, dt=i32)
            self.slot_logits = z(B, hp["vocab"])
            # cos | sin row of rotary position r, all three axes equal: the token fed at cache position p of a prompt sits at r = p + delta
            p = torch.arange(self.max_len)
            self.slot_rope = self._c(text_rope_table(p[None].expand(3, -1), hp["mrope"], hp["theta"], HEAD_DIM).reshape(self.max_len, HEAD_DIM), f32)
        self._pk_vis, self._pk_txt, self._grid_tables = {}, {}, {}
        self.last_rungs = None                                       # (patch capacity, row capacity) of the last packed fill
        if self.packed:
            B = self.slots
            self.pk_rows, self.pk_img = B * self.max_prompt, B * self.img_rows.shape[0]      # top capacities: text rows, merged image rows
            self.pk_vis_ladder, self.pk_txt_ladder = packed_ladder(4 * self.pk_img), packed_ladder(self.pk_rows)
            self.pk_rows = self.pk_txt_ladder[-1]
            self.pk_cat = z(self.pk_rows + self.pk_vis_ladder[-1] // 4, C)         # fp32 [token embeddings | image rows]: the stream's gather source
            self.pk_state = z(abi.SLOT_FIELDS, abi.SLOTS_MAX, dt=i32)            # the staging state block of a fill
            self.pk_state[abi.SLOT_DONE] = 1
            self.pk_out = z(B, self.max_new, dt=i32)
            self.pk_logits = z(B, hp["vocab"])

    @classmethod
    def from_directory(cls, root, **kw):
        ck = read_checkpoint(root)
        return cls(ck["state_dict"], ck["hp"], **kw)

    # ------------------------------------------------------------------------------------------
    def _c(self, t, dtype=None):
        return packing.on_device(t, self.device, dtype if dtype is not None else self.tdt)

    def _pack(self, sd):
        """every linear as the triple (W, None, bias or None) of core/ml/packing.py, LayerNorms as (gamma, beta), RMSNorms as (gamma, None)"""
        hp = self.hp
        f32 = torch.float32
        Cv, vh = hp["v_dim"], hp["v_heads"]
        vd = Cv // vh

        def ln(key):
            return packing.layer_norm(sd, key, self.device)

        def lin(*keys):
            return packing.linear(sd, *keys, device=self.device, dtype=self.tdt)

        def lin_nb(*ws):
            return (self._c(torch.cat(ws, 0)), None, None)

        W = {}
        pw = sd[V + "embeddings.patch_embedding.weight"]
        k = pw[0].numel()
        self.patch_k, self.patch_kp = k, (k + 7) // 8 * 8
        pk = torch.zeros(Cv, self.patch_kp)
        pk[:, :k] = pw.reshape(Cv, k)
        W["pe"] = (self._c(pk), None, self._c(sd[V + "embeddings.patch_embedding.bias"], f32))
        self.pos_table = sd[V + "embeddings.position_embedding.weight"]                       # fp32, host: resampled per grid
        side = int(round(self.pos_table.shape[0] ** 0.5))
        if side * side != self.pos_table.shape[0] or side != hp["image"] // hp["patch"]:
            raise ModelError(f"{WHAT}: the vision position table does not match image_size / patch_size")
        self.v_layers = []
        for i in range(hp["v_layers"]):
            p = f"{V}encoder.layers.{i}."
            a = p + "self_attn."
            qkv_w = torch.cat([interleave_rows(sd[a + "q_proj.weight"], vh, vd), interleave_rows(sd[a + "k_proj.weight"], vh, vd), sd[a + "v_proj.weight"]], 0)
            qkv_b = torch.cat([interleave_rows(sd[a + "q_proj.bias"], vh, vd), interleave_rows(sd[a + "k_proj.bias"], vh, vd), sd[a + "v_proj.bias"]], 0)
            self.v_layers.append(dict(ln1=ln(p + "layer_norm1"), ln2=ln(p + "layer_norm2"), qkv=(self._c(qkv_w), None, self._c(qkv_b, f32)),
                                      proj=lin(a + "out_proj"), fc1=lin(p + "mlp.fc1"), fc2=lin(p + "mlp.fc2")))
        W["v_ln"] = ln(V + "post_layernorm")
        W["p_ln"] = ln(P + "pre_norm")
        W["p1"], W["p2"] = lin(P + "linear_1"), lin(P + "linear_2")
        if sd[L + "embed_tokens.weight"].shape != (hp["vocab"], hp["t_dim"]) or sd["lm_head.weight"].shape != (hp["vocab"], hp["t_dim"]):
            raise ModelError(f"{WHAT}: the embedding table / head do not match vocab_size x hidden_size")
        W["tok"] = self._c(sd[L + "embed_tokens.weight"])
        W["head"] = (W["tok"] if torch.equal(sd["lm_head.weight"], sd[L + "embed_tokens.weight"]) else self._c(sd["lm_head.weight"]), None, None)
        th, tkv = hp["t_heads"], hp["t_kv"]
        self.t_layers = []
        for i in range(hp["t_layers"]):
            p = f"{L}layers.{i}."
            a = p + "self_attn."
            self.t_layers.append(dict(
                n1=(self._c(sd[p + "input_layernorm.weight"], f32), None), n2=(self._c(sd[p + "post_attention_layernorm.weight"], f32), None),
                qkv=lin_nb(interleave_rows(sd[a + "q_proj.weight"], th, HEAD_DIM), interleave_rows(sd[a + "k_proj.weight"], tkv, HEAD_DIM), sd[a + "v_proj.weight"]),
                o=lin_nb(sd[a + "o_proj.weight"]), gu=lin_nb(sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]), down=lin_nb(sd[p + "mlp.down_proj.weight"])))
        W["t_norm"] = (self._c(sd[L + "norm.weight"], f32), None)
        self.W = W

    # ---- vision ----------------------------------------------------------------------------------
    def _vision(self, gh: int, gw: int):
        if (gh, gw) in self._vis:
            return self._vis[(gh, gw)]
        from transformers.vision_utils import get_vision_interpolation_indices_and_weights
        hp, W = self.hp, self.W
        if gh % 2 or gw % 2 or gh * gw // 4 > self.img_rows.shape[0]:
            raise ModelError(f"{WHAT}: an image grid of {gh} x {gw} patches is not served (even sides, at most {self.img_rows.shape[0]} merged tokens)")
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        N, C, heads, Ct = gh * gw, hp["v_dim"], hp["v_heads"], hp["t_dim"]
        d = C // heads
        side = hp["image"] // hp["patch"]
        idx, wts = get_vision_interpolation_indices_and_weights(torch.tensor([[1, gh, gw]]), num_grid_per_side=side, mode="bilinear", align_corners=True,
                                                                spatial_merge_size=1)
        pos = pb.const((self.pos_table[idx] * wts[:, :, None].float()).sum(1), torch.float32)               # [N, C]
        rope = pb.const(vision_rope_table(gh, gw, d))
        patches = pb.buf((N, self.patch_kp), self.tdt, zero=True)
        layer_norm, linear, close_branch = vit_common.trunk_helpers(pb, hp["v_eps"], self.tdt, self.dtype, stream32=True)
        act = abi.ACT_GELU_TANH if hp["v_act"] == "gelu_pytorch_tanh" else abi.ACT_GELU
        x = close_branch(patches, W["pe"], N, C, self.patch_kp, pos, "patch_embed")
        for i, Lr in enumerate(self.v_layers):
            tag = f"vis{i}"
            qkv = linear(layer_norm(x, N, C, Lr["ln1"], tag + ".ln1"), Lr["qkv"], N, 3 * C, C, tag + ".qkv")
            pb.qk_rope(Act(qkv.view(1, 1, N, 3 * C), 1, 1, N, 2 * C), rope, d, label=tag + ".rope")
            o = pb.buf((N, C), self.tdt)
            st = (N * 3 * C, 3 * C, d)
            pb.attention(qkv, qkv, qkv, o, 1, heads, N, N, d, st, st, st, (N * C, C, d), 1.0 / math.sqrt(d), k_off=C, v_off=2 * C, label=tag + ".attn")
            x1 = close_branch(o, Lr["proj"], N, C, C, x, tag + ".proj")
            h = linear(layer_norm(x1, N, C, Lr["ln2"], tag + ".ln2"), Lr["fc1"], N, hp["v_mlp"], C, tag + ".fc1", act=act)
            x = close_branch(h, Lr["fc2"], N, C, hp["v_mlp"], x1, tag + ".fc2")
        y32 = pb.norm(x, pb.buf((N, C), torch.float32), N, C, gamma=W["v_ln"][0], beta=W["v_ln"][1], eps=hp["v_eps"], dtype=abi.F32, out_dtype=abi.F32, label="vis.post_ln")
        y = pb.norm(y32, pb.buf((N, C), self.tdt), N, C, gamma=W["p_ln"][0], beta=W["p_ln"][1], eps=1e-5, dtype=abi.F32, out_dtype=self.dtype, label="proj.pre_norm")
        # 2 x 2 merge: merged row (hb, wb) = the four source rows (2 hb + m1, 2 wb + m2) side by side, so [N / 4][4 C] is a plain view
        hb, wb, m1, m2 = torch.meshgrid(torch.arange(gh // 2), torch.arange(gw // 2), torch.arange(2), torch.arange(2), indexing="ij")
        src = pb.const(((hb * 2 + m1) * gw + wb * 2 + m2).reshape(-1).to(torch.int32))
        merged = pb.row_gather(y, pb.buf((N, C), self.tdt), src, N, C, label="proj.merge")
        M = N // 4
        h1 = linear(merged, W["p1"], M, 4 * C, 4 * C, "proj.linear_1", act=abi.ACT_GELU)
        linear(h1, W["p2"], M, Ct, 4 * C, "proj.linear_2", out=self.img_rows, out_f32=True)
        plan = pb.build()
        plan.patches, plan.tokens = patches, M
        self._vis[(gh, gw)] = plan
        return plan

    # ---- the text decoder ------------------------------------------------------------------------
    def _layers(self, pb, x, rows, rope, lin, close, slots: int = 0, packed=None):
        """the decoder layers on `rows` rows of the fp32 stream x; -> the stream after the last layer.  slots = B > 0: the rows are the
        steps of B independent sequences on the slot caches (MTX_OP_CAUSAL_STEP_BATCH).  packed = (seg, pool): the rows are up to SLOTS_MAX
        whole prompts packed row-wise, prompt s = rows [seg[s], seg[s + 1]) of the device table, into the EMPTY slot cache s
        (MTX_OP_CAUSAL_PREFILL_SLOTS); every layer then works in the same activation buffers, kept in the dict `pool`"""
        hp = self.hp
        C, heads, kv, I = hp["t_dim"], hp["t_heads"], hp["t_kv"], hp["t_mlp"]
        qw = (heads + 2 * kv) * HEAD_DIM
        seg, pool = packed if packed is not None else (None, None)

        def buf(key, shape, dt):
            if pool is None:
                return pb.buf(shape, dt)
            if key not in pool:
                pool[key] = pb.buf(shape, dt)
            return pool[key]
        ws = None
        if slots:
            ws = pb.buf((slots * abi.causal_ws_bytes(heads, self.max_len),), torch.uint8, zero=True)
        elif rows == 1:
            ws = pb.buf((abi.causal_ws_bytes(heads, self.max_len),), torch.uint8, zero=True)
        for i, Lr in enumerate(self.t_layers):
            tag = f"dec{i}"
            kc, vc = self.caches[i]
            a = pb.norm(x, buf("norm1", (rows, C), self.tdt), rows, C, gamma=Lr["n1"][0], eps=hp["t_eps"], kind=1, dtype=abi.F32, out_dtype=self.dtype, label=tag + ".norm1")
            qkv = lin(a, Lr["qkv"], qw, C, tag + ".qkv")
            pb.qk_rope(Act(qkv.view(1, 1, rows, qw), 1, 1, rows, (heads + kv) * HEAD_DIM), rope, HEAD_DIM, label=tag + ".rope")
            if seg is not None:
                skc, svc = self.slot_caches[i]
                o = pb.causal_prefill_slots(qkv, skc, svc, seg, buf("attn", (rows, heads * HEAD_DIM), self.tdt), rows, heads, kv, HEAD_DIM, self.max_len,
                                            HEAD_DIM ** -0.5, label=tag + ".attn")
            elif slots:
                skc, svc = self.slot_caches[i]
                o = pb.causal_step_batch(qkv, skc, svc, self.slot_state, pb.buf((rows, heads * HEAD_DIM), self.tdt), slots, heads, kv, HEAD_DIM, self.max_len,
                                         HEAD_DIM ** -0.5, workspace=ws, label=tag + ".attn")
            else:
                o = pb.causal_attention(qkv, kc, vc, self.state[0:1], pb.buf((rows, heads * HEAD_DIM), self.tdt), rows, heads, kv, HEAD_DIM, self.max_len,
                                        HEAD_DIM ** -0.5, workspace=ws, label=tag + ".attn")
            x1 = close(o, Lr["o"], C, heads * HEAD_DIM, x, tag + ".o_proj")
            b = pb.norm(x1, buf("norm2", (rows, C), self.tdt), rows, C, gamma=Lr["n2"][0], eps=hp["t_eps"], kind=1, dtype=abi.F32, out_dtype=self.dtype, label=tag + ".norm2")
            gu = lin(b, Lr["gu"], 2 * I, C, tag + ".gate_up")
            g4 = gu.view(1, 1, rows, 2 * I)
            hmid = pb.ew(abi.EW_SWIGLU, Act(g4, 1, 1, rows, I, 0), b=Act(g4, 1, 1, rows, I, I), out=Act(buf("swiglu", (1, 1, rows, I), self.tdt), 1, 1, rows, I),
                         label=tag + ".swiglu").t.view(rows, I)
            x = close(hmid, Lr["down"], C, I, x1, tag + ".down")
        return x

    def _head(self, pb, x_last, advance, slots: int = 0, staging: bool = False):
        """final norm, the head and the pick on the last row — or, with slots = B > 0, on the B rows of the batched step; `staging`: on the B last
        rows of a packed fill, against the staging logits, state block and output rows"""
        hp = self.hp
        C = hp["t_dim"]
        rows, logits = (slots, self.slot_logits) if slots else (1, self.logits)
        state, out = (self.slot_state, self.slot_out) if slots else (self.state, self.out)
        if staging:
            logits, state, out = self.pk_logits, self.pk_state, self.pk_out
        a = pb.norm(x_last, pb.buf((rows, C), self.tdt), rows, C, gamma=self.W["t_norm"][0], eps=hp["t_eps"], kind=1, dtype=abi.F32, out_dtype=self.dtype, label="final_norm")
        if self.route(1, hp["vocab"], C) == "rowlin":
            pb.row_linear(a, self.W["head"][0], rows, hp["vocab"], C, out=logits, out_f32=True, label="head")
        else:
            pb.gemm(a, self.W["head"][0], rows, hp["vocab"], C, out=logits, out_f32=True, label="head")
        if slots:
            pb.greedy_pick_batch(logits, state, out, slots, hp["vocab"], self.max_new, eos=hp["eos"], advance=advance)
        else:
            pb.greedy_pick(logits, state, out, hp["vocab"], self.max_new, eos=hp["eos"], advance=advance)

    def _prefill(self, T: int, start: int, n_img: int):
        key = (T, start, n_img)
        if key in self._pre:
            return self._pre[key]
        hp = self.hp
        C = hp["t_dim"]
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        ids = pb.buf((T,), torch.int32, zero=True)
        rope = pb.buf((T, 2, HEAD_DIM // 2), torch.float32, zero=True)
        e16 = pb.row_gather(self.W["tok"], pb.buf((T, C), self.tdt), ids, T, C, label="embed")
        x = pb.cvt_f32(Act(e16.view(1, 1, T, C), 1, 1, T, C), self.dtype, label="embed.f32").t.view(T, C)
        if n_img:
            pb.ew(abi.EW_COPY, Act(self.img_rows[:n_img].view(1, 1, n_img, C), 1, 1, n_img, C), out=Act(x[start:start + n_img].view(1, 1, n_img, C), 1, 1, n_img, C),
                  label="embed.image_rows", dtype=abi.F32)
        _, linear, close_branch = vit_common.trunk_helpers(pb, hp["t_eps"], self.tdt, self.dtype, stream32=True)
        x = self._layers(pb, x, T, rope, lambda a, wb, n, k, label: linear(a, wb, T, n, k, label),
                         lambda a, wb, n, k, res, label: close_branch(a, wb, T, n, k, res, label))
        self._head(pb, x[T - 1:T], advance=T)
        plan = pb.build()
        plan.ids, plan.rope = ids, rope
        self._pre[key] = plan
        return plan

    def _stepper(self):
        if self._step is not None:
            return self._step
        hp = self.hp
        C = hp["t_dim"]
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        e16 = pb.row_gather(self.W["tok"], pb.buf((1, C), self.tdt), self.state[3:4], 1, C, label="embed")
        x = pb.cvt_f32(Act(e16.view(1, 1, 1, C), 1, 1, 1, C), self.dtype, label="embed.f32").t.view(1, C)
        rope = pb.row_gather(self.step_rope, pb.buf((1, HEAD_DIM), torch.float32), self.state[0:1], 1, HEAD_DIM, label="rope.row", dtype=abi.F32)
        lin, close = self._step_linears(pb, 1)
        x = self._layers(pb, x, 1, rope, lin, close)
        self._head(pb, x, advance=1)
        self._step = pb.build()
        return self._step

    def _step_linears(self, pb, rows):
        """(lin, close) of a step plan on `rows` rows; the kernel per shape is the single step's (`route(1, n, k)`), whatever `rows`"""
        def lin(a, wb, n, k, label):
            if self.route(1, n, k) == "rowlin":
                return pb.row_linear(a, wb[0], rows, n, k, label=label)
            return pb.gemm(a, wb[0], rows, n, k, label=label)

        def close(a, wb, n, k, res, label):
            """stream <- res + a @ W^T in fp32 (the skinny-row kernel takes no fp32 residual: its fp32 output and one fp32 add)"""
            if self.route(1, n, k) != "rowlin":
                return pb.gemm(a, wb[0], rows, n, k, res=res, res_f32=True, out_f32=True, label=label)
            y = pb.row_linear(a, wb[0], rows, n, k, out_f32=True, label=label)
            return pb.ew(abi.EW_ADD, Act(y.view(1, 1, rows, n), 1, 1, rows, n), Act(res.view(1, 1, rows, n), 1, 1, rows, n),
                         out=Act(pb.buf((1, 1, rows, n), torch.float32), 1, 1, rows, n), label=label + ".add", dtype=abi.F32).t.view(rows, n)
        return lin, close

    def _stepper_batch(self):
        """ONE plan on B = slots rows, captured once: row s is slot s's step, fed from its lane of the state block"""
        if self._step_b is not None:
            return self._step_b
        hp, B = self.hp, self.slots
        C = hp["t_dim"]
        st = self.slot_state
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        e16 = pb.row_gather(self.W["tok"], pb.buf((B, C), self.tdt), st[abi.SLOT_TOKEN], B, C, label="embed")
        x = pb.cvt_f32(Act(e16.view(1, 1, B, C), 1, 1, B, C), self.dtype, label="embed.f32").t.view(B, C)
        rope = pb.row_gather(self.slot_rope, pb.buf((B, HEAD_DIM), torch.float32), st[abi.SLOT_ROPE], B, HEAD_DIM, label="rope.row", dtype=abi.F32)
        lin, close = self._step_linears(pb, B)
        x = self._layers(pb, x, B, rope, lin, close, slots=B)
        self._head(pb, x, advance=1, slots=B)
        self._step_b = pb.build()
        return self._step_b

    # ---- the packed fill (packed_prefill=True) ----------------------------------------------------
    def _grid(self, gh: int, gw: int):
        """host tables of one patch grid, kept for the grids seen lately: resampled position rows fp32 [N, C], 2-D rotary rows fp32
        [N, 2, d / 2], the 2 x 2 merge gather indices int32 [N] (relative to the image's first patch)"""
        key = (gh, gw)
        if key in self._grid_tables:
            self._grid_tables[key] = self._grid_tables.pop(key)      # most recently used last
            return self._grid_tables[key]
        from transformers.vision_utils import get_vision_interpolation_indices_and_weights
        hp = self.hp
        side = hp["image"] // hp["patch"]
        idx, wts = get_vision_interpolation_indices_and_weights(torch.tensor([[1, gh, gw]]), num_grid_per_side=side, mode="bilinear", align_corners=True,
                                                                spatial_merge_size=1)
        pos = (self.pos_table[idx] * wts[:, :, None].float()).sum(1).to(torch.float32).contiguous()
        rope = vision_rope_table(gh, gw, hp["v_dim"] // hp["v_heads"])
        hb, wb, m1, m2 = torch.meshgrid(torch.arange(gh // 2), torch.arange(gw // 2), torch.arange(2), torch.arange(2), indexing="ij")
        src = ((hb * 2 + m1) * gw + wb * 2 + m2).reshape(-1).to(torch.int32)
        self._grid_tables[key] = (pos, rope, src)
        while len(self._grid_tables) > 16:
            self._grid_tables.pop(next(iter(self._grid_tables)))
        return self._grid_tables[key]

    def _packed_vision(self, cap: int):
        """the vision tower, the post norms, the 2 x 2 merge and the projector on `cap` patch rows that hold up to SEGS_MAX images packed row-wise;
        the merged rows of all images land, packed in the same order, in the image half of `pk_cat`.  Every per-grid table is per-launch data"""
        if cap in self._pk_vis:
            return self._pk_vis[cap]
        hp, W = self.hp, self.W
        f32 = torch.float32
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        N, C, heads, Ct = cap, hp["v_dim"], hp["v_heads"], hp["t_dim"]
        d, M = C // heads, cap // 4
        patches = pb.buf((N, self.patch_kp), self.tdt, zero=True)
        pos = pb.buf((N, C), f32, zero=True)
        rope = pb.buf((N, 2, d // 2), f32, zero=True)
        src = pb.buf((N,), torch.int32, zero=True)
        seg = pb.buf((abi.SEGS_MAX + 1,), torch.int32, zero=True)
        act = abi.ACT_GELU_TANH if hp["v_act"] == "gelu_pytorch_tanh" else abi.ACT_GELU
        ln16, qkv, o, h = pb.buf((N, C), self.tdt), pb.buf((N, 3 * C), self.tdt), pb.buf((N, C), self.tdt), pb.buf((N, hp["v_mlp"]), self.tdt)
        xa, xb = pb.buf((N, C), f32), pb.buf((N, C), f32)

        def norm16(x, wb, label):
            return pb.norm(x, ln16, N, C, gamma=wb[0], beta=wb[1], eps=hp["v_eps"], dtype=abi.F32, out_dtype=self.dtype, label=label)

        def linear(a, wb, n, k, out, label, **kw):               # a 16-bit output: the M-independent route
            return pb.gemm(a, wb[0], N, n, k, bias=wb[2], w_lo=wb[1], out=out, flags=PACKED_GEMM_FLAGS, label=label, **kw)

        def close(a, wb, n, k, res, out, label, rows=N):         # stream <- res + a @ W^T + b in fp32: the 128-tile family whatever M is
            return pb.gemm(a, wb[0], rows, n, k, bias=wb[2], w_lo=wb[1], res=res, res_f32=True, out_f32=True, out=out, label=label)
        x = close(patches, W["pe"], C, self.patch_kp, pos, xa, "patch_embed")
        st = (3 * C, d)
        for i, Lr in enumerate(self.v_layers):
            tag = f"vis{i}"
            linear(norm16(x, Lr["ln1"], tag + ".ln1"), Lr["qkv"], 3 * C, C, qkv, tag + ".qkv")
            pb.qk_rope(Act(qkv.view(1, 1, N, 3 * C), 1, 1, N, 2 * C), rope, d, label=tag + ".rope")
            pb.segment_attention(qkv, qkv, qkv, o, seg, heads, d, N, st, st, st, (C, d), 1.0 / math.sqrt(d), k_off=C, v_off=2 * C, label=tag + ".attn")
            x1 = close(o, Lr["proj"], C, C, x, xb, tag + ".proj")
            linear(norm16(x1, Lr["ln2"], tag + ".ln2"), Lr["fc1"], hp["v_mlp"], C, h, tag + ".fc1", act=act)
            x = close(h, Lr["fc2"], C, hp["v_mlp"], x1, xa, tag + ".fc2")
        y32 = pb.norm(x, xb, N, C, gamma=W["v_ln"][0], beta=W["v_ln"][1], eps=hp["v_eps"], dtype=abi.F32, out_dtype=abi.F32, label="vis.post_ln")
        y = pb.norm(y32, ln16, N, C, gamma=W["p_ln"][0], beta=W["p_ln"][1], eps=1e-5, dtype=abi.F32, out_dtype=self.dtype, label="proj.pre_norm")
        # 2 x 2 merge: merged row (hb, wb) of an image = its four source rows side by side, so [N / 4][4 C] is a plain view
        merged = pb.row_gather(y, o, src, N, C, label="proj.merge")
        h1 = pb.gemm(merged, W["p1"][0], M, 4 * C, 4 * C, bias=W["p1"][2], w_lo=W["p1"][1], act=abi.ACT_GELU, flags=PACKED_GEMM_FLAGS, label="proj.linear_1")
        pb.gemm(h1, W["p2"][0], M, Ct, 4 * C, bias=W["p2"][2], w_lo=W["p2"][1], out=self.pk_cat[self.pk_rows:self.pk_rows + M], out_f32=True, label="proj.linear_2")
        plan = pb.build()
        plan.patches, plan.pos, plan.rope, plan.src, plan.seg, plan.cap = patches, pos, rope, src, seg, cap
        self._pk_vis[cap] = plan
        return plan

    def _packed_text(self, cap: int):
        """the prompt pass on `cap` stream rows that hold up to `slots` prompts packed row-wise (table index = slot), then the head and the pick on
        each segment's last row against the staging state block"""
        if cap in self._pk_txt:
            return self._pk_txt[cap]
        hp, B = self.hp, self.slots
        f32, i32 = torch.float32, torch.int32
        C, R = hp["t_dim"], cap
        pb = PlanBuilder(self.lib, self.device, self.dtype)
        ids, src, last = pb.buf((R,), i32, zero=True), pb.buf((R,), i32, zero=True), pb.buf((abi.SLOTS_MAX,), i32, zero=True)
        rope = pb.buf((R, 2, HEAD_DIM // 2), f32, zero=True)
        seg = pb.buf((abi.SLOTS_MAX + 1,), i32, zero=True)
        e16 = pb.row_gather(self.W["tok"], pb.buf((R, C), self.tdt), ids, R, C, label="embed")
        pb.cvt_f32(Act(e16.view(1, 1, R, C), 1, 1, R, C), self.dtype, label="embed.f32", out=Act(self.pk_cat[:R].view(1, 1, R, C), 1, 1, R, C))
        # a text row takes its own embedding, an image placeholder row its merged image row: one gather over [token embeddings | image rows]
        x = pb.row_gather(self.pk_cat, pb.buf((R, C), f32), src, R, C, label="embed.stream", dtype=abi.F32)
        pool = {}

        def out_of(label, n, dt):
            key = label.split(".", 1)[1]
            if key not in pool:
                pool[key] = pb.buf((R, n), dt)
            return pool[key]

        def lin(a, wb, n, k, label):                               # a 16-bit output: the M-independent route
            return pb.gemm(a, wb[0], R, n, k, out=out_of(label, n, self.tdt), flags=PACKED_GEMM_FLAGS, label=label)

        def close(a, wb, n, k, res, label):                        # fp32 output: the 128-tile family whatever M is
            return pb.gemm(a, wb[0], R, n, k, res=res, res_f32=True, out_f32=True, out=out_of(label, n, f32), label=label)
        x = self._layers(pb, x, R, rope, lin, close, packed=(seg, pool))
        xl = pb.row_gather(x, pb.buf((B, C), f32), last, B, C, label="last_rows", dtype=abi.F32)
        self._head(pb, xl, advance=1, slots=B, staging=True)
        plan = pb.build()
        plan.ids, plan.src, plan.last, plan.rope, plan.seg, plan.cap = ids, src, last, rope, seg, cap
        self._pk_txt[cap] = plan
        return plan

    def _prepare(self, item):
        """what a packed fill needs of one checked item, or the ModelError its prompt earns (placeholders that do not match the grid): no device work"""
        hp = self.hp
        ids = item["input_ids"][0].to(torch.long).cpu()
        thw = item["image_grid_thw"]
        gh, gw = int(thw[0, 1]), int(thw[0, 2])
        is_img = ids == hp["image_token"]
        pos3 = rope_positions(is_img, gh, gw, hp["merge"])
        T = int(ids.numel())
        return dict(ids=ids, T=T, gh=gh, gw=gw, is_img=is_img, pos3=pos3, next_rope=max(int(pos3.max()) + 1, 0),
                    pix=item["pixel_values"].reshape(gh * gw, self.patch_k))

    @staticmethod
    def _rung(ladder, need, what):
        for cap in ladder:
            if cap >= need:
                return cap
        raise ModelError(f"{WHAT}: a pack of {need} {what} exceeds the largest packed plan ({ladder[-1]})")

    def _fill_packed(self, assign):
        """assign: [(slot, prepared item)] for FREE slots, at most one item per slot.  One vision pack (images in the order given), one text pack
        (prompts in slot order, table index = slot), the pick on a staging state block, then the filled lanes move into the slot state.
        Nothing of a slot that is not in `assign` is read or written"""
        hp = self.hp
        f32, i32 = torch.float32, torch.int32
        assign = list(assign)
        assert 1 <= len(assign) <= self.slots and len({s for s, _ in assign}) == len(assign)
        # ---- vision pack
        n_patches = sum(p["gh"] * p["gw"] for _, p in assign)
        vis = self._packed_vision(self._rung(self.pk_vis_ladder, n_patches, "patches"))
        vseg = torch.zeros(abi.SEGS_MAX + 1, dtype=i32)
        src = torch.zeros(vis.cap, dtype=i32)
        pix = torch.zeros(n_patches, self.patch_k)
        pos = torch.empty(n_patches, hp["v_dim"], dtype=f32)
        rope = torch.empty(n_patches, 2, hp["v_dim"] // hp["v_heads"] // 2, dtype=f32)
        off, img_off = 0, {}
        for k, (slot, p) in enumerate(assign):
            n = p["gh"] * p["gw"]
            g_pos, g_rope, g_src = self._grid(p["gh"], p["gw"])
            pix[off:off + n], pos[off:off + n], rope[off:off + n], src[off:off + n] = p["pix"].to(f32), g_pos, g_rope, g_src + off
            img_off[slot] = off // 4
            off += n
            vseg[k + 1:] = off
        vis.patches[:n_patches, :self.patch_k].copy_(pix.to(self.tdt))
        vis.pos[:n_patches].copy_(pos)
        vis.rope[:n_patches].copy_(rope)
        vis.src.copy_(src)
        vis.seg.copy_(vseg)
        # ---- text pack
        by_slot = sorted(assign, key=lambda sp: sp[0])
        n_rows = sum(p["T"] for _, p in by_slot)
        txt = self._packed_text(self._rung(self.pk_txt_ladder, n_rows, "prompt rows"))
        tseg = torch.zeros(abi.SLOTS_MAX + 1, dtype=i32)
        ids, rows_src = torch.zeros(txt.cap, dtype=i32), torch.zeros(txt.cap, dtype=i32)
        trope = torch.zeros(txt.cap, 2, HEAD_DIM // 2, dtype=f32)
        last = torch.zeros(abi.SLOTS_MAX, dtype=i32)
        state = torch.zeros(abi.SLOT_FIELDS, abi.SLOTS_MAX, dtype=i32)
        state[abi.SLOT_DONE] = 1
        off = 0
        for slot, p in by_slot:
            T = p["T"]
            ids[off:off + T] = p["ids"].to(i32)
            own = torch.arange(off, off + T, dtype=i32)
            image = self.pk_rows + img_off[slot] + torch.arange(int(p["is_img"].sum()), dtype=i32)
            own[p["is_img"]] = image
            rows_src[off:off + T] = own
            trope[off:off + T] = text_rope_table(p["pos3"], hp["mrope"], hp["theta"], HEAD_DIM)
            off += T
            tseg[slot + 1:] = off
            last[slot] = off - 1
            # the pick advances pos and the rotary row by one: the lane ends at pos = T, n_out = 1, rope row = the prompt's largest position id + 1
            state[abi.SLOT_POS, slot], state[abi.SLOT_DONE, slot], state[abi.SLOT_ROPE, slot] = T - 1, 0, p["next_rope"] - 1
        txt.ids.copy_(ids); txt.src.copy_(rows_src); txt.rope.copy_(trope); txt.last.copy_(last); txt.seg.copy_(tseg)
        self.pk_state.copy_(state)
        vis.run(graph=self._graph)
        txt.run(graph=self._graph)
        for slot, _ in by_slot:
            self.slot_state[:, slot].copy_(self.pk_state[:, slot])
            self.slot_out[slot, 0:1].copy_(self.pk_out[slot, 0:1])
        self.last_rungs = (vis.cap, txt.cap)
        return [p["T"] for _, p in assign]

    def fill_slots(self, pairs, max_new_tokens: Optional[int] = None):
        """packed fill of the given FREE slots, [(slot, item)], outside `generate_many` (tests, benchmarks): the item checks of `generate_many`,
        then one vision pack and one text pack.  -> the prompt lengths"""
        if not self.packed:
            raise ModelError(f"{WHAT}: fill_slots needs packed_prefill=True")
        budget = self.max_new if max_new_tokens is None else int(max_new_tokens)
        assign = []
        for slot, item in pairs:
            if not 0 <= int(slot) < self.slots:
                raise ModelError(f"{WHAT}: slot {slot!r} is outside 0 .. {self.slots - 1}")
            self._check_item(item, budget)
            assign.append((int(slot), self._prepare(item)))
        with self._lock:
            return self._fill_packed(assign)

    # ---- running ---------------------------------------------------------------------------------
    def _check_inputs(self, input_ids, pixel_values, image_grid_thw, kw):
        if kw.get("pixel_values_videos") is not None or kw.get("video_grid_thw") is not None:
            raise ModelError(f"{WHAT}: video inputs are not built")
        if input_ids is None or input_ids.dim() != 2 or input_ids.shape[0] != 1:
            raise ModelError(f"{WHAT}: one prompt at a time (batch 1)")
        if pixel_values is None or image_grid_thw is None or image_grid_thw.shape[0] != 1 or int(image_grid_thw[0, 0]) != 1:
            raise ModelError(f"{WHAT}: exactly one image per prompt")
        if kw.get("do_sample"):
            raise ModelError(f"{WHAT}: sampling (do_sample) is not built; decoding is greedy")
        for name in ("num_beams", "repetition_penalty"):
            if kw.get(name) is not None and float(kw[name]) != 1.0:
                raise ModelError(f"{WHAT}: {name}={kw[name]!r} is not built; decoding is greedy")

    def prefill(self, input_ids, pixel_values, image_grid_thw) -> int:
        """vision + prompt; leaves the first generated token in the device state.  Returns T"""
        hp = self.hp
        ids = input_ids[0].to(torch.long).cpu()
        T = int(ids.numel())
        gh, gw = int(image_grid_thw[0, 1]), int(image_grid_thw[0, 2])
        if T > self.max_prompt:
            raise ModelError(f"{WHAT}: a prompt of {T} tokens exceeds the {self.max_prompt} this model was built for")
        if pixel_values.shape[0] != gh * gw or pixel_values[0].numel() != self.patch_k:
            raise ModelError(f"{WHAT}: pixel_values {tuple(pixel_values.shape)} do not match the grid {gh} x {gw}")
        is_img = ids == hp["image_token"]
        pos3 = rope_positions(is_img, gh, gw, hp["merge"])
        vis = self._vision(gh, gw)
        vis.patches[:, :self.patch_k].copy_(pixel_values.reshape(gh * gw, self.patch_k).to(self.device, self.tdt))
        vis.run()
        start = int(is_img.nonzero()[0])
        pre = self._prefill(T, start, vis.tokens)
        pre.ids.copy_(ids.to(torch.int32))
        pre.rope.copy_(text_rope_table(pos3, hp["mrope"], hp["theta"], HEAD_DIM))
        # the token fed at cache position p >= T sits at rotary position p + delta, all three axes equal
        delta = int(pos3.max()) + 1 - T
        p = (torch.arange(self.max_len) + delta).clamp_min(0)
        self.step_rope.copy_(text_rope_table(p[None].expand(3, -1), hp["mrope"], hp["theta"], HEAD_DIM).reshape(self.max_len, HEAD_DIM))
        self.state.zero_()
        pre.run()
        return T

    def read_state(self):
        return [int(v) for v in self.state.cpu().tolist()]

    def generate(self, input_ids=None, pixel_values=None, image_grid_thw=None, max_new_tokens: Optional[int] = None, check_every: Optional[int] = None, **ignored):
        """greedy decoding, as `GenerationMixin.generate` returns it: int64 [1, T + n], the prompt then the generated tokens, EOS included"""
        self._check_inputs(input_ids, pixel_values, image_grid_thw, ignored)
        budget = self.max_new if max_new_tokens is None else int(max_new_tokens)
        if not 1 <= budget <= self.max_new:
            raise ModelError(f"{WHAT}: max_new_tokens {budget} is outside 1 .. {self.max_new} this model was built for")
        every = self.check_every if check_every is None else max(1, int(check_every))
        with self._lock:
            self.prefill(input_ids, pixel_values, image_grid_thw)
            step = self._stepper()
            _, n_out, done, _ = self.read_state()
            while not done and n_out < budget:
                for _ in range(min(every, budget - n_out)):
                    step.run(graph=self._graph)
                _, n_out, done, _ = self.read_state()
            n = min(n_out, budget)
            new = self.out[:n].to(torch.long).cpu()
        eos = [i for i, t in enumerate(new.tolist()) if t in self.hp["eos"]]
        if eos:
            new = new[:eos[0] + 1]
        return torch.cat([input_ids[0].to(torch.long).cpu(), new])[None].to(input_ids.device)

    def _check_item(self, item, budget):
        """everything `generate` would refuse about one item of `generate_many`, before any device work"""
        if not isinstance(item, dict):
            raise ModelError(f"{WHAT}: generate_many takes dicts with input_ids, pixel_values and image_grid_thw")
        ids, pix, thw = item.get("input_ids"), item.get("pixel_values"), item.get("image_grid_thw")
        self._check_inputs(ids, pix, thw, {k: v for k, v in item.items() if k not in ("input_ids", "pixel_values", "image_grid_thw")})
        T = int(ids.shape[1])
        gh, gw = int(thw[0, 1]), int(thw[0, 2])
        if T > self.max_prompt:
            raise ModelError(f"{WHAT}: a prompt of {T} tokens exceeds the {self.max_prompt} this model was built for")
        if gh % 2 or gw % 2 or gh * gw // 4 > self.img_rows.shape[0]:
            raise ModelError(f"{WHAT}: an image grid of {gh} x {gw} patches is not served (even sides, at most {self.img_rows.shape[0]} merged tokens)")
        if pix.shape[0] != gh * gw or pix[0].numel() != self.patch_k:
            raise ModelError(f"{WHAT}: pixel_values {tuple(pix.shape)} do not match the grid {gh} x {gw}")
        if not 1 <= budget <= self.max_new:
            raise ModelError(f"{WHAT}: max_new_tokens {budget} is outside 1 .. {self.max_new} this model was built for")

    def _fill_slot(self, slot: int, item) -> int:
        """vision + prefill on the staging set, then device copies (same stream) of cache rows [0, T) and the state into the slot.  -> T"""
        ids = item["input_ids"]
        T = self.prefill(ids, item["pixel_values"], item["image_grid_thw"])
        for (kc, vc), (skc, svc) in zip(self.caches, self.slot_caches):
            skc[slot, :T].copy_(kc[:T])
            svc[slot, :T].copy_(vc[:T])
        self.slot_state[:4, slot].copy_(self.state)
        # the token fed at cache position T sits at rotary position T + delta = the prompt's largest position id + 1 (as `prefill`'s step_rope)
        tok = ids[0].to(torch.long).cpu()
        gh, gw = int(item["image_grid_thw"][0, 1]), int(item["image_grid_thw"][0, 2])
        delta = int(rope_positions(tok == self.hp["image_token"], gh, gw, self.hp["merge"]).max()) + 1 - T
        self.slot_state[abi.SLOT_ROPE, slot] = max(T + delta, 0)
        self.slot_out[slot, 0:1].copy_(self.out[0:1])
        return T

    def generate_many(self, items, max_new_tokens: Optional[int] = None, check_every: Optional[int] = None) -> list:
        """`generate` for a list of prompts, up to `slots` of them in flight in one batched step plan: -> [int64 [1, T + n] | ModelError], in
        the order given, each tensor exactly what `generate` returns for that item.  A refused item leaves its ModelError in its place and
        does not stop the others.  The host reads 20 bytes of state per slot every `check_every` steps.  With `packed_prefill` every look at
        the state fills ALL free slots from the pending list in one vision pack and one text pack (no waiting: a single free slot is filled
        alone through the same plans); the tokens are then the packed fill's, held to the oracle, not bit for bit `generate`'s."""
        budget = self.max_new if max_new_tokens is None else int(max_new_tokens)
        every = self.check_every if check_every is None else max(1, int(check_every))
        items = list(items)
        results = [None] * len(items)
        pending = []
        for i, item in enumerate(items):
            try:
                self._check_item(item, budget)
                pending.append(i)
            except ModelError as e:
                results[i] = e
        if self.slots == 1:
            for i in pending:
                try:
                    it = items[i]
                    results[i] = self.generate(input_ids=it["input_ids"], pixel_values=it["pixel_values"], image_grid_thw=it["image_grid_thw"],
                                               max_new_tokens=budget, check_every=every)
                except ModelError as e:
                    results[i] = e
            return results
        B = self.slots
        pending.reverse()                                            # pop() takes them in the order given
        with self._lock:
            step = self._stepper_batch()
            owner = [None] * B                                       # slot -> item index
            n_out = [0] * B
            self.fill_log = []
            self.slot_state[abi.SLOT_DONE] = 1
            while pending or any(o is not None for o in owner):
                assign = []                                          # packed fill: ALL free slots from the pending list in one vision and one text pack
                for s in ([t for t in range(B) if owner[t] is None] if self.packed else ()):
                    while pending:
                        i = pending.pop()
                        try:
                            assign.append((s, i, self._prepare(items[i])))
                            break
                        except ModelError as e:                      # (a prompt whose placeholders do not match its grid: found before the pack is built,
                            results[i] = e                           # it takes no slot)
                if assign:
                    self._fill_packed([(s, p) for s, _, p in assign])
                    for s, i, _ in assign:
                        self.fill_log.append((i, s, [(owner[t], n_out[t]) for t in range(B) if t != s and owner[t] is not None]))
                        owner[s], n_out[s] = i, 1
                for s in (() if self.packed else range(B)):
                    while owner[s] is None and pending:
                        i = pending.pop()
                        try:
                            self._fill_slot(s, items[i])
                        except ModelError as e:                      # (a prompt whose placeholders do not match its grid: the slot stays free)
                            results[i] = e
                            self.slot_state[abi.SLOT_DONE, s] = 1
                            continue
                        self.fill_log.append((i, s, [(owner[t], n_out[t]) for t in range(B) if t != s and owner[t] is not None]))
                        owner[s], n_out[s] = i, 1
                st = self.slot_state[:, :B].cpu()
                harvested = False
                for s in range(B):
                    if owner[s] is None:
                        continue
                    n_out[s] = int(st[abi.SLOT_NOUT, s])
                    if not int(st[abi.SLOT_DONE, s]) and n_out[s] < budget:
                        continue
                    ids = items[owner[s]]["input_ids"]
                    new = self.slot_out[s, :min(n_out[s], budget)].to(torch.long).cpu()
                    eos = [k for k, t in enumerate(new.tolist()) if t in self.hp["eos"]]
                    if eos:
                        new = new[:eos[0] + 1]
                    results[owner[s]] = torch.cat([ids[0].to(torch.long).cpu(), new])[None].to(ids.device)
                    self.slot_state[abi.SLOT_DONE, s] = 1
                    owner[s], harvested = None, True
                if harvested and pending:
                    continue                                         # refill before stepping
                live = [budget - n_out[s] for s in range(B) if owner[s] is not None]
                if not live:
                    continue
                for _ in range(min(every, max(live))):
                    step.run(graph=self._graph)
        return results

    def step_logits(self, token: int) -> torch.Tensor:
        """teacher forcing (parity tests): feed `token` at the current position instead of the model's own pick -> fp32 logits [vocab] of the next"""
        st = self.read_state()
        self.state.copy_(torch.tensor([st[0], 0, 0, int(token)], dtype=torch.int32))
        self._stepper().run(graph=self._graph)
        return self.logits[0].float().cpu().clone()

    def slot_step_logits(self, slot: int, token: int) -> torch.Tensor:
        """teacher forcing on the batched stepper (parity tests): feed `token` at slot `slot`'s current position instead of the model's own pick
        -> fp32 logits [vocab] of the next.  The other slots keep their lanes (a finished or empty one sits out)"""
        st = self.slot_state.cpu()
        st[abi.SLOT_NOUT, slot], st[abi.SLOT_DONE, slot], st[abi.SLOT_TOKEN, slot] = 0, 0, int(token)
        self.slot_state.copy_(st)
        self._stepper_batch().run(graph=self._graph)
        return self.slot_logits[slot].float().cpu().clone()

    def close(self):
        for p in [*self._pk_vis.values(), *self._pk_txt.values()]:
            p.close()
        self._pk_vis.clear()
        self._pk_txt.clear()
        for p in [self._step, self._step_b, *self._vis.values(), *self._pre.values()]:
            if p is not None:
                p.close()
        self._step = self._step_b = None
        self._vis.clear()
        self._pre.clear()


class GenerateShim:
    """what `extract_text_with_paddle_ocr_vl` calls `model`: `.device` and `.generate(**inputs, max_new_tokens=)`"""

    def __init__(self, model: PaddleOcrVlHip):
        self.model = model
        self.device = torch.device("cpu")          # the processor's tensors stay on the host: `generate` uploads what the plans need

    def generate(self, **kw):
        return self.model.generate(**kw)

    @property
    def slots(self) -> int:
        return self.model.slots

    def generate_many(self, items, **kw):
        return self.model.generate_many(items, **kw)

    def close(self):
        self.model.close()


def build_processor(root):
    """the wheel's `PaddleOCRVLProcessor`, assembled by hand from the staged files (AutoProcessor demands torchvision through AutoImageProcessor):
    image processor from the json's image-processor section — torchvision's when it imports, PIL's otherwise — the tokenizer and the chat
    template, all with local_files_only"""
    root = Path(root)
    from transformers import AutoTokenizer
    from transformers.models.paddleocr_vl.processing_paddleocr_vl import PaddleOCRVLProcessor
    section = {}
    for name in ("processor_config.json", "preprocessor_config.json"):
        if (root / name).is_file():
            js = json.loads((root / name).read_text())
            section = js.get("image_processor", js) if name == "processor_config.json" else js
            if section:
                break
    section = {k: v for k, v in section.items() if k not in ("image_processor_type", "processor_class", "auto_map")}
    try:
        import torchvision  # noqa: F401
        from transformers.models.paddleocr_vl.image_processing_paddleocr_vl import PaddleOCRVLImageProcessor as IP
    except Exception:
        from transformers.models.paddleocr_vl.image_processing_pil_paddleocr_vl import PaddleOCRVLImageProcessorPil as IP
    tok = AutoTokenizer.from_pretrained(str(root), local_files_only=True)
    template = None
    for name in ("chat_template.jinja", "chat_template.json"):
        if (root / name).is_file():
            text = (root / name).read_text()
            template = json.loads(text)["chat_template"] if name.endswith(".json") else text
            break
    if template is None:
        template = getattr(tok, "chat_template", None)
    if template is None:
        raise ModelError(f"{WHAT} is not staged: no chat template in {root}")
    return PaddleOCRVLProcessor(image_processor=IP(**section), tokenizer=tok, chat_template=template)


def load_pair(root, device="cuda", lib=None, dtype: int = abi.F16, **kw):
    """(processor, model shim) from a staged directory"""
    model = PaddleOcrVlHip.from_directory(root, device=device, lib=lib, dtype=dtype, **kw)
    return build_processor(root), GenerateShim(model)
