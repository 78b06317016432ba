"""CPU tier of the manga-ocr work: the decode-step kernels on the simulator (checks in manga_ocr_checks.py)."""
import functools

import pytest

import manga_ocr_checks as mc
from mangatranslator_amd.hip import abi

DTYPES = [abi.BF16, abi.F16]
KERNEL_DTYPES = DTYPES + [abi.F32]          # the two decode kernels also come in fp32 (the recogniser's storage "f32")
ROWLIN_SHAPES = [(768, 768), (6144, 768), (136, 72), (2050, 520)]          # NW = 1, 4, 1, 2 (manga_ocr_checks.rowlin_tiling)


@pytest.mark.parametrize("dtype", KERNEL_DTYPES)
@pytest.mark.parametrize("n_keys", [1, 2, 64, 128])
def test_decode_attention_exact(emu_lib, dtype, n_keys):
    mc.check_decode_attn_exact(emu_lib, dtype, n_keys)


@pytest.mark.parametrize("dtype", KERNEL_DTYPES)
@pytest.mark.parametrize("rows", [1, 3, 4])
def test_decode_attention_random(emu_lib, dtype, rows):
    for pos in (0, 1, 63, 64, 65, 299):
        mc.check_decode_attn_random(emu_lib, dtype, rows, pos)


def test_decode_attention_refuses_other_head_widths(emu_lib):
    mc.check_decode_attn_refuses_d32(emu_lib)


@pytest.mark.parametrize("dtype", KERNEL_DTYPES)
@pytest.mark.parametrize("n,k", ROWLIN_SHAPES)
@pytest.mark.parametrize("rows", [1, 4, 5])
def test_row_linear_exact(emu_lib, dtype, rows, n, k):
    for out_f32 in ((True,) if dtype == abi.F32 else (False, True)):
        mc.check_rowlin_exact(emu_lib, dtype, rows, n, k, out_f32)


@pytest.mark.parametrize("dtype", KERNEL_DTYPES)
@pytest.mark.parametrize("n,k", ROWLIN_SHAPES)
def test_row_linear_random(emu_lib, dtype, n, k):
    for out_f32 in ((True,) if dtype == abi.F32 else (False, True)):
        mc.check_rowlin_random(emu_lib, dtype, 5, n, k, out_f32)


# ---- the model on the simulator (tiny configuration; oracle = the transformers model in fp32) --------------------------------------------------
# Bounds: twice the largest value the simulator gives over seeds 0-7 (docs/experiments.md, "manga-ocr on the HIP path", beside the MI355X's).
# The figures are large for a log-prob because the test model is: with initializer_range 0.3 its logits span +-25 and rounding ONLY THE WEIGHTS
# of the fp32 oracle to f16 already moves a log-prob by up to 2.7 (bf16: 6.3) — the graphs sit on that floor.
SIM_BOUNDS = {abi.F16: dict(tf=(2 * 2.55, 2 * 0.202), lock=(2 * 3.54, 2 * 0.265)), abi.BF16: dict(tf=(2 * 11.01, 2 * 1.04), lock=(2 * 9.84, 2 * 1.08)),
              abi.F32: dict(tf=(2 * 0.002454, 2 * 0.000209), lock=(2 * 0.001968, 2 * 0.000171))}
TF_MAX_F32 = 0.002454        # the simulator's teacher-forced maximum with fp32 storage, seeds 0-7
SEEDS = range(8)


@pytest.mark.parametrize("dtype", KERNEL_DTYPES)
@pytest.mark.parametrize("seed", SEEDS)
def test_teacher_forced_log_probs(emu_lib, dtype, seed):
    mx, rms = mc.check_teacher_forced(emu_lib, dtype, seed)
    print(f"teacher-forced seed {seed} dtype {dtype}: max {mx:.4f} rms {rms:.4f}")
    assert mx <= SIM_BOUNDS[dtype]["tf"][0] and rms <= SIM_BOUNDS[dtype]["tf"][1]


@pytest.mark.parametrize("dtype", KERNEL_DTYPES)
@pytest.mark.parametrize("seed", SEEDS)
def test_lockstep_beams(emu_lib, dtype, seed):
    mx, rms, reorders = mc.check_lockstep_beams(emu_lib, dtype, seed)
    print(f"lock-step seed {seed} dtype {dtype}: max {mx:.4f} rms {rms:.4f}, {reorders} reordered steps")
    assert reorders >= 10, "the beams were hardly reordered: the cache indirection is not under test"
    assert mx <= SIM_BOUNDS[dtype]["lock"][0] and rms <= SIM_BOUNDS[dtype]["lock"][1]


GREEDY_DELTA = 0.05


@functools.lru_cache(maxsize=1)
def _decided_lengths():
    """decided prefix length per seed, from the oracle alone (computed once for the eight cases)"""
    return [mc.decided_prefix(s, GREEDY_DELTA)[1] for s in SEEDS]


@pytest.mark.parametrize("seed", SEEDS)
def test_greedy_tokens_on_decided_prefixes(emu_lib, seed):
    """The device's greedy tokens equal the oracle's over each seed's decided prefix: the steps before the oracle's own top-1 / top-2 log-prob gap
    first drops below delta.  The prefix comes from the oracle alone, and at least 100 of the 160 steps (8 seeds x 20) must be decided.
    delta = 0.05 stands if the measured maximum log-prob error of the teacher-forced test is <= delta / 4 = 0.0125.  With fp32 storage it is
    0.0025 on the simulator (0.0022 on the MI355X): delta = 0.05 stands, 121 steps are decided ([20, 20, 20, 19, 4, 12, 6, 20]).
    With 16-bit storage the rule cannot be met on this test model — measured maxima 1.47 (f16) / 11.0 (bf16) on the MI355X, 2.55 / 11.0 on the
    simulator; rounding ONLY THE WEIGHTS of the fp32 oracle to f16 already gives up to 2.7 — and delta = 4 x the error leaves no decided step at
    all (decided steps at delta 0.1: 104, 0.5: 30, 1.0: 1), so there is no prefix to hold the 16-bit graphs to: their bar is the log-prob bounds
    above and, at the published widths, 0.0022 of the oracle."""
    assert TF_MAX_F32 <= GREEDY_DELTA / 4
    decided = _decided_lengths()
    assert sum(decided) >= 100, f"only {sum(decided)} of 160 steps are decided at delta = {GREEDY_DELTA}"
    assert mc.check_greedy_tokens(emu_lib, abi.F32, seed, GREEDY_DELTA) == decided[seed]


@pytest.mark.parametrize("historical", [False, True])
def test_end_to_end_from_a_staged_directory(emu_lib, tmp_path, historical):
    """config.json + safetensors (transformers 5 key names, and the hub's historical ones) + vocab.txt + preprocessor_config.json -> a string"""
    from PIL import Image
    from mangatranslator_amd.core.ml import manga_ocr as mo
    root = mc.stage_directory(tmp_path / "manga-ocr-base", gen=dict(mc.GEN, max_length=8), historical=historical)
    ocr = mo.MangaOcrHip.from_directory(root, device="cpu", lib=emu_lib)
    import numpy as np
    yy, xx = np.mgrid[0:37, 0:50]
    text = ocr(Image.fromarray(((xx * 7 + yy * 13) % 97 + 80).astype(np.uint8)).convert("RGB"))
    ocr.close()
    assert isinstance(text, str) and not any(ch.isspace() for ch in text) and "[" not in text
    _E2E_TEXTS.append(text)
    assert len(set(_E2E_TEXTS)) == 1, "the two key layouts of one checkpoint read differently"


_E2E_TEXTS = []


def test_nothing_staged_is_a_model_error(tmp_path, monkeypatch):
    from mangatranslator_amd.core.image import ocr_detection as od
    from mangatranslator_amd.core.ml.model_manager import ModelType, get_model_manager
    from mangatranslator_amd.utils.exceptions import ModelError
    mgr = get_model_manager()
    monkeypatch.setitem(mgr.model_paths, ModelType.MANGA_OCR, tmp_path / "manga-ocr-base")
    monkeypatch.setitem(mgr.models, ModelType.MANGA_OCR, None)
    assert not mgr.manga_ocr_available()
    with pytest.raises(ModelError):
        mgr.get_manga_ocr()
    (tmp_path / "manga-ocr-base").mkdir()
    (tmp_path / "manga-ocr-base" / "config.json").write_text("{}")
    with pytest.raises(ModelError):
        mgr.get_manga_ocr()
    from PIL import Image
    assert od.extract_text_with_manga_ocr([Image.new("RGB", (8, 8))]) == ["[OCR FAILED]"]


# ---- routes the cases above leave open: rows 5..8 and other head counts in the attention, padded strides, the skinny linear against float64 ----
@pytest.mark.parametrize("dtype", KERNEL_DTYPES)
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("rows", [5, 8])
def test_decode_attention_exact_eight_slots(emu_lib, dtype, heads, rows):
    """decode_attn_kernel<T> on a grid (heads, rows) with blockIdx.y up to 7 and heads != 2"""
    for n_keys in (2, 64):
        mc.check_decode_attn_exact(emu_lib, dtype, n_keys, rows=rows, slots=8, heads=heads)


@pytest.mark.parametrize("dtype", KERNEL_DTYPES)
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("rows", [5, 8])
def test_decode_attention_random_eight_slots(emu_lib, dtype, heads, rows):
    worst = max(mc.check_decode_attn_random(emu_lib, dtype, rows, pos, slots=8, heads=heads) for pos in (0, 32, 33, 299))
    print(f"decode attention rows {rows} heads {heads} dtype {dtype}: worst error {worst:.3f} x bound")


@pytest.mark.parametrize("dtype", KERNEL_DTYPES)
def test_decode_attention_padded_strides(emu_lib, dtype):
    mc.check_decode_attn_padded_strides(emu_lib, dtype)


CONTRACT_K = (lambda n: 136 if n == 4100 else 520)          # the simulator tier shortens K at the widest N
CONTRACT_TYPES = [(abi.BF16, False), (abi.F16, False), (abi.F16, True), (abi.F32, True)]


@pytest.mark.parametrize("dtype,out_f32", CONTRACT_TYPES)
@pytest.mark.parametrize("n,nw", [(257, 1), (2050, 2), (4100, 4)])
@pytest.mark.parametrize("rows,rt", [(1, 1), (3, 4), (5, 8)])
def test_row_linear_contract_exact(emu_lib, dtype, out_f32, n, nw, rows, rt):
    """rowlin_kernel<T, RT, NW> for every (RT, NW), against float64 with the contract's rounding points"""
    share = mc.check_rowlin_contract_exact(emu_lib, dtype, rows, n, CONTRACT_K(n), False, out_f32, (rt, nw))
    print(f"row linear contract {rows}x{n} dtype {dtype}: rounding share {share}")
