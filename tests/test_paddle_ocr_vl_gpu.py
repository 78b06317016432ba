"""GPU tier of the PaddleOCR-VL work: causal grouped-query attention, the greedy pick, the rotary turn at head width 72 and the model on the
MI355X (checks in paddle_ocr_vl_checks.py)."""
import pytest

import paddle_ocr_vl_checks as pc
from mangatranslator_amd.hip import abi

DTYPES = [abi.BF16, abi.F16]
pytestmark = pytest.mark.gpu


def test_abi_is_12(hip_lib):
    assert abi.ABI_VERSION == 12 and hip_lib.mtx_abi_version() == 12


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", pc.HEADS)
@pytest.mark.parametrize("rows", pc.ROWS)
def test_causal_attention_selects_exactly(hip_lib, dtype, heads, kv, rows):
    for pos in pc.POSITIONS:
        for winner in ("own", "pos", "zero"):
            pc.check_causal_selection(hip_lib, dtype, rows, pos, heads, kv, winner)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", pc.HEADS)
@pytest.mark.parametrize("rows", pc.ROWS)
def test_causal_attention_random(hip_lib, dtype, heads, kv, rows):
    worst = max(pc.check_causal_random(hip_lib, dtype, rows, pos, heads, kv) for pos in pc.POSITIONS)
    print(f"causal attention rows {rows} heads {heads}/{kv} dtype {dtype}: worst error {worst:.3f} x bound")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, pc.TQ + 1])
def test_causal_attention_full_cache_is_a_no_op(hip_lib, dtype, rows):
    pc.check_causal_full_cache_is_a_no_op(hip_lib, dtype, rows, 4, 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", [(4, 2), (16, 2)])
def test_prefill_equals_steps(hip_lib, dtype, heads, kv):
    diff = pc.check_prefill_equals_steps(hip_lib, dtype, pc.TQ + pc.TK + 3, 2 * pc.S - 30, heads, kv)
    print(f"prefill vs steps heads {heads}/{kv} dtype {dtype}: {diff} elements differ by one step")


@pytest.mark.parametrize("dtype", DTYPES)
def test_step_is_deterministic(hip_lib, dtype):
    pc.check_step_is_deterministic(hip_lib, dtype, 4 * pc.S + 9, 16, 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 3])
def test_gqa_mapping(hip_lib, dtype, rows):
    pc.check_gqa_mapping(hip_lib, dtype, rows)


def test_causal_attention_refusals(hip_lib):
    pc.check_causal_refusals(hip_lib)


@pytest.mark.parametrize("vocab", pc.VOCABS)
def test_greedy_pick_argmax(hip_lib, vocab):
    pc.check_greedy_argmax(hip_lib, vocab)


def test_greedy_pick_state(hip_lib):
    pc.check_greedy_state(hip_lib)


def test_greedy_pick_run_of_steps(hip_lib):
    pc.check_greedy_run_of_steps(hip_lib)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rope_at_width_72(hip_lib, dtype):
    res = pc.check_rope_widths(hip_lib, dtype)
    print(f"qk_rope dtype {dtype}: " + ", ".join(f"d={d}: {u:.2f} ulp, {n} differ" for d, (u, n) in res.items()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [8, 64, 72, 128])
def test_rope_exact(hip_lib, dtype, d):
    pc.check_rope_exact(hip_lib, dtype, d)


def test_rope_refuses_other_widths(hip_lib):
    pc.check_rope_refusals(hip_lib)


# ---- the model on the MI355X (tiny configuration; oracle = the wheel's model in fp32 on the CPU) ---------------------------------------------
# Bounds: twice the largest value the MI355X gives over seeds 0-7 (docs/experiments.md, "PaddleOCR-VL on the HIP path", beside the simulator's
# and beside the floor: rounding ONLY THE WEIGHTS of the fp32 oracle to f16 moves a log-prob by up to 0.013, to bf16 by up to 0.11).
GPU_TF = {abi.F16: (0.027125, 0.004248), abi.BF16: (0.252164, 0.036560)}          # measured on the MI355X (max, rms), sigma 0.1
GPU_TF_GREEDY_F16 = 0.006420                                                      # measured max at the greedy test's sigma (0.06)
SEEDS = range(8)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", SEEDS)
def test_teacher_forced_log_probs(hip_lib, dtype, seed):
    mx, rms = pc.check_teacher_forced(hip_lib, dtype, seed)
    from parity_log import record
    record(f"paddle_ocr_vl_teacher_forced_{dtype}_{seed}", max=mx, rms=rms)
    print(f"teacher-forced seed {seed} dtype {dtype}: max {mx:.5f} rms {rms:.5f}")
    assert mx <= 2 * GPU_TF[dtype][0] and rms <= 2 * GPU_TF[dtype][1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_second_grid_and_prompt_shape(hip_lib, dtype):
    """a non-square grid (2 x 8) under a prompt with more text before the image and less after it: the resampled position table and the 3-D
    position ids are the wheel's"""
    mx, rms = pc.check_teacher_forced(hip_lib, dtype, 0, grid=(2, 8), before=(1, 10, 11, 12, 13), after=(20,))
    print(f"teacher-forced grid 2x8 dtype {dtype}: max {mx:.5f} rms {rms:.5f}")
    assert mx <= 2 * GPU_TF[dtype][0] and rms <= 2 * GPU_TF[dtype][1]


def test_oracle_greedy_is_the_wheels_generate():
    pc.check_generate_matches_wheel()


@pytest.mark.parametrize("seed", SEEDS)
def test_greedy_tokens_on_decided_prefixes(hip_lib, seed):
    """The device loop's f16 tokens equal the oracle's over each seed's decided prefix: the steps before the oracle's own top-1 / top-2 log-prob
    gap first drops below delta = 4 x the measured teacher-forced maximum.  At least half of the 160 steps (8 seeds x 20) must be decided.
    At sigma = 0.1 they are not: delta = 4 x 0.0282 = 0.113 leaves 20 decided steps ([1, 6, 2, 0, 4, 1, 3, 3]), because a prefix ends at the
    FIRST small gap and one step in eight has one.  Lowering sigma shrinks the error faster than the gaps: measured on the simulator (teacher-
    forced maximum, decided steps, distinct tokens per seed; the MI355X gives 0.0064 and the same 107 at sigma 0.06) sigma 0.07: 0.0077, 74, 7-17; 0.065: 0.0078, 81; 0.06: 0.0063, 107
    ([20, 3, 1, 5, 20, 18, 20, 20]), distinct tokens [1, 9, 4, 10, 1, 10, 9, 9]; 0.05: 0.0041, 108 but 1-4 distinct tokens; 0.03: the tied head
    repeats one or two tokens.  sigma = 0.06 is the largest with room above 80, and six of its eight runs still vary."""
    delta = 4 * GPU_TF_GREEDY_F16
    decided = [pc.decided_prefix(s, delta)[1] for s in SEEDS]
    assert sum(decided) >= 80, f"only {sum(decided)} of 160 steps are decided at delta = {delta}"
    assert pc.check_greedy_tokens(hip_lib, abi.F16, seed, delta) == decided[seed]


def test_greedy_sigma_teacher_forced_error(hip_lib):
    """the figure delta is made of, held to twice its measured value like the others (seed 5 gave the maximum)"""
    mx, _ = pc.check_teacher_forced(hip_lib, abi.F16, 5, sigma=pc.GREEDY_SIGMA)
    assert mx <= 2 * GPU_TF_GREEDY_F16


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_resident_loop(hip_lib, dtype):
    pc.check_device_loop(hip_lib, dtype)


def test_model_refusals(hip_lib):
    pc.check_refusals()
    pc.check_input_refusals(hip_lib)


def test_end_to_end_from_a_staged_directory(hip_lib, tmp_path, monkeypatch):
    pc.check_end_to_end(hip_lib, tmp_path, monkeypatch)


# ---- the published widths (GPU file only) ------------------------------------------------------------------------------------------------------
GPU_REAL = {abi.F16: (0.002624, 0.000577)}          # measured on the MI355X (max, rms)


def test_published_widths(hip_lib):
    """seeded weights at the wheel's default sizes with the vocabulary cut to 8 192, grid 20 x 28, 40 teacher-forced tokens, positions 0-9 and
    30-39 against the fp32 oracle"""
    from parity_log import record
    mx, rms = pc.check_published_widths(hip_lib, abi.F16)
    record("paddle_ocr_vl_published_f16", max=mx, rms=rms)
    print(f"published widths f16: max {mx:.5f} rms {rms:.5f}")
    assert mx <= 2 * GPU_REAL[abi.F16][0] and rms <= 2 * GPU_REAL[abi.F16][1]


# ---- head layouts of the step kernels that HEADS does not reach (G = 4; more than one chunk of query heads per kv head), strides, greedy edges ----
LAYOUTS_AND_16 = pc.STEP_LAYOUTS + [(16, 2)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", pc.STEP_LAYOUTS)
def test_step_layouts_random(hip_lib, dtype, heads, kv):
    """causal_step_kernel<T, G> at (G, nz) = step_layout(heads, kv) and the prefill's h / G, against the fp32 reference under the bound of
    test_causal_attention_random (derived for up to 300 keys; the largest case here has 2 S + 6 = 134)"""
    pc.assert_layout(heads, kv)
    assert max(pc.STEP_POSITIONS) + 1 <= 300 and pc.TK + 1 + pc.TQ + 3 <= 300
    worst = max(pc.check_causal_random(hip_lib, dtype, 1, pos, heads, kv) for pos in pc.STEP_POSITIONS)
    worst = max(worst, pc.check_causal_random(hip_lib, dtype, pc.TQ + 3, pc.TK + 1, heads, kv))
    print(f"step layouts heads {heads}/{kv} (G, nz) {pc.step_layout(heads, kv)} dtype {dtype}: worst error {worst:.3f} x bound")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", LAYOUTS_AND_16)
@pytest.mark.parametrize("rows", [1, pc.TQ + 1])
def test_causal_attention_selects_exactly_per_head(hip_lib, dtype, heads, kv, rows):
    pc.assert_layout(heads, kv)
    for pos in pc.STEP_POSITIONS:
        pc.check_causal_selection_per_head(hip_lib, dtype, rows, pos, heads, kv)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", [(32, 2), (24, 2)])
def test_step_layouts_deterministic(hip_lib, dtype, heads, kv):
    pc.assert_layout(heads, kv)
    assert pc.LAYOUT_OF[(heads, kv)][1] > 1
    pc.check_step_is_deterministic(hip_lib, dtype, 4 * pc.S + 9, heads, kv)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads,kv", pc.STEP_LAYOUTS)
@pytest.mark.parametrize("rows", [1, 3])
def test_gqa_mapping_step_layouts(hip_lib, dtype, heads, kv, rows):
    pc.assert_layout(heads, kv)
    pc.check_gqa_mapping(hip_lib, dtype, rows, heads, kv)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, pc.TQ + 1])
def test_causal_attention_padded_strides(hip_lib, dtype, rows):
    pc.check_causal_padded_strides(hip_lib, dtype, rows)


def test_greedy_pick_65_chunks(hip_lib):
    pc.check_greedy_65_chunks(hip_lib)


def test_greedy_pick_damaged_state(hip_lib):
    pc.check_greedy_damaged_state(hip_lib)


@pytest.mark.parametrize("vocab", [1, 300, 4097])
def test_greedy_pick_all_nan(hip_lib, vocab):
    pc.check_greedy_all_nan(hip_lib, vocab)
