"""Hardware tier of the lane-hazard tests (tests/lane_hazard_checks.py): a DiT step built with the text stream on the side lane equals the
same step built on one lane, bit for bit — eagerly (two streams) and as a hipGraph replay (two branches), three runs of each.  Every kernel
is order-independent by construction, so this holds exactly; finding overlaps is the static analysis' job (tests/test_lane_hazards_sim.py),
this tier confirms that the lane machinery and the capture of the real plans do what that analysis assumes.  No plan the analysis flags is run."""
import pytest
import torch

import flux_checks as fc
import lane_hazard_checks as lh
from mangatranslator_amd.core.ml import flux as fx
from mangatranslator_amd.core.ml import flux2 as f2

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", ["kontext", "kontext.cached", "kontext.fp8", "klein", "klein.fp8"])
def test_lanes_on_and_off_give_the_same_bytes(hip_lib, variant):
    lh.check_lanes_bit_equal(hip_lib, "cuda:0", variant, "small")


@pytest.mark.parametrize("kind,fp8", [("kontext", False), ("klein", True)])
def test_lanes_on_and_off_at_production_width(hip_lib, kind, fp8):
    """d = 3072, 24 heads, 2 double + 1 single block, t_txt 512, T = 2048: the text GEMMs really run beside the image GEMMs, the K-slice
    workspaces of both lanes and the attention workspaces are live.  Kontext in its default 16-bit form, Klein in its fp8 form (the
    attention then writes the projections' fp8 operand).  The weights are seeded once and shared by the two builds."""
    shapes = (fx if kind == "kontext" else f2).dit_param_shapes(lh.production_cfg(kind))
    seeded, cache = fc.named_provider(shapes, "cuda:0", seed=4), {}

    def provider(name):
        if name not in cache:
            cache[name] = seeded(name)
        return cache[name]
    lh.check_production_lanes_bit_equal(hip_lib, "cuda:0", kind, provider, fp8=fp8)
    torch.cuda.empty_cache()
