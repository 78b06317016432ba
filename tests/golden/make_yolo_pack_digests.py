"""Golden for the packed detector weights: sha256 of `W` / `DW` as `YoloSegHip._pack` / `Yolo11Hip._pack` leave them for the seeded state dicts of the
simulator tests (tests/yolo11_checks.py `pack_digests`).  Recorded at the commit BEFORE the two classes shared one `_put`, so the test pins that the
shared method packs bit for bit what the two separate ones did.

    python tests/golden/make_yolo_pack_digests.py        # rewrites tests/golden/yolo_pack_digests.json
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent.parent), str(HERE.parent)]

from mangatranslator_amd.hip.lib import _open_simulator_for_tests  # noqa: E402
import yolo11_checks  # noqa: E402

lib = _open_simulator_for_tests(HERE.parent / "emu" / "libmtx_emu.so")
(HERE / "yolo_pack_digests.json").write_text(json.dumps(yolo11_checks.pack_digests(lib), indent=1) + "\n")
