"""CPU tier: under `integration.install(osb_payload=True)` the module served as `core.outside_text_processor` hands the reference's
unchanged `process_outside_text(...)` call the translation payload of the outside-bubble text; under plain `install()`
it returns `(page, [])` as before.  Each case runs in a fresh interpreter (tests/osb_integration_child.py): `install()` refuses to run
once `core` is imported.  Neither needs the reference."""
import json
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
GOLD = json.loads((HERE / "golden" / "osb_payload.json").read_text())


def run_child(mode, lib):
    r = subprocess.run([sys.executable, str(HERE / "osb_integration_child.py"), mode, str(lib.path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_installed_module_builds_the_payload(emu_lib):
    out = run_child("payload", emu_lib)
    gold = GOLD["flux"]["data"]
    assert out["served"] and out["calls"] == len(GOLD["flux"]["calls"])
    assert len(out["data"]) == len(gold) > 0
    assert [d["bbox"] for d in out["data"]] == [g["bbox"] for g in gold]
    assert [d["text_color_rgb"] for d in out["data"]] == [g["text_color_rgb"] for g in gold]
    assert all(d["mime_type"] == "image/png" and d["b64"] > 0 and min(d["crop"]) > 0 for d in out["data"])


def test_plain_install_keeps_the_vision_only_result(emu_lib):
    out = run_child("plain", emu_lib)
    assert out["served"] and out["data"] == [] and out["calls"] == len(GOLD["flux"]["calls"])
