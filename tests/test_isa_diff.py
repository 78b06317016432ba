"""tools/isa_diff.py, the gate for kernel refactors: a tree compared with itself is `same` everywhere, and one edited constant is found in the
kernel that holds it.  Cross-compiles quant.hip, the smallest kernel file; no GPU."""
import shutil
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "mangatranslator_amd" / "csrc"
sys.path.insert(0, str(ROOT / "tools"))


def test_isa_diff_finds_one_edited_constant(tmp_path, capsys):
    import isa_diff
    assert isa_diff.main([str(CSRC), str(CSRC), "quant.hip"]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "quant.hip:" in ln]
    assert len([ln for ln in lines if "quant_mx_kernel" in ln]) == 2 and all(ln.startswith("same") for ln in lines)      # bf16 and f16

    edited = tmp_path / "csrc"
    edited.mkdir()
    for name in ("quant.hip", "mtx_device.h", "Makefile"):
        shutil.copy(CSRC / name, edited / name)
    text = (edited / "quant.hip").read_text()
    assert text.count("1.f + __expf(-f[e])") == 1
    (edited / "quant.hip").write_text(text.replace("1.f + __expf(-f[e])", "2.f + __expf(-f[e])"))
    assert isa_diff.main([str(CSRC), str(edited), "quant.hip"]) == 1
    out = capsys.readouterr().out
    diff = [ln for ln in out.splitlines() if ln.startswith("DIFF")]
    assert len(diff) == 2 and all("quant_mx_kernel" in ln for ln in diff), out
    # the same difference, allowed by name
    assert isa_diff.main([str(CSRC), str(edited), "quant.hip", "--allow", "quant_mx_kernel"]) == 0
