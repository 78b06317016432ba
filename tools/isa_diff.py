"""Does a change to csrc/ move the generated gfx950 code?  Compiles two trees with the product Makefile's HIPFLAGS and compares the
assembly text kernel by kernel.  The gate for kernel refactors: the attention and GEMM kernels were tuned by schedule, and
sharing code between them has changed register allocation and instruction order before.  No GPU needed: hipcc cross-compiles.

    python tools/isa_diff.py A B [file.hip ...] [--allow REGEX]      # default: every .hip of tree A

A and B are csrc directories or git revisions (extracted with `git archive` into a temporary directory).  Before the comparison comment
lines and the .file / .loc / .ident directives are dropped; the text is cut at every `_Z...:` symbol (a kernel's piece holds its code, its
descriptor and its resource figures, not the preamble of the function emitted after it, so a kernel added behind it does not show) and
ends at the module's tail (the end-of-code padding, the compilation-unit id, a hash of the file's path, and the metadata).
Prints `same` or `DIFF` with both line counts per symbol.
Exit status 1 if a symbol outside --allow differs or the two trees do not define the same symbols."""
import argparse
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from isa_audit import CSRC, ROOT, compile_to_isa  # noqa: E402


def hipflags(csrc: Path):
    """HIPFLAGS of the tree's Makefile with $(ARCH) filled in.  The -I is a fallback for a bare copy of csrc/ that has no
    ../../include next to it: the quoted relative include then resolves against this repository's header."""
    text = (csrc / "Makefile").read_text()
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS := (.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    return flags + [f"-I{CSRC}"]


def tree(spec: str, td: Path, name: str) -> Path:
    if Path(spec).is_dir():
        return Path(spec).resolve()
    out = td / name
    out.mkdir()
    ar = subprocess.run(["git", "-C", str(ROOT), "archive", spec, "include", "mangatranslator_amd/csrc"], capture_output=True)
    if ar.returncode != 0:
        raise SystemExit(f"{spec}: neither a directory nor a git revision\n{ar.stderr.decode()[-500:]}")
    subprocess.run(["tar", "-x", "-C", str(out)], input=ar.stdout, check=True)
    return out / "mangatranslator_amd" / "csrc"


def symbols(asm: Path):
    """symbol -> normalised lines"""
    out, cur = {}, None
    for line in asm.read_text().splitlines():
        t = line.strip()
        if not t or t.startswith((";", ".file", ".loc", ".ident")):
            continue
        if "__hip_cuid_" in t or t.startswith(".amdgpu_metadata"):
            break
        if t.startswith(".p2alignl"):                          # the padding behind the module's last function: the tail starts here
            if cur and cur[-1] == ".text":
                cur.pop()
            break
        if re.match(r"\.section\s+\.text\.", t):               # the next function's preamble (section, visibility, alignment, type) names
            cur = None                                         # THAT function: it is no part of the piece before it
            continue
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        if cur is not None:
            cur.append(t)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a", help="csrc directory or git revision")
    ap.add_argument("b", help="csrc directory or git revision")
    ap.add_argument("sources", nargs="*", help="file names inside csrc (default: every .hip of A)")
    ap.add_argument("--allow", metavar="REGEX", help="symbols that may differ")
    args = ap.parse_args(argv)
    bad = 0
    with tempfile.TemporaryDirectory() as tds:
        td = Path(tds)
        ta, tb = tree(args.a, td, "a"), tree(args.b, td, "b")
        names = [Path(s).name for s in args.sources] or sorted(p.name for p in ta.glob("*.hip"))
        jobs = []
        for side, t in (("a", ta), ("b", tb)):
            (td / f"isa_{side}").mkdir()
            jobs += [(t / n, td / f"isa_{side}", hipflags(t)) for n in names]
        with ThreadPoolExecutor(max_workers=6) as pool:
            built = list(pool.map(lambda j: compile_to_isa(*j)[0], jobs))
        for n, asm_a, asm_b in zip(names, built[:len(names)], built[len(names):]):
            sa, sb = symbols(asm_a), symbols(asm_b)
            for k in sorted(set(sa) | set(sb)):
                if k not in sa or k not in sb:
                    print(f"DIFF {len(sa.get(k, [])):6d} {len(sb.get(k, [])):6d}  {n}: {k}  (only in {'A' if k in sa else 'B'})")
                    bad += 1
                    continue
                same = sa[k] == sb[k]
                print(f"{'same' if same else 'DIFF'} {len(sa[k]):6d} {len(sb[k]):6d}  {n}: {k}")
                if not same and not (args.allow and re.search(args.allow, k)):
                    bad += 1
    print(f"{bad} symbol(s) differ outside --allow" if bad else "no symbol differs outside --allow")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
