"""CPU tier: the host half of the page stage — csrc/host_contours.cpp and csrc/host_png.cpp, raw-buffer C++ — under AddressSanitizer and
UndefinedBehaviorSanitizer.  tests/host/host_stage_main.cpp (a stand-alone program with its own `main`) is compiled together with the two
sources by the project's host compiler and run as a child process on a case file written here from authored and seeded data; every buffer
it hands over is a heap block of exactly the size the callee may touch.  Its results are compared with the oracle (oracle/cleaning_ref.py),
the PNG files are decoded with Pillow.  Nothing is loaded into this process and `LD_PRELOAD` is left alone.

Leak checking is switched off in the child: LeakSanitizer stops the process through ptrace, which test machines may deny; the two sources
own memory through containers only."""
import io
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

from oracle import cleaning_ref as cr

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "mangatranslator_amd" / "csrc"
OP_TEXT_MASK, OP_FILL, OP_OUTLINE, OP_CHAMFER, OP_PNG = 1, 2, 3, 4, 5


def _host_compiler():
    """the Makefile's CLANGXX (csrc/Makefile), else whatever C++ compiler the machine has"""
    for cand in (os.environ.get("CLANGXX"), "/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if cand and (os.path.isfile(cand) or shutil.which(cand)):
            return cand
    pytest.fail("no host C++ compiler found")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("host_stage") / "host_stage_main"
    cxx = _host_compiler()
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan" if os.path.basename(cxx).startswith("g++") else "-static-libsan",
           str(ROOT / "tests" / "host" / "host_stage_main.cpp"), str(CSRC / "host_contours.cpp"), str(CSRC / "host_png.cpp"), "-o", str(exe), "-lz", "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "building the sanitized host program failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr
    return exe


def _run(program, tmp_path, records: bytes) -> bytes:
    case, result = tmp_path / "cases.bin", tmp_path / "results.bin"
    case.write_bytes(records)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = ":".join(v for v in (env.get("ASAN_OPTIONS"), "detect_leaks=0", "abort_on_error=0") if v)
    env["UBSAN_OPTIONS"] = ":".join(v for v in (env.get("UBSAN_OPTIONS"), "print_stacktrace=1") if v)
    r = subprocess.run([str(program), str(case), str(result)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, f"the sanitized host program ended with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    return result.read_bytes()


class _Results:
    def __init__(self, data):
        self.data, self.at = data, 0

    def take(self, fmt):
        v = struct.unpack_from("<" + fmt, self.data, self.at)
        self.at += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def array(self, dtype, n):
        a = np.frombuffer(self.data, dtype, n, self.at)
        self.at += a.nbytes
        return a


# ---- contour functions ------------------------------------------------------------------------------------------------------------
def _images():
    """(name, 0 / 255 image) — the shapes a border walk, a flood fill and a padded raster pass can get wrong"""
    out = [("1 x 1 set", np.full((1, 1), 255)), ("1 x 1 empty", np.zeros((1, 1))), ("1 x 9 set", np.full((1, 9), 255)),
           ("1 x 9 alternating", (np.arange(9)[None, :] % 2 == 0) * 255), ("1 x 9 two runs", np.array([[255, 255, 255, 0, 0, 255, 255, 255, 255]])),
           ("9 x 1 set", np.full((9, 1), 255)), ("9 x 1 alternating", (np.arange(9)[:, None] % 2 == 0) * 255), ("all set", np.full((12, 10), 255))]
    b = np.zeros((20, 24))
    b[0:4, 0:4] = b[0:3, 20:24] = b[16:20, 0:3] = b[17:20, 21:24] = 255                      # every corner
    b[0:3, 9:14] = b[17:20, 8:15] = b[8:12, 0:3] = b[7:13, 21:24] = 255                      # every border
    b[7:13, 8:16] = 255
    out.append(("blobs on every border and corner", b))
    out.append(("diagonal chain", np.eye(12) * 255))
    d = np.zeros((9, 15)); d[4, 2:13] = 255
    out.append(("1-px stroke", d))
    ring = np.zeros((16, 18)); ring[2:14, 3:15] = 255; ring[5:11, 6:12] = 0
    out.append(("blob with a hole", ring))
    nested = np.zeros((24, 24)); nested[1:23, 1:23] = 255; nested[4:20, 4:20] = 0; nested[7:17, 7:17] = 255; nested[10:14, 10:14] = 0; nested[11:13, 11:13] = 255
    out.append(("nested rings", nested))
    rng = np.random.default_rng(81)
    for k, density in enumerate(np.linspace(0.1, 0.9, 20)):
        out.append((f"noise {k} at density {density:.2f}", (rng.random((40, 48)) < density) * 255))
    return [(name, np.ascontiguousarray(img, dtype=np.uint8)) for name, img in out]


def _want_text_mask(img, ero, ox, oy, pw, ph, min_area):
    """the contour half of oracle/cleaning_ref.process_single_bubble on a crop at page offset (ox, oy)"""
    h, w = img.shape
    valid = []
    for c in cr.find_external_contours(img):
        cen = cr.contour_centroid(c)
        if not cr.contour_area(c) > min_area or cen is None:
            continue
        cx, cy = cen
        if 0 <= cx + ox < pw and 0 <= cy + oy < ph and 0 <= cx < w and 0 <= cy < h and ero[cy, cx] == 255:
            valid.append(c)
    if not valid:
        return 0, np.zeros_like(img), (-77,) * 4
    largest = max(cr.find_external_contours(cr.draw_filled(valid, img.shape)), key=cr.contour_area)
    x, y, bw, bh = cr.bounding_rect(largest)
    return len(valid), cr.draw_filled([largest], img.shape), (x + ox, y + oy, bw, bh)


def _want_outline(img):
    """ultralytics' largest polygon: the blob with the most border points, the first of them in raster order"""
    blobs = cr.find_external_contours(img)[::-1]
    if not blobs:
        return np.zeros((0, 2), np.int32)
    best = blobs[0]
    for c in blobs[1:]:
        if len(c) > len(best):
            best = c
    return best.astype(np.int32)


def test_contour_functions_under_sanitizers(program, tmp_path):
    records, expect = [], []
    k3 = np.ones((3, 3), np.uint8)
    for name, img in _images():
        h, w = img.shape
        outline = _want_outline(img)
        records.append(struct.pack("<iii", OP_CHAMFER, w, h) + img.tobytes())
        expect.append(("chamfer", name, img, None))
        for min_area in (0.0, 4.0):
            records.append(struct.pack("<iiid", OP_FILL, w, h, min_area) + img.tobytes())
            expect.append(("fill", name, img, min_area))
        for cap in sorted({0, max(len(outline) - 1, 0), len(outline), len(outline) + 3}):         # nothing, one short, exact, generous
            records.append(struct.pack("<iiii", OP_OUTLINE, w, h, cap) + img.tobytes())
            expect.append(("outline", name, outline, cap))
        full = np.full_like(img, 255)
        # offsets (3, 4) on a wide page; the constraint mask eroded; a centroid pushed off the page to the left and to the right
        for ero, ox, oy, pw, ph, min_area in ((full, 3, 4, 100, 100, 6.0), (full, 3, 4, 100, 100, -1.0), (cr.erode(img, k3), 0, 0, w, h, 0.0),
                                              (full, -w, 0, 100, 100, 0.0), (full, 100, 2, 100, 100, 0.0), (full, 0, 0, w, h, 50.0)):
            records.append(struct.pack("<iiiiiiid", OP_TEXT_MASK, w, h, ox, oy, pw, ph, min_area) + img.tobytes() + np.ascontiguousarray(ero).tobytes())
            expect.append(("text_mask", name, img, (ero, ox, oy, pw, ph, min_area)))
    res = _Results(_run(program, tmp_path, b"".join(records)))
    counts = {"valid fragments": 0, "off-page rejections": 0}
    for kind, name, img, arg in expect:
        rc = res.take("i")
        if kind == "chamfer":
            got = res.array(np.float32, img.size).reshape(img.shape)
            want = cr.distance_transform_l2_5x5(img)
            assert rc == 0 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"chamfer, {name}"
        elif kind == "fill":
            got = res.array(np.uint8, img.size).reshape(img.shape)
            want, drawn = np.zeros_like(img), 0
            for c in cr.find_external_contours(img):
                if cr.contour_area(c) >= arg:
                    want |= cr.draw_filled([c], img.shape)
                    drawn += 1
            assert rc == drawn and np.array_equal(got, want), f"fill_components (min area {arg}), {name}: {rc} drawn, wanted {drawn}"
        elif kind == "outline":
            got = res.array(np.int32, 2 * arg).reshape(-1, 2)
            n = min(arg, len(img))
            assert rc == len(img), f"mask_outline, {name}: {rc} points, wanted {len(img)}"
            assert np.array_equal(got[:n], img[:n]) and (got[n:] == -77).all(), f"mask_outline with room for {arg}, {name}"
        else:
            ero, ox, oy, pw, ph, min_area = arg
            got = res.array(np.uint8, img.size).reshape(img.shape)
            bbox = tuple(int(v) for v in res.array(np.int32, 4))
            n, want, want_bbox = _want_text_mask(img, ero, ox, oy, pw, ph, min_area)
            assert rc == n and np.array_equal(got, want) and bbox == want_bbox, f"text_mask {arg[1:]}, {name}: {rc} fragments / {bbox}, wanted {n} / {want_bbox}"
            counts["valid fragments"] += n
            if ox in (-img.shape[1], 100):
                assert n == 0, "the shifted centroid must land outside the page"
                counts["off-page rejections"] += int(_want_text_mask(img, ero, 0, 0, img.shape[1], img.shape[0], min_area)[0] > 0)
    assert res.at == len(res.data)
    assert counts["valid fragments"] > 40 and counts["off-page rejections"] > 20, counts


# ---- PNG writer -------------------------------------------------------------------------------------------------------------------
def _png_cases():
    """(w, h, channels, level, threads, reduce, pixels, tag): 1 x 1, 1 x 5000, 5000 x 1, 3 x 2 and 513 x 257 (two deflate stripes on five
    threads); 1 to 4 channels; images that reduce (grey RGB, opaque alpha) and that do not; reduce on and off; 1 and 5 threads"""
    rng = np.random.default_rng(91)
    cases = []
    for w, h in ((1, 1), (1, 5000), (5000, 1), (3, 2), (513, 257)):
        yy, xx = np.mgrid[0:h, 0:w]
        smooth = ((xx * 3 + yy * 5) % 256).astype(np.uint8)
        for c in (1, 2, 3, 4):
            variants = {"plain": np.stack([np.roll(smooth, k, axis=1) ^ rng.integers(0, 4, (h, w), dtype=np.uint8) for k in range(c)], -1)}
            if c >= 3:
                g = variants["plain"].copy(); g[..., 1] = g[..., 0]; g[..., 2] = g[..., 0]
                variants["grey"] = g
            if c in (2, 4):
                for name in list(variants):
                    o = variants[name].copy(); o[..., c - 1] = 255
                    variants[name + ", opaque"] = o
            for name, px in variants.items():
                if c >= 3 and name.startswith("plain") and w * h > 1:
                    px[-1, -1, 1] = px[-1, -1, 0] ^ 1                                 # never grey by accident
                if c in (2, 4) and "opaque" not in name:
                    px[0, 0, c - 1] = 254
                for reduce in (0, 1):
                    for threads in (1, 5):
                        cases.append((w, h, c, 2, threads, reduce, np.ascontiguousarray(px), f"{w} x {h} x {c} {name}, reduce {reduce}, {threads} threads"))
    w, h = 513, 257
    px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for level in (0, 9):
        cases.append((w, h, 3, level, 5, 1, px, f"{w} x {h} x 3 noise, level {level}"))
    return cases


def _reduced(px, reduce):
    """the pixels and Pillow mode a reader must see"""
    c = px.shape[2]
    if reduce:
        if c in (2, 4) and (px[..., c - 1] == 255).all():
            px, c = px[..., :c - 1], c - 1
        if c >= 3 and (px[..., 0] == px[..., 1]).all() and (px[..., 1] == px[..., 2]).all():
            px = np.concatenate([px[..., :1], px[..., 3:]], -1)
            c = px.shape[2]
    return px, {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[c]


def test_png_encoder_under_sanitizers(program, tmp_path):
    cases = _png_cases()
    records = [struct.pack("<iiiiiii", OP_PNG, w, h, c, level, threads, reduce) + px.tobytes() for w, h, c, level, threads, reduce, px, _ in cases]
    res = _Results(_run(program, tmp_path, b"".join(records)))
    modes = set()
    for w, h, c, level, threads, reduce, px, tag in cases:
        size = res.take("q")
        assert size > 0, f"{tag}: size query returned {size}"
        rc_exact = res.take("q")
        data = bytes(res.array(np.uint8, size))
        rc_short, untouched = res.take("qi")
        assert rc_exact == size, f"{tag}: exact capacity returned {rc_exact}, the size query {size}"
        assert rc_short == size and untouched == 1, f"{tag}: a buffer one byte short returned {rc_short} and was {'left alone' if untouched else 'written'}"
        im = Image.open(io.BytesIO(data))
        im.load()
        want, mode = _reduced(px, reduce)
        assert im.mode == mode and im.size == (w, h), f"{tag}: decoded as {im.mode} {im.size}, wanted {mode}"
        assert np.array_equal(np.asarray(im).reshape(want.shape), want), f"{tag}: decoded pixels differ"
        modes.add((c, mode))
    assert res.at == len(res.data)
    assert modes == {(1, "L"), (2, "LA"), (2, "L"), (3, "RGB"), (3, "L"), (4, "RGBA"), (4, "RGB"), (4, "LA"), (4, "L")}, modes
