"""§8(f)2 output formats: P3 exactly as the reference prints it, P6, and the reader for
the committed UTF-16LE/CRLF image.ppm."""
import gzip
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from raytracingproject_amd import ppm

GOLDEN = Path(__file__).resolve().parent / "golden"


def golden_rgb():
    raw = gzip.open(GOLDEN / "image_ref_p6.ppm.gz").read()
    return ppm.read_ppm(raw)


def test_p3_of_golden_pixels_is_the_reference_stdout():
    ref = json.loads((GOLDEN / "image_ref.json").read_text())
    assert hashlib.sha256(ppm.p3_bytes(golden_rgb())).hexdigest() == ref["sha256_lf_ascii"]


def test_utf16_crlf_roundtrip():
    rgb = golden_rgb()[:7, :9]
    text = ppm.p3_bytes(rgb).decode().replace("\n", "\r\n")
    windows = b"\xff\xfe" + text.encode("utf-16-le")          # what PowerShell '>' wrote
    assert np.array_equal(ppm.read_ppm(windows), rgb)
    assert ppm.normalize_text(windows) == ppm.p3_bytes(rgb)


def test_p6_roundtrip_and_nan_guard(tmp_path):
    rgb = golden_rgb()
    ppm.write_p6(tmp_path / "a.ppm", rgb)
    assert np.array_equal(ppm.read_ppm((tmp_path / "a.ppm").read_bytes()), rgb)
    bad = rgb.copy()
    bad[0, 0, 0] = -2147483648
    with pytest.raises(ValueError):
        ppm.p6_bytes(bad)
    assert b"-2147483648 " in ppm.p3_bytes(bad[:1, :1])


def test_reference_image_if_present():
    # the reference's committed image, byte for byte (tests/golden/make_golden.py stores it)
    raw = gzip.open(GOLDEN / "image_ref_utf16.ppm.gz").read()
    assert raw[:2] == b"\xff\xfe" and b"\r\x00\n\x00" in raw[:64]
    assert np.array_equal(ppm.read_ppm(raw), golden_rgb())
