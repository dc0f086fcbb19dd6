"""host/image_io.hpp jpeg_coefficients (`image_dump <in> <out> coeffs`): the blob the device reconstructs keyframe JPEGs
from (pcp_jpeg_header, include/pcp_hip.h).  A numpy restatement of the device's arithmetic (tests/_jpeg_ref.py) fed from
the blob must give the host decoder's BGR and Pillow's (libjpeg-turbo) decode byte for byte.  CPU only."""
import subprocess

import numpy as np
import pytest

import _jpeg_ref as ref

PIL = pytest.importorskip("PIL.Image")


def _exe():
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    return host_build.build()["image_dump"]


def _run(path, mode=None):
    out = str(path) + (".blob" if mode == "coeffs" else ".raw")
    r = subprocess.run([_exe(), str(path), out] + ([mode] if mode else []), capture_output=True, text=True)
    if r.returncode != 0:
        return None
    return open(out, "rb").read()


def _bgr(path):
    raw = _run(path)
    head, _, body = raw.partition(b"\n")
    w, h, c = map(int, head.split())
    return np.frombuffer(body, np.uint8).reshape(h, w, c)


def _picture(h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    im = np.stack([128 + 100 * np.sin(x / 7.0 + y / 13.0), 128 + 90 * np.cos(x / 5.0 - y / 9.0),
                   128 + 80 * np.sin((x + y) / 11.0)], 2) + rng.normal(0, 12, (h, w, 3))
    return np.clip(im, 0, 255).astype(np.uint8)


def _check(path):
    """blob -> numpy restatement == image_dump BGR == Pillow; the blob's size is exactly its sections'."""
    blob = _run(path, "coeffs")
    assert blob is not None, path
    p = ref.parse(blob)
    nb, nv = p["n_blocks"], p["n_values"]
    assert p["magic"] == ref.MAGIC and p["version"] == 1
    assert int(p["offsets"][-1]) + bin(int(p["masks"][-1])).count("1") == nv
    # 12 B per block + 2 B per nonzero coefficient + the header (header, quantisation tables, 16-B alignment)
    head = p["value_off"] - 12 * nb
    assert len(blob) == head + 12 * nb + 2 * nv
    assert p["quant_off"] == ref.HEADER_BYTES and p["value_off"] % 16 == 0 and p["mask_off"] % 16 == 0
    assert 0 <= head - ref.HEADER_BYTES - 128 * p["ncomp"] < 32
    got = ref.decode_bgr(blob)
    host = _bgr(path)
    pil = np.array(PIL.open(path).convert("RGB"))[:, :, ::-1]
    assert np.array_equal(host, pil), path
    assert np.array_equal(got, host), (path, int(np.abs(got.astype(int) - host).max()))
    return p


@pytest.mark.parametrize("size", [(64, 64), (37, 53), (135, 240), (17, 9), (8, 8), (100, 3), (1, 1)])
@pytest.mark.parametrize("subsampling", [0, 1, 2])
def test_blob_reconstructs_libjpeg_pixels(tmp_path, size, subsampling):
    h, w = size
    for q in (25, 30, 75, 96, 100):
        p = tmp_path / f"t_{q}.jpg"
        PIL.fromarray(_picture(h, w, q)).save(p, quality=q, subsampling=subsampling)
        got = _check(p)
        assert got["width"] == w and got["height"] == h and got["ncomp"] == 3
        hv = {0: (1, 1), 1: (2, 1), 2: (2, 2)}[subsampling]
        assert (got["comps"][0]["h"], got["comps"][0]["v"]) == hv


def test_optimized_tables_long_codes_restart_and_grey(tmp_path):
    im = _picture(120, 200, 5)
    p = tmp_path / "opt.jpg"  # image-specific Huffman tables
    PIL.fromarray(im).save(p, quality=88, optimize=True, subsampling=2)
    _check(p)
    # white noise at q100: rare (run, size) symbols whose standard-table codes are longer than 9 bits (the bit loop)
    noise = np.random.default_rng(3).integers(0, 256, (96, 160, 3), dtype=np.uint8)
    p = tmp_path / "noise.jpg"
    PIL.fromarray(noise).save(p, quality=100, subsampling=0)
    assert _check(p)["n_values"] > 0.8 * 64 * _check(p)["n_blocks"]
    p = tmp_path / "rst.jpg"
    PIL.fromarray(im).save(p, quality=85, subsampling=2, restart_marker_blocks=3)
    _check(p)
    p = tmp_path / "grey.jpg"
    PIL.fromarray(im[:, :, 1]).save(p, quality=80)
    assert _check(p)["ncomp"] == 1


def test_long_codes_are_used(tmp_path):
    """The q100 noise image really needs codes longer than 9 bits: its AC table has them and the decode agrees."""
    noise = np.random.default_rng(4).integers(0, 256, (64, 64), dtype=np.uint8)
    p = tmp_path / "n.jpg"
    PIL.fromarray(noise).save(p, quality=100)
    data = p.read_bytes()
    # the DHT segments' code length counts: some AC table has codes of 10..16 bits
    i, longest = 2, 0
    while i < len(data) - 4:
        if data[i] == 0xFF and data[i + 1] == 0xC4:
            n = (data[i + 2] << 8) | data[i + 3]
            seg = data[i + 4:i + 2 + n]
            j = 0
            while j < len(seg):
                counts = seg[j + 1:j + 17]
                longest = max([longest] + [l + 1 for l in range(16) if counts[l]])
                j += 17 + sum(counts)
            i += 2 + n
        else:
            i += 1
    assert longest > 9
    _check(p)


def test_full_size_frame(tmp_path):
    from pointcloudprocessor_amd import synth

    p = tmp_path / "big.jpg"
    PIL.fromarray(synth.make_image(0, 4096, 3000)[:, :, ::-1]).save(p, quality=92)
    got = _check(p)
    assert got["n_blocks"] == 256 * 188 * 6  # 16x16 MCUs of 4 Y + Cb + Cr blocks


def test_refused_files(tmp_path):
    im = _picture(40, 60)
    p = tmp_path / "prog.jpg"
    PIL.fromarray(im).save(p, quality=85, progressive=True)
    assert _run(p, "coeffs") is None
    p = tmp_path / "img.png"
    PIL.fromarray(im).save(p)
    assert _run(p, "coeffs") is None
    assert np.array_equal(_bgr(p), im[:, :, ::-1])  # the BGR mode still reads it
    p = tmp_path / "png_named.jpg"
    PIL.fromarray(im).save(p, format="PNG")
    assert _run(p, "coeffs") is None and _run(p) is not None
    # truncated files: cut inside the headers, both modes refuse; cut inside the scan, both accept (the missing bits
    # decode as zeros) and give the same pixels
    p = tmp_path / "whole.jpg"
    PIL.fromarray(im).save(p, quality=85)
    data = p.read_bytes()
    p = tmp_path / "trunc_head.jpg"
    p.write_bytes(data[:200])
    assert _run(p, "coeffs") is None and _run(p) is None
    for cut in (len(data) // 2, len(data) - 10):
        p = tmp_path / f"trunc_{cut}.jpg"
        p.write_bytes(data[:cut])
        blob = _run(p, "coeffs")
        assert blob is not None and np.array_equal(ref.decode_bgr(blob), _bgr(p)), cut
