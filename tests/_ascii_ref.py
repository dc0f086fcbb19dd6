"""What the device PCD writer must print, built in Python: '%.8g' of the fp32 as a double (glibc's snprintf("%.8g") and
host/pcd_io.hpp's detail::put_float print the same bytes; every NaN is 'nan'), the rgb column as the packed word
0xff000000 | r<<16 | g<<8 | b, single spaces, one newline per row.  Shared by the CPU and GPU suites; computed once."""
import functools

import numpy as np

XYZI, XYZRGB, XYZRGBMASK, POINTNORMAL = 0, 1, 2, 3
FLOATS = {XYZI: 4, XYZRGB: 3, XYZRGBMASK: 3, POINTNORMAL: 7}
BOUND = {XYZI: 60, XYZRGB: 56, XYZRGBMASK: 62, POINTNORMAL: 105}

# ties and carries of round-half-even on the exact binary value, and what they print as
TIES = {1234567.25: "1234567.2", 1234567.75: "1234567.8", 123456.125: "123456.12", 123456.375: "123456.38",
        12345.0625: "12345.062", 12345.1875: "12345.188", 99999996.0: "1e+08", 99999992.0: "99999992",
        1e-4: "9.9999997e-05"}
EXTRA = (3000000.25, 4194303.75, 999999.125)


def g8(values) -> list:
    """the byte strings of fp32 values"""
    with np.errstate(invalid="ignore"):  # (signalling NaNs are among the values)
        d = np.asarray(values, np.float32).astype(np.float64).tolist()
    return [b"nan" if v != v else (b"%.8g" % v) for v in d]


@functools.lru_cache(maxsize=None)
def value_set() -> np.ndarray:
    """every biased exponent and both signs x mantissas {0, 1, 0x3fffff, 0x400000, 0x7fffff} + 1500 seeded random ones; the
    ties, carries, zeros, infinities, the smallest subnormal and FLT_MAX (read-only)"""
    rng = np.random.default_rng(20241008)
    mant = np.concatenate([np.tile(np.array([0, 1, 0x3FFFFF, 0x400000, 0x7FFFFF], np.uint32), (512, 1)),
                           rng.integers(0, 1 << 23, (512, 1500), dtype=np.uint32)], axis=1)
    se = (np.arange(512, dtype=np.uint32) << 23)[:, None]  # sign and exponent: bits 31..23
    grid = (se | mant).reshape(-1).view(np.float32)
    special = np.array(list(TIES) + list(EXTRA) + [0.0, -0.0, np.inf, -np.inf], np.float32)
    edge = np.array([1, 0x7F7FFFFF, 0x80000001, 0xFF7FFFFF], np.uint32).view(np.float32)
    v = np.concatenate([grid, special, edge])
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def value_text() -> tuple:
    return tuple(g8(value_set()))


def as_rows(values: np.ndarray, nf: int) -> np.ndarray:
    """values packed as rows of nf floats (zero padded)"""
    n = -(-len(values) // nf)
    f = np.zeros(n * nf, np.float32)
    f[: len(values)] = values
    return f.reshape(n, nf)


def float_rows_text(texts, nf: int) -> bytes:
    """rows of nf float columns from per-value byte strings (padded with b'0')"""
    t = list(texts) + [b"0"] * (-len(texts) % nf)
    return b"".join(b" ".join(t[i:i + nf]) + b"\n" for i in range(0, len(t), nf))


def rgb_words(rgb: np.ndarray) -> np.ndarray:
    c = np.asarray(rgb, np.uint8).reshape(-1, 3).astype(np.uint32)
    return np.uint32(0xFF000000) | (c[:, 0] << 16) | (c[:, 1] << 8) | c[:, 2]


def rows_text(kind: int, f, rgb=None, mask=None) -> bytes:
    """the text of n rows of a kind from arrays (f: n x FLOATS[kind])"""
    f = np.asarray(f, np.float32).reshape(-1, FLOATS[kind])
    cols = [g8(f[:, c]) for c in range(f.shape[1])]
    if kind in (XYZRGB, XYZRGBMASK):
        cols.append([b"%d" % w for w in rgb_words(rgb).tolist()])
    if kind == XYZRGBMASK:
        cols.append([b"%d" % m for m in np.asarray(mask).reshape(-1).tolist()])
    return b"".join(b" ".join(r) + b"\n" for r in zip(*cols))


def first_difference(got: bytes, want: bytes) -> str:
    """a message naming the first row that differs"""
    if got == want:
        return ""
    gl, wl = got.split(b"\n"), want.split(b"\n")
    for i, (a, b) in enumerate(zip(gl, wl)):
        if a != b:
            return f"row {i}: got {a!r}, want {b!r}"
    return f"{len(got)} bytes / {len(gl)} lines, want {len(want)} / {len(wl)}"


def mixed_rows(kind: int, n: int, seed: int = 5):
    """n rows whose fields mix 1-byte ('0', '5') and 14-byte ('-1.1754944e-38') values: row lengths vary by 4x inside a
    wavefront and the tiles' text starts at every residue mod 16"""
    rng = np.random.default_rng(seed + 1000 * kind + n)
    pool = np.array([0.0, 5.0, -1.1754944e-38, -3.4028235e+38, 1.5, -0.25, 1234567.25, -9.9999997e-05], np.float32)
    f = pool[rng.integers(0, len(pool), (n, FLOATS[kind]))]
    short = rng.random(n) < 0.3  # whole rows of 1-byte fields
    f[short] = pool[rng.integers(0, 2, (int(short.sum()), FLOATS[kind]))]
    rgb = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    mask = rng.choice(np.array([0, 9, 10, 255, 65535], np.uint16), n)
    return f, rgb, mask
