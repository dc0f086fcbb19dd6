"""What the device PCD reader must return, from two independent sources: glibc's strtof through ctypes (what
host/pcd_io.hpp's loadPCDFile calls) and the exact rounding of the decimal value with fractions.Fraction.  Shared by the CPU and
GPU suites; the large sets are computed once."""
import ctypes
import functools
import struct
from fractions import Fraction

import numpy as np

import _ascii_ref as ref

_libc = ctypes.CDLL("libc.so.6")
_libc.strtof.restype = ctypes.c_float
_libc.strtof.argtypes = [ctypes.c_char_p, ctypes.c_void_p]

XYZI = (0, 1, 2, 3)


def strtof_bits(tokens) -> np.ndarray:
    """the bit patterns strtof returns for byte-string tokens"""
    f = _libc.strtof
    return np.array([f(t, None) for t in tokens], np.float32).view(np.uint32)


def exact_bits(token: str) -> int:
    """the fp32 nearest the exact decimal value of a finite decimal token, ties to even (subnormals, overflow to inf)"""
    neg = token.lstrip().startswith("-")
    v = abs(Fraction(token))
    sign = 0x80000000 if neg else 0
    if v == 0:
        return sign
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    assert Fraction(2) ** e <= v < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    m = round(v / quantum)  # Fraction rounds half to even
    r = m * quantum
    if r >= Fraction(2) ** 128:
        return sign | 0x7F800000
    return sign | struct.unpack("<I", struct.pack("<f", float(r)))[0]


def bits_of(arrays) -> np.ndarray:
    """x y z intensity arrays of a parse, interleaved back into token order, as bit patterns"""
    return np.stack([np.asarray(a, np.float32).view(np.uint32) for a in arrays[:4]], 1).reshape(-1)


def g9(values) -> list:
    with np.errstate(invalid="ignore"):
        d = np.asarray(values, np.float32).astype(np.float64).tolist()
    return [b"nan" if v != v else (b"%.9g" % v) for v in d]


@functools.lru_cache(maxsize=None)
def value_text9() -> tuple:
    return tuple(g9(ref.value_set()))


@functools.lru_cache(maxsize=None)
def value_bits(digits: int) -> np.ndarray:
    """strtof of the writer's value set printed with 8 or 9 significant digits, padded to whole rows of four with '0'"""
    texts = ref.value_text() if digits == 8 else value_text9()
    b = strtof_bits(list(texts) + [b"0"] * (-len(texts) % 4))
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def value_rows(digits: int) -> bytes:
    return ref.float_rows_text(ref.value_text() if digits == 8 else value_text9(), 4)


@functools.lru_cache(maxsize=None)
def random_tokens(n: int = 200_000, seed: int = 77) -> tuple:
    """seeded tokens of 1 - 19 digits, a point anywhere (in front, inside, behind, none), exponents -70 .. +50, signs"""
    rng = np.random.default_rng(seed)
    nd = rng.integers(1, 20, n)
    digits = rng.integers(0, 10, (n, 19))
    point = rng.integers(-1, 21, n)  # -1 / beyond the digits: none
    exp = rng.integers(-70, 51, n)
    form = rng.integers(0, 8, n)  # 0: no exponent; odd: 'e', even: 'E'; bit 2: explicit '+'
    neg = rng.random(n) < 0.3
    out = []
    for i in range(n):
        d = "".join(map(str, digits[i, : nd[i]].tolist()))
        p = int(point[i])
        if 0 <= p <= nd[i]:
            d = d[:p] + "." + d[p:]
        e = int(exp[i])
        if form[i]:
            d += ("e" if form[i] & 1 else "E") + ("+" if e >= 0 and form[i] & 4 else "") + str(e)
        out.append(("-" if neg[i] else "").encode() + d.encode())
    return tuple(out)
