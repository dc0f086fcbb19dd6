"""numpy restatement of the device's JPEG reconstruction (csrc/pcp_jpeg.hip) from the coefficient blob that
`image_dump <in> <out> coeffs` writes (pcp_jpeg_header, include/pcp_hip.h): dequantisation + libjpeg's islow IDCT
(jidctint.c), fancy / box upsampling with the edge rules of jdsample.c, the jdcolor.c YCbCr->RGB tables, grey = Y.
Integer arithmetic throughout (int64 here; the values stay inside int32 for 8-bit JPEGs)."""
from __future__ import annotations

import numpy as np

MAGIC = 0x4A504350  # "PCPJ"
HEADER_BYTES = 144


def parse(blob: bytes) -> dict:
    b = np.frombuffer(blob, np.uint8)
    u32 = b[:24].view(np.uint32)
    i32 = b[:96].view(np.int32)
    i64 = b[96:144].view(np.int64)
    ncomp = int(i32[4])
    comps = [dict(zip(("h", "v", "blocks_w", "blocks_h", "down_w", "down_h"), map(int, i32[6 + 6 * c: 12 + 6 * c])))
             for c in range(ncomp)]
    n_blocks, n_values, quant_off, mask_off, offset_off, value_off = map(int, i64)
    return dict(magic=int(u32[0]), version=int(u32[1]), width=int(i32[2]), height=int(i32[3]), ncomp=ncomp, comps=comps,
                n_blocks=n_blocks, n_values=n_values, quant_off=quant_off, mask_off=mask_off, offset_off=offset_off,
                value_off=value_off,
                quant=b[quant_off:quant_off + 128 * ncomp].view(np.uint16).reshape(ncomp, 64).astype(np.int64),
                masks=b[mask_off:mask_off + 8 * n_blocks].view(np.uint64),
                offsets=b[offset_off:offset_off + 4 * n_blocks].view(np.uint32),
                values=b[value_off:value_off + 2 * n_values].view(np.int16))


def _coefficients(p: dict) -> np.ndarray:
    """(n_blocks, 64) int64, natural order, from masks + values."""
    nb = p["n_blocks"]
    bits = ((p["masks"][:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    out = np.zeros((nb, 64), np.int64)
    out[bits] = p["values"].astype(np.int64)  # row-major boolean fill = block order, natural order within a block
    return out


F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _pass(x0, x1, x2, x3, x4, x5, x6, x7):
    """One 1-D islow pass (jidctint.c), before descaling: returns the eight sums in output order."""
    z2, z3 = x2, x6
    z1 = (z2 + z3) * F_0_541
    tmp2 = z1 + z3 * (-F_1_847)
    tmp3 = z1 + z2 * F_0_765
    tmp0 = (x0 + x4) * 8192
    tmp1 = (x0 - x4) * 8192
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x7, x5, x3, x1
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F_1_175
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F_0_298, tmp1 * F_2_053, tmp2 * F_3_072, tmp3 * F_1_501
    z1, z2, z3, z4 = z1 * -F_0_899, z2 * -F_2_562, z3 * -F_1_961 + z5, z4 * -F_0_390 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def idct_blocks(coef: np.ndarray, quant: np.ndarray) -> np.ndarray:
    """(nb, 64) coefficients, (nb, 64) quantisers -> (nb, 8, 8) uint8 samples."""
    d = (coef * quant).reshape(-1, 8, 8)  # [block, row(v), col(u)]
    cols = _pass(*[d[:, r, :] for r in range(8)])  # per column: 8 outputs (rows)
    ws = np.stack([_descale(v, 11) for v in cols], 1)  # [block, row, col]
    rows = _pass(*[ws[:, :, c] for c in range(8)])  # per row: 8 outputs (columns)
    px = np.stack([_descale(v, 18) + 128 for v in rows], 2)
    return np.clip(px, 0, 255).astype(np.uint8)


def planes(p: dict) -> list:
    ncomp, comps = p["ncomp"], p["comps"]
    hmax = max(c["h"] for c in comps)
    vmax = max(c["v"] for c in comps)
    w, h = p["width"], p["height"]
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    # decode order: MCU row, MCU, component, v, h
    comp_of, by_of, bx_of = [], [], []
    for c in range(ncomp):
        for by in range(comps[c]["v"]):
            for bx in range(comps[c]["h"]):
                comp_of.append(c), by_of.append(by), bx_of.append(bx)
    per = len(comp_of)
    assert p["n_blocks"] == mcux * mcuy * per
    m = np.arange(p["n_blocks"]) // per
    r = np.arange(p["n_blocks"]) % per
    comp_of, by_of, bx_of = np.array(comp_of)[r], np.array(by_of)[r], np.array(bx_of)[r]
    my, mx = m // mcux, m % mcux
    px = idct_blocks(_coefficients(p), p["quant"][comp_of])
    out = []
    for c in range(ncomp):
        cc = comps[c]
        pl = np.zeros((cc["blocks_h"] * 8, cc["blocks_w"] * 8), np.uint8)
        sel = comp_of == c
        brow = my[sel] * cc["v"] + by_of[sel]
        bcol = mx[sel] * cc["h"] + bx_of[sel]
        pl.reshape(cc["blocks_h"], 8, cc["blocks_w"], 8)[brow, :, bcol, :] = px[sel]
        out.append(pl)
    return out


def upsample(p: dict, c: int, pl: np.ndarray) -> np.ndarray:
    comps = p["comps"]
    hmax = max(x["h"] for x in comps)
    vmax = max(x["v"] for x in comps)
    w, h = p["width"], p["height"]
    cc = comps[c]
    dw, dh = cc["down_w"], cc["down_h"]
    if cc["h"] == hmax and cc["v"] == vmax:
        return pl[:h, :w].copy()
    x = np.arange(w)
    i = x >> 1
    odd = (x & 1) == 1
    if cc["h"] * 2 == hmax and cc["v"] == vmax:  # h2v1
        rows = pl[:h].astype(np.int64)
        if dw <= 2:
            return rows[:, i].astype(np.uint8)
        cur = rows[:, i] * 3
        left = rows[:, np.maximum(i - 1, 0)]
        right = rows[:, np.minimum(i + 1, dw - 1)]
        v = np.where(odd, (cur + right + 2) >> 2, (cur + left + 1) >> 2)
        v = np.where(~odd & (i == 0), rows[:, 0:1], v)
        v = np.where(odd & (i == dw - 1), rows[:, dw - 1:dw], v)
        return v.astype(np.uint8)
    assert cc["h"] * 2 == hmax and cc["v"] * 2 == vmax  # h2v2
    y = np.arange(h)
    r = y >> 1
    if dw <= 2:
        return pl[r][:, i].astype(np.uint8)
    rn = np.where((y & 1) == 0, np.maximum(r - 1, 0), np.minimum(r + 1, dh - 1))
    cs = pl[r].astype(np.int64) * 3 + pl[rn].astype(np.int64)  # column sums, (h, blocks_w * 8)
    cur = cs[:, i]
    left = cs[:, np.maximum(i - 1, 0)]
    right = cs[:, np.minimum(i + 1, dw - 1)]
    v = np.where(odd, (cur * 3 + right + 7) >> 4, (cur * 3 + left + 8) >> 4)
    v = np.where(~odd & (i == 0), (cur * 4 + 8) >> 4, v)
    v = np.where(odd & (i == dw - 1), (cur * 4 + 7) >> 4, v)
    return v.astype(np.uint8)


def decode_bgr(blob: bytes) -> np.ndarray:
    """(H, W, 3) BGR, as cv::imread / image_io.hpp's read_image_bgr."""
    p = parse(blob)
    assert p["magic"] == MAGIC and p["version"] == 1
    pls = planes(p)
    Y = upsample(p, 0, pls[0]).astype(np.int64)
    if p["ncomp"] == 1:
        return np.repeat(Y.astype(np.uint8)[:, :, None], 3, axis=2)
    cb = upsample(p, 1, pls[1]).astype(np.int64) - 128
    cr = upsample(p, 2, pls[2]).astype(np.int64) - 128
    r = Y + ((91881 * cr + 32768) >> 16)
    g = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], 2), 0, 255).astype(np.uint8)
