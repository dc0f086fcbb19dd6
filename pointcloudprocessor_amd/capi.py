"""ctypes binding of include/pcp_hip.h (libpcp_hip.so).

This is the Python view of the drop-in boundary used by tests and bench.py; the
C++ host shim (pointcloudprocessor_amd/host/) binds the same symbols.  There is
no fallback: if the library is missing or no GPU is usable, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

from . import _build

# error classes (pcp_hip.h)
PCP_OK = 0
PCP_ERR_INVALID = -1
PCP_ERR_STATE = -2
PCP_ERR_DEVICE = -3
PCP_ERR_NOMEM = -4
PCP_ERR_RANGE = -5

NID_EVAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                          C.POINTER(C.c_int32))
K_PROJECT, K_DEPTH, K_COLOUR, K_VISIBILITY, K_MLS_GRID, K_MLS_FIT, K_MISC, K_SOR, K_MLS_VOXEL, K_TILE_MASK, K_NID, K_HPR = range(12)
K_COLOUR_SMOOTH = 12
K_COUNT = 13


class PcpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"pcp error {code}: {msg}")
        self.code = code


class Pose(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("x", "y", "z", "qw", "qx", "qy", "qz")]


class Camera(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")] + [
        (k, C.c_int32) for k in ("image_width", "image_height", "cull_width", "cull_height")
    ]


class CullParams(C.Structure):
    _fields_ = [
        ("enable_depth_buffer_culling", C.c_int32),
        ("downsample_factor", C.c_int32),
        ("depth_slack", C.c_double),
        ("cull_mode", C.c_int32),   # CULL_ZBUFFER / CULL_HPR_CANDIDATES / CULL_HPR
        ("match_mode", C.c_int32),  # MATCH_IDENTITY / MATCH_ROUNDTRIP / MATCH_RADIUS
        ("hpr_flip_radius", C.c_double),  # hidden_points_removal_max_z, view_culling.hpp:14
    ]


CULL_ZBUFFER, CULL_HPR_CANDIDATES, CULL_HPR = 0, 1, 2
MATCH_IDENTITY, MATCH_ROUNDTRIP = 0, 1
# the reference's whole match-back: every map point within 1e-5 m of a sample's world position receives it
# (PointCloudProcessor.cpp:480-482,571-592); whole-map contexts only (pcp_hip.h PCP_MATCH_RADIUS)
MATCH_RADIUS = 2


# MLSParams.upsampling (pcp_hip.h PCP_UPSAMPLING_*: this library's codes, not the reference enum's positions)
UPSAMPLING_NONE = 0
UPSAMPLING_SAMPLE_LOCAL_PLANE = 1
UPSAMPLING_VOXEL_GRID_DILATION = 3
# SAMPLE_LOCAL_PLANE tables: radius / step <= MLS_SLP_MAX_RATIO (pcp_set_mls_local_plane)
MLS_SLP_MAX_RATIO = 512


class MLSParams(C.Structure):
    _fields_ = [
        ("search_radius", C.c_double),
        ("sqr_gauss_param", C.c_double),
        ("polynomial_order", C.c_int32),
        ("compute_normals", C.c_int32),
        ("upsampling", C.c_int32),
        ("vgd_iterations", C.c_int32),
        ("vgd_voxel_size", C.c_float),
        ("sor_mean_k", C.c_int32),
        ("sor_std_mul", C.c_double),
    ]


def declared_symbols() -> list[str]:
    """Every function include/pcp_hip.h declares (parsed from the header)."""
    with open(os.path.join(_build.INCLUDE, "pcp_hip.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pcp_[a-z0-9_]+)\s*\(", text)))


_lib = None


def load(build_if_needed: bool = True) -> C.CDLL:
    """dlopen libpcp_hip.so (building it in-tree first when stale)."""
    global _lib
    if _lib is not None:
        return _lib
    if build_if_needed:
        try:
            _build.build()
        except Exception:
            if not os.path.exists(_build.LIB_PATH):
                raise
    if not os.path.exists(_build.LIB_PATH):
        raise PcpError(PCP_ERR_DEVICE, f"{_build.LIB_PATH} is missing: the HIP extension is not built")
    # One HIP runtime per process: torch ships its own libamdhip64.so.7 and must initialise it
    # before another copy of the same SONAME is mapped (otherwise torch later reports "No HIP
    # GPUs are available").  Importing torch first makes libpcp_hip.so bind to torch's copy.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    # PCP_HIP_LIBRARY: an alternative build of the same ABI (kernel experiments); never a CPU stand-in
    L = C.CDLL(os.environ.get("PCP_HIP_LIBRARY") or _build.LIB_PATH)
    L.pcp_last_error.restype = C.c_char_p
    L.pcp_last_error.argtypes = [C.c_void_p]
    L.pcp_kernel_name.restype = C.c_char_p
    L.pcp_cloud_size.restype = C.c_int64
    L.pcp_sor_chunk_points.restype = C.c_int64
    L.pcp_sor_chunk_points.argtypes = []
    L.pcp_cloud_size.argtypes = [C.c_void_p]
    L.pcp_frame_count.restype = C.c_int32
    L.pcp_frame_count.argtypes = [C.c_void_p]
    L.pcp_destroy.restype = None
    L.pcp_destroy.argtypes = [C.c_void_p]
    for name in ("pcp_default_camera", "pcp_default_cull_params", "pcp_default_mls_params", "pcp_default_balance_params"):
        getattr(L, name).restype = None
    _lib = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def mls_local_plane_samples(radius: float, step: float):
    """(u, v) float32 arrays of the SAMPLE_LOCAL_PLANE table for (radius, step) in emission order
    (pcp_mls_local_plane_samples: host only, no GPU)."""
    L = load()
    n = C.c_int64()
    rc = L.pcp_mls_local_plane_samples(C.c_double(radius), C.c_double(step), C.c_int64(0), None, None, C.byref(n))
    if rc != PCP_OK:
        raise PcpError(rc, f"pcp_mls_local_plane_samples: radius {radius!r}, step {step!r} refused")
    u = np.empty(n.value, np.float32)
    v = np.empty(n.value, np.float32)
    rc = L.pcp_mls_local_plane_samples(C.c_double(radius), C.c_double(step), C.c_int64(n.value), _ptr(u), _ptr(v), C.byref(n))
    if rc != PCP_OK:
        raise PcpError(rc, "pcp_mls_local_plane_samples failed")
    return u, v


# row kinds of the device PCD writer (pcp_ascii_rows*)
ROWS_XYZI, ROWS_XYZRGB, ROWS_XYZRGBMASK, ROWS_POINTNORMAL = 0, 1, 2, 3
_ROW_FLOATS = {ROWS_XYZI: 4, ROWS_XYZRGB: 3, ROWS_XYZRGBMASK: 3, ROWS_POINTNORMAL: 7}


def ascii_row_bound(kind: int) -> int:
    """Longest row of a kind in bytes, newline included; negative for an unknown kind (pcp_ascii_row_bound)."""
    L = load()
    L.pcp_ascii_row_bound.restype = C.c_int64
    return int(L.pcp_ascii_row_bound(C.c_int32(kind)))


def _ascii_rows_args(kind: int, f, rgb, mask):
    nf = _ROW_FLOATS.get(kind, 1)
    f = np.ascontiguousarray(f, np.float32).reshape(-1, nf)
    rgb = None if rgb is None else np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    mask = None if mask is None else np.ascontiguousarray(mask, np.uint16).reshape(-1)
    return f, rgb, mask


def _ascii_rows_call(fn, check, kind, f, rgb, mask, capacity, out):
    """Shared by the host and device forms: returns the text as a numpy.uint8 array.  capacity None sizes the buffer by the
    row bound; out: a caller's uint8 buffer to fill instead (its size is the capacity).  A failure raises PcpError whose
    `bytes` is the exact byte count the call reported."""
    f, rgb, mask = _ascii_rows_args(kind, f, rgb, mask)
    n = f.shape[0]
    if out is None:
        cap = max(0, n * ascii_row_bound(kind)) if capacity is None else capacity
        out = np.empty(max(cap, 0), np.uint8)
    else:
        cap = out.size if capacity is None else capacity
    nbytes = C.c_int64(-1)
    try:
        check(fn(C.c_int32(kind), C.c_int64(n), _ptr(f), _ptr(rgb), _ptr(mask), C.c_int64(cap), _ptr(out), C.byref(nbytes)))
    except PcpError as e:
        e.bytes = nbytes.value
        raise
    return out[: nbytes.value]


def ascii_rows_host(kind: int, f, rgb=None, mask=None, capacity: int | None = None, out=None) -> np.ndarray:
    """PCD ASCII rows formatted on the CPU by the formatter the kernels use (pcp_ascii_rows_host: no context, no GPU).
    f: n rows of 4 | 3 | 3 | 7 floats, rgb n x 3 bytes, mask n uint16."""
    L = load()

    def check(rc):
        if rc != PCP_OK:
            raise PcpError(rc, L.pcp_last_error(None).decode())

    return _ascii_rows_call(L.pcp_ascii_rows_host, check, kind, f, rgb, mask, capacity, out)


# sizes of the device PCD reader (pcp_ascii_parse_limit)
PARSE_LIMIT_ROW, PARSE_LIMIT_TILE, PARSE_LIMIT_PIECE, PARSE_LIMIT_TILE_ROWS, PARSE_LIMIT_WINDOW = 0, 1, 2, 3, 4


def ascii_parse_limit(which: int) -> int:
    """A size the device PCD reader works with (pcp_ascii_parse_limit): the longest row, the LDS staging tile, the upload piece,
    the rows per workgroup, the longest window; negative for an unknown one."""
    L = load()
    L.pcp_ascii_parse_limit.restype = C.c_int64
    return int(L.pcp_ascii_parse_limit(C.c_int32(which)))


def _ascii_parse_call(fn, check, text, columns, col, final, max_rows, out):
    """Shared by the host and device forms: (x, y, z, intensity, consumed, bad_row), the arrays cut to the rows parsed.
    text: bytes or a uint8 array.  max_rows None: every row of the window.  out: four caller's float32 arrays (of max_rows
    entries or more) to fill instead of fresh ones."""
    buf = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text, np.uint8).reshape(-1)
    if max_rows is None:
        max_rows = int(np.count_nonzero(buf == 10)) + 1
    if out is None:
        out = tuple(np.empty(max(max_rows, 0), np.float32) for _ in range(4))
    carr = None if col is None else (C.c_int32 * 4)(*[int(c) for c in col])
    rows, consumed, bad = C.c_int64(-1), C.c_int64(-1), C.c_int64(-2)
    check(fn(_ptr(buf) if buf.size else None, C.c_int64(buf.size), C.c_int32(columns), carr, C.c_int32(1 if final else 0), C.c_int64(max_rows),
             _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), C.byref(rows), C.byref(consumed), C.byref(bad)))
    n = rows.value
    return out[0][:n], out[1][:n], out[2][:n], out[3][:n], consumed.value, bad.value


def ascii_parse_host(text, columns: int, col, final: bool = True, max_rows: int | None = None, out=None):
    """PCD ASCII rows parsed on the CPU by the parser the kernels use (pcp_ascii_parse_host: no context, no GPU).
    columns: scalars per row; col: the 0-based columns of x, y, z, intensity (-1: no intensity, 0.0)."""
    L = load()

    def check(rc):
        if rc != PCP_OK:
            raise PcpError(rc, L.pcp_last_error(None).decode())

    return _ascii_parse_call(L.pcp_ascii_parse_host, check, text, columns, col, final, max_rows, out)


def exposure_gains(n, sum, sigma_n: float = 10.0, sigma_g: float = 0.1) -> np.ndarray:
    """One exposure gain per keyframe from the pair matrices of Context.view_pair_stats (pcp_exposure_gains: host only, no
    context, no GPU).  n, sum: (F, F) uint64.  Keyframes without a pair get exactly 1.0."""
    L = load()
    n = np.ascontiguousarray(n, np.uint64)
    sum = np.ascontiguousarray(sum, np.uint64)
    if n.ndim != 2 or n.shape[0] != n.shape[1] or sum.shape != n.shape:
        raise ValueError(f"exposure_gains: two square matrices of one size expected, got {n.shape} and {sum.shape}")
    out = np.empty(n.shape[0], np.float64)
    rc = L.pcp_exposure_gains(C.c_int32(n.shape[0]), _ptr(n), _ptr(sum), C.c_double(sigma_n), C.c_double(sigma_g), _ptr(out))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return out


def voxel_reduce_host(leaf: float, xyz, rgb, label=None, capacity: int | None = None) -> dict:
    """The voxel-grid output of n coloured rows computed on the CPU by the arithmetic the kernels use (pcp_voxel_reduce_host:
    no context, no GPU; DESIGN.md "Voxel-grid output").  xyz (n, 3) float32, rgb (n, 3) uint8, label n uint8 or None:
    dict(xyz, rgb[, label], count, voxels), one row per occupied voxel in key order; voxels is the true count even when
    capacity is smaller."""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    label = None if label is None else np.ascontiguousarray(label, np.uint8).reshape(-1)
    n = xyz.shape[0]
    if rgb.shape[0] != n or (label is not None and label.shape[0] != n):
        raise ValueError("voxel_reduce_host: xyz, rgb and label differ in their number of rows")
    cap = n if capacity is None else capacity
    oxyz = np.empty((max(cap, 0), 3), np.float32)
    orgb = np.empty((max(cap, 0), 3), np.uint8)
    olab = np.empty(max(cap, 0), np.uint8) if label is not None else None
    ocnt = np.empty(max(cap, 0), np.uint32)
    vox = C.c_int64()
    rc = L.pcp_voxel_reduce_host(C.c_float(leaf), C.c_int64(n), _ptr(xyz), _ptr(rgb), _ptr(label), C.c_int64(cap), _ptr(oxyz), _ptr(orgb),
                                 _ptr(olab), _ptr(ocnt), C.byref(vox))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    m = min(vox.value, cap)
    out = dict(xyz=oxyz[:m], rgb=orgb[:m], count=ocnt[:m], voxels=vox.value)
    if label is not None:
        out["label"] = olab[:m]
    return out


class OrthoFrame(C.Structure):
    """pcp_ortho_frame: origin, axes u (image x) / v (image y, down) / n (viewing direction), metres per pixel, raster size
    and depth window of an orthographic map ("Orthographic maps", OM1)."""
    _fields_ = [("o", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3), ("n", C.c_float * 3), ("gsd", C.c_float),
                ("width", C.c_int32), ("height", C.c_int32), ("d_min", C.c_float), ("d_max", C.c_float)]

    def as_dict(self) -> dict:
        return dict(o=[float(x) for x in self.o], u=[float(x) for x in self.u], v=[float(x) for x in self.v], n=[float(x) for x in self.n],
                    gsd=float(self.gsd), width=int(self.width), height=int(self.height), d_min=float(self.d_min), d_max=float(self.d_max))


def ortho_frame(frame) -> OrthoFrame:
    """An OrthoFrame from a dict(o, u, v, n, gsd, width, height, d_min, d_max) (or a copy of one); the values go through
    float32 as the library takes them."""
    if isinstance(frame, OrthoFrame):
        frame = frame.as_dict()
    f = OrthoFrame()
    for k in ("o", "u", "v", "n"):
        vals = np.asarray(frame[k], np.float32).reshape(3)
        setattr(f, k, (C.c_float * 3)(*[float(x) for x in vals]))
    f.gsd = float(np.float32(frame["gsd"]))
    f.width, f.height = int(frame["width"]), int(frame["height"])
    f.d_min, f.d_max = float(np.float32(frame["d_min"])), float(np.float32(frame["d_max"]))
    return f


def ortho_host(frame, xyz, rgb, label=None, has=None, index_base: int = 0, fill_radius: int = 0) -> dict:
    """The orthographic map of n rows computed on the CPU by the arithmetic the kernels use (pcp_ortho_host: no context, no
    GPU; DESIGN.md "Orthographic maps", OM8).  xyz (n, 3) float32, rgb (n, 3) uint8, label / has n uint8 or None:
    dict(index, depth, rgb[, label], status, source, contributors, occupied, filled)."""
    L = load()
    f = ortho_frame(frame)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    label = None if label is None else np.ascontiguousarray(label, np.uint8).reshape(-1)
    has = None if has is None else np.ascontiguousarray(has, np.uint8).reshape(-1)
    n = xyz.shape[0]
    if rgb.shape[0] != n or (label is not None and label.shape[0] != n) or (has is not None and has.shape[0] != n):
        raise ValueError("ortho_host: xyz, rgb, label and has differ in their number of rows")
    h, w = max(int(f.height), 0), max(int(f.width), 0)
    big = w > 16384 or h > 16384 or w * h > (1 << 26)  # (refused by the library: nothing to allocate)
    shape = (0, 0) if big else (h, w)
    out = dict(index=np.empty(shape, np.uint32), depth=np.empty(shape, np.float32), rgb=np.empty(shape + (3,), np.uint8),
               status=np.empty(shape, np.uint8), source=np.empty(shape, np.int32))
    olab = np.empty(shape, np.uint8) if label is not None else None
    cnt, occ, fil = C.c_int64(), C.c_int64(), C.c_int64()
    rc = L.pcp_ortho_host(C.byref(f), C.c_int64(n), _ptr(xyz), _ptr(rgb), _ptr(label), _ptr(has), C.c_int64(index_base),
                          C.c_int32(fill_radius), _ptr(out["index"]), _ptr(out["depth"]), _ptr(out["rgb"]), _ptr(olab),
                          _ptr(out["status"]), _ptr(out["source"]), C.byref(cnt), C.byref(occ), C.byref(fil))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    if label is not None:
        out["label"] = olab
    out.update(contributors=cnt.value, occupied=occ.value, filled=fil.value)
    return out


class OrthoDefectParams(C.Structure):
    """pcp_ortho_defect_params ("Surface defects on ortho maps", SD1)."""
    _fields_ = [("threshold", C.c_float), ("window_px", C.c_int32), ("refine", C.c_int32), ("min_support", C.c_int32),
                ("min_pixels", C.c_int32), ("classes", C.c_int32)]


DEFECT_OUT = ("kept", "dropped", "hollow_pixels", "bulge_pixels", "unsupported", "refused", "first_pass", "surface")
DEFECT_ROW = ("class", "pixels", "measured", "sum_dev", "max_dev", "max_pixel", "col_min", "col_max", "row_min", "row_max", "sum_col",
              "sum_row", "open", "first_pixel", "first_pass", "zero")
DEFECT_HOLLOW, DEFECT_BULGE = 1, 2


def ortho_defect_params(threshold: float = 0.002, window: int = 0, refine: bool = False, min_support: int = 1, min_pixels: int = 1,
                        classes: int = 3) -> OrthoDefectParams:
    return OrthoDefectParams(float(np.float32(threshold)), int(window), int(refine), int(min_support), int(min_pixels), int(classes))


def ortho_defects_host(depth, status, threshold: float = 0.002, window: int = 0, refine: bool = False, min_support: int = 1,
                       min_pixels: int = 1, classes: int = 3) -> dict:
    """The surface defects of a map's (H, W) depth and status layers computed on the CPU by the arithmetic the kernels use
    (pcp_ortho_defects_host: no context, no GPU; DESIGN.md "Surface defects on ortho maps", SD9):
    dict(out (8 int64, DEFECT_OUT), dev int32, cls uint8, region int32, rows (N, 16) int64 (DEFECT_ROW))."""
    L = load()
    depth = np.ascontiguousarray(depth, np.float32)
    status = np.ascontiguousarray(status, np.uint8)
    if depth.ndim != 2 or status.shape != depth.shape:
        raise ValueError("ortho_defects_host: depth and status are a map's height x width layers")
    h, w = depth.shape
    p = ortho_defect_params(threshold, window, refine, min_support, min_pixels, classes)
    out = np.zeros(8, np.int64)
    res = dict(out=out, dev=np.empty((h, w), np.int32), cls=np.empty((h, w), np.uint8), region=np.empty((h, w), np.int32))
    n = C.c_int64()
    rows = np.zeros((4096, 16), np.int64)  # (a second call only where a raster keeps more regions than this)
    for _ in range(2):
        rc = L.pcp_ortho_defects_host(C.c_int32(w), C.c_int32(h), _ptr(depth), _ptr(status), C.byref(p), _ptr(out), _ptr(res["dev"]),
                                      _ptr(res["cls"]), _ptr(res["region"]), _ptr(rows), C.c_int64(len(rows)), C.byref(n))
        if rc != PCP_OK:
            raise PcpError(rc, L.pcp_last_error(None).decode())
        if n.value <= len(rows):
            break
        rows = np.zeros((n.value, 16), np.int64)
    rows = rows[:n.value].copy()
    res["rows"] = rows
    return res


def ortho_fit_frame_host(xyz, gsd: float, has=None, viewer=None) -> OrthoFrame:
    """A frame that looks straight at the rows (pcp_ortho_fit_frame_host: host only, fp64): the plane of their covariance's
    smallest eigenvalue, n signed away from `viewer` (3 numbers; None: largest component negative)."""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    has = None if has is None else np.ascontiguousarray(has, np.uint8).reshape(-1)
    if has is not None and has.shape[0] != xyz.shape[0]:
        raise ValueError("ortho_fit_frame_host: xyz and has differ in their number of rows")
    viewer = None if viewer is None else np.ascontiguousarray(viewer, np.float64).reshape(3)
    f = OrthoFrame()
    rc = L.pcp_ortho_fit_frame_host(C.c_int64(xyz.shape[0]), _ptr(xyz), _ptr(has), _ptr(viewer), C.c_float(gsd), C.byref(f))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return f


class CylFrame(C.Structure):
    """pcp_cyl_frame: a point c of the axis, the unit axis a (image y), e / b (theta = 0 / pi/2), radius, metres per pixel,
    raster size, depth window and side of a cylinder's unrolled map ("Cylindrical facets", CY1)."""
    _fields_ = [("c", C.c_float * 3), ("a", C.c_float * 3), ("e", C.c_float * 3), ("b", C.c_float * 3), ("radius", C.c_float),
                ("gsd", C.c_float), ("width", C.c_int32), ("height", C.c_int32), ("d_min", C.c_float), ("d_max", C.c_float),
                ("side", C.c_int32)]

    def as_dict(self) -> dict:
        return dict(c=[float(x) for x in self.c], a=[float(x) for x in self.a], e=[float(x) for x in self.e], b=[float(x) for x in self.b],
                    radius=float(self.radius), gsd=float(self.gsd), width=int(self.width), height=int(self.height),
                    d_min=float(self.d_min), d_max=float(self.d_max), side=int(self.side))


CY_STATS = ("rows", "rms", "dev_min", "dev_max", "arc", "ev0", "ev1", "ev2")  # pcp_cyl_fit_host's out_stats


def cyl_frame(frame) -> CylFrame:
    """A CylFrame from a dict(c, a, e, b, radius, gsd, width, height, d_min, d_max, side) (or a copy of one); the values go
    through float32 as the library takes them."""
    if isinstance(frame, CylFrame):
        frame = frame.as_dict()
    f = CylFrame()
    for k in ("c", "a", "e", "b"):
        vals = np.asarray(frame[k], np.float32).reshape(3)
        setattr(f, k, (C.c_float * 3)(*[float(x) for x in vals]))
    f.radius = float(np.float32(frame["radius"]))
    f.gsd = float(np.float32(frame["gsd"]))
    f.width, f.height = int(frame["width"]), int(frame["height"])
    f.d_min, f.d_max = float(np.float32(frame["d_min"])), float(np.float32(frame["d_max"]))
    f.side = int(frame["side"])
    return f


def ortho_cyl_host(frame, xyz, rgb, label=None, has=None, index_base: int = 0, fill_radius: int = 0) -> dict:
    """ortho_host under a cylinder's frame (pcp_ortho_cyl_host: no context, no GPU; DESIGN.md "Cylindrical facets", CY5): the
    same arguments and the same dict."""
    L = load()
    f = cyl_frame(frame)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    label = None if label is None else np.ascontiguousarray(label, np.uint8).reshape(-1)
    has = None if has is None else np.ascontiguousarray(has, np.uint8).reshape(-1)
    n = xyz.shape[0]
    if rgb.shape[0] != n or (label is not None and label.shape[0] != n) or (has is not None and has.shape[0] != n):
        raise ValueError("ortho_cyl_host: xyz, rgb, label and has differ in their number of rows")
    h, w = max(int(f.height), 0), max(int(f.width), 0)
    big = w > 16384 or h > 16384 or w * h > (1 << 26)  # (refused by the library: nothing to allocate)
    shape = (0, 0) if big else (h, w)
    out = dict(index=np.empty(shape, np.uint32), depth=np.empty(shape, np.float32), rgb=np.empty(shape + (3,), np.uint8),
               status=np.empty(shape, np.uint8), source=np.empty(shape, np.int32))
    olab = np.empty(shape, np.uint8) if label is not None else None
    cnt, occ, fil = C.c_int64(), C.c_int64(), C.c_int64()
    rc = L.pcp_ortho_cyl_host(C.byref(f), C.c_int64(n), _ptr(xyz), _ptr(rgb), _ptr(label), _ptr(has), C.c_int64(index_base),
                              C.c_int32(fill_radius), _ptr(out["index"]), _ptr(out["depth"]), _ptr(out["rgb"]), _ptr(olab),
                              _ptr(out["status"]), _ptr(out["source"]), C.byref(cnt), C.byref(occ), C.byref(fil))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    if label is not None:
        out["label"] = olab
    out.update(contributors=cnt.value, occupied=occ.value, filled=fil.value)
    return out


def cyl_angle_host(s, t) -> np.ndarray:
    """theta in [0, 2 pi] of the pairs (s, t) of doubles by the kernels' fixed sequence of fp64 operations (pcp_cyl_angle_host;
    DESIGN.md "Cylindrical facets", CY3)."""
    L = load()
    s = np.ascontiguousarray(s, np.float64).reshape(-1)
    t = np.ascontiguousarray(t, np.float64).reshape(-1)
    if s.shape != t.shape:
        raise ValueError("cyl_angle_host: s and t differ in their number of rows")
    out = np.empty(s.shape, np.float64)
    rc = L.pcp_cyl_angle_host(C.c_int64(s.size), _ptr(s), _ptr(t), _ptr(out))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return out


def cyl_fit_host(xyz, normal, gsd: float, has=None, viewer=None) -> tuple[CylFrame, dict]:
    """The cylinder of the rows that have a valid normal and the frame that unrolls them (pcp_cyl_fit_host: host only, fp64,
    closed form; DESIGN.md "Cylindrical facets", CY6).  Returns (CylFrame, dict of CY_STATS)."""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    normal = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    has = None if has is None else np.ascontiguousarray(has, np.uint8).reshape(-1)
    if normal.shape[0] != xyz.shape[0] or (has is not None and has.shape[0] != xyz.shape[0]):
        raise ValueError("cyl_fit_host: xyz, normal and has differ in their number of rows")
    viewer = None if viewer is None else np.ascontiguousarray(viewer, np.float64).reshape(3)
    f = CylFrame()
    stats = np.zeros(8, np.float64)
    rc = L.pcp_cyl_fit_host(C.c_int64(xyz.shape[0]), _ptr(xyz), _ptr(normal), _ptr(has), _ptr(viewer), C.c_float(gsd), C.byref(f),
                            _ptr(stats))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return f, {k: (int(v) if k == "rows" else float(v)) for k, v in zip(CY_STATS, stats)}


class OrthoTextureParams(C.Structure):
    """pcp_ortho_texture_params ("Orthophotos", OT2)."""
    _fields_ = [("scale", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("views", C.c_int32),
                ("interpolate", C.c_int32), ("max_step", C.c_float)]


def ortho_texture_params(scale: int, views: int = 1, interpolate: bool = True, max_step: float = 0.05, rect=None) -> OrthoTextureParams:
    """rect: (x0, y0, w, h) in ortho pixels, or None for the whole raster"""
    x0, y0, w, h = (0, 0, 0, 0) if rect is None else (int(v) for v in rect)
    return OrthoTextureParams(int(scale), x0, y0, w, h, int(views), 1 if interpolate else 0, float(max_step))


def _ortho_texture_shape(frame: OrthoFrame, p: OrthoTextureParams) -> tuple[int, int]:
    """(h k, w k) of the call's output; (0, 0) for parameters the library refuses (nothing to allocate)"""
    w, h = (int(frame.width), int(frame.height)) if p.w == 0 and p.h == 0 else (int(p.w), int(p.h))
    k = int(p.scale)
    if not (1 <= k <= 16 and w >= 1 and h >= 1 and w * h * k * k <= (1 << 28)):
        return 0, 0
    return h * k, w * k


def ortho_texture_points_host(frame, source, depth, scale: int, interpolate: bool = True, max_step: float = 0.05, rect=None) -> dict:
    """The surface points behind the fine pixels of an orthophoto, computed on the CPU by the arithmetic the kernel uses
    (pcp_ortho_texture_points_host: no context, no GPU; DESIGN.md "Orthophotos", OT2, OT3, OT9).  source / depth: the map's
    (H, W) layers as ortho_fetch / ortho_host return them.  dict(xyz (h k, w k, 3) float32, ok (h k, w k) uint8)."""
    L = load()
    f = ortho_frame(frame)
    p = ortho_texture_params(scale, 1, interpolate, max_step, rect)
    source = np.ascontiguousarray(source, np.int32)
    depth = np.ascontiguousarray(depth, np.float32)
    if source.size != int(f.width) * int(f.height) or depth.size != source.size:
        raise ValueError("ortho_texture_points_host: source and depth are the map's height x width layers")
    fh, fw = _ortho_texture_shape(f, p)
    out = dict(xyz=np.empty((fh, fw, 3), np.float32), ok=np.empty((fh, fw), np.uint8))
    rc = L.pcp_ortho_texture_points_host(C.byref(f), C.byref(p), _ptr(source), _ptr(depth), _ptr(out["xyz"]), _ptr(out["ok"]))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return out


def ortho_texture_points_cyl_host(frame, source, depth, scale: int, interpolate: bool = True, max_step: float = 0.05, rect=None) -> dict:
    """ortho_texture_points_host under a cylinder's frame (pcp_ortho_texture_points_cyl_host: no context, no GPU; DESIGN.md
    "Orthophotos of unrolled maps", CT2, CT5): the same arguments and the same dict; ok is 0 where rho <= 0 too."""
    L = load()
    f = cyl_frame(frame)
    p = ortho_texture_params(scale, 1, interpolate, max_step, rect)
    source = np.ascontiguousarray(source, np.int32)
    depth = np.ascontiguousarray(depth, np.float32)
    if source.size != int(f.width) * int(f.height) or depth.size != source.size:
        raise ValueError("ortho_texture_points_cyl_host: source and depth are the map's height x width layers")
    fh, fw = _ortho_texture_shape(f, p)
    out = dict(xyz=np.empty((fh, fw, 3), np.float32), ok=np.empty((fh, fw), np.uint8))
    rc = L.pcp_ortho_texture_points_cyl_host(C.byref(f), C.byref(p), _ptr(source), _ptr(depth), _ptr(out["xyz"]), _ptr(out["ok"]))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return out


def cyl_sincos_host(theta) -> tuple[np.ndarray, np.ndarray]:
    """(sin, cos) of the angles theta in [0, 64) by the kernels' fixed sequence of fp64 operations (pcp_cyl_sincos_host; DESIGN.md
    "Orthophotos of unrolled maps", CT1)."""
    L = load()
    theta = np.ascontiguousarray(theta, np.float64).reshape(-1)
    s, c = np.empty(theta.shape, np.float64), np.empty(theta.shape, np.float64)
    rc = L.pcp_cyl_sincos_host(C.c_int64(theta.size), _ptr(theta), _ptr(s), _ptr(c))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return s, c


def normals_moments_host(radius: float, xyz) -> np.ndarray:
    """The moments of pcp_estimate_normals computed on the CPU by brute force over the pairs, with the arithmetic the kernel
    uses (pcp_normals_moments_host: no context, no GPU; DESIGN.md "Geometry maps", GN2-GN4).  xyz (n, 3) float32, n <= 65536:
    (n, 10) int64 -- n S1x S1y S1z S2xx xy xz yy yz zz per point."""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    out = np.zeros((xyz.shape[0], 10), np.int64)
    rc = L.pcp_normals_moments_host(C.c_float(radius), C.c_int64(xyz.shape[0]), _ptr(xyz), _ptr(out))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return out


class CompareParams(C.Structure):
    """pcp_compare_params ("Map comparison", MC2-MC6)."""
    _fields_ = [("cyl_radius", C.c_float), ("cyl_half_length", C.c_float), ("reg_error", C.c_float), ("min_points", C.c_int32),
                ("orient_mode", C.c_int32), ("orient", C.c_float * 3)]


MC_SUMS = ("nA", "s1A", "s2aA", "s2bA", "nB", "s1B", "s2aB", "s2bB")  # MC4: the columns of sums
MC_STATS = ("core", "measured", "positive", "negative", "no_counterpart", "too_few_own", "most_candidates", "reserved")
MC_NOT_CORE, MC_NO_COUNTERPART, MC_TOO_FEW_OWN, MC_MEASURED, MC_POSITIVE, MC_NEGATIVE = range(6)  # MC6: the status byte


def compare_params(radius: float = 0.03, half_length: float = 0.05, reg_error: float = 0.0, min_points: int = 5,
                   orient_mode: int = 0, orient=(0.0, 0.0, 0.0)) -> CompareParams:
    orient = np.asarray(orient, np.float32).reshape(3)
    return CompareParams(radius, half_length, reg_error, min_points, orient_mode, (C.c_float * 3)(*[float(v) for v in orient]))


def _compare_outputs(n: int) -> dict:
    return dict(distance=np.zeros(n, np.float32), lod=np.zeros(n, np.float32), status=np.zeros(n, np.uint8),
                sums=np.zeros((n, 8), np.int64), direction=np.zeros((n, 3), np.int32))


def compare_host(xyz, normals, base_xyz, radius: float = 0.03, half_length: float = 0.05, reg_error: float = 0.0,
                 min_points: int = 5, orient_mode: int = 0, orient=(0.0, 0.0, 0.0)) -> dict:
    """The map comparison of n <= 65536 map points against n_base <= 65536 base rows computed on the CPU by brute force over
    the pairs with the arithmetic the kernel uses (pcp_compare_host: no context, no GPU; DESIGN.md "Map comparison").  xyz,
    normals (n, 3) float32, base_xyz (n_base, 3) float32 -> dict(distance, lod (n,) float32, status (n,) uint8, sums (n, 8)
    int64 with the columns MC_SUMS, direction (n, 3) int32, stats (8,) int64 with the entries MC_STATS)."""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    base_xyz = np.ascontiguousarray(base_xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    if normals.shape[0] != n:
        raise ValueError("compare_host: xyz and normals differ in their number of rows")
    prm = compare_params(radius, half_length, reg_error, min_points, orient_mode, orient)
    out = _compare_outputs(min(n, 65536))  # (more rows are refused by the library: nothing to allocate)
    stats = np.zeros(8, np.int64)
    rc = L.pcp_compare_host(C.byref(prm), C.c_int64(n), _ptr(xyz), _ptr(normals), C.c_int64(base_xyz.shape[0]), _ptr(base_xyz),
                            _ptr(out["distance"]), _ptr(out["lod"]), _ptr(out["status"]), _ptr(out["sums"]), _ptr(out["direction"]),
                            _ptr(stats))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    out["stats"] = stats
    return out


class RegisterParams(C.Structure):
    """pcp_register_params ("Map registration", RG3-RG7)."""
    _fields_ = [("match_radius", C.c_float), ("max_plane_distance", C.c_float), ("sample_stride", C.c_int32),
                ("max_iterations", C.c_int32), ("min_pairs", C.c_int32), ("tolerance", C.c_double), ("cond_tol", C.c_double)]


RG_TERMS = tuple(f"g{a}g{b}" for a in range(6) for b in range(a, 6)) + tuple(f"g{a}h" for a in range(6)) + ("hh", "N2", "one")  # RG5
RG_LOG = ("pairs", "rms", "dof", "rotation", "shift")  # RG8: the columns of the log
RG_CONVERGED, RG_ITERATION_LIMIT, RG_TOO_FEW_PAIRS = range(3)  # RG8: the status
RG_DEFAULT_COND_TOL = 6.2e-3


def register_params(match_radius: float = 0.05, max_plane_distance: float = 0.02, sample_stride: int = 1, max_iterations: int = 20,
                    min_pairs: int = 100, tolerance: float = 1e-5, cond_tol: float = RG_DEFAULT_COND_TOL) -> RegisterParams:
    return RegisterParams(match_radius, max_plane_distance, sample_stride, max_iterations, min_pairs, tolerance, cond_tol)


def _register_result(T, log, status) -> dict:
    rows = int(status[1])
    log = log[:rows].copy()
    return dict(T=T, log=log, status=int(status[0]), iterations=rows, rms=float(log[-1, 1]) if rows else 0.0,
                dof=int(log[-1, 2]) if rows else 0, pairs=int(log[-1, 0]) if rows else 0)


def register_solve_host(sums60, ell: float, cond_tol: float = RG_DEFAULT_COND_TOL) -> dict:
    """RG6 for 60 int64 words of sums (pcp_register_solve_host: host only): dict(omega (3,), dt (3,), rms, eigenvalues (6,),
    dof)."""
    L = load()
    sums = np.ascontiguousarray(sums60, np.int64).reshape(60)
    upd, eig, dof = np.zeros(7, np.float64), np.zeros(6, np.float64), C.c_int32()
    rc = L.pcp_register_solve_host(_ptr(sums), C.c_double(ell), C.c_double(cond_tol), _ptr(upd), _ptr(eig), C.byref(dof))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return dict(omega=upd[:3].copy(), dt=upd[3:6].copy(), rms=float(upd[6]), eigenvalues=eig, dof=dof.value)


def compare_register_host(xyz, normals, base_xyz, T_in=None, loop: bool = True, **params) -> dict:
    """The registration of n_base <= 65536 base rows onto n <= 65536 map points on the CPU by brute force over the pairs with
    the arithmetic the kernels use (pcp_compare_register_host: no context, no GPU; DESIGN.md "Map registration").  loop False:
    one evaluation at T_in (None: the identity) -> dict(sums (60,) int64, T, rows); else the loop from T_in -> also log, status,
    iterations, rms, dof, pairs.  params: those of register_params."""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    base_xyz = np.ascontiguousarray(base_xyz, np.float32).reshape(-1, 3)
    if normals.shape[0] != xyz.shape[0]:
        raise ValueError("compare_register_host: xyz and normals differ in their number of rows")
    prm = register_params(**params)
    T_in = None if T_in is None else np.ascontiguousarray(T_in, np.float64).reshape(16)
    sums, T = np.zeros(60, np.int64), np.zeros((4, 4), np.float64)
    log, status = np.zeros((max(1, min(prm.max_iterations, 1000)), 5), np.float64), np.zeros(2, np.int32)
    rows = np.zeros((min(base_xyz.shape[0], 65536), 3), np.float32)
    rc = L.pcp_compare_register_host(C.byref(prm), C.c_int64(xyz.shape[0]), _ptr(xyz), _ptr(normals), C.c_int64(base_xyz.shape[0]),
                                     _ptr(base_xyz), _ptr(T_in), C.c_int32(1 if loop else 0), _ptr(sums), _ptr(T), _ptr(log),
                                     _ptr(status), _ptr(rows))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    out = _register_result(T, log, status) if loop else dict(T=T)
    out["sums"] = sums
    out["rows"] = rows
    return out


class CoarseParams(C.Structure):
    """pcp_coarse_params ("Coarse registration", CG1-CG9)."""
    _fields_ = [("support_radius", C.c_float), ("normal_radius", C.c_float), ("inlier_distance", C.c_float), ("min_side", C.c_float),
                ("side_tolerance", C.c_float), ("min_angle_deg", C.c_float), ("map_stride", C.c_int32), ("base_stride", C.c_int32),
                ("min_neighbours", C.c_int32), ("min_offplane_permille", C.c_int32), ("ratio_q8", C.c_int32), ("mutual", C.c_int32),
                ("hypotheses", C.c_int32), ("min_inliers", C.c_int32), ("seed", C.c_uint64)]


CG_REPORT = ("keypoints_map", "keypoints_base", "valid_map", "valid_base", "correspondences", "scored", "refused", "winner", "runner_up",
             "refit", "kept", "status", "winner_h")  # CG8: the first thirteen words of the report; the triple follows
CG_FOUND, CG_TOO_FEW_INLIERS = 0, 2  # CG8: the status
CG_ACCEPTED, CG_REPEAT, CG_SHORT_SIDE, CG_SIDE_MISMATCH, CG_THIN = range(5)  # CG4: the refusal codes
CG_MAP, CG_BASE = 0, 1  # the sides
CG_NO_KEY = (1 << 64) - 1


def coarse_params(support_radius: float = 0.2, normal_radius: float = 0.1, inlier_distance: float = 0.05, min_side: float = 0.3,
                  side_tolerance: float = 0.05, min_angle_deg: float = 15.0, map_stride: int = 4, base_stride: int = 4,
                  min_neighbours: int = 20, min_offplane_permille: int = 100, ratio_q8: int = 230, mutual: int = 1, hypotheses: int = 4096,
                  min_inliers: int = 10, seed: int = 1) -> CoarseParams:
    return CoarseParams(support_radius, normal_radius, inlier_distance, min_side, side_tolerance, min_angle_deg, map_stride, base_stride,
                        min_neighbours, min_offplane_permille, ratio_q8, int(bool(mutual)), hypotheses, min_inliers, seed)


def _coarse_slots(prm: CoarseParams, side: int, rows: int) -> int:
    stride = max(1, prm.base_stride if side == CG_BASE else prm.map_stride)
    return (rows + stride - 1) // stride


def _coarse_report(report, T, inliers) -> dict:
    out = {k: int(report[i]) for i, k in enumerate(CG_REPORT)}
    out.update(triple=tuple(int(v) for v in report[13:16]), T=T, inliers=inliers[:int(report[4])].copy(), report=report)
    return out


def _host_check(rc):
    if rc != PCP_OK:
        raise PcpError(rc, load().pcp_last_error(None).decode())


def coarse_descriptors_host(side: int, xyz, normals, **params) -> dict:
    """CG1 + CG2 of one cloud of n <= 65536 rows on the CPU by brute force with the arithmetic the kernel uses
    (pcp_coarse_descriptors_host): dict(desc (slots, 64) uint16, total (slots,) uint32, state (slots,) uint8, slots, keypoints,
    valid).  side picks the stride (CG_MAP / CG_BASE).  params: those of coarse_params."""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if normals.shape[0] != xyz.shape[0]:
        raise ValueError("coarse_descriptors_host: xyz and normals differ in their number of rows")
    prm = coarse_params(**params)
    slots = _coarse_slots(prm, side, min(xyz.shape[0], 65536))
    desc, total, state = np.zeros((slots, 64), np.uint16), np.zeros(slots, np.uint32), np.zeros(slots, np.uint8)
    counts = np.zeros(3, np.int64)
    _host_check(L.pcp_coarse_descriptors_host(C.byref(prm), C.c_int32(side), C.c_int64(xyz.shape[0]), _ptr(xyz), _ptr(normals), _ptr(desc),
                                              _ptr(total), _ptr(state), _ptr(counts)))
    return dict(desc=desc, total=total, state=state, slots=int(counts[0]), keypoints=int(counts[1]), valid=int(counts[2]))


def coarse_match_host(base_desc, map_desc, **params) -> dict:
    """CG3 over the valid descriptors of the two sides, (K, 64) uint16 each, on the CPU (pcp_coarse_match_host): dict(pairs (C, 2)
    int32: base ordinal, map ordinal; base_keys (K_base, 2), map_keys (K_map, 2) uint64: best, second, CG_NO_KEY = none)."""
    L = load()
    db = np.ascontiguousarray(base_desc, np.uint16).reshape(-1, 64)
    dm = np.ascontiguousarray(map_desc, np.uint16).reshape(-1, 64)
    prm = coarse_params(**params)
    pairs, count = np.zeros((max(1, min(db.shape[0], 65536)), 2), np.int32), C.c_int64()
    bk, mk = np.zeros((db.shape[0], 2), np.uint64), np.zeros((dm.shape[0], 2), np.uint64)
    _host_check(L.pcp_coarse_match_host(C.byref(prm), C.c_int64(db.shape[0]), _ptr(db), C.c_int64(dm.shape[0]), _ptr(dm), _ptr(pairs),
                                        C.byref(count), _ptr(bk), _ptr(mk)))
    return dict(pairs=pairs[:count.value].copy(), base_keys=bk, map_keys=mk)


def coarse_hypothesis_host(cb, cm, pivot, h: int, **params) -> dict:
    """CG4 for hypothesis h over the correspondences' coordinates cb, cm (C, 3) float32 about `pivot`
    (pcp_coarse_hypothesis_host): dict(code, triple, frame (15,) float64: R row-major, pivot, t)."""
    L = load()
    cb = np.ascontiguousarray(cb, np.float32).reshape(-1, 3)
    cm = np.ascontiguousarray(cm, np.float32).reshape(-1, 3)
    if cb.shape != cm.shape:
        raise ValueError("coarse_hypothesis_host: cb and cm differ in shape")
    pivot = np.ascontiguousarray(pivot, np.float64).reshape(3)
    prm = coarse_params(**params)
    code, triple, frame = C.c_int32(), np.zeros(3, np.int32), np.zeros(15, np.float64)
    _host_check(L.pcp_coarse_hypothesis_host(C.byref(prm), C.c_int64(cb.shape[0]), _ptr(cb), _ptr(cm), _ptr(pivot), C.c_int32(h),
                                             C.byref(code), _ptr(triple), _ptr(frame)))
    return dict(code=code.value, triple=tuple(int(v) for v in triple), frame=frame)


def coarse_score_host(frames, cb, cm, flags: bool = False, **params) -> dict:
    """CG5 for frames (F, 15) float64 over the correspondences' coordinates on the CPU (pcp_coarse_score_host): dict(counts (F,)
    int64, and with flags flags (F, C) uint8)."""
    L = load()
    frames = np.ascontiguousarray(frames, np.float64).reshape(-1, 15)
    cb = np.ascontiguousarray(cb, np.float32).reshape(-1, 3)
    cm = np.ascontiguousarray(cm, np.float32).reshape(-1, 3)
    if cb.shape != cm.shape:
        raise ValueError("coarse_score_host: cb and cm differ in shape")
    prm = coarse_params(**params)
    counts = np.zeros(frames.shape[0], np.int64)
    fl = np.zeros((frames.shape[0], cb.shape[0]), np.uint8) if flags else None
    _host_check(L.pcp_coarse_score_host(C.byref(prm), C.c_int64(frames.shape[0]), _ptr(frames), C.c_int64(cb.shape[0]), _ptr(cb), _ptr(cm),
                                        _ptr(counts), _ptr(fl)))
    return dict(counts=counts, flags=fl) if flags else dict(counts=counts)


def coarse_refit_host(cb, cm, flags, pivot_base, pivot_map) -> np.ndarray:
    """CG6's refit over the flagged correspondences (pcp_coarse_refit_host): the frame, (15,) float64."""
    L = load()
    cb = np.ascontiguousarray(cb, np.float32).reshape(-1, 3)
    cm = np.ascontiguousarray(cm, np.float32).reshape(-1, 3)
    flags = np.ascontiguousarray(flags, np.uint8).reshape(-1)
    if cb.shape != cm.shape or flags.shape[0] != cb.shape[0]:
        raise ValueError("coarse_refit_host: cb, cm and flags differ in their number of rows")
    pb, pm = np.ascontiguousarray(pivot_base, np.float64).reshape(3), np.ascontiguousarray(pivot_map, np.float64).reshape(3)
    frame = np.zeros(15, np.float64)
    _host_check(L.pcp_coarse_refit_host(C.c_int64(cb.shape[0]), _ptr(cb), _ptr(cm), _ptr(flags), _ptr(pb), _ptr(pm), _ptr(frame)))
    return frame


def compare_register_coarse_host(xyz, normals, base_xyz, base_normals, **params) -> dict:
    """The whole coarse registration of n_base <= 65536 base rows onto n <= 65536 map points on the CPU with the arithmetic the
    kernels use (pcp_compare_register_coarse_host; DESIGN.md "Coarse registration"): dict with the entries CG_REPORT, triple, T
    (4, 4) base -> map (the identity with status CG_TOO_FEW_INLIERS), inliers (C,) uint8, report (16,) int64."""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    base_xyz = np.ascontiguousarray(base_xyz, np.float32).reshape(-1, 3)
    base_normals = np.ascontiguousarray(base_normals, np.float32).reshape(-1, 3)
    if normals.shape[0] != xyz.shape[0] or base_normals.shape[0] != base_xyz.shape[0]:
        raise ValueError("compare_register_coarse_host: a cloud and its normals differ in their number of rows")
    prm = coarse_params(**params)
    report, T, inliers = np.zeros(16, np.int64), np.zeros((4, 4), np.float64), np.zeros(1 << 18, np.uint8)
    _host_check(L.pcp_compare_register_coarse_host(C.byref(prm), C.c_int64(xyz.shape[0]), _ptr(xyz), _ptr(normals),
                                                   C.c_int64(base_xyz.shape[0]), _ptr(base_xyz), _ptr(base_normals), _ptr(report), _ptr(T),
                                                   _ptr(inliers)))
    return _coarse_report(report, T, inliers)


def coarse_then_fine_host(xyz, normals, base_xyz, base_normals, coarse=None, fine=None) -> dict:
    """Context.coarse_then_fine on the CPU: compare_register_coarse_host, then compare_register_host from its T with match_radius =
    2 inlier_distance (the other parameters at their defaults), then from that T with `fine` (the defaults)."""
    coarse = dict(coarse or {})
    first = compare_register_coarse_host(xyz, normals, base_xyz, base_normals, **coarse)
    if first["status"] != CG_FOUND:
        return dict(coarse=first, wide=None, fine=None, T=first["T"], status=first["status"])
    inlier = coarse_params(**coarse).inlier_distance
    wide = compare_register_host(xyz, normals, base_xyz, T_in=first["T"], match_radius=2.0 * inlier)
    last = compare_register_host(xyz, normals, base_xyz, T_in=wide["T"], **dict(fine or {}))
    return dict(coarse=first, wide=wide, fine=last, T=last["T"], status=last["status"])


def mask_edt_host(gray, threshold: int = 0) -> dict:
    """The mask distance maps of a (H, W) uint8 mask computed on the CPU with the arithmetic the kernels use
    (pcp_mask_edt_host: no context, no GPU; DESIGN.md "Mask distance maps").  A row stride above the width is passed on
    as it is.  dict(d2 (H, W) uint32, nearest (H, W) int32)."""
    L = load()
    gray = np.asarray(gray, np.uint8)
    if gray.ndim != 2:
        raise ValueError(f"mask_edt_host: a (H, W) mask is needed, got shape {gray.shape}")
    if gray.size and gray.strides[1] != 1:
        gray = np.ascontiguousarray(gray)
    hh, ww = gray.shape
    d2 = np.empty((hh, ww), np.uint32)
    nearest = np.empty((hh, ww), np.int32)
    rc = L.pcp_mask_edt_host(C.c_int32(ww), C.c_int32(hh), _ptr(gray), C.c_int64(gray.strides[0] if gray.size else 0),
                             C.c_int32(threshold), _ptr(d2), _ptr(nearest))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return dict(d2=d2, nearest=nearest)


class BalanceParams(C.Structure):
    """pcp_balance_params (20 bytes): stages (BALANCE_CLAHE | BALANCE_GAMMA), tiles, clip limit, gamma"""
    _fields_ = [("stages", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32), ("clip_limit", C.c_float), ("gamma", C.c_float)]


BALANCE_CLAHE, BALANCE_GAMMA = 1, 2


def balance_params(stages: int | None = None, tiles=None, clip_limit: float | None = None, gamma: float | None = None) -> BalanceParams:
    """pcp_default_balance_params (the autonomous script's main(): both stages, 8 x 8 tiles, clip 1.0, gamma 0.8) with the
    given fields replaced; tiles = (tiles_x, tiles_y)."""
    p = BalanceParams()
    load().pcp_default_balance_params(C.byref(p))
    if stages is not None:
        p.stages = int(stages)
    if tiles is not None:
        p.tiles_x, p.tiles_y = int(tiles[0]), int(tiles[1])
    if clip_limit is not None:
        p.clip_limit = float(clip_limit)
    if gamma is not None:
        p.gamma = float(gamma)
    return p


def _as_balance(balance) -> BalanceParams | None:
    """None / False: off; True: the defaults; a dict: balance_params(**dict); a BalanceParams as it is"""
    if balance is None or balance is False:
        return None
    if balance is True:
        return balance_params()
    if isinstance(balance, dict):
        return balance_params(**balance)
    return balance


def _balance_call(fn, who, head, params, bgr, want_stages: bool):
    bgr = np.asarray(bgr, np.uint8)
    if bgr.ndim != 3 or bgr.shape[2] != 3:
        raise ValueError(f"{who}: a (H, W, 3) BGR image is needed, got shape {bgr.shape}")
    if bgr.size and (bgr.strides[2] != 1 or bgr.strides[1] != 3):
        bgr = np.ascontiguousarray(bgr)
    hh, ww = bgr.shape[:2]
    p = _as_balance(params) or BalanceParams()
    out = np.empty((hh, ww, 3), np.uint8)
    tiles = max(p.tiles_x, 0) * max(p.tiles_y, 0) if (p.stages & BALANCE_CLAHE) and want_stages else 0
    hist = np.zeros((tiles, 256), np.uint32) if tiles else None
    lut = np.zeros((tiles, 256), np.uint8) if tiles else None
    rc = fn(*head, C.byref(p), C.c_int32(ww), C.c_int32(hh), _ptr(bgr), C.c_int64(bgr.strides[0] if bgr.size else 0), _ptr(out),
            _ptr(hist), _ptr(lut))
    res = dict(bgr=out)
    if tiles:
        res["hist"] = hist.reshape(p.tiles_y, p.tiles_x, 256)
        res["lut"] = lut.reshape(p.tiles_y, p.tiles_x, 256)
    return rc, res


def image_balance_host(bgr, params=True, stages: bool = False):
    """The keyframe colour balance of a (H, W, 3) BGR image on the CPU with the arithmetic the kernels use
    (pcp_image_balance_host: no context, no GPU; DESIGN.md "Image balance").  Returns the balanced (H, W, 3) image, or with
    stages=True dict(bgr, hist (tiles_y, tiles_x, 256) uint32, lut (tiles_y, tiles_x, 256) uint8) (hist, lut with CLAHE only)."""
    L = load()
    rc, res = _balance_call(L.pcp_image_balance_host, "image_balance_host", (), params, bgr, True)
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return res if stages else res["bgr"]


def gamma_table_host(gamma: float) -> np.ndarray:
    """adjust_gamma's 256-byte table (pcp_gamma_table_host)."""
    L = load()
    out = np.empty(256, np.uint8)
    rc = L.pcp_gamma_table_host(C.c_float(gamma), _ptr(out))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return out


class CrackParams(C.Structure):
    _fields_ = [("threshold", C.c_int32), ("plane_radius_px", C.c_int32)]


# the flag byte of the crack width maps (DESIGN.md "Crack width maps", CW9)
CW_SITE, CW_CENTRE, CW_NEAR, CW_FAR, CW_PLANE, CW_RAYS, CW_WIDTH = 1, 2, 4, 8, 16, 32, 64
CW_OUTPUTS = ("flags", "edges", "w2d2", "width", "points", "plane", "moments")


def crack_width_host(gray, index, xyz_cam, threshold: int = 0, plane_radius: int = 150) -> dict:
    """The integer part of the crack width maps computed on the CPU with the arithmetic the kernels use (pcp_crack_width_host:
    no context, no GPU; DESIGN.md "Crack width maps"): gray (H, W) uint8 mask, index (H, W) int32 and xyz_cam (H, W, 3)
    float32 as frame_geometry returns them.  dict(flags (H, W) uint8, bits 0-3 only; edges (H, W, 4) int32; w2d2 (H, W)
    uint32; moments (H, W, 13) int64)."""
    L = load()
    gray = np.asarray(gray, np.uint8)
    if gray.ndim != 2:
        raise ValueError(f"crack_width_host: a (H, W) mask is needed, got shape {gray.shape}")
    if gray.size and gray.strides[1] != 1:
        gray = np.ascontiguousarray(gray)
    hh, ww = gray.shape
    index = np.ascontiguousarray(index, np.int32)
    xyz_cam = np.ascontiguousarray(xyz_cam, np.float32)
    if index.shape != (hh, ww) or xyz_cam.shape != (hh, ww, 3):
        raise ValueError(f"crack_width_host: index {index.shape} / xyz_cam {xyz_cam.shape} do not match the mask {gray.shape}")
    flags = np.empty((hh, ww), np.uint8)
    edges = np.empty((hh, ww, 4), np.int32)
    w2d2 = np.empty((hh, ww), np.uint32)
    moments = np.empty((hh, ww, 13), np.int64)
    prm = CrackParams(threshold, plane_radius)
    rc = L.pcp_crack_width_host(C.c_int32(ww), C.c_int32(hh), _ptr(gray), C.c_int64(gray.strides[0] if gray.size else 0), _ptr(index),
                                _ptr(xyz_cam), C.byref(prm), _ptr(flags), _ptr(edges), _ptr(w2d2), _ptr(moments))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return dict(flags=flags, edges=edges, w2d2=w2d2, moments=moments)


class CrackLinkParams(C.Structure):
    _fields_ = [("min_views", C.c_int32), ("radius", C.c_float)]


# the state of the crack widths on the map, one array of n per field (DESIGN.md "Crack widths on the map", CF1-CF6)
CF_STATE = (("seen", np.uint32), ("views", np.uint32), ("centres", np.uint32), ("min_q", np.uint32), ("max_q", np.uint32),
            ("best_q", np.uint32), ("sum_q", np.uint64), ("best_key", np.uint64))
CF_OUTPUTS = (("width_mean", np.float32), ("width_best", np.float32), ("best_frame", np.int32), ("views", np.uint32), ("seen", np.uint32),
              ("centres", np.uint32), ("min_q", np.uint32), ("max_q", np.uint32), ("sum_q", np.uint64))


def crack_fuse_state(n: int) -> dict:
    """A fresh accumulation of n points as pcp_crack_fuse_begin creates it, for crack_fuse_host."""
    st = {k: np.zeros(n, t) for k, t in CF_STATE}
    st["min_q"][:] = 0xFFFFFFFF
    st["best_key"][:] = 0xFFFFFFFFFFFFFFFF
    return st


def crack_fuse_host(state: dict, index, pixel, range_, frame: int, flags, width) -> int:
    """One keyframe's add on the CPU with the arithmetic the kernel uses (pcp_crack_fuse_host: no context, no GPU): `state` from
    crack_fuse_state is updated in place by the m contributors (index into the state, pixel y * W + x, fp32 range) against
    the (H, W) flags and width images of crack_width.  Returns the number of credited contributors."""
    L = load()
    n = len(state["seen"])
    for k, t in CF_STATE:
        if state[k].dtype != t or state[k].shape != (n,) or not state[k].flags.c_contiguous:
            raise ValueError(f"crack_fuse_host: state[{k!r}] is not a contiguous {np.dtype(t).name} array of {n}")
    index = np.ascontiguousarray(index, np.int32)
    pixel = np.ascontiguousarray(pixel, np.int32)
    range_ = np.ascontiguousarray(range_, np.float32)
    flags = np.ascontiguousarray(flags, np.uint8)
    width = np.ascontiguousarray(width, np.float32)
    if flags.ndim != 2 or width.shape != flags.shape or not (index.shape == pixel.shape == range_.shape) or index.ndim != 1:
        raise ValueError("crack_fuse_host: (H, W) flags and width images and three contributor arrays of one length are needed")
    hh, ww = flags.shape
    credited = C.c_int64()
    rc = L.pcp_crack_fuse_host(C.c_int64(n), *[_ptr(state[k]) for k, _ in CF_STATE], C.c_int64(len(index)), _ptr(index), _ptr(pixel),
                               _ptr(range_), C.c_int32(frame), C.c_int32(ww), C.c_int32(hh), _ptr(flags), _ptr(width), C.byref(credited))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return credited.value


def crack_components_host(xyz, views, min_views: int = 1, radius: float = 0.02) -> np.ndarray:
    """The labels of pcp_crack_components computed on the CPU by brute force over the pairs (pcp_crack_components_host: no
    context, no GPU): xyz (n, 3) float32, views (n,) uint32, n <= 65536 -> (n,) int32, the lowest index of the point's
    component, -1 for a point that is no crack point."""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    views = np.ascontiguousarray(views, np.uint32)
    if views.shape != (xyz.shape[0],):
        raise ValueError(f"crack_components_host: {xyz.shape[0]} views expected, got shape {views.shape}")
    label = np.empty(xyz.shape[0], np.int32)
    rc = L.pcp_crack_components_host(C.c_int64(xyz.shape[0]), _ptr(xyz), _ptr(views), C.c_int32(min_views), C.c_float(radius), _ptr(label), None)
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return label


class FacetParams(C.Structure):
    """pcp_facet_params ("Planar facets", FA2-FA5)."""
    _fields_ = [("link_radius", C.c_float), ("angle_deg", C.c_float), ("plane_tol", C.c_float), ("max_curvature", C.c_float),
                ("min_points", C.c_int32)]


FA_ROW = ("points", "s1x", "s1y", "s1z", "s2xx", "s2xy", "s2xz", "s2yy", "s2yz", "s2zz")  # FA6: the columns of rows
FA_PLANE = ("cx", "cy", "cz", "nx", "ny", "nz", "rms")  # FA7: the columns of facet_plane_host


def facets_host(xyz, normal, curvature, link_radius: float = 0.1, angle_deg: float = 10.0, plane_tol: float = 0.01,
                max_curvature: float = 0.02, min_points: int = 1000) -> dict:
    """The facets of n <= 65536 points computed on the CPU by brute force over the pairs (pcp_facets_host: no context, no GPU):
    xyz, normal (n, 3) float32, curvature (n,) float32 -> dict(label (n,) int32, the lowest index of the point's facet, -1 for a
    point in none; ids (F,) int32 ascending; rows (F, 10) int64, the columns FA_ROW; box (F, 6) float32: min xyz, max xyz)."""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    normal = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    curvature = np.ascontiguousarray(curvature, np.float32).reshape(-1)
    n = xyz.shape[0]
    if normal.shape[0] != n or curvature.shape[0] != n:
        raise ValueError("facets_host: xyz, normal and curvature differ in their number of rows")
    prm = FacetParams(link_radius, angle_deg, plane_tol, max_curvature, min_points)
    cap = min(n, 65536)  # (more rows are refused by the library: nothing to allocate)
    label = np.empty(n, np.int32)
    ids = np.empty(cap, np.int32)
    rows = np.empty((cap, 10), np.int64)
    box = np.empty((cap, 6), np.float32)
    got = C.c_int64()
    rc = L.pcp_facets_host(C.c_int64(n), _ptr(xyz), _ptr(normal), _ptr(curvature), C.byref(prm), _ptr(label), _ptr(ids), _ptr(rows),
                           _ptr(box), C.byref(got))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    f = got.value
    return dict(label=label, ids=ids[:f].copy(), rows=rows[:f].copy(), box=box[:f].copy())


def facet_plane_host(root, row) -> np.ndarray:
    """The plane of one facet from its integers (pcp_facet_plane_host: host only, fp64): root = the coordinates of the facet's
    id point (3 float32), row = its 10 integers -> (7,) float64, the columns FA_PLANE (centroid, unit normal with its largest
    component positive, rms in metres)."""
    L = load()
    root = np.ascontiguousarray(root, np.float32).reshape(3)
    row = np.ascontiguousarray(row, np.int64).reshape(10)
    out = np.empty(7, np.float64)
    rc = L.pcp_facet_plane_host(_ptr(root), _ptr(row), _ptr(out))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    return out


NO_POS = 0xFFFFFFFFFFFFFFFF  # pos of a point that is no crack point (DESIGN.md "Crack lengths on the map", CL5)
CL_ROW = ("end_a", "end_b", "length_q", "hops", "path_sum_w", "path_min_w", "path_max_w")  # CL7: the columns of rows


def crack_lengths_host(xyz, views, min_views: int = 1, radius: float = 0.02, sum_q=None) -> dict:
    """What Context.crack_lengths returns, computed on the CPU by brute force over the pairs and a binary-heap Dijkstra
    (pcp_crack_lengths_host: no context, no GPU): xyz (n, 3) float32, views (n,) uint32, sum_q (n,) uint64 or None (every
    fused width 0), n <= 65536."""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    views = np.ascontiguousarray(views, np.uint32)
    n = xyz.shape[0]
    if views.shape != (n,):
        raise ValueError(f"crack_lengths_host: {n} views expected, got shape {views.shape}")
    if sum_q is not None:
        sum_q = np.ascontiguousarray(sum_q, np.uint64)
        if sum_q.shape != (n,):
            raise ValueError(f"crack_lengths_host: {n} sums expected, got shape {sum_q.shape}")
    pos = np.empty(n, np.uint64)
    ids = np.empty(n, np.int32)
    rows = np.empty((n, 7), np.int64)
    offsets = np.zeros(n + 1, np.int64)
    path = np.empty(n, np.int32)
    cracks, entries = C.c_int64(), C.c_int64()
    rc = L.pcp_crack_lengths_host(C.c_int64(n), _ptr(xyz), _ptr(views), C.c_int32(min_views), C.c_float(radius), _ptr(sum_q), _ptr(pos),
                                  _ptr(ids), _ptr(rows), _ptr(offsets), _ptr(path), C.byref(cracks), C.byref(entries))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    c, e = cracks.value, entries.value
    return dict(pos=pos, ids=ids[:c].copy(), rows=rows[:c].copy(), offsets=offsets[:c + 1].copy(), path=path[:e].copy(), cracks=c, path_points=e)


CD_WORD = ("links", "s1x", "s1y", "s1z", "s2xx", "s2xy", "s2xz", "s2yy", "s2yz", "s2zz")  # CD2: the moment words; CD4: a row holds (lo, hi) of each


def crack_axis_host(rows) -> dict:
    """CD5 on the rows of crack_directions (pcp_crack_axis_host: host only, fp64): rows (C, 20) int64 -> dict(link_count (C,)
    float64, the ordered links of every crack; axis (C, 3) float64, the unit direction of the crack with its largest component
    positive, zeros where there is none; axis_anisotropy (C,) float64)."""
    L = load()
    rows = np.ascontiguousarray(rows, np.int64).reshape(-1, 20)
    out = np.zeros((rows.shape[0], 5), np.float64)
    for k in range(rows.shape[0]):
        rc = L.pcp_crack_axis_host(_ptr(rows[k]), _ptr(out[k]))
        if rc != PCP_OK:
            raise PcpError(rc, L.pcp_last_error(None).decode())
    return dict(link_count=out[:, 0].copy(), axis=out[:, 1:4].copy(), axis_anisotropy=out[:, 4].copy())


def crack_directions_host(xyz, views, min_views: int = 1, radius: float = 0.02) -> dict:
    """What Context.crack_directions returns (with the moments, without the labels), computed on the CPU by brute force over the
    pairs (pcp_crack_directions_host: no context, no GPU): xyz (n, 3) float32, views (n,) uint32, n <= 65536."""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    views = np.ascontiguousarray(views, np.uint32)
    n = xyz.shape[0]
    if views.shape != (n,):
        raise ValueError(f"crack_directions_host: {n} views expected, got shape {views.shape}")
    tangent = np.zeros((n, 3), np.float32)
    anisotropy = np.zeros(n, np.float32)
    links = np.zeros(n, np.int32)
    moments = np.zeros((n, 10), np.int64)
    ids = np.empty(n, np.int32)
    rows = np.empty((n, 20), np.int64)
    cracks = C.c_int64()
    rc = L.pcp_crack_directions_host(C.c_int64(n), _ptr(xyz), _ptr(views), C.c_int32(min_views), C.c_float(radius), _ptr(tangent),
                                     _ptr(anisotropy), _ptr(links), _ptr(moments), _ptr(ids), _ptr(rows), C.byref(cracks))
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    c = cracks.value
    out = dict(tangent=tangent, anisotropy=anisotropy, links=links, moments=moments, ids=ids[:c].copy(), rows=rows[:c].copy(), cracks=c)
    out.update(crack_axis_host(out["rows"]))
    return out


CS_NODE = ("crack_row", "band", "points", "sum_w", "min_w", "max_w", "sum_qx", "sum_qy", "sum_qz", "degree")  # CS4: the columns of nodes
CS_EDGE = ("u", "v", "links")  # CS5
CS_CRACK = ("nodes", "edges", "ends", "junctions", "loops", "max_degree")  # CS6


def crack_skeleton_step(radius: float) -> float:
    """CS2's default in the host layers: 2 * radius, in fp32"""
    return float(np.float32(2.0) * np.float32(radius))


def crack_skeleton_metres(nodes, edges, cracks) -> dict:
    """CS7, host arithmetic on the integers of the three tables: centroids (N, 3) fp64 metres = (sum_q / points) * 2^-20 per
    axis, edge_length_m (E,) = sqrt((dx * dx + dy * dy) + dz * dz) of the two centroids, skeleton_length_m (C,) = the sum of a
    crack's edge lengths in row order."""
    nodes, edges = np.asarray(nodes, np.int64).reshape(-1, 10), np.asarray(edges, np.int64).reshape(-1, 3)
    centroids = (nodes[:, 6:9].astype(np.float64) / nodes[:, 2:3].astype(np.float64)) * 2.0 ** -20
    d = centroids[edges[:, 1]] - centroids[edges[:, 0]]
    edge_length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    length = np.zeros(len(np.asarray(cracks).reshape(-1, 6)), np.float64)
    np.add.at(length, nodes[edges[:, 0], 0], edge_length)  # (unbuffered: one addition per edge, in row order)
    return dict(centroids=centroids, edge_length_m=edge_length, skeleton_length_m=length)


def crack_skeleton_host(xyz, views, min_views: int = 1, radius: float = 0.02, step=None, sum_q=None) -> dict:
    """What Context.crack_skeleton returns, computed on the CPU by brute force over the pairs (pcp_crack_skeleton_host: no
    context, no GPU): xyz (n, 3) float32, views (n,) uint32, sum_q (n,) uint64 or None (every fused width 0), n <= 65536."""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    views = np.ascontiguousarray(views, np.uint32)
    n = xyz.shape[0]
    if views.shape != (n,):
        raise ValueError(f"crack_skeleton_host: {n} views expected, got shape {views.shape}")
    if sum_q is not None:
        sum_q = np.ascontiguousarray(sum_q, np.uint64)
        if sum_q.shape != (n,):
            raise ValueError(f"crack_skeleton_host: {n} sums expected, got shape {sum_q.shape}")
    if step is None:
        step = crack_skeleton_step(radius)
    node = np.empty(n, np.int32)
    ids = np.empty(n, np.int32)
    nodes = np.empty((n, 10), np.int64)
    cracks = np.empty((n, 6), np.int64)
    capacity = 4 * n + 16
    while True:
        edges = np.empty((capacity, 3), np.int64)
        kn, ke, kc = C.c_int64(), C.c_int64(), C.c_int64()
        rc = L.pcp_crack_skeleton_host(C.c_int64(n), _ptr(xyz), _ptr(views), C.c_int32(min_views), C.c_float(radius), C.c_float(step),
                                       _ptr(sum_q), _ptr(node), _ptr(ids), _ptr(nodes), C.c_int64(capacity), _ptr(edges), _ptr(cracks),
                                       C.byref(kn), C.byref(ke), C.byref(kc))
        if rc != PCP_OK:
            raise PcpError(rc, L.pcp_last_error(None).decode())
        if ke.value <= capacity:
            break
        capacity = ke.value  # (more edges than four per point: once more with room for all)
    out = dict(node=node, ids=ids[:kn.value].copy(), nodes=nodes[:kn.value].copy(), edges=edges[:ke.value].copy(), cracks=cracks[:kc.value].copy())
    out.update(crack_skeleton_metres(out["nodes"], out["edges"], out["cracks"]))
    return out


CB_ROW = ("crack_row", "nodes", "edges_inside", "attachments", "junction_u", "junction_v", "points", "sum_w", "min_w", "max_w",
          "pos_min", "pos_max", "sum_qx", "sum_qy", "sum_qz")  # CB5: the columns of rows
CB_CRACK = ("branches", "bridges", "junctions_kept", "ends_kept", "pruned_branches", "pruned_nodes", "pruned_points")  # CB7
CB_NO_POINT, CB_JUNCTION, CB_PRUNED = -1, -2, -3  # CB4: branch[] of a point outside every branch
CB_BRIDGE, CB_EDGE_PRUNED = -1, -2  # CB7: edge_branch[] of an edge outside every branch


def crack_branches_metres(rows, moments, edge_branch, nodes, edges, cracks) -> dict:
    """CB8 and the other host arithmetic on the integers of the branch tables: length_m (B,) = the sum, in edge-row order and
    one addition after the other, of CS7's edge lengths over the edges of the branch; kept_length_m (C,) = the same over a
    crack's edges that have no pruned end; centroid (B, 3) = (sum_q / points) * 2^-20; mean_width (B,) = (sum_w / points) * 2^-20
    metres; axis (B, 3), anisotropy (B,) and link_count (B,) by crack_axis_host on the moments."""
    rows = np.asarray(rows, np.int64).reshape(-1, 15)
    nodes, edges = np.asarray(nodes, np.int64).reshape(-1, 10), np.asarray(edges, np.int64).reshape(-1, 3)
    edge_branch = np.asarray(edge_branch, np.int32).reshape(-1)
    nodes, edges, edge_branch = np.ascontiguousarray(nodes), np.ascontiguousarray(edges), np.ascontiguousarray(edge_branch)
    length = np.zeros(len(rows), np.float64)
    kept = np.zeros(len(np.asarray(cracks).reshape(-1, 7)), np.float64)
    L = load()
    rc = L.pcp_crack_branch_lengths_host(C.c_int64(len(nodes)), _ptr(nodes), C.c_int64(len(edges)), _ptr(edges), _ptr(edge_branch),
                                         C.c_int64(len(length)), C.c_int64(len(kept)), _ptr(length), _ptr(kept))  # CB8, the one expression
    if rc != PCP_OK:
        raise PcpError(rc, L.pcp_last_error(None).decode())
    points = rows[:, 6:7].astype(np.float64)
    axes = crack_axis_host(moments)
    return dict(length_m=length, kept_length_m=kept, centroid=(rows[:, 12:15].astype(np.float64) / points) * 2.0 ** -20,
                mean_width=(rows[:, 7].astype(np.float64) / points[:, 0]) * 2.0 ** -20, axis=axes["axis"],
                anisotropy=axes["axis_anisotropy"], link_count=axes["link_count"])


def crack_branches_host(xyz, views, min_views: int = 1, radius: float = 0.02, step=None, prune: float = 0.0, sum_q=None) -> dict:
    """What Context.crack_branches returns, computed on the CPU by brute force over the pairs (pcp_crack_branches_host and
    pcp_crack_skeleton_host: no context, no GPU): xyz (n, 3) float32, views (n,) uint32, sum_q (n,) uint64 or None (every
    fused width 0), n <= 65536."""
    L = load()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    views = np.ascontiguousarray(views, np.uint32)
    n = xyz.shape[0]
    if views.shape != (n,):
        raise ValueError(f"crack_branches_host: {n} views expected, got shape {views.shape}")
    if sum_q is not None:
        sum_q = np.ascontiguousarray(sum_q, np.uint64)
        if sum_q.shape != (n,):
            raise ValueError(f"crack_branches_host: {n} sums expected, got shape {sum_q.shape}")
    if step is None:
        step = crack_skeleton_step(radius)
    branch = np.empty(n, np.int32)
    ids = np.empty(n, np.int32)
    rows = np.empty((n, 15), np.int64)
    moments = np.empty((n, 20), np.int64)
    cracks = np.empty((n, 7), np.int64)
    capacity = 4 * n + 16
    while True:
        edge_branch = np.empty(capacity, np.int32)
        kb, ke, kc = C.c_int64(), C.c_int64(), C.c_int64()
        rc = L.pcp_crack_branches_host(C.c_int64(n), _ptr(xyz), _ptr(views), C.c_int32(min_views), C.c_float(radius), C.c_float(step),
                                       C.c_float(prune), _ptr(sum_q), _ptr(branch), _ptr(ids), _ptr(rows), _ptr(moments), C.c_int64(capacity),
                                       _ptr(edge_branch), _ptr(cracks), C.byref(kb), C.byref(ke), C.byref(kc))
        if rc != PCP_OK:
            raise PcpError(rc, L.pcp_last_error(None).decode())
        if ke.value <= capacity:
            break
        capacity = ke.value  # (more edges than four per point: once more with room for all)
    out = dict(branch=branch, ids=ids[:kb.value].copy(), rows=rows[:kb.value].copy(), moments=moments[:kb.value].copy(),
               edge_branch=edge_branch[:ke.value].copy(), cracks=cracks[:kc.value].copy())
    sk = crack_skeleton_host(xyz, views, min_views, radius, step, sum_q)
    out.update(crack_branches_metres(out["rows"], out["moments"], out["edge_branch"], sk["nodes"], sk["edges"], out["cracks"]))
    return out


def default_camera() -> Camera:
    cam = Camera()
    load().pcp_default_camera(C.byref(cam))
    return cam


def camera_from_dict(d: dict) -> Camera:
    cam = Camera()
    for k, _ in Camera._fields_:
        setattr(cam, k, d[k])
    return cam


def default_cull_params() -> CullParams:
    p = CullParams()
    load().pcp_default_cull_params(C.byref(p))
    return p


def default_mls_params() -> MLSParams:
    p = MLSParams()
    load().pcp_default_mls_params(C.byref(p))
    return p


def pose_to_matrices(pose, T_opt=None):
    p = Pose(*[float(v) for v in pose])
    w2c = np.zeros(12, np.float32)
    c2w = np.zeros(12, np.float32)
    T = None if T_opt is None else np.ascontiguousarray(T_opt, np.float64).reshape(16)
    rc = load().pcp_pose_to_matrices(C.byref(p), _ptr(T), _ptr(w2c), _ptr(c2w))
    if rc != PCP_OK:
        raise PcpError(rc, load().pcp_last_error(None).decode())
    return w2c, c2w


class Context:
    """Owns one pcp_context (one GPU)."""

    def __init__(self, device: int = 0):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.pcp_create(C.c_int32(device), C.byref(h))
        if rc != PCP_OK:
            raise PcpError(rc, self.lib.pcp_last_error(None).decode())
        self.h = h
        self.n = 0
        self.normals_radius = None  # radius of the live pcp_estimate_normals result (None: none on this cloud)
        self.n_frames = 0
        self.camera = None
        self.cull = None

    # -- plumbing ---------------------------------------------------------
    def _check(self, rc: int):
        if rc != PCP_OK:
            raise PcpError(rc, self.lib.pcp_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.pcp_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr: int | None):
        self._check(self.lib.pcp_set_stream(self.h, C.c_void_p(stream_ptr or 0)))

    def synchronize(self):
        self._check(self.lib.pcp_synchronize(self.h))

    # -- configuration ----------------------------------------------------
    def set_camera(self, cam: Camera, cull: CullParams | None = None):
        self.camera = cam
        self.cull = cull if cull is not None else default_cull_params()
        self._check(self.lib.pcp_set_camera(self.h, C.byref(cam), C.byref(self.cull)))

    @property
    def map_shape(self):
        ds = self.cull.downsample_factor
        return (self.camera.cull_height // ds, self.camera.cull_width // ds)

    def upload_cloud(self, x, y, z):
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(y, np.float32)
        z = np.ascontiguousarray(z, np.float32)
        assert len(x) == len(y) == len(z)
        self.normals_radius = None
        self._check(self.lib.pcp_upload_cloud(self.h, _ptr(x), _ptr(y), _ptr(z), C.c_int64(len(x))))
        self.n = len(x)

    def upload_cloud_aos(self, pts: np.ndarray):
        pts = np.ascontiguousarray(pts)
        self.normals_radius = None
        self._check(self.lib.pcp_upload_cloud_aos(self.h, _ptr(pts), C.c_int64(pts.shape[0]),
                                                  C.c_int64(pts.strides[0])))
        self.n = pts.shape[0]

    def upload_cloud_from_result(self, src: "Context") -> int:
        """The rows of `src`'s latest smoothing result become this context's cloud, device to device
        (pcp_upload_cloud_from_result); returns the number of points."""
        n = C.c_int64()
        self.normals_radius = None
        self._check(self.lib.pcp_upload_cloud_from_result(self.h, src.h, C.byref(n)))
        self.n = n.value
        return n.value

    def set_frames(self, poses, T_opt=None):
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        F = len(poses)
        arr = (Pose * max(F, 1))()
        if F:
            C.memmove(arr, poses.ctypes.data, poses.nbytes)
        T = None
        stride = 0
        if T_opt is not None:
            T = np.ascontiguousarray(T_opt, np.float64).reshape(-1)
            stride = 16 if (T.size == 16 * F and F > 1) else 0
        self._check(self.lib.pcp_set_frames(self.h, arr, C.c_int32(F), _ptr(T), C.c_int32(stride)))
        self.n_frames = F

    def upload_image(self, frame: int, bgr: np.ndarray):
        bgr = np.ascontiguousarray(bgr, np.uint8)
        assert bgr.shape == (self.camera.image_height, self.camera.image_width, 3), bgr.shape
        self._check(self.lib.pcp_upload_image(self.h, C.c_int32(frame), _ptr(bgr), C.c_int64(bgr.strides[0])))

    def upload_image_async(self, frame: int, bgr: np.ndarray):
        """Queues the transfer only: `bgr` (ideally pinned) must stay alive and unchanged until synchronize()."""
        assert bgr.dtype == np.uint8 and bgr.flags.c_contiguous
        assert bgr.shape == (self.camera.image_height, self.camera.image_width, 3), bgr.shape
        self._check(self.lib.pcp_upload_image_async(self.h, C.c_int32(frame), _ptr(bgr), C.c_int64(bgr.strides[0])))

    def upload_images_block(self, first_frame: int, block: np.ndarray):
        """Keyframes first_frame ... from one (count, H, W, 3) array (ideally pinned): DMA in blocks, packed on the device."""
        assert block.dtype == np.uint8 and block.flags.c_contiguous and block.ndim == 4
        assert block.shape[1:] == (self.camera.image_height, self.camera.image_width, 3), block.shape
        self._check(self.lib.pcp_upload_images_block(self.h, C.c_int32(first_frame), C.c_int32(block.shape[0]), _ptr(block),
                                                     C.c_int64(block.strides[1]), C.c_int64(block.strides[0])))

    def upload_image_async_ptr(self, frame: int, ptr: int, row_stride_bytes: int):
        """The same from a raw address: pinned host memory or DEVICE memory (e.g. frames all-gathered over xGMI)."""
        self._check(self.lib.pcp_upload_image_async(self.h, C.c_int32(frame), C.c_void_p(ptr), C.c_int64(row_stride_bytes)))

    def upload_image_jpeg(self, frame: int, blob: np.ndarray):
        """A keyframe JPEG's coefficient blob (host/image_io.hpp jpeg_coefficients, `image_dump <in> <out> coeffs`; layout:
        pcp_jpeg_header in pcp_hip.h), reconstructed and packed on the device; returns once the texels are written."""
        blob = np.ascontiguousarray(blob, np.uint8).reshape(-1)
        self._check(self.lib.pcp_upload_image_jpeg(self.h, C.c_int32(frame), _ptr(blob), C.c_int64(blob.size)))

    def upload_image_jpeg_async(self, frame: int, blob: np.ndarray):
        """Queues the copy and the kernels only: `blob` must stay alive and unchanged until synchronize()."""
        assert blob.dtype == np.uint8 and blob.flags.c_contiguous
        self._check(self.lib.pcp_upload_image_jpeg_async(self.h, C.c_int32(frame), _ptr(blob), C.c_int64(blob.size)))

    def set_image_adjust(self, enable: bool = True, saturation_scale: float = 1.0, brightness_scale: float = 1.0):
        """generateColorMap's 8-bit BGR -> HSV -> BGR round trip applied to the images uploaded from now on."""
        self._check(self.lib.pcp_set_image_adjust(self.h, C.c_int32(1 if enable else 0), C.c_float(saturation_scale),
                                                  C.c_float(brightness_scale)))

    def set_image_balance(self, balance=True):
        """The keyframe colour balance (CLAHE on V, gamma table) applied on the device to the images uploaded from now on,
        before set_image_adjust's round trip (pcp_set_image_balance).  True: the defaults; a dict of balance_params()'s
        arguments; a BalanceParams; None / False: off."""
        p = _as_balance(balance)
        self._check(self.lib.pcp_set_image_balance(self.h, C.byref(p) if p is not None else None))

    def image_balance(self, bgr, params=True, stages: bool = False):
        """image_balance_host's computation on the device, by the kernels the upload path runs (pcp_image_balance);
        independent of the camera and of set_image_balance / set_image_adjust.  Same returns."""
        rc, res = _balance_call(self.lib.pcp_image_balance, "image_balance", (self.h,), params, bgr, True)
        self._check(rc)
        return res if stages else res["bgr"]

    def download_image(self, frame: int):
        """(bgr (H, W, 3), mask (H, W)) of one keyframe as the kernels sample it."""
        hh, ww = self.camera.image_height, self.camera.image_width
        bgr = np.empty((hh, ww, 3), np.uint8)
        mask = np.empty((hh, ww), np.uint8)
        self._check(self.lib.pcp_download_image(self.h, C.c_int32(frame), _ptr(bgr), _ptr(mask)))
        return bgr, mask

    def upload_mask(self, frame: int, gray: np.ndarray):
        gray = np.ascontiguousarray(gray, np.uint8)
        assert gray.shape == (self.camera.image_height, self.camera.image_width), gray.shape
        self._check(self.lib.pcp_upload_mask(self.h, C.c_int32(frame), _ptr(gray), C.c_int64(gray.strides[0])))

    # -- single keyframe --------------------------------------------------
    def project_frame(self, frame: int, want_pixel=True, want_cam=True, device_only=False):
        if device_only:
            self._check(self.lib.pcp_project_frame(self.h, C.c_int32(frame), None, None, None, None))
            return None
        n = self.n
        cell = np.empty(n, np.int32)
        rng = np.empty(n, np.float32)
        pix = np.empty(n, np.int32) if want_pixel else None
        cam = np.empty((3, n), np.float32) if want_cam else None
        self._check(self.lib.pcp_project_frame(self.h, C.c_int32(frame), _ptr(cell), _ptr(pix), _ptr(rng), _ptr(cam)))
        out = dict(cell=cell, range=rng)
        if want_pixel:
            out["pixel"] = pix
        if want_cam:
            out.update(xc=cam[0], yc=cam[1], zc=cam[2])
        return out

    def cull_frame(self, frame: int):
        keep = np.empty(self.n, np.uint8)
        mh, mw = self.map_shape
        dmap = np.empty(mh * mw, np.float32)
        kept = C.c_int64()
        self._check(self.lib.pcp_cull_frame(self.h, C.c_int32(frame), _ptr(keep), C.byref(kept), _ptr(dmap)))
        return keep, dmap.reshape(mh, mw), kept.value

    def cull_frame_into(self, frame: int, device_ptr: int) -> int:
        """pcp_cull_frame with the n keep flags written to DEVICE memory of this context's GPU (ABI v5): the multi-GPU hosts
        exchange them with RCCL.  Returns the number kept."""
        kept = C.c_int64()
        self._check(self.lib.pcp_cull_frame(self.h, C.c_int32(frame), C.c_void_p(device_ptr), C.byref(kept), None))
        return kept.value

    def hull_flags_import_ptr(self, frame: int, device_ptr: int):
        """pcp_hull_flags_import from device memory (n flags of THIS context's points)."""
        self._check(self.lib.pcp_hull_flags_import(self.h, C.c_int32(frame), C.c_void_p(device_ptr)))

    def hpr_stats(self) -> dict:
        """Counters of the last hidden_points_removal run (pcp_hpr_stats)."""
        out = np.zeros(10, np.int64)
        self._check(self.lib.pcp_hpr_stats(self.h, _ptr(out)))
        keys = ("visible", "hidden", "exact_path", "trial_normals", "test_batches", "reserved", "unresolved",
                "exact_evaluations", "cells", "candidates")
        return {k: int(v) for k, v in zip(keys, out)}

    def frame_visible(self, frame: int, capacity: int | None = None):
        cap = self.n if capacity is None else capacity
        idx = np.empty(cap, np.int32)
        rgb = np.empty((cap, 3), np.uint8)
        mv = np.empty(cap, np.uint16)
        cam = np.empty((cap, 3), np.float32)
        wrd = np.empty((cap, 3), np.float32)
        cnt = C.c_int64()
        self._check(self.lib.pcp_frame_visible(self.h, C.c_int32(frame), C.c_int64(cap), _ptr(idx), _ptr(rgb), _ptr(mv),
                                               _ptr(cam), _ptr(wrd), C.byref(cnt)))
        m = min(cnt.value, cap)
        return dict(index=idx[:m], rgb=rgb[:m], mask=mv[:m], xyz_cam=cam[:m], xyz_world=wrd[:m], count=cnt.value)

    # -- whole run --------------------------------------------------------
    def depth_pass(self, f0: int = 0, f1: int | None = None):
        self._check(self.lib.pcp_depth_pass(self.h, C.c_int32(f0), C.c_int32(self.n_frames if f1 is None else f1)))

    def depth_maps_device(self):
        p = C.c_void_p()
        n = C.c_int64()
        self._check(self.lib.pcp_depth_maps_device(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def set_depth_source(self, batched: bool):
        """PCP_DEPTH_BATCHED: the single-keyframe calls use the maps pcp_depth_pass left (MIN-merged across shards)."""
        self._check(self.lib.pcp_set_depth_source(self.h, C.c_int32(1 if batched else 0)))

    def hull_flags_import(self, frame: int, keep):
        """PCP_CULL_HPR on an index shard: the verdicts of keyframe `frame` for this context's points, from a whole-map context."""
        a = np.ascontiguousarray(keep, np.uint8)
        assert len(a) == self.n
        self._check(self.lib.pcp_hull_flags_import(self.h, C.c_int32(frame), _ptr(a)))

    def download_depth_map(self, frame: int):
        mh, mw = self.map_shape
        d = np.empty(mh * mw, np.float32)
        self._check(self.lib.pcp_download_depth_map(self.h, C.c_int32(frame), _ptr(d)))
        return d.reshape(mh, mw)

    # depth-map accumulator: survives the uploads (a chunk of a streamed cloud is an index shard in time)
    def depth_accum_reset(self):
        self._check(self.lib.pcp_depth_accum_reset(self.h))

    def depth_accum_merge(self):
        self._check(self.lib.pcp_depth_accum_merge(self.h))

    def depth_accum_apply(self):
        self._check(self.lib.pcp_depth_accum_apply(self.h))

    def depth_accum_device(self):
        p = C.c_void_p()
        n = C.c_int64()
        self._check(self.lib.pcp_depth_accum_device(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def colour_compact(self, capacity: int | None = None, want_label: bool = False):
        """removePointsWithNoColor on the device (pcp_colour_compact): dict(index, xyz, rgb[, label], count) of the rows of
        the colour result that have a colour, input order; count is the true count even when capacity is smaller."""
        cap = self.n if capacity is None else capacity
        idx = np.empty(cap, np.int32)
        xyz = np.empty((cap, 3), np.float32)
        rgb = np.empty((cap, 3), np.uint8)
        label = np.empty(cap, np.uint8) if want_label else None
        cnt = C.c_int64()
        self._check(self.lib.pcp_colour_compact(self.h, C.c_int64(cap), _ptr(idx), _ptr(xyz), _ptr(rgb), _ptr(label), C.byref(cnt)))
        m = min(cnt.value, cap)
        out = dict(index=idx[:m], xyz=xyz[:m], rgb=rgb[:m], count=cnt.value)
        if want_label:
            out["label"] = label[:m]
        return out

    # -- device PCD writer ---------------------------------------------------
    def ascii_rows(self, kind: int, f, rgb=None, mask=None, capacity: int | None = None, out=None) -> np.ndarray:
        """ascii_rows_host's rows formatted on the device (pcp_ascii_rows): the text as a numpy.uint8 array."""
        fn = lambda *a: self.lib.pcp_ascii_rows(self.h, *a)  # noqa: E731
        return _ascii_rows_call(fn, self._check, kind, f, rgb, mask, capacity, out)

    def _ascii_window(self, call, bound: int, total_rows: int, first_row: int, max_rows: int | None, capacity: int | None):
        if max_rows is None:
            max_rows = max(0, total_rows - first_row)
        cap = max(0, min(max_rows, max(0, total_rows - first_row))) * bound if capacity is None else capacity
        out = np.empty(max(cap, 0), np.uint8)
        rows = C.c_int64(-1)
        nbytes = C.c_int64(-1)
        try:
            self._check(call(C.c_int64(first_row), C.c_int64(max_rows), C.c_int64(cap), _ptr(out), C.byref(rows), C.byref(nbytes)))
        except PcpError as e:
            e.bytes = nbytes.value
            raise
        return out[: nbytes.value], rows.value

    def colour_compact_ascii(self, with_label: bool = False, first_row: int = 0, max_rows: int | None = None,
                             capacity: int | None = None):
        """(text, rows): rows [first_row, first_row + max_rows) of colour_compact() as XYZRGB text, or XYZRGBMASK text with
        the fused label (pcp_colour_compact_ascii); max_rows None = to the end."""
        kind = ROWS_XYZRGBMASK if with_label else ROWS_XYZRGB
        call = lambda *a: self.lib.pcp_colour_compact_ascii(self.h, C.c_int32(1 if with_label else 0), *a)  # noqa: E731
        return self._ascii_window(call, ascii_row_bound(kind), self.n, first_row, max_rows, capacity)

    def mls_fetch_ascii(self, count: int, first_row: int = 0, max_rows: int | None = None, capacity: int | None = None):
        """(text, rows): rows [first_row, first_row + max_rows) of mls_fetch(count) as PointNormal text
        (pcp_mls_fetch_ascii); count = the rows of the latest smoothing result."""
        call = lambda *a: self.lib.pcp_mls_fetch_ascii(self.h, *a)  # noqa: E731
        return self._ascii_window(call, ascii_row_bound(ROWS_POINTNORMAL), count, first_row, max_rows, capacity)

    # -- device PCD reader ---------------------------------------------------
    def ascii_parse(self, text, columns: int, col, final: bool = True, max_rows: int | None = None, out=None):
        """ascii_parse_host's window parsed on the device (pcp_ascii_parse): (x, y, z, intensity, consumed, bad_row)."""
        fn = lambda *a: self.lib.pcp_ascii_parse(self.h, *a)  # noqa: E731
        return _ascii_parse_call(fn, self._check, text, columns, col, final, max_rows, out)

    def colour_reset(self):
        self._check(self.lib.pcp_colour_reset(self.h))

    def colour_pass(self, f0: int = 0, f1: int | None = None):
        self._check(self.lib.pcp_colour_pass(self.h, C.c_int32(f0), C.c_int32(self.n_frames if f1 is None else f1)))

    def colour_finalise(self, want_top: bool = False, download: bool = True):
        n = self.n
        rgb = np.empty((n, 3), np.uint8) if download else None
        has = np.empty(n, np.uint8) if download else None
        cnt = np.empty(n, np.int32) if want_top else None
        ts = np.empty((n, 5), np.float32) if want_top else None
        tr = np.empty((n, 5), np.uint32) if want_top else None
        tf = np.empty((n, 5), np.int32) if want_top else None
        self._check(self.lib.pcp_colour_finalise(self.h, _ptr(rgb), _ptr(has), _ptr(cnt), _ptr(ts), _ptr(tr), _ptr(tf)))
        return dict(rgb=rgb, has=has, count=cnt, top_score=ts, top_rgb=tr, top_frame=tf)

    def colorize(self, download: bool = True):
        n = self.n
        rgb = np.empty((n, 3), np.uint8) if download else None
        has = np.empty(n, np.uint8) if download else None
        self._check(self.lib.pcp_colorize(self.h, _ptr(rgb), _ptr(has)))
        return dict(rgb=rgb, has=has)

    def colorize_from_depth(self, download: bool = True):
        n = self.n
        rgb = np.empty((n, 3), np.uint8) if download else None
        has = np.empty(n, np.uint8) if download else None
        self._check(self.lib.pcp_colorize_from_depth(self.h, _ptr(rgb), _ptr(has)))
        return dict(rgb=rgb, has=has)

    def download_result_packed(self, out: np.ndarray | None = None, out_ptr: int | None = None):
        """n uint32 words r | g<<8 | b<<16 | has<<24 (out_ptr: e.g. a pinned host buffer)."""
        if out_ptr is not None:
            self._check(self.lib.pcp_download_result_packed(self.h, C.c_void_p(out_ptr)))
            return None
        if out is None:
            out = np.empty(self.n, np.uint32)
        self._check(self.lib.pcp_download_result_packed(self.h, _ptr(out)))
        return out

    def download_result_packed_async(self, out_ptr: int):
        """Enqueue the device-to-host copy on the copy stream; valid after synchronize()."""
        self._check(self.lib.pcp_download_result_packed_async(self.h, C.c_void_p(out_ptr)))

    def download_wait_previous(self):
        self._check(self.lib.pcp_download_wait_previous(self.h))

    def colour_result_device(self):
        p = C.c_void_p()
        n = C.c_int64()
        self._check(self.lib.pcp_colour_result_device(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def set_label_fusion(self, enable: bool = True):
        """Fused segmentation labels (pcp_hip.h): with it on, every colour result carries label / hits / views per point
        from the masks of the point's top-5 views.  PCP_ERR_STATE while a top-5 accumulation is live."""
        self._check(self.lib.pcp_set_label_fusion(self.h, C.c_int32(1 if enable else 0)))

    def colour_labels(self):
        """dict(label, hits, views): n uint8 each, input order, of the latest colour result (produced with fusion on)."""
        n = self.n
        label, hits, views = (np.empty(n, np.uint8) for _ in range(3))
        self._check(self.lib.pcp_colour_labels(self.h, _ptr(label), _ptr(hits), _ptr(views)))
        return dict(label=label, hits=hits, views=views)

    def colour_labels_device(self):
        """(device pointer, n) of the packed words label | hits<<8 | views<<16; valid until the next colour result begins
        (one buffer, not double-buffered)."""
        p = C.c_void_p()
        n = C.c_int64()
        self._check(self.lib.pcp_colour_labels_device(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    # -- exposure gains ("Exposure gains") -------------------------
    def view_pair_stats(self):
        """(n, sum): (F, F) uint64 each -- over the live top-5 lists, the pairs of usable views of one point from two
        keyframes and the luma sums of the row keyframe's side (pcp_view_pair_stats).  Additive over index shards."""
        F = self.n_frames
        n = np.zeros((F, F), np.uint64)
        s = np.zeros((F, F), np.uint64)
        self._check(self.lib.pcp_view_pair_stats(self.h, _ptr(n), _ptr(s)))
        return n, s

    def view_pair_stats_counters(self) -> dict:
        """What the latest view_pair_stats() issued (pcp_view_pair_stats_counters)."""
        out = np.zeros(5, np.int64)
        self._check(self.lib.pcp_view_pair_stats_counters(self.h, _ptr(out)))
        keys = ("flush_adds", "direct_adds", "wave_partials", "workgroups", "table_slots")
        return {k: int(v) for k, v in zip(keys, out)}

    def set_frame_gains(self, gains):
        """One gain per keyframe, applied per listed view by colour_finalise (pcp_set_frame_gains); None switches it off.
        colorize() / colorize_from_depth() raise PCP_ERR_STATE while gains are set; set_frames clears them."""
        if gains is None:
            self._check(self.lib.pcp_set_frame_gains(self.h, None, C.c_int32(0)))
            return
        g = np.ascontiguousarray(gains, np.float64).reshape(-1)
        self._check(self.lib.pcp_set_frame_gains(self.h, _ptr(g), C.c_int32(g.size)))

    # -- voxel-grid output ("Voxel-grid output") ----------------------
    def voxel_reduce_begin(self, leaf: float, initial_slots: int = 0):
        """Starts an empty voxel accumulation of edge `leaf` on this context (pcp_voxel_reduce_begin); it outlives uploads,
        colour resets, set_frames and set_camera."""
        self._check(self.lib.pcp_voxel_reduce_begin(self.h, C.c_float(leaf), C.c_int64(initial_slots)))

    def voxel_reduce_add(self) -> int:
        """Adds the coloured rows of the current colour result (those colour_compact() returns); returns their number."""
        rows = C.c_int64()
        self._check(self.lib.pcp_voxel_reduce_add(self.h, C.byref(rows)))
        return rows.value

    def voxel_reduce_finish(self) -> int:
        """Sorts the occupied voxels by key and computes their rows; returns their number."""
        vox = C.c_int64()
        self._check(self.lib.pcp_voxel_reduce_finish(self.h, C.byref(vox)))
        return vox.value

    def voxel_reduce_fetch(self, first: int = 0, max_rows: int | None = None, want_label: bool = False) -> dict:
        """dict(xyz, rgb[, label], count) of rows [first, first + max_rows) of the finished result; max_rows None = to the end."""
        if max_rows is None:
            max_rows = max(0, self.voxel_reduce_stats()["voxels"] - first)
        cap = max(max_rows, 0)
        xyz = np.empty((cap, 3), np.float32)
        rgb = np.empty((cap, 3), np.uint8)
        label = np.empty(cap, np.uint8) if want_label else None
        cnt = np.empty(cap, np.uint32)
        rows = C.c_int64()
        self._check(self.lib.pcp_voxel_reduce_fetch(self.h, C.c_int64(first), C.c_int64(max_rows), _ptr(xyz), _ptr(rgb), _ptr(label),
                                                    _ptr(cnt), C.byref(rows)))
        m = rows.value
        out = dict(xyz=xyz[:m], rgb=rgb[:m], count=cnt[:m])
        if want_label:
            out["label"] = label[:m]
        return out

    def voxel_reduce_stats(self) -> dict:
        out = np.zeros(6, np.int64)
        self._check(self.lib.pcp_voxel_reduce_stats(self.h, _ptr(out)))
        keys = ("rows", "voxels", "slots", "growths", "wave_partials", "global_adds")
        return {k: int(v) for k, v in zip(keys, out)}

    def voxel_reduce_end(self):
        self._check(self.lib.pcp_voxel_reduce_end(self.h))

    # -- orthographic maps ("Orthographic maps") -------------------------
    def ortho_begin(self, frame):
        """Starts an empty orthographic map of `frame` (an OrthoFrame, or a dict of its fields) on this context
        (pcp_ortho_begin); it outlives uploads, colour resets, set_frames and set_camera."""
        f = ortho_frame(frame)
        self._check(self.lib.pcp_ortho_begin(self.h, C.byref(f)))
        self._ortho_frame = f  # (only of a begin the library took: a refused one leaves the live map, and its frame, as they were)

    def ortho_begin_cyl(self, frame):
        """Starts an empty unrolled map of the cylinder `frame` (a CylFrame, or a dict of its fields) on this context
        (pcp_ortho_begin_cyl; DESIGN.md, "Cylindrical facets"); the adds, finish, fetch, stats and end are ortho_begin's."""
        f = cyl_frame(frame)
        self._check(self.lib.pcp_ortho_begin_cyl(self.h, C.byref(f)))
        self._ortho_frame = f  # (the shape of the last begin the library took, of either kind)

    def ortho_add(self, index_base: int = 0) -> int:
        """Adds the coloured rows of the current colour result under the global indices index_base + row; returns the
        number of contributors (rows inside the raster and the depth window)."""
        rows = C.c_int64()
        self._check(self.lib.pcp_ortho_add(self.h, C.c_int64(index_base), C.byref(rows)))
        return rows.value

    def ortho_add_facet(self, facet_id: int, index_base: int = 0) -> int:
        """ortho_add restricted to the rows whose facet label (the last facets call) is facet_id: the colour and fused-label
        layers are kept (pcp_ortho_add_facet).  Returns the number of contributors."""
        rows = C.c_int64()
        self._check(self.lib.pcp_ortho_add_facet(self.h, C.c_int32(facet_id), C.c_int64(index_base), C.byref(rows)))
        return rows.value

    def ortho_add_packed(self, rgba, index_base: int = 0) -> int:
        """Adds the uploaded cloud with the caller's words r | g<<8 | b<<16 | has<<24 (n of them: a numpy array, or an int
        that is a device pointer of this context's GPU); the label is 0.  Returns the number of contributors."""
        rows = C.c_int64()
        if isinstance(rgba, int):
            words = C.c_void_p(rgba)
        else:
            keep = np.ascontiguousarray(rgba, np.uint32).reshape(-1)
            if keep.size != self.n:
                raise ValueError(f"ortho_add_packed: {self.n} words expected, got shape {keep.shape}")
            words = _ptr(keep)
        self._check(self.lib.pcp_ortho_add_packed(self.h, words, C.c_int64(index_base), C.byref(rows)))
        return rows.value

    def ortho_finish(self, fill_radius: int = 0) -> tuple[int, int]:
        """Ends the adds; fill_radius > 0 fills empty pixels from their nearest occupied pixel within that many pixels.
        Returns (occupied, filled)."""
        occ, fil = C.c_int64(), C.c_int64()
        self._check(self.lib.pcp_ortho_finish(self.h, C.c_int32(fill_radius), C.byref(occ), C.byref(fil)))
        return occ.value, fil.value

    def ortho_fetch(self, want_label: bool = False) -> dict:
        """dict(index, depth, rgb[, label], status, source) of the finished map, each (H, W) (rgb (H, W, 3))."""
        f = getattr(self, "_ortho_frame", None)
        if f is None:  # no map was ever begun on this context: the library says so
            self._check(self.lib.pcp_ortho_fetch(self.h, None, None, None, None, None, None))
            raise PcpError(PCP_ERR_STATE, "ortho_fetch: no map")
        h, w = int(f.height), int(f.width)
        out = dict(index=np.empty((h, w), np.uint32), depth=np.empty((h, w), np.float32), rgb=np.empty((h, w, 3), np.uint8),
                   status=np.empty((h, w), np.uint8), source=np.empty((h, w), np.int32))
        label = np.empty((h, w), np.uint8) if want_label else None
        self._check(self.lib.pcp_ortho_fetch(self.h, _ptr(out["index"]), _ptr(out["depth"]), _ptr(out["rgb"]), _ptr(label),
                                             _ptr(out["status"]), _ptr(out["source"])))
        if want_label:
            out["label"] = label
        return out

    def ortho_stats(self) -> dict:
        out = np.zeros(6, np.int64)
        self._check(self.lib.pcp_ortho_stats(self.h, _ptr(out)))
        keys = ("contributors", "atomics", "occupied", "filled", "adds", "pixels")
        return {k: int(v) for k, v in zip(keys, out)}

    def ortho_end(self):
        self._check(self.lib.pcp_ortho_end(self.h))
        self._ortho_frame = None

    # -- surface defects on ortho maps ("Surface defects on ortho maps") ---
    def ortho_defects(self, threshold: float = 0.002, window: int = 0, refine: bool = False, min_support: int = 1, min_pixels: int = 1,
                      classes: int = 3) -> dict:
        """The surface defects of the live, finished map (pcp_ortho_defects): hollows and bulges of its depth layer beyond
        `threshold` metres against the mean of a (2 window + 1)-pixel square (window 0: against the frame's own surface).
        Returns the eight counts (DEFECT_OUT); the layers and the table stay on the device for ortho_defects_fetch / _table."""
        p = ortho_defect_params(threshold, window, refine, min_support, min_pixels, classes)
        out = np.zeros(8, np.int64)
        self._check(self.lib.pcp_ortho_defects(self.h, C.byref(p), _ptr(out)))
        return {k: int(v) for k, v in zip(DEFECT_OUT, out)}

    def ortho_defects_fetch(self) -> dict:
        """dict(dev int32 in quanta of 2^-20 m, cls uint8 (0, 1 hollow, 2 bulge), region int32 (0: none)), each (H, W)."""
        f = getattr(self, "_ortho_frame", None)
        if f is None:  # no map was ever begun on this context: the library says so
            self._check(self.lib.pcp_ortho_defects_fetch(self.h, None, None, None))
            raise PcpError(PCP_ERR_STATE, "ortho_defects_fetch: no map")
        self._check(self.lib.pcp_ortho_defects_fetch(self.h, None, None, None))  # (the state, before anything is allocated)
        h, w = int(f.height), int(f.width)
        out = dict(dev=np.empty((h, w), np.int32), cls=np.empty((h, w), np.uint8), region=np.empty((h, w), np.int32))
        self._check(self.lib.pcp_ortho_defects_fetch(self.h, _ptr(out["dev"]), _ptr(out["cls"]), _ptr(out["region"])))
        return out

    def ortho_defects_table(self, first: int = 0, max_rows: int | None = None) -> np.ndarray:
        """Rows first .. first + max_rows - 1 (None: every row from `first`) of the last ortho_defects call's table
        (pcp_ortho_defects_table): (rows, 16) int64, the columns of DEFECT_ROW."""
        have = C.c_int64()
        self._check(self.lib.pcp_ortho_defects_table(self.h, C.c_int64(first), C.c_int64((1 << 62) if max_rows is None else max_rows), None,
                                                     C.byref(have)))
        rows = np.zeros((have.value, 16), np.int64)
        if have.value:
            got = C.c_int64()
            self._check(self.lib.pcp_ortho_defects_table(self.h, C.c_int64(first), C.c_int64(have.value), _ptr(rows), C.byref(got)))
        return rows

    def ortho_texture(self, scale: int, views: int = 1, interpolate: bool = True, max_step: float = 0.05, rect=None) -> dict:
        """The orthophoto of the finished map at `scale` fine pixels per ortho pixel and axis, coloured straight from the
        keyframe images (pcp_ortho_texture; DESIGN.md, "Orthophotos").  rect: (x0, y0, w, h) in ortho pixels, None: the whole
        raster.  dict(rgb (h k, w k, 3), mask, status, view (int16), count, surface, textured, unseen, skipped_pairs)."""
        return self._ortho_texture(self.lib.pcp_ortho_texture, scale, views, interpolate, max_step, rect)

    def _ortho_texture(self, fn, scale, views, interpolate, max_step, rect) -> dict:
        p = ortho_texture_params(scale, views, interpolate, max_step, rect)
        f = getattr(self, "_ortho_frame", None)
        fh, fw = _ortho_texture_shape(f, p) if f is not None else (0, 0)
        out = dict(rgb=np.empty((fh, fw, 3), np.uint8), mask=np.empty((fh, fw), np.uint8), status=np.empty((fh, fw), np.uint8),
                   view=np.empty((fh, fw), np.int16), count=np.empty((fh, fw), np.uint8))
        counts = np.zeros(4, np.int64)
        self._check(fn(self.h, C.byref(p), _ptr(out["rgb"]), _ptr(out["mask"]), _ptr(out["status"]), _ptr(out["view"]),
                       _ptr(out["count"]), _ptr(counts)))
        out.update(surface=int(counts[0]), textured=int(counts[1]), unseen=int(counts[2]), skipped_pairs=int(counts[3]))
        return out

    def ortho_texture_cyl(self, scale: int, views: int = 1, interpolate: bool = True, max_step: float = 0.05, rect=None) -> dict:
        """ortho_texture for the finished unrolled map of a cylinder (pcp_ortho_texture_cyl; DESIGN.md, "Orthophotos of unrolled
        maps"): the same keywords and the same dict.  A planar map is refused, as ortho_texture refuses a cylinder's."""
        return self._ortho_texture(self.lib.pcp_ortho_texture_cyl, scale, views, interpolate, max_step, rect)

    # -- geometry maps ("Geometry maps") ---------------------------------
    def estimate_normals(self, radius: float, want_moments: bool = False):
        """A normal, a curvature and a neighbour count per point of the uploaded cloud, kept on the device until the next
        upload (pcp_estimate_normals).  Returns the number of valid points; with want_moments (valid, moments (n, 10) int64)."""
        valid = C.c_int64()
        mom = np.zeros((self.n, 10), np.int64) if want_moments else None
        self.normals_radius = None
        self._check(self.lib.pcp_estimate_normals(self.h, C.c_float(radius), C.byref(valid), _ptr(mom)))
        self.normals_radius = radius
        return (valid.value, mom) if want_moments else valid.value

    def normals_fetch(self) -> dict:
        """dict(normal (n, 3) float32, curvature (n,) float32, neighbours (n,) int32) of the last estimate, input order."""
        nrm = np.zeros((self.n, 3), np.float32)
        cur = np.zeros(self.n, np.float32)
        cnt = np.zeros(self.n, np.int32)
        self._check(self.lib.pcp_normals_fetch(self.h, _ptr(nrm), _ptr(cur), _ptr(cnt)))
        return dict(normal=nrm, curvature=cur, neighbours=cnt)

    def frame_geometry(self, frame: int, normals: bool = True) -> dict:
        """The geometry maps of one keyframe at camera resolution (pcp_frame_geometry): dict(index (H, W) int32, -1 = empty,
        range (H, W) float32, xyz_cam (H, W, 3) float32, pixels = occupied count, and with normals normal_cam (H, W, 3))."""
        hh, ww = self.camera.image_height, self.camera.image_width
        idx = np.empty((hh, ww), np.int32)
        rng = np.empty((hh, ww), np.float32)
        cam = np.empty((hh, ww, 3), np.float32)
        nrm = np.empty((hh, ww, 3), np.float32) if normals else None
        px = C.c_int64()
        self._check(self.lib.pcp_frame_geometry(self.h, C.c_int32(frame), _ptr(idx), _ptr(rng), _ptr(cam), _ptr(nrm), C.byref(px)))
        out = dict(index=idx, range=rng, xyz_cam=cam, pixels=px.value)
        if normals:
            out["normal_cam"] = nrm
        return out

    # -- map comparison ("Map comparison") ---------------------------------
    def compare_set_base(self, base_xyz):
        """The earlier survey the map is compared with: (n_base, >= 3) float32 rows, xyz first (pcp_compare_set_base).  Kept
        across uploads until compare_end or close; a second call replaces the first."""
        base = np.ascontiguousarray(base_xyz, np.float32)
        if base.ndim != 2 or base.shape[1] < 3:
            base = base.reshape(-1, 3)
        stride = 4 * base.shape[1]
        self._check(self.lib.pcp_compare_set_base(self.h, _ptr(base), C.c_int64(base.shape[0]), C.c_int64(stride)))
        self.n_base = base.shape[0]  # (the coarse registration's fetches are sized by it)

    def compare(self, radius: float = 0.03, half_length: float = 0.05, reg_error: float = 0.0, min_points: int = 5,
                orient_mode: int = 0, orient=(0.0, 0.0, 0.0), normals=None) -> dict:
        """The signed distance of every core point of the uploaded cloud to the base along its oriented normal, with its level
        of detection (pcp_compare and its fetch): dict(distance, lod (n,) float32, status (n,) uint8, sums (n, 8) int64 with the
        columns MC_SUMS, direction (n, 3) int32, stats (8,) int64 with the entries MC_STATS).  normals: (n, 3) float32, or
        None for the live estimate of estimate_normals."""
        if normals is not None:
            normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
            if normals.shape[0] != self.n:
                raise ValueError("compare: normals must hold one row per point of the uploaded cloud")
        prm = compare_params(radius, half_length, reg_error, min_points, orient_mode, orient)
        stats = np.zeros(8, np.int64)
        self._check(self.lib.pcp_compare(self.h, C.byref(prm), _ptr(normals), _ptr(stats)))
        out = self.compare_fetch()
        out["stats"] = stats
        return out

    def compare_fetch(self) -> dict:
        """The arrays of the last compare, input order (pcp_compare_fetch)."""
        out = _compare_outputs(self.n)
        self._check(self.lib.pcp_compare_fetch(self.h, _ptr(out["distance"]), _ptr(out["lod"]), _ptr(out["status"]),
                                               _ptr(out["sums"]), _ptr(out["direction"])))
        return out

    def compare_end(self):
        """Drops the base and the result (pcp_compare_end)."""
        self._check(self.lib.pcp_compare_end(self.h))

    # -- map registration ("Map registration") -----------------------------
    def _register_normals(self, who, normals):
        if normals is None:
            return None
        normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if normals.shape[0] != self.n:
            raise ValueError(f"{who}: normals must hold one row per point of the uploaded cloud")
        return normals

    def compare_register_sums(self, normals=None, **params):
        """One evaluation of the registration's sums at the base's current transform (pcp_compare_register_sums): (60,) int64,
        term k of RG_TERMS in words 2 k (low parts) and 2 k + 1 (high parts).  params: those of register_params."""
        normals = self._register_normals("compare_register_sums", normals)
        prm = register_params(**params)
        sums = np.zeros(60, np.int64)
        self._check(self.lib.pcp_compare_register_sums(self.h, C.byref(prm), _ptr(normals), _ptr(sums)))
        return sums

    def compare_register(self, normals=None, **params) -> dict:
        """Brings the base onto the uploaded cloud by point-to-plane ICP from its current transform (pcp_compare_register):
        dict(T (4, 4) float64, log (iterations, 5) float64 with the columns RG_LOG, status, iterations, rms, dof, pairs of the
        last iteration).  The rms is what a caller may pass to compare as reg_error."""
        normals = self._register_normals("compare_register", normals)
        prm = register_params(**params)
        T = np.zeros((4, 4), np.float64)
        log, status = np.zeros((max(1, min(prm.max_iterations, 1000)), 5), np.float64), np.zeros(2, np.int32)
        self._check(self.lib.pcp_compare_register(self.h, C.byref(prm), _ptr(normals), _ptr(T), _ptr(log), _ptr(status)))
        return _register_result(T, log, status)

    def compare_base_transform(self) -> dict:
        """The base's current transform (pcp_compare_base_transform): dict(T (4, 4) float64, pivot (3,), ell)."""
        T, pivot, ell = np.zeros((4, 4), np.float64), np.zeros(3, np.float64), C.c_double()
        self._check(self.lib.pcp_compare_base_transform(self.h, _ptr(T), _ptr(pivot), C.byref(ell)))
        return dict(T=T, pivot=pivot, ell=ell.value)

    def compare_set_base_transform(self, T):
        """Sets the base's transform to a caller's rigid 4 x 4; the identity restores the original rows
        (pcp_compare_set_base_transform)."""
        T = np.ascontiguousarray(T, np.float64).reshape(16)
        self._check(self.lib.pcp_compare_set_base_transform(self.h, _ptr(T)))

    # -- coarse registration ("Coarse registration") -----------------------
    def _coarse_normals(self, who, side, normals):
        if normals is None:
            return None
        normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        rows = self.n if side == CG_MAP else getattr(self, "n_base", 0)
        if normals.shape[0] != rows:
            raise ValueError(f"{who}: normals must hold one row per {'point of the uploaded cloud' if side == CG_MAP else 'row of the base'}")
        return normals

    def _coarse_live(self) -> dict:
        # what the library holds after the calls made through this Context: the valid descriptors per side (CG_MAP, CG_BASE) and
        # the correspondences ("pairs").  The fetches copy as much as the library holds, so their buffers are sized from here and
        # never from a caller's figure; an entry is missing whenever this Context cannot vouch for it.
        if not hasattr(self, "_cg_live"):
            self._cg_live = {}
        return self._cg_live

    def coarse_descriptors(self, side: int, normals=None, fetch: bool = True, **params) -> dict:
        """The keypoints and spin-image descriptors of one side on the device (pcp_coarse_descriptors and its fetch): dict(slots,
        keypoints, valid, and with fetch desc (slots, 64) uint16, total (slots,) uint32, state (slots,) uint8, xyz (slots, 3)
        float32).  side CG_MAP: normals (n, 3) or None for the live estimate; CG_BASE: normals (n_base, 3) or None to estimate them
        on the device at normal_radius.  params: those of coarse_params."""
        normals = self._coarse_normals("coarse_descriptors", side, normals)
        prm = coarse_params(**params)
        counts = np.zeros(3, np.int64)
        live = self._coarse_live()
        live.pop(side, None), live.pop("pairs", None)  # (the library drops both first; a failed call leaves neither)
        self._check(self.lib.pcp_coarse_descriptors(self.h, C.byref(prm), C.c_int32(side), _ptr(normals), _ptr(counts)))
        out = dict(slots=int(counts[0]), keypoints=int(counts[1]), valid=int(counts[2]))
        live[side] = out["valid"]
        if fetch:
            s = out["slots"]
            out.update(desc=np.zeros((s, 64), np.uint16), total=np.zeros(s, np.uint32), state=np.zeros(s, np.uint8), xyz=np.zeros((s, 3), np.float32))
            self._check(self.lib.pcp_coarse_descriptors_fetch(self.h, C.c_int32(side), _ptr(out["desc"]), _ptr(out["total"]), _ptr(out["state"]),
                                                              _ptr(out["xyz"])))
        return out

    def compare_base_normals_fetch(self) -> np.ndarray:
        """The base's normals as the coarse registration estimated them, (n_base, 3) float32 (pcp_compare_base_normals_fetch)."""
        out = np.zeros((getattr(self, "n_base", 0), 3), np.float32)
        self._check(self.lib.pcp_compare_base_normals_fetch(self.h, _ptr(out)))
        return out

    def coarse_match(self, **params) -> dict:
        """CG3 over the two sides' live descriptors (pcp_coarse_match and its fetch): dict(pairs (C, 2) int32: base ordinal, map
        ordinal; base_keys, map_keys (K, 2) uint64: best, second per valid keypoint, CG_NO_KEY = none), K the number of valid
        descriptors that coarse_descriptors reported for that side."""
        prm = coarse_params(**params)
        count = C.c_int64()
        live = self._coarse_live()
        live.pop("pairs", None)
        self._check(self.lib.pcp_coarse_match(self.h, C.byref(prm), C.byref(count)))
        if CG_BASE not in live or CG_MAP not in live:  # (descriptors this Context did not make: their number is not known here)
            raise ValueError("coarse_match: the descriptors of both sides must come from coarse_descriptors or compare_register_coarse "
                             "of this Context, which sizes the fetch by their counts")
        pairs = np.zeros((count.value, 2), np.int32)
        bk, mk = np.zeros((live[CG_BASE], 2), np.uint64), np.zeros((live[CG_MAP], 2), np.uint64)
        self._check(self.lib.pcp_coarse_match_fetch(self.h, _ptr(pairs), _ptr(bk), _ptr(mk)))
        live["pairs"] = count.value
        return dict(pairs=pairs, base_keys=bk, map_keys=mk)

    def coarse_score(self, frames, flags: bool = False, **params) -> dict:
        """CG5 for a caller's frames (F, 15) float64 over the live correspondences (pcp_coarse_score): dict(counts (F,) int64, and
        with flags flags (F, C) uint8, C the number of correspondences of the last match)."""
        frames = np.ascontiguousarray(frames, np.float64).reshape(-1, 15)
        prm = coarse_params(**params)
        counts = np.zeros(frames.shape[0], np.int64)
        fl = None
        if flags:
            pairs = self._coarse_live().get("pairs")
            if pairs is None:
                raise ValueError("coarse_score: flags need a match made by coarse_match or compare_register_coarse of this Context, "
                                 "which sizes them by its correspondences")
            fl = np.zeros((frames.shape[0], pairs), np.uint8)
        self._check(self.lib.pcp_coarse_score(self.h, C.byref(prm), C.c_int64(frames.shape[0]), _ptr(frames), _ptr(counts), _ptr(fl)))
        return dict(counts=counts, flags=fl) if flags else dict(counts=counts)

    def compare_register_coarse(self, normals=None, base_normals=None, **params) -> dict:
        """Brings the base near the uploaded cloud from an arbitrary pose (pcp_compare_register_coarse): dict with the entries
        CG_REPORT, triple, T (4, 4) the base's transform after the call, inliers (C,) uint8, report (16,) int64.  Status
        CG_TOO_FEW_INLIERS leaves the transform as it was."""
        normals = self._coarse_normals("compare_register_coarse", CG_MAP, normals)
        base_normals = self._coarse_normals("compare_register_coarse", CG_BASE, base_normals)
        prm = coarse_params(**params)
        report, T, inliers = np.zeros(16, np.int64), np.zeros((4, 4), np.float64), np.zeros(1 << 18, np.uint8)
        live = self._coarse_live()
        live.clear()  # (the call describes and matches anew)
        self._check(self.lib.pcp_compare_register_coarse(self.h, C.byref(prm), _ptr(normals), _ptr(base_normals), _ptr(report), _ptr(T),
                                                         _ptr(inliers)))
        out = _coarse_report(report, T, inliers)
        live.update({CG_MAP: out["valid_map"], CG_BASE: out["valid_base"], "pairs": out["correspondences"]})
        return out

    def coarse_then_fine(self, normals=None, base_normals=None, coarse=None, fine=None) -> dict:
        """compare_register_coarse, then compare_register with match_radius = 2 inlier_distance (the other parameters at
        their defaults), then compare_register with `fine` (register_params; the defaults): dict(coarse, wide, fine, T, status =
        the last stage's that ran).  A coarse status CG_TOO_FEW_INLIERS ends it there."""
        coarse = dict(coarse or {})
        first = self.compare_register_coarse(normals=normals, base_normals=base_normals, **coarse)
        if first["status"] != CG_FOUND:
            return dict(coarse=first, wide=None, fine=None, T=first["T"], status=first["status"])
        inlier = coarse_params(**coarse).inlier_distance
        wide = self.compare_register(normals=normals, match_radius=2.0 * inlier)
        last = self.compare_register(normals=normals, **dict(fine or {}))
        return dict(coarse=first, wide=wide, fine=last, T=last["T"], status=last["status"])

    # -- planar facets ("Planar facets") -----------------------------------
    def facets(self, link_radius: float = 0.1, angle_deg: float = 10.0, plane_tol: float = 0.01, max_curvature: float = 0.02,
               min_points: int = 1000) -> dict:
        """The planar facets of the uploaded cloud under the live normals (pcp_facets and its fetch): label (n,) int32, the
        lowest input index of the point's facet, -1 for a point in none; ids (F,) int32 ascending; rows (F, 10) int64, the
        columns FA_ROW; box (F, 6) float32: min xyz, max xyz; plus facet_points, components and facets (counts)."""
        prm = FacetParams(link_radius, angle_deg, plane_tol, max_curvature, min_points)
        label = np.empty(self.n, np.int32)
        pts, comps, fac = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.pcp_facets(self.h, C.byref(prm), _ptr(label), C.byref(pts), C.byref(comps), C.byref(fac)))
        out = self.facets_fetch(0, fac.value)
        assert len(out["ids"]) == fac.value, (len(out["ids"]), fac.value)
        out.update(label=label, facet_points=pts.value, components=comps.value, facets=fac.value)
        return out

    def facets_fetch(self, first: int = 0, max_rows: int = 1 << 24) -> dict:
        """Rows first .. first + max_rows - 1 of the last facets call's table (pcp_facets_fetch): dict(ids, rows, box)."""
        have = C.c_int64()
        self._check(self.lib.pcp_facets_fetch(self.h, C.c_int64(first), C.c_int64(max_rows), None, None, None, C.byref(have)))
        rows = have.value
        ids = np.empty(rows, np.int32)
        tab = np.empty((rows, 10), np.int64)
        box = np.empty((rows, 6), np.float32)
        got = C.c_int64()
        self._check(self.lib.pcp_facets_fetch(self.h, C.c_int64(first), C.c_int64(rows), _ptr(ids), _ptr(tab), _ptr(box), C.byref(got)))
        assert got.value == rows, (got.value, rows)
        return dict(ids=ids, rows=tab, box=box)

    # -- mask distance maps ("Mask distance maps") ------------------------
    def mask_edt(self, frame: int, threshold: int = 0, want_nearest: bool = True) -> dict:
        """The exact squared distance from every pixel of the keyframe's mask to the nearest background pixel (mask byte
        <= threshold) and that pixel's linear index, lowest index among equals (pcp_mask_edt): dict(d2 (H, W) uint32,
        and with want_nearest nearest (H, W) int32).  A mask without background: d2 0xFFFFFFFF, nearest -1."""
        out = self.mask_edt_frames(frame, 1, threshold, want_nearest)
        return {k: v[0] for k, v in out.items()}

    def mask_edt_frames(self, first: int, count: int, threshold: int = 0, want_nearest: bool = True) -> dict:
        """mask_edt of keyframes first .. first + count - 1 in one call (pcp_mask_edt_frames): dict(d2 (count, H, W) uint32,
        nearest (count, H, W) int32)."""
        hh, ww = self.camera.image_height, self.camera.image_width
        shape = (max(count, 0), hh, ww)
        d2 = np.empty(shape, np.uint32)
        nearest = np.empty(shape, np.int32) if want_nearest else None
        self._check(self.lib.pcp_mask_edt_frames(self.h, C.c_int32(first), C.c_int32(count), C.c_int32(threshold), _ptr(d2),
                                                 _ptr(nearest)))
        out = dict(d2=d2)
        if want_nearest:
            out["nearest"] = nearest
        return out

    # -- crack width maps ("Crack width maps") ----------------------------
    def crack_width(self, frame: int, threshold: int = 0, plane_radius: int = 150,
                    want=("flags", "edges", "w2d2", "width", "points", "plane")) -> dict:
        """Per foreground pixel of the keyframe's mask: the two edge points along the EDT direction, the plane of the position
        image's window and the 3-D width between the edge rays on it (pcp_crack_width).  want: any of CW_OUTPUTS; dict of
        flags (H, W) uint8, edges (H, W, 4) int32 (doubled, -1 = missing), w2d2 (H, W) uint32, width (H, W) float32 metres,
        points (H, W, 6) float32, plane (H, W, 4) float32, moments (H, W, 13) int64, plus sites and widths (counts)."""
        unknown = set(want) - set(CW_OUTPUTS)
        if unknown:
            raise ValueError(f"crack_width: unknown outputs {sorted(unknown)}")
        hh, ww = (self.camera.image_height, self.camera.image_width) if self.camera is not None else (0, 0)  # (the library refuses)
        spec = dict(flags=((hh, ww), np.uint8), edges=((hh, ww, 4), np.int32), w2d2=((hh, ww), np.uint32), width=((hh, ww), np.float32),
                    points=((hh, ww, 6), np.float32), plane=((hh, ww, 4), np.float32), moments=((hh, ww, 13), np.int64))
        arr = {k: (np.empty(*spec[k]) if k in want else None) for k in CW_OUTPUTS}
        prm = CrackParams(threshold, plane_radius)
        sites, widths = C.c_int64(), C.c_int64()
        self._check(self.lib.pcp_crack_width(self.h, C.c_int32(frame), C.byref(prm), *[_ptr(arr[k]) for k in CW_OUTPUTS],
                                             C.byref(sites), C.byref(widths)))
        out = {k: v for k, v in arr.items() if v is not None}
        out["sites"], out["widths"] = sites.value, widths.value
        return out

    # -- crack widths on the map ("Crack widths on the map") -----------------
    def crack_fuse_begin(self):
        """A fresh accumulation for the uploaded cloud (pcp_crack_fuse_begin); the uploads, set_camera and set_frames drop it."""
        self._check(self.lib.pcp_crack_fuse_begin(self.h))

    def crack_fuse_add(self, frame: int, threshold: int = 0, plane_radius: int = 150) -> tuple[int, int]:
        """Adds the keyframe's crack widths to the points that see them (pcp_crack_fuse_add): (contributors, credited)."""
        prm = CrackParams(threshold, plane_radius)
        m, c = C.c_int64(), C.c_int64()
        self._check(self.lib.pcp_crack_fuse_add(self.h, C.c_int32(frame), C.byref(prm), C.byref(m), C.byref(c)))
        return m.value, c.value

    def crack_fuse_fetch(self, want=("width_mean", "width_best", "best_frame", "views", "seen", "centres", "min_q", "max_q", "sum_q")) -> dict:
        """The accumulated state per map point, input order (pcp_crack_fuse_fetch): any of width_mean / width_best (float32,
        metres), best_frame (int32, -1 without a view), views / seen / centres / min_q / max_q (uint32), sum_q (uint64)."""
        names = [k for k, _ in CF_OUTPUTS]
        unknown = set(want) - set(names)
        if unknown:
            raise ValueError(f"crack_fuse_fetch: unknown outputs {sorted(unknown)}")
        arr = {k: (np.zeros(self.n, t) if k in want else None) for k, t in CF_OUTPUTS}
        self._check(self.lib.pcp_crack_fuse_fetch(self.h, *[_ptr(arr[k]) for k in names]))
        return {k: v for k, v in arr.items() if v is not None}

    def crack_fuse_end(self):
        self._check(self.lib.pcp_crack_fuse_end(self.h))

    def crack_components(self, min_views: int = 1, radius: float = 0.02) -> dict:
        """The map's cracks from the live accumulation (pcp_crack_components and its fetch): label (n,) int32, the lowest input
        index of the point's connected component under the link radius, -1 for a point that is no crack point; ids (C,) int32
        ascending; stats (C, 5) int64: points, sum_w, min_w, max_w, centre_points; box (C, 6) float32: min xyz, max xyz; plus
        crack_points and components (counts)."""
        prm = CrackLinkParams(min_views, radius)
        label = np.empty(self.n, np.int32)
        pts, comps = C.c_int64(), C.c_int64()
        self._check(self.lib.pcp_crack_components(self.h, C.byref(prm), _ptr(label), C.byref(pts), C.byref(comps)))
        rows = comps.value
        ids = np.empty(rows, np.int32)
        stats = np.empty((rows, 5), np.int64)
        box = np.empty((rows, 6), np.float32)
        got = C.c_int64()
        self._check(self.lib.pcp_crack_components_fetch(self.h, C.c_int64(0), C.c_int64(rows), _ptr(ids), _ptr(stats), _ptr(box), C.byref(got)))
        assert got.value == rows, (got.value, rows)
        return dict(label=label, ids=ids, stats=stats, box=box, crack_points=pts.value, components=rows)

    # -- crack lengths on the map ("Crack lengths on the map") ----------------
    def crack_lengths(self, min_views: int = 1, radius: float = 0.02) -> dict:
        """The length, ends and centreline of every crack of the map from the live accumulation (pcp_crack_lengths and its
        fetches): pos (n,) uint64, the arc position of a crack point along its crack in units of 2^-20 m, NO_POS for every other
        point; ids (C,) int32 ascending, the rows of crack_components; rows (C, 7) int64, the columns CL_ROW; offsets (C + 1,)
        int64 and path (int32 input indices): crack k's polyline from end_a to end_b is path[offsets[k]:offsets[k + 1]]; plus
        cracks and path_points (counts)."""
        prm = CrackLinkParams(min_views, radius)
        pos = np.empty(self.n, np.uint64)
        cracks, entries = C.c_int64(), C.c_int64()
        self._check(self.lib.pcp_crack_lengths(self.h, C.byref(prm), _ptr(pos), C.byref(cracks), C.byref(entries)))
        c, e = cracks.value, entries.value
        ids = np.empty(c, np.int32)
        rows = np.empty((c, 7), np.int64)
        offsets = np.zeros(c + 1, np.int64)
        path = np.empty(e, np.int32)
        got = C.c_int64()
        self._check(self.lib.pcp_crack_lengths_fetch(self.h, C.c_int64(0), C.c_int64(c), _ptr(ids), _ptr(rows), _ptr(offsets), C.byref(got)))
        assert got.value == c, (got.value, c)
        self._check(self.lib.pcp_crack_paths_fetch(self.h, C.c_int64(0), C.c_int64(e), _ptr(path), C.byref(got)))
        assert got.value == e, (got.value, e)
        return dict(pos=pos, ids=ids, rows=rows, offsets=offsets, path=path, cracks=c, path_points=e)

    # -- crack directions on the map ("Crack directions on the map") -------------
    def crack_directions(self, min_views: int = 1, radius: float = 0.02, want_moments: bool = False) -> dict:
        """Which way every crack of the map runs, from the live accumulation (pcp_crack_directions and its fetch): tangent
        (n, 3) float32, the unit direction of the crack at a crack point with its largest component positive, and anisotropy
        (n,) float32 (1 on a line), zeros where there is none; links (n,) int32; with want_moments moments (n, 10) int64, the
        columns CD_WORD; ids (C,) int32 ascending, the rows of crack_components; rows (C, 20) int64, (lo, hi) of the summed
        words; per crack, through crack_axis_host, axis (C, 3), axis_anisotropy (C,) and link_count (C,) float64; plus
        crack_points and cracks (counts)."""
        prm = CrackLinkParams(min_views, radius)
        tangent = np.empty((self.n, 3), np.float32)
        anisotropy = np.empty(self.n, np.float32)
        links = np.empty(self.n, np.int32)
        moments = np.empty((self.n, 10), np.int64) if want_moments else None
        pts, cracks = C.c_int64(), C.c_int64()
        self._check(self.lib.pcp_crack_directions(self.h, C.byref(prm), _ptr(tangent), _ptr(anisotropy), _ptr(links), _ptr(moments),
                                                  C.byref(pts), C.byref(cracks)))
        c = cracks.value
        ids = np.empty(c, np.int32)
        rows = np.empty((c, 20), np.int64)
        got = C.c_int64()
        self._check(self.lib.pcp_crack_directions_fetch(self.h, C.c_int64(0), C.c_int64(c), _ptr(ids), _ptr(rows), C.byref(got)))
        assert got.value == c, (got.value, c)
        out = dict(tangent=tangent, anisotropy=anisotropy, links=links, ids=ids, rows=rows, crack_points=pts.value, cracks=c)
        if want_moments:
            out["moments"] = moments
        out.update(crack_axis_host(rows))
        return out

    # -- crack skeletons on the map ("Crack skeletons on the map") --------------
    def crack_skeleton(self, min_views: int = 1, radius: float = 0.02, step=None) -> dict:
        """The level-set diagram of every crack of the map from the live accumulation (pcp_crack_skeleton and its fetches):
        node (n,) int32, the id of a crack point's node (the lowest input index among its points), -1 for every other point; ids
        (N,) int32 ascending; nodes (N, 10) int64, the columns CS_NODE; edges (E, 3) int64, the columns CS_EDGE, ascending by
        (u, v); cracks (C, 6) int64, the columns CS_CRACK, the rows of crack_components; plus centroids (N, 3), edge_length_m
        (E,) and skeleton_length_m (C,), fp64 metres from the integers.  step: the band width in metres, default 2 * radius."""
        prm = CrackLinkParams(min_views, radius)
        if step is None:
            step = crack_skeleton_step(radius)
        node = np.empty(self.n, np.int32)
        kn, ke, got = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.pcp_crack_skeleton(self.h, C.byref(prm), C.c_float(step), _ptr(node), C.byref(kn), C.byref(ke)))
        ids = np.empty(kn.value, np.int32)
        nodes = np.empty((kn.value, 10), np.int64)
        edges = np.empty((ke.value, 3), np.int64)
        self._check(self.lib.pcp_crack_skeleton_nodes_fetch(self.h, C.c_int64(0), C.c_int64(kn.value), _ptr(ids), _ptr(nodes), C.byref(got)))
        assert got.value == kn.value, (got.value, kn.value)
        self._check(self.lib.pcp_crack_skeleton_edges_fetch(self.h, C.c_int64(0), C.c_int64(ke.value), _ptr(edges), C.byref(got)))
        assert got.value == ke.value, (got.value, ke.value)
        self._check(self.lib.pcp_crack_skeleton_cracks_fetch(self.h, C.c_int64(0), C.c_int64(2 ** 62), None, C.byref(got)))
        cracks = np.empty((got.value, 6), np.int64)
        self._check(self.lib.pcp_crack_skeleton_cracks_fetch(self.h, C.c_int64(0), C.c_int64(len(cracks)), _ptr(cracks), C.byref(got)))
        assert got.value == len(cracks), (got.value, len(cracks))
        out = dict(node=node, ids=ids, nodes=nodes, edges=edges, cracks=cracks)
        out.update(crack_skeleton_metres(nodes, edges, cracks))
        return out

    # -- crack branches on the map ("Crack branches on the map") ----------------
    def crack_branches(self, min_views: int = 1, radius: float = 0.02, step=None, prune: float = 0.0) -> dict:
        """Every crack of the map arm by arm, from the live accumulation (pcp_crack_branches and its fetches): the diagram of
        crack_skeleton cut at its junctions, branches with one attachment and fewer than prune / step nodes pruned (metres; 0
        prunes nothing).  branch (n,) int32, the id of a crack point's branch (the lowest input index among its points), -1 for
        a point that is no crack point, -2 on a kept junction, -3 on a pruned node; ids (B,) int32 ascending; rows (B, 15) int64,
        the columns CB_ROW; moments (B, 20) int64, the rows of crack_directions restricted to the links inside a branch;
        edge_branch (E,) int32 per edge of crack_skeleton (-1 a bridge, -2 an edge with a pruned end); cracks (C, 7) int64, the
        columns CB_CRACK, the rows of crack_components; plus what crack_branches_metres makes of them: length_m,
        kept_length_m, centroid, mean_width, axis, anisotropy, link_count.  It leaves the tables crack_skeleton leaves."""
        prm = CrackLinkParams(min_views, radius)
        if step is None:
            step = crack_skeleton_step(radius)
        branch = np.empty(self.n, np.int32)
        kb, kp, got = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.pcp_crack_branches(self.h, C.byref(prm), C.c_float(step), C.c_float(prune), _ptr(branch), C.byref(kb), C.byref(kp)))
        ids = np.empty(kb.value, np.int32)
        rows = np.empty((kb.value, 15), np.int64)
        moments = np.empty((kb.value, 20), np.int64)
        self._check(self.lib.pcp_crack_branches_fetch(self.h, C.c_int64(0), C.c_int64(kb.value), _ptr(ids), _ptr(rows), _ptr(moments), C.byref(got)))
        assert got.value == kb.value, (got.value, kb.value)
        self._check(self.lib.pcp_crack_branch_edges_fetch(self.h, C.c_int64(0), C.c_int64(2 ** 62), None, C.byref(got)))
        edge_branch = np.empty(got.value, np.int32)
        self._check(self.lib.pcp_crack_branch_edges_fetch(self.h, C.c_int64(0), C.c_int64(len(edge_branch)), _ptr(edge_branch), C.byref(got)))
        assert got.value == len(edge_branch), (got.value, len(edge_branch))
        self._check(self.lib.pcp_crack_branch_cracks_fetch(self.h, C.c_int64(0), C.c_int64(2 ** 62), None, C.byref(got)))
        cracks = np.empty((got.value, 7), np.int64)
        self._check(self.lib.pcp_crack_branch_cracks_fetch(self.h, C.c_int64(0), C.c_int64(len(cracks)), _ptr(cracks), C.byref(got)))
        assert got.value == len(cracks), (got.value, len(cracks))
        edges = np.empty((len(edge_branch), 3), np.int64)
        self._check(self.lib.pcp_crack_skeleton_nodes_fetch(self.h, C.c_int64(0), C.c_int64(2 ** 62), None, None, C.byref(got)))
        nodes = np.empty((got.value, 10), np.int64)
        self._check(self.lib.pcp_crack_skeleton_nodes_fetch(self.h, C.c_int64(0), C.c_int64(len(nodes)), None, _ptr(nodes), C.byref(got)))
        self._check(self.lib.pcp_crack_skeleton_edges_fetch(self.h, C.c_int64(0), C.c_int64(len(edges)), _ptr(edges), C.byref(got)))
        assert got.value == len(edges), (got.value, len(edges))
        out = dict(branch=branch, ids=ids, rows=rows, moments=moments, edge_branch=edge_branch, cracks=cracks, pruned_branches=kp.value)
        out.update(crack_branches_metres(rows, moments, edge_branch, nodes, edges, cracks))
        return out

    def colour_smooth_local(self, radius: float) -> int:
        """smoothColorsWithLocalRegion (PointCloudProcessor.cpp:634-703) in place on the colour result; returns the number
        of points with a colour afterwards.  The downloads then return the smoothed words."""
        cnt = C.c_int64()
        self._check(self.lib.pcp_colour_smooth_local(self.h, C.c_float(radius), C.byref(cnt)))
        return cnt.value

    def colour_smooth_local_packed(self, radius: float, rgba) -> tuple[np.ndarray, int]:
        """The same over caller-supplied packed words (n uint32 r | g<<8 | b<<16 | has<<24, input order):
        (smoothed words, points with a colour)."""
        words = np.ascontiguousarray(rgba, np.uint32)
        if words.shape != (self.n,):
            raise ValueError(f"colour_smooth_local_packed: {self.n} words expected, got shape {words.shape}")
        out = np.empty(self.n, np.uint32)
        cnt = C.c_int64()
        self._check(self.lib.pcp_colour_smooth_local_packed(self.h, C.c_float(radius), _ptr(words), _ptr(out), C.byref(cnt)))
        return out, cnt.value

    # -- MLS --------------------------------------------------------------
    def set_mls_local_plane(self, upsampling_radius: float = 0.05, upsampling_step: float = 0.01):
        """SAMPLE_LOCAL_PLANE's radius and step for the context's later MLS calls (pcp_create sets the reference's
        0.05 / 0.01, PointCloudProcessor.cpp:74-75)."""
        self._check(self.lib.pcp_set_mls_local_plane(self.h, C.c_double(upsampling_radius), C.c_double(upsampling_step)))

    def mls_process(self, params: MLSParams) -> int:
        cnt = C.c_int64()
        self._check(self.lib.pcp_mls_process(self.h, C.byref(params), C.byref(cnt)))
        return cnt.value

    def mls_stream_begin(self, params: "MLSParams", chunk_capacity: int):
        """(total voxels, chunks) of a chunked VOXEL_GRID_DILATION emission (pcp_mls_stream_begin)."""
        total = C.c_int64()
        chunks = C.c_int32()
        self._check(self.lib.pcp_mls_stream_begin(self.h, C.byref(params), C.c_int64(chunk_capacity), C.byref(total),
                                                  C.byref(chunks)))
        return total.value, chunks.value

    def mls_stream_next(self) -> int:
        m = C.c_int64()
        self._check(self.lib.pcp_mls_stream_next(self.h, C.byref(m)))
        return m.value

    def cloud_smooth_stream_begin(self, params: "MLSParams", chunk_capacity: int):
        """CloudSmooth::process whole, its last two stages streamed (pcp_cloud_smooth_stream_begin): (rows of the upsampled
        cloud, rows the trailing outlier removal keeps, chunks)."""
        total, kept = C.c_int64(), C.c_int64()
        chunks = C.c_int32()
        self._check(self.lib.pcp_cloud_smooth_stream_begin(self.h, C.byref(params), C.c_int64(chunk_capacity), C.byref(total),
                                                           C.byref(kept), C.byref(chunks)))
        return total.value, kept.value, chunks.value

    def cloud_smooth_stream_next(self) -> int:
        """Survivors of the next chunk (fetch them with mls_fetch); 0 after the last one."""
        m = C.c_int64()
        self._check(self.lib.pcp_cloud_smooth_stream_next(self.h, C.byref(m)))
        return m.value

    def cloud_smooth_stream_stats(self) -> dict:
        out = (C.c_double * 13)()
        self._check(self.lib.pcp_cloud_smooth_stream_stats(self.h, out))
        return {"halo_planes": int(out[0]), "chunks_redone": int(out[1]), "threshold": float(out[2]),
                "max_displacement_m": float(out[3]), "min_margin_m": float(out[4]), "rows_computed": int(out[5]),
                "sampled_displacement_m": float(out[6]), "device_bytes_held": int(out[7]),
                "begin_seconds": {"filter_fit_voxels": round(out[8], 4), "allocations": round(out[9], 4),
                                  "sweep0": round(out[10], 4), "sweep1_threshold": round(out[11], 4)},
                "allocated_GB": round(out[12] / 1e9, 2)}

    def cloud_smooth_stream_end(self):
        """Ends the stream and frees the device memory it holds (pcp_cloud_smooth_stream_end)."""
        self._check(self.lib.pcp_cloud_smooth_stream_end(self.h))

    def cloud_smooth_stream_seek(self, chunk: int):
        """The chunk the next cloud_smooth_stream_next emits (0 .. chunks; any chunk may be emitted again)."""
        self._check(self.lib.pcp_cloud_smooth_stream_seek(self.h, C.c_int32(chunk)))

    def mls_stream_seek(self, chunk: int):
        self._check(self.lib.pcp_mls_stream_seek(self.h, C.c_int32(chunk)))

    def mls_process_shard(self, params: MLSParams, index_begin: int, index_end: int) -> int:
        cnt = C.c_int64()
        self._check(self.lib.pcp_mls_process_shard(self.h, C.byref(params), C.c_int64(index_begin), C.c_int64(index_end),
                                                   C.byref(cnt)))
        return cnt.value

    def mls_process_slab(self, params: MLSParams, slab: int, n_slabs: int) -> int:
        """Queries of one slab of the stage's own spatial order (1 / n_slabs of the work whatever the caller's point order)."""
        cnt = C.c_int64()
        self._check(self.lib.pcp_mls_process_slab(self.h, C.byref(params), C.c_int32(slab), C.c_int32(n_slabs), C.byref(cnt)))
        return cnt.value

    def cloud_smooth(self, params: MLSParams) -> int:
        cnt = C.c_int64()
        self._check(self.lib.pcp_cloud_smooth(self.h, C.byref(params), C.byref(cnt)))
        return cnt.value

    def mls_fetch(self, count: int):
        xyz = np.empty((count, 3), np.float32)
        nrm = np.empty((count, 3), np.float32)
        curv = np.empty(count, np.float32)
        idx = np.empty(count, np.int32)
        self._check(self.lib.pcp_mls_fetch(self.h, C.c_int64(count), _ptr(xyz), _ptr(nrm), _ptr(curv), _ptr(idx)))
        return dict(xyz=xyz, normal=nrm, curvature=curv, index=idx)

    def mls_fetch_index(self, count: int) -> np.ndarray:
        """Only the source indices of the latest smoothing result (4 B per row cross PCIe)."""
        idx = np.empty(count, np.int32)
        self._check(self.lib.pcp_mls_fetch(self.h, C.c_int64(count), None, None, None, _ptr(idx)))
        return idx

    def sor(self, mean_k: int = 60, std_mul: float = 0.7):
        keep = np.empty(self.n, np.uint8)
        kept = C.c_int64()
        self._check(self.lib.pcp_sor(self.h, C.c_int32(mean_k), C.c_double(std_mul), _ptr(keep), C.byref(kept)))
        return keep, kept.value

    def sor_chunk_points(self) -> int:
        return int(self.lib.pcp_sor_chunk_points())

    def sor_partial(self, mean_k: int, slab: int, n_slabs: int):
        """Slab `slab` of `n_slabs` of sor(): (first chunk, (sum, sum of squares) per chunk of the slab)."""
        c = self.sor_chunk_points()
        chunks = (self.n + c - 1) // c
        out = np.zeros((max(chunks, 1), 2), np.float64)
        first, cnt = C.c_int64(), C.c_int64()
        self._check(self.lib.pcp_sor_partial(self.h, C.c_int32(mean_k), C.c_int32(slab), C.c_int32(n_slabs), C.c_int64(len(out)),
                                             _ptr(out), C.byref(first), C.byref(cnt)))
        return first.value, out[:cnt.value].copy()

    def sor_finish(self, std_mul: float, all_chunk_sums: np.ndarray, slab: int, n_slabs: int):
        """Keep flags of the slab's points (n bytes under the caller's indices, 0 for the other slabs' points)."""
        sums = np.ascontiguousarray(all_chunk_sums, np.float64)
        keep = np.empty(self.n, np.uint8)
        kept = C.c_int64()
        self._check(self.lib.pcp_sor_finish(self.h, C.c_double(std_mul), _ptr(sums), C.c_int64(len(sums)), C.c_int32(slab),
                                            C.c_int32(n_slabs), _ptr(keep), C.byref(kept)))
        return keep, kept.value

    def close_pairs(self, radius: float = 2.5e-5) -> int:
        """Map points with another map point closer than `radius` (precondition of the index match-back: expect 0)."""
        cnt = C.c_int64()
        self._check(self.lib.pcp_close_pairs(self.h, C.c_double(radius), C.byref(cnt)))
        return cnt.value

    # -- NID extrinsic refinement -----------------------------------------
    def sor_distances(self) -> np.ndarray:
        """mean distance to the mean_k nearest neighbours per uploaded point, from the last sor() call"""
        out = np.empty(self.n, np.float32)
        self._check(self.lib.pcp_sor_distances(self.h, C.c_int64(len(out)), _ptr(out)))
        return out

    def sor_redo_fraction(self) -> float:
        v = C.c_double()
        self._check(self.lib.pcp_sor_redo_fraction(self.h, C.byref(v)))
        return v.value

    def upload_intensity(self, intensity):
        a = np.ascontiguousarray(intensity, np.float32)
        self._check(self.lib.pcp_upload_intensity(self.h, _ptr(a), C.c_int64(len(a))))

    def nid_prepare(self) -> int:
        cnt = C.c_int64()
        self._check(self.lib.pcp_nid_prepare(self.h, C.byref(cnt)))
        return cnt.value

    def nid_evaluate(self, T, T_init=None, bins: int = 16):
        T = np.ascontiguousarray(T, np.float64).reshape(16)
        Ti = None if T_init is None else np.ascontiguousarray(T_init, np.float64).reshape(16)
        cost = C.c_double()
        grad = np.zeros(6, np.float64)
        valid = C.c_int32()
        self._check(self.lib.pcp_nid_evaluate(self.h, _ptr(T), _ptr(Ti), C.c_int32(bins), C.byref(cost), _ptr(grad),
                                              C.byref(valid)))
        return cost.value, grad, bool(valid.value)

    def nid_optimize(self, T_init, bins: int = 16, max_outer_iterations: int = 10):
        Ti = np.ascontiguousarray(T_init, np.float64).reshape(16)
        out = np.zeros(16, np.float64)
        cost = C.c_double()
        evals = C.c_int32()
        self._check(self.lib.pcp_nid_optimize(self.h, _ptr(Ti), C.c_int32(bins), C.c_int32(max_outer_iterations), _ptr(out),
                                              C.byref(cost), C.byref(evals)))
        return out.reshape(4, 4), cost.value, evals.value

    # NID over an index-sharded map: accumulate -> all-reduce(SUM) of the histograms -> finish
    def nid_accumulate(self, T, bins: int = 16):
        T = np.ascontiguousarray(T, np.float64).reshape(16)
        self._check(self.lib.pcp_nid_accumulate(self.h, _ptr(T), C.c_int32(bins)))

    def nid_histograms_device(self):
        p = C.c_void_p()
        n = C.c_int64()
        self._check(self.lib.pcp_nid_histograms_device(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def nid_finish(self, bins: int = 16):
        cost = C.c_double()
        grad = np.zeros(6, np.float64)
        valid = C.c_int32()
        self._check(self.lib.pcp_nid_finish(self.h, C.c_int32(bins), C.byref(cost), _ptr(grad), C.byref(valid)))
        return cost.value, grad, bool(valid.value)

    def nid_optimize_with(self, evaluate, T_init, bins: int = 16, max_outer_iterations: int = 10):
        """pcp_nid_optimize_with: evaluate(T 4x4, bins) -> (cost, grad6, valid), e.g. the sharded evaluation."""
        errors = []

        @NID_EVAL_FN
        def trampoline(_user, T, b, cost, grad, valid):
            try:
                c, g, ok = evaluate(np.ctypeslib.as_array(T, (16,)).copy().reshape(4, 4), int(b))
                cost[0] = float(c)
                for k in range(6):
                    grad[k] = float(g[k])
                valid[0] = 1 if ok else 0
                return 0
            except Exception as e:  # noqa: BLE001 -- reported through the status code, re-raised below
                errors.append(e)
                return -3

        Ti = np.ascontiguousarray(T_init, np.float64).reshape(16)
        out = np.zeros(16, np.float64)
        cost = C.c_double()
        evals = C.c_int32()
        rc = self.lib.pcp_nid_optimize_with(self.h, trampoline, None, _ptr(Ti), C.c_int32(bins), C.c_int32(max_outer_iterations),
                                            _ptr(out), C.byref(cost), C.byref(evals))
        if errors:
            raise errors[0]
        self._check(rc)
        return out.reshape(4, 4), cost.value, evals.value

    # -- measurement ------------------------------------------------------
    def timing_enable(self, on: bool = True):
        self._check(self.lib.pcp_timing_enable(self.h, C.c_int32(1 if on else 0)))

    def timing_reset(self):
        self._check(self.lib.pcp_timing_reset(self.h))

    def timing_get(self, kernel_id: int):
        ms = C.c_double()
        cnt = C.c_int64()
        self._check(self.lib.pcp_timing_get(self.h, C.c_int32(kernel_id), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def tile_mask_density(self) -> float:
        v = C.c_double()
        self._check(self.lib.pcp_tile_mask_density(self.h, C.byref(v)))
        return v.value

    def selftest_arithmetic(self, samples: int = 1 << 26, seed: int = 1):
        """(fp64 mismatches, fp32 mismatches) of the short exact division sequences against `/`."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self.lib.pcp_selftest_arithmetic(self.h, C.c_int64(samples), C.c_uint64(seed), C.byref(a), C.byref(b)))
        return a.value, b.value

    def selftest_visit_forms(self, samples: int = 1 << 24, seed: int = 1):
        """(projection, cell rule, square root) mismatches of the visit's short forms against the written ones, and whether
        the configured p1, p2 let the short distortion run."""
        a, b, c, f = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        self._check(self.lib.pcp_selftest_visit_forms(self.h, C.c_int64(samples), C.c_uint64(seed), C.byref(a), C.byref(b), C.byref(c),
                                                      C.byref(f)))
        return a.value, b.value, c.value, bool(f.value)

    def selftest_k3_term(self, samples: int = 1 << 24, seed: int = 1):
        """(mismatches of the batched passes' projection form against the written one, whether the configured camera lets
        the k3 term go)."""
        a, f = C.c_int64(), C.c_int32()
        self._check(self.lib.pcp_selftest_k3_term(self.h, C.c_int64(samples), C.c_uint64(seed), C.byref(a), C.byref(f)))
        return a.value, bool(f.value)

    def selftest_eigen33(self, form: int, matrices=None, args=None):
        """The device's smallest_eigenpair, mls_rcp and mls_rsqrt on the caller's inputs (pcp_selftest_eigen33).  matrices
        (n, 6) float64 in the order xx xy xz yy yz zz, args (m,) float64, either may be None; form 0 = built without
        contraction (map normals, crack width, crack direction), 1 = with (MLS fit).  Returns (ev (n,), vec (n, 3), rcp (m,),
        rsqrt (m,)), NaNs and infinities as the device produced them."""
        mat = np.zeros((0, 6)) if matrices is None else np.ascontiguousarray(matrices, np.float64).reshape(-1, 6)
        arg = np.zeros(0) if args is None else np.ascontiguousarray(args, np.float64).reshape(-1)
        n, m = len(mat), len(arg)
        ev, vec, rcp, rsq = np.zeros(n), np.zeros((n, 3)), np.zeros(m), np.zeros(m)
        self._check(self.lib.pcp_selftest_eigen33(self.h, C.c_int32(form), C.c_int64(n), _ptr(mat), _ptr(ev), _ptr(vec), C.c_int64(m),
                                                  _ptr(arg), _ptr(rcp), _ptr(rsq)))
        return ev, vec, rcp, rsq

    def tile_masks(self) -> np.ndarray:
        """(tiles, mask_words) uint32: the tile x keyframe masks as the last depth pass left them."""
        t, w = C.c_int64(), C.c_int32()
        self._check(self.lib.pcp_tile_masks(self.h, C.byref(t), C.byref(w), None))
        out = np.empty((t.value, w.value), np.uint32)
        self._check(self.lib.pcp_tile_masks(self.h, None, None, _ptr(out)))
        return out

    def cloud_order(self) -> np.ndarray:
        """(n,) int32: the input index of the point at every sorted place (tile t = places 64 t .. 64 t + 63)."""
        out = np.empty(int(self.lib.pcp_cloud_size(self.h)), np.int32)
        self._check(self.lib.pcp_cloud_order(self.h, _ptr(out)))
        return out

    def tile_bounds(self) -> tuple[np.ndarray, np.ndarray]:
        """(tiles, 8) and (groups, 8) float32: centre, radius, half-extents, 0 of every tile and of every group of 16 tiles."""
        t = C.c_int64()
        self._check(self.lib.pcp_tile_bounds(self.h, C.byref(t), None))
        groups = (t.value + 15) // 16
        out = np.empty((t.value + groups, 8), np.float32)
        self._check(self.lib.pcp_tile_bounds(self.h, None, _ptr(out)))
        return out[:t.value], out[t.value:]

    def kernel_name(self, kernel_id: int) -> str:
        return self.lib.pcp_kernel_name(C.c_int32(kernel_id)).decode()
