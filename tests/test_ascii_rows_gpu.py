"""GPU suite of the device PCD writer (csrc/pcp_ascii.hip): pcp_ascii_rows, pcp_colour_compact_ascii and pcp_mls_fetch_ascii
against text built in Python from the binary results ('%.8g' of the fp32, tests/_ascii_ref.py).  Every comparison is byte for
byte.  A tile is 256 rows and the single-workgroup scan carries 1024 tile sums per round (262 144 rows): the long case's
2^21 + 77 rows take nine rounds and two windows of text."""
import numpy as np
import pytest

import _ascii_ref as ref
from conftest import cam_struct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory()


def _same(got, want):
    got = got.tobytes()
    assert got == want, ref.first_difference(got, want)


@pytest.mark.parametrize("kind", [ref.XYZI, ref.POINTNORMAL])
def test_device_arithmetic_on_every_exponent(ctx, kind):
    nf = ref.FLOATS[kind]
    _same(ctx.ascii_rows(kind, ref.as_rows(ref.value_set(), nf)), ref.float_rows_text(ref.value_text(), nf))


@pytest.mark.parametrize("kind", sorted(ref.BOUND))
def test_small_row_counts_all_kinds(ctx, kind):
    residues = set()
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        f, rgb, mask = ref.mixed_rows(kind, n)
        want = ref.rows_text(kind, f, rgb, mask)
        _same(ctx.ascii_rows(kind, f, rgb, mask), want)
        if n == 1025:
            lens = np.array([len(r) + 1 for r in want.split(b"\n")[:-1]])
            # (the rgb column is always ten digits: those kinds vary by 3x, the float-only kinds by more than 4x)
            assert lens.max() >= (3 if kind in (ref.XYZRGB, ref.XYZRGBMASK) else 4) * lens.min()
            residues = {int(v) % 16 for v in np.cumsum(lens)[255::256]}
    assert len(residues) >= 3  # the later tiles start off the 16-byte grid


def test_one_long_case_crosses_the_scan_carry_and_a_window(ctx):
    n = (1 << 21) + 77
    rng = np.random.default_rng(3)
    pool = np.concatenate([ref.value_set()[rng.integers(0, len(ref.value_set()), 4000)],
                           rng.uniform(-60, 60, 96).astype(np.float32)])
    ptext = np.array(ref.g8(pool), dtype=object)
    pick = rng.integers(0, len(pool), (n, 3))
    cpool = rng.integers(0, 256, (64, 3), dtype=np.uint8)
    ctext = np.array([b"%d" % w for w in ref.rgb_words(cpool).tolist()], dtype=object)
    cpick = rng.integers(0, 64, n)
    sp, nl = np.array(b" ", dtype=object), np.array(b"\n", dtype=object)
    rows = ptext[pick[:, 0]] + sp + ptext[pick[:, 1]] + sp + ptext[pick[:, 2]] + sp + ctext[cpick] + nl
    want = b"".join(rows.tolist())
    assert len(want) > (64 << 20), "more than one window of text"
    _same(ctx.ascii_rows(ref.XYZRGB, pool[pick], cpool[cpick]), want)


def test_capacity_contract(ctx):
    from pointcloudprocessor_amd import capi

    f, rgb, mask = ref.mixed_rows(ref.XYZRGBMASK, 700)
    want = ref.rows_text(ref.XYZRGBMASK, f, rgb, mask)
    out = np.full(len(want) + 8, 0xA5, np.uint8)
    with pytest.raises(capi.PcpError) as e:
        ctx.ascii_rows(ref.XYZRGBMASK, f, rgb, mask, capacity=len(want) - 1, out=out)
    assert e.value.code == capi.PCP_ERR_RANGE and e.value.bytes == len(want)
    assert (out == 0xA5).all(), "a short capacity leaves the buffer untouched"
    got = ctx.ascii_rows(ref.XYZRGBMASK, f, rgb, mask, capacity=len(want), out=out)
    assert got.tobytes() == want and (out[len(want):] == 0xA5).all()
    assert ctx.ascii_rows(ref.XYZI, np.zeros((0, 4), np.float32)).size == 0
    for bad in (dict(capacity=-1), dict(rgb=None)):
        with pytest.raises(capi.PcpError) as e:
            ctx.ascii_rows(ref.XYZRGB, f, **{"rgb": rgb, **bad})
        assert e.value.code == capi.PCP_ERR_INVALID


# ---- the resident forms ---------------------------------------------------------------------------------------------------

def _coloured(gpu_ctx_factory, s, fusion):
    from pointcloudprocessor_amd import capi

    c = gpu_ctx_factory()
    c.set_camera(cam_struct(capi, s["cam"]))
    c.upload_cloud(s["x"], s["y"], s["z"])
    c.set_frames(s["poses"])
    for f, im in enumerate(s["images"]):
        c.upload_image(f, im)
        c.upload_mask(f, s["masks"][f])
    c.set_label_fusion(fusion)
    return c


@pytest.mark.parametrize("fusion", [False, True])
def test_colour_compact_ascii_equals_the_text_of_colour_compact(gpu_ctx_factory, small_scene, fusion):
    from pointcloudprocessor_amd import capi

    c = _coloured(gpu_ctx_factory, small_scene, fusion)
    with pytest.raises(capi.PcpError) as e:  # no result yet
        c.colour_compact_ascii()
    assert e.value.code == capi.PCP_ERR_STATE
    c.colorize(download=False)
    rows = c.colour_compact(want_label=fusion)
    m = rows["count"]
    assert 1000 < m < c.n
    kind = ref.XYZRGBMASK if fusion else ref.XYZRGB
    want = ref.rows_text(kind, rows["xyz"], rows["rgb"], rows["label"] if fusion else None)
    text, got_rows = c.colour_compact_ascii(with_label=fusion)
    assert got_rows == m
    _same(text, want)
    # windows of 1, 777 and the rest concatenate to the whole; a window past the end is empty
    parts, first = [], 0
    for size in (1, 777, None):
        t, r = c.colour_compact_ascii(with_label=fusion, first_row=first, max_rows=size)
        assert r == (size if size is not None else m - first)
        parts.append(t.tobytes())
        first += r
    assert first == m and b"".join(parts) == want
    t, r = c.colour_compact_ascii(with_label=fusion, first_row=m, max_rows=5, capacity=1024)
    assert r == 0 and t.size == 0
    with pytest.raises(capi.PcpError) as e:
        c.colour_compact_ascii(with_label=fusion, capacity=len(want) - 1)
    assert e.value.code == capi.PCP_ERR_RANGE and e.value.bytes == len(want)
    with pytest.raises(capi.PcpError) as e:
        c.colour_compact_ascii(with_label=fusion, first_row=-1)
    assert e.value.code == capi.PCP_ERR_INVALID
    if not fusion:
        with pytest.raises(capi.PcpError) as e:  # a label column of a result made without fusion
            c.colour_compact_ascii(with_label=True)
        assert e.value.code == capi.PCP_ERR_STATE
    assert np.array_equal(c.colour_compact(want_label=fusion)["xyz"], rows["xyz"]), "the binary call is unchanged"


def test_mls_fetch_ascii_equals_the_text_of_mls_fetch(gpu_ctx_factory):
    from pointcloudprocessor_amd import capi

    rng = np.random.default_rng(17)
    a = rng.uniform(-0.2, 0.2, (5000, 2))
    pts = np.stack([a[:, 0] + 3.0, a[:, 1] - 2.0, 1.5 + 0.3 * a[:, 0] + rng.normal(0, 1e-3, 5000)], 1).astype(np.float32)
    c = gpu_ctx_factory()
    c.upload_cloud(pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy())
    mp = capi.default_mls_params()
    mp.upsampling = 0
    m = c.mls_process(mp)
    rows = c.mls_fetch(m)
    assert m > 4000
    f = np.concatenate([rows["xyz"], rows["normal"], rows["curvature"][:, None]], 1)
    want = ref.rows_text(ref.POINTNORMAL, f)
    assert b"e-0" in want, "normals and curvature bring the exponent notation"
    text, r = c.mls_fetch_ascii(m)
    assert r == m
    _same(text, want)
    t1, r1 = c.mls_fetch_ascii(m, first_row=0, max_rows=1001)
    t2, r2 = c.mls_fetch_ascii(m, first_row=1001)
    assert (r1, r2) == (1001, m - 1001) and t1.tobytes() + t2.tobytes() == want
    t3, r3 = c.mls_fetch_ascii(m, first_row=m, max_rows=10, capacity=64)
    assert r3 == 0 and t3.size == 0
