"""Which call ends which smoothing stream (include/pcp_hip.h): the emission stream of pcp_mls_stream_* and the chain stream of
pcp_cloud_smooth_stream_*.  A stream is ENDED when its _next and its _seek return PCP_ERR_STATE; it is OPEN when its next chunk
is, bit for bit, the chunk an undisturbed stream gave at that place.  What the streams emit is test_mls_gpu.py's and
test_smooth_stream_gpu.py's; here only their lifetime."""
import re

import numpy as np
import pytest

from test_smooth_stream_gpu import _strip

pytestmark = pytest.mark.gpu

EMISSION_CAPACITY = 32768  # the minimum of pcp_mls_stream_begin
CHAIN_CAPACITY = 4096      # the minimum of pcp_cloud_smooth_stream_begin
ROW_KEYS = ("index", "xyz", "normal", "curvature")


def _params(upsampling=3):
    from pointcloudprocessor_amd import capi

    mp = capi.default_mls_params()
    mp.upsampling = upsampling
    mp.vgd_voxel_size = 0.003
    mp.vgd_iterations = 2
    return mp


class Emission:
    """pcp_mls_stream_*"""

    name = "emission"

    @staticmethod
    def begin(ctx, mp=None, capacity=EMISSION_CAPACITY):
        return ctx.mls_stream_begin(mp or _params(), capacity)[-1]

    @staticmethod
    def next(ctx):
        return ctx.mls_stream_next()

    @staticmethod
    def seek(ctx, chunk):
        ctx.mls_stream_seek(chunk)


class Chain:
    """pcp_cloud_smooth_stream_*"""

    name = "chain"

    @staticmethod
    def begin(ctx, mp=None, capacity=CHAIN_CAPACITY):
        return ctx.cloud_smooth_stream_begin(mp or _params(), capacity)[-1]

    @staticmethod
    def next(ctx):
        return ctx.cloud_smooth_stream_next()

    @staticmethod
    def seek(ctx, chunk):
        ctx.cloud_smooth_stream_seek(chunk)


KINDS = (Emission, Chain)


@pytest.fixture(scope="module")
def cloud():
    return _strip(seed=8, n=4000, half_x=0.3, half_y=0.1)


@pytest.fixture(scope="module")
def undisturbed(cloud):
    """per kind of stream: the rows of every chunk of a stream nothing came between, in order"""
    from pointcloudprocessor_amd import capi

    rows = {}
    with capi.Context(0) as ctx:
        ctx.upload_cloud(*cloud)
        for kind in KINDS:
            chunks = kind.begin(ctx)
            rows[kind] = []
            while True:
                m = kind.next(ctx)
                if m == 0:
                    break
                rows[kind].append(ctx.mls_fetch(m))
            assert len(rows[kind]) == chunks, kind.name  # (no chunk without rows: chunk c of the stream is rows[kind][c])
    return rows


def _ctx(gpu_ctx_factory, cloud):
    ctx = gpu_ctx_factory()
    ctx.upload_cloud(*cloud)
    return ctx


def _assert_open_at(ctx, kind, undisturbed, chunk, why):
    want = undisturbed[kind][chunk]
    m = kind.next(ctx)
    assert m == len(want["index"]), (kind.name, chunk, why)
    got = ctx.mls_fetch(m)
    for k in ROW_KEYS:
        assert np.array_equal(got[k], want[k]), (kind.name, chunk, k, why)


def _assert_ended(ctx, kind, why):
    from pointcloudprocessor_amd import capi

    for call in (lambda: kind.next(ctx), lambda: kind.seek(ctx, 0)):
        with pytest.raises(capi.PcpError) as e:
            call()
        assert e.value.code == capi.PCP_ERR_STATE, (kind.name, why)


def _open_past_chunk_0(ctx, kind, undisturbed):
    """a stream of this kind, its chunk 0 emitted: chunk 1 is next"""
    kind.begin(ctx)
    _assert_open_at(ctx, kind, undisturbed, 0, "a new stream")


def test_the_input_cuts_into_several_chunks(undisturbed):
    assert len(undisturbed[Emission]) >= 2
    assert len(undisturbed[Chain]) >= 3


def test_calls_that_end_both_streams(gpu_ctx_factory, cloud, undisturbed):
    """an upload, every one-shot smoothing call, and a radius stage (pcp_close_pairs stands for them)"""
    ctx = _ctx(gpu_ctx_factory, cloud)
    plain = _params(upsampling=0)
    enders = {
        "pcp_upload_cloud": lambda: ctx.upload_cloud(*cloud),
        "pcp_mls_process": lambda: ctx.mls_process(plain),
        "pcp_mls_process_shard": lambda: ctx.mls_process_shard(plain, 0, 100),
        "pcp_mls_process_slab": lambda: ctx.mls_process_slab(plain, 0, 2),
        "pcp_cloud_smooth": lambda: ctx.cloud_smooth(plain),
        "pcp_close_pairs": lambda: ctx.close_pairs(1e-3),
    }
    for kind in KINDS:
        for name, call in enders.items():
            _open_past_chunk_0(ctx, kind, undisturbed)
            call()
            _assert_ended(ctx, kind, name)


def test_a_begin_of_one_kind_ends_the_other_kind(gpu_ctx_factory, cloud, undisturbed):
    """at most one of the two streams is ever open"""
    ctx = _ctx(gpu_ctx_factory, cloud)
    _open_past_chunk_0(ctx, Emission, undisturbed)
    Chain.begin(ctx)
    _assert_ended(ctx, Emission, "pcp_cloud_smooth_stream_begin")
    _assert_open_at(ctx, Chain, undisturbed, 0, "pcp_cloud_smooth_stream_begin")
    Emission.begin(ctx)
    _assert_ended(ctx, Chain, "pcp_mls_stream_begin")
    _assert_open_at(ctx, Emission, undisturbed, 0, "pcp_mls_stream_begin")


def test_an_outlier_removal_ends_the_emission_stream_only(gpu_ctx_factory, cloud, undisturbed):
    ctx = _ctx(gpu_ctx_factory, cloud)
    removals = {"pcp_sor": lambda: ctx.sor(60, 0.7), "pcp_sor_partial": lambda: ctx.sor_partial(60, 0, 2)}
    for name, call in removals.items():
        _open_past_chunk_0(ctx, Emission, undisturbed)
        call()
        _assert_ended(ctx, Emission, name)
    _open_past_chunk_0(ctx, Chain, undisturbed)
    for chunk, (name, call) in enumerate(removals.items(), start=1):
        call()
        _assert_open_at(ctx, Chain, undisturbed, chunk, name)  # (the chain's next chunk is the one it was)


def test_reading_calls_leave_a_stream_open(gpu_ctx_factory, cloud, undisturbed):
    """_next, _seek, pcp_mls_fetch and pcp_cloud_smooth_stream_stats; a _seek names the chunk the next _next emits"""
    from pointcloudprocessor_amd import capi

    ctx = _ctx(gpu_ctx_factory, cloud)
    with pytest.raises(capi.PcpError) as e:
        ctx.cloud_smooth_stream_stats()  # (a context that never built a chain stream has no numbers)
    assert e.value.code == capi.PCP_ERR_STATE
    for kind in KINDS:
        last = len(undisturbed[kind]) - 1
        _open_past_chunk_0(ctx, kind, undisturbed)
        if kind is Chain:
            ctx.cloud_smooth_stream_stats()
        _assert_open_at(ctx, kind, undisturbed, 1, "_next, pcp_mls_fetch, _stats")
        kind.seek(ctx, last)
        _assert_open_at(ctx, kind, undisturbed, last, "_seek to the last chunk")
        kind.seek(ctx, 0)
        _assert_open_at(ctx, kind, undisturbed, 0, "_seek back to chunk 0")
        kind.seek(ctx, last + 1)
        assert kind.next(ctx) == 0  # (past the last chunk: no rows, no error, still a stream)
        kind.seek(ctx, 1)
        _assert_open_at(ctx, kind, undisturbed, 1, "_seek from past the end")


def test_the_chains_numbers_outlive_its_stream(gpu_ctx_factory, cloud, undisturbed):
    """pcp_cloud_smooth_stream_end ends the chain stream and frees what it held; pcp_cloud_smooth_stream_stats goes on
    returning the numbers of the last stream built, after _end and after an upload"""
    ctx = _ctx(gpu_ctx_factory, cloud)
    _open_past_chunk_0(ctx, Chain, undisturbed)
    built = ctx.cloud_smooth_stream_stats()
    assert built["device_bytes_held"] > 0
    ctx.cloud_smooth_stream_end()
    _assert_ended(ctx, Chain, "pcp_cloud_smooth_stream_end")
    held_nothing = dict(built, device_bytes_held=0)
    assert ctx.cloud_smooth_stream_stats() == held_nothing
    ctx.upload_cloud(*cloud)
    assert ctx.cloud_smooth_stream_stats() == held_nothing
    _open_past_chunk_0(ctx, Chain, undisturbed)
    ctx.upload_cloud(*cloud)  # (an upload does not free the distances: the numbers are the open stream's to the byte)
    again = ctx.cloud_smooth_stream_stats()
    assert again["device_bytes_held"] == built["device_bytes_held"] and again["threshold"] == built["threshold"]


def test_a_refused_begin_leaves_the_streams_as_they_were(gpu_ctx_factory, cloud, undisturbed):
    """refused for its arguments: a capacity below the minimum, an upsampling other than VOXEL_GRID_DILATION"""
    from pointcloudprocessor_amd import capi

    ctx = _ctx(gpu_ctx_factory, cloud)
    refused = {
        "pcp_mls_stream_begin, capacity": lambda: Emission.begin(ctx, _params(), EMISSION_CAPACITY - 1),
        "pcp_mls_stream_begin, upsampling": lambda: Emission.begin(ctx, _params(upsampling=0)),
        "pcp_cloud_smooth_stream_begin, capacity": lambda: Chain.begin(ctx, _params(), CHAIN_CAPACITY - 1),
        "pcp_cloud_smooth_stream_begin, upsampling": lambda: Chain.begin(ctx, _params(upsampling=0)),
    }
    for kind in KINDS:
        _open_past_chunk_0(ctx, kind, undisturbed)
        for name, call in refused.items():
            with pytest.raises(capi.PcpError) as e:
                call()
            assert e.value.code == capi.PCP_ERR_INVALID, name
        _assert_open_at(ctx, kind, undisturbed, 1, "refused _begin calls")


def test_an_upload_from_a_result_leaves_the_sources_stream_open(gpu_ctx_factory, cloud, undisturbed):
    """pcp_upload_cloud_from_result into another context changes nothing of the source"""
    src = _ctx(gpu_ctx_factory, cloud)
    dst = gpu_ctx_factory()
    for kind in KINDS:
        _open_past_chunk_0(src, kind, undisturbed)
        assert dst.upload_cloud_from_result(src) == len(undisturbed[kind][0]["index"])
        _assert_open_at(src, kind, undisturbed, 1, "pcp_upload_cloud_from_result")


def _balls(ctx, capfd, ball):
    """A new chain stream under PCP_CSS_DEBUG: the ball of the trailing filter it reports at its first chunk (as printed), and
    the ball its last chunk leaves when the first one starts from `ball` -- the rule of pcp_cloud_smooth_stream_begin replayed
    on the shares of flagged rows it reports, checked against every ball it printed."""
    capfd.readouterr()
    Chain.begin(ctx)
    lines = re.findall(r"chunk \d+: ball (\d+\.\d+), (\d+\.\d+) of the own rows flagged", capfd.readouterr().err)
    assert len(lines) >= 3
    for printed, flagged in lines:
        assert printed == "%.3f" % ball
        if float(flagged) > 0.03:
            ball = min(2.4, ball * 1.26)
        elif float(flagged) < 0.003:
            ball = max(1.0, ball / 1.12)
    return lines[0][0], ball


def test_the_chains_ball_outlives_a_stream_and_resets_at_an_upload(gpu_ctx_factory, cloud, monkeypatch, capfd):
    """the ball moves from chunk to chunk by what the selection flagged; the next stream of the same cloud starts from where
    the last chunks left it, a stream after an upload from the default 1.2"""
    monkeypatch.setenv("PCP_CSS_DEBUG", "1")
    ctx = _ctx(gpu_ctx_factory, cloud)
    first, left = _balls(ctx, capfd, 1.2)
    assert first == "1.200" and "%.3f" % left != "1.200"  # (it moves on this input: else nothing below says anything)
    ctx.cloud_smooth_stream_end()
    carried, left_again = _balls(ctx, capfd, left)
    assert carried == "%.3f" % left
    ctx.upload_cloud(*cloud)
    assert _balls(ctx, capfd, 1.2) == (first, left)
