"""PCP_MATCH_RADIUS without a GPU: the constants of the C header and of capi, the Python refusal of the sharded form and the
command line's parse-time checks of --matchBack."""
import os
import re
import subprocess

import pytest


def test_header_and_capi_constants():
    from pointcloudprocessor_amd import _build, capi

    with open(os.path.join(_build.INCLUDE, "pcp_hip.h")) as f:
        text = f.read()
    assert re.search(r"#define PCP_MATCH_RADIUS 2\b", text)
    assert re.search(r"#define PCP_ABI_VERSION 6\b", text) and re.search(r"PCP_K_COUNT\s*=\s*13", text)
    assert (capi.MATCH_IDENTITY, capi.MATCH_ROUNDTRIP, capi.MATCH_RADIUS) == (0, 1, 2)
    assert capi.default_cull_params().match_mode == capi.MATCH_ROUNDTRIP  # the default does not move
    assert "pcp_match.hip" in _build.SOURCES


class _Engine:
    match_mode = 2


def test_pipeline_refuses_radius_over_ranks():
    from pointcloudprocessor_amd import capi
    from pointcloudprocessor_amd.pipeline import PointCloudColorizer

    assert _Engine.match_mode == capi.MATCH_RADIUS
    with pytest.raises(ValueError, match="MATCH_RADIUS"):
        PointCloudColorizer(engine=_Engine(), rank=0, world=2).run()


def _cli(tmp_path, *args):
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    exe = host_build.build()["PointCloudProcessor"]
    # the input files do not exist: options that passed the parser would fail later, on reading the cloud
    return subprocess.run([exe, *args, "-p", str(tmp_path / "none.pcd"), "-o", str(tmp_path / "odo.txt"), "-i",
                           str(tmp_path) + "/"], capture_output=True, text=True)


def test_cli_rejects_bad_match_back(tmp_path):
    p = _cli(tmp_path, "--matchBack", "bogus")
    assert p.returncode == 254
    assert "the argument ('bogus') for option '--matchBack' is invalid (roundtrip, radius)" in p.stderr
    assert "Couldn't read point cloud file." not in p.stderr


@pytest.mark.parametrize("order", [("--gpus", "3", "--matchBack", "radius"), ("--matchBack", "radius", "--gpus", "3")])
def test_cli_rejects_radius_on_several_gpus(tmp_path, order):
    p = _cli(tmp_path, *order)
    assert p.returncode == 254 and "--matchBack radius" in p.stderr and "--gpus 1" in p.stderr
    assert "Couldn't read point cloud file." not in p.stderr


@pytest.mark.parametrize("value", ["roundtrip", "radius"])
def test_cli_accepts_match_back(tmp_path, value):
    p = _cli(tmp_path, "--matchBack", value)
    assert p.returncode == 254 and "Couldn't read point cloud file." in p.stderr  # parsed; failed on the missing cloud
