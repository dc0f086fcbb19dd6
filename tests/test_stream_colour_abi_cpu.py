"""CPU suite: the entry points of the streamed colourisation are declared in include/pcp_hip.h, exported by libpcp_hip.so and
bound by capi; the header still compiles as C; the ABI version did not move (entry points added, no layout changed)."""
import os
import subprocess

NEW = ("pcp_upload_cloud_from_result", "pcp_depth_accum_reset", "pcp_depth_accum_merge", "pcp_depth_accum_apply",
       "pcp_depth_accum_device", "pcp_cloud_smooth_stream_seek", "pcp_colour_compact")


def test_new_symbols_are_declared_exported_and_bound():
    from pointcloudprocessor_amd import _build, capi

    _build.build()
    lib = capi.load()
    names = capi.declared_symbols()
    for s in NEW:
        assert s in names, s
        assert hasattr(lib, s), s
    for m in ("upload_cloud_from_result", "depth_accum_reset", "depth_accum_merge", "depth_accum_apply", "depth_accum_device",
              "cloud_smooth_stream_seek", "colour_compact"):
        assert callable(getattr(capi.Context, m)), m
    assert lib.pcp_abi_version() == 6


def test_header_with_the_new_entry_points_is_plain_c(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "abi.c"
    calls = "\n".join(f"  (void){s};" for s in NEW)
    src.write_text('#include "pcp_hip.h"\nint main(void) {\n' + calls + "\n  return PCP_ABI_VERSION == 6 ? 0 : 1;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(root, "include"), "-c", str(src),
                    "-o", str(tmp_path / "abi.o")], check=True, capture_output=True)


def test_generator_is_part_of_the_pipeline():
    from pointcloudprocessor_amd import pipeline

    assert callable(pipeline.CloudSmooth.process_and_colourise_streamed)
