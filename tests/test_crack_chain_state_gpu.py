"""The lifetime rules of the crack chain's tables ("The crack chain as one piece"), written down as data and walked:
from every starting state every event, then the return code of all six fetches, and for a table the event keeps the same bytes
as before it.  The scene is that of test_crack_skeleton_gpu.py::test_state_rules_and_windows (64 x 64 keyframes, a small Y and
700 uniform points before a wall): several cracks, several nodes per crack and edges, so every table has rows."""
import numpy as np
import pytest

import _crack_fuse_ref as ref
import _crack_skeleton_ref as cs_ref
import _crack_width_ref as cw_ref
from test_crack_fuse_gpu import _case_scene, _setup

pytestmark = pytest.mark.gpu

RADIUS = 0.005
STEP = 0.01
LEVELS = ("components", "lengths", "skeleton")
# the tables a starting state leaves readable (the fusion is live in all of them)
STATES = {"fresh": (), "added": (), "components": ("components",), "lengths": ("components", "lengths"),
          "skeleton": ("components", "lengths", "skeleton")}
# event -> what becomes of each table: "made" (readable after it), "kept" (as before it, and the same bytes), "gone"
EVENTS = {
    "add": dict(components="gone", lengths="gone", skeleton="gone"),
    "components": dict(components="made", lengths="kept", skeleton="kept"),
    "lengths": dict(components="made", lengths="made", skeleton="gone"),
    "skeleton": dict(components="made", lengths="made", skeleton="made"),
    "end": dict(components="gone", lengths="gone", skeleton="gone"),
    "upload": dict(components="gone", lengths="gone", skeleton="gone"),
    "set_frames": dict(components="gone", lengths="gone", skeleton="gone"),
}


def test_every_event_from_every_state(gpu_ctx_factory):
    from pointcloudprocessor_amd import capi

    C = capi.C
    cases = ref.component_cases(RADIUS)
    xyz = np.concatenate([cs_ref.small_y(1), cases["uniform"][0][:700] + np.array([0.0, 0.2, 0.0], np.float32)]).astype(np.float32)
    cloud, poses, masks = _case_scene(xyz)
    cam = cw_ref.camera((64, 64))
    cam.update(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)
    got = C.c_int64(-1)
    ctx = gpu_ctx_factory()
    L, h = ctx.lib, ctx.h
    # (level, fetch, the widths of its output arrays after first and max_rows: None for an array this walk does not read)
    fetches = (("components", L.pcp_crack_components_fetch, (("i4", 1), ("i8", 5), ("f4", 6))),
               ("lengths", L.pcp_crack_lengths_fetch, (("i4", 1), ("i8", 7), None)),
               ("lengths", L.pcp_crack_paths_fetch, (("i4", 1),)),
               ("skeleton", L.pcp_crack_skeleton_nodes_fetch, (("i4", 1), ("i8", 10))),
               ("skeleton", L.pcp_crack_skeleton_edges_fetch, (("i8", 3),)),
               ("skeleton", L.pcp_crack_skeleton_cracks_fetch, (("i8", 6),)))

    def codes():
        return [fn(h, C.c_int64(0), C.c_int64(1), *([None] * len(outs)), C.byref(got)) for _, fn, outs in fetches]

    def full(level):
        """every row of the level's tables, as bytes"""
        blob = []
        for lv, fn, outs in fetches:
            if lv != level:
                continue
            assert fn(h, C.c_int64(0), C.c_int64(2 ** 62), *([None] * len(outs)), C.byref(got)) == capi.PCP_OK
            rows = got.value
            assert rows > 0, (level, fn.__name__, "the scene is wrong: an empty table")
            arrs = [None if o is None else np.zeros((rows, o[1]), o[0]) for o in outs]
            assert fn(h, C.c_int64(0), C.c_int64(rows), *[capi._ptr(a) for a in arrs], C.byref(got)) == capi.PCP_OK and got.value == rows
            blob += [a.tobytes() for a in arrs if a is not None]
        return blob

    def reach(state):
        _setup(ctx, cam, cloud, poses, masks)
        ctx.crack_fuse_begin()
        if state != "fresh":
            ctx.crack_fuse_add(0, 0, 150)
        if state == "components":
            ctx.crack_components(1, RADIUS)
        elif state == "lengths":
            ctx.crack_lengths(1, RADIUS)
        elif state == "skeleton":
            ctx.crack_skeleton(1, RADIUS, STEP)

    def apply(event, state):
        if event == "add":
            ctx.crack_fuse_add(0 if state == "fresh" else 1, 0, 150)
        elif event == "components":
            ctx.crack_components(1, 0.008)
        elif event == "lengths":
            ctx.crack_lengths(1, RADIUS)
        elif event == "skeleton":
            ctx.crack_skeleton(1, RADIUS, STEP)
        elif event == "end":
            ctx.crack_fuse_end()
        elif event == "upload":
            ctx.upload_cloud(cloud[:, 0].copy(), cloud[:, 1].copy(), cloud[:, 2].copy())
        else:
            ctx.set_frames(np.asarray(poses, np.float64))

    ok = {True: capi.PCP_OK, False: capi.PCP_ERR_STATE}
    assert codes() == [capi.PCP_ERR_STATE] * 6  # no fusion at all
    for state, readable in STATES.items():
        for event, rule in EVENTS.items():
            reach(state)
            assert codes() == [ok[lv in readable] for lv, _, _ in fetches], (state, "before", event)
            kept = [lv for lv in LEVELS if rule[lv] == "kept" and lv in readable]
            before = {lv: full(lv) for lv in kept}
            apply(event, state)
            after = {lv: rule[lv] == "made" or (rule[lv] == "kept" and lv in readable) for lv in LEVELS}
            assert codes() == [ok[after[lv]] for lv, _, _ in fetches], (state, event)
            for lv in kept:
                assert full(lv) == before[lv], (state, event, lv)
