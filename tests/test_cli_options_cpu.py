"""The command line as a whole (pointcloudprocessor_amd/host/cli_options.hpp), without a GPU and without the HIP runtime:
host/options_probe parses a few thousand command lines in one process and prints, per line, the error or the fields of
Options that differ from the defaults.

tests/golden/cli_options.txt holds what the hand-written parser of the commit before the option table answered to the same
corpus (the same probe source compiled against that main.cpp); tests/golden/cli_help.txt is that commit's --help.  The
corpus is built here, from the table the probe prints (--rows): a new flag extends it without an edit.

Probe values per reader kind: the full product of flags and values is about 9000 lines, 0.6 MB; every kind sees the values
that tell it from another kind (booleans see no comma lists and no large numbers, numbers see no boolean words but "true"),
the irregular flags see every value.  Nothing is sampled.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

BASIC = ["", "0", "1", "2", "-1", " 1", "1 ", "1abc", "abc"]
BOOLISH = ["true", "YES", "on", "Off", "maybe"]
REALS = ["0.5", "1e-4", "9.9e-5", "0.005", "0.0049", "1.0001", "1e9", "nan", "inf", "-inf", "0x1p-3", "1e-50", "1e39", "0.01abc", "-0"]
LISTS = ["8,8", "0,17", "1,2,", "0,0,1", "0,0,0", "1,2,3,4,5,6,7,8,9", "1,2,3,4,5,6,7,8"]
BIG = ["2147483647", "2147483648", "99999999999999999999"]
FRAME_WORDS = ["auto", "facets"]

M = ["-m", "masks/"]
G2 = ["--gpus", "2"]
CM = ["--compareMap", "b.pcd"]
S = ["--streamColour", "1", "--enableMLS", "1", "--skip_filtered_dumps", "1"]
FUSE = M + ["--crackFuse", "1"]

# what a flag needs beside it to be stored and not refused; a flag that marks a value-flag group must stand here or in NO_SWITCH
ENABLE = {
    "--claheClip": ["--balanceImages", "1"], "--claheTiles": ["--balanceImages", "1"], "--balanceGamma": ["--balanceImages", "1"],
    "--registerRadius": CM + ["--compareRegister", "1"], "--registerMaxDistance": CM + ["--compareRegister", "1"],
    "--registerStride": CM + ["--compareRegister", "1"], "--registerIterations": CM + ["--compareRegister", "1"],
    "--defectThreshold": ["--orthoMap", "1", "--orthoDefects", "1"], "--defectWindow": ["--orthoMap", "1", "--orthoDefects", "1"],
    "--defectRefine": ["--orthoMap", "1", "--orthoDefects", "1", "--defectWindow", "3"],
    "--defectMinSupport": ["--orthoMap", "1", "--orthoDefects", "1"], "--defectMinPixels": ["--orthoMap", "1", "--orthoDefects", "1"],
    "--defectClasses": ["--orthoMap", "1", "--orthoDefects", "1"],
    "--orthoTextureViews": ["--orthoMap", "1", "--orthoTexture", "2"], "--orthoTextureInterp": ["--orthoMap", "1", "--orthoTexture", "2"],
    "--orthoTextureStep": ["--orthoMap", "1", "--orthoTexture", "2"],
    "--orthoTexture": ["--orthoMap", "1"], "--orthoDefects": ["--orthoMap", "1"],
    "--orthoTextureCylinders": ["--facets", "1", "--facetCylinders", "1", "--orthoMap", "1", "--orthoFrame", "facets", "--orthoTexture", "2"],
    "--skip_full_cloud": ["--outputLeaf", "0.05"],
    "--fuseMasks": M, "--crackMaps": M, "--crackWidth": M, "--crackFuse": M,
    "--crackLength": FUSE, "--crackSkeleton": FUSE, "--crackDirection": FUSE, "--crackBranches": FUSE,
    "--crackSkeletonStep": FUSE + ["--crackSkeleton", "1"],
    "--facetCylinders": ["--facets", "1"], "--orthoFrame": ["--facets", "1"],
    "--streamColour": ["--enableMLS", "1", "--skip_filtered_dumps", "1"],
    "--compareRegister": CM,
}
NO_SWITCH = {"--point_cloud_path", "--odometry_path", "--images_folder", "--crackPrune"}  # mark a field, need no other flag

# the cross-flag rules in the order in which they are checked: a minimal command line for each
RULES = [
    ["--matchBack", "radius"] + G2,
    ["--fuseMasks", "1"],
    ["--deviceWriter", "1"] + G2,
    ["--skip_full_cloud", "1"],
    ["--outputLeaf", "0.05"] + G2,
    ["--orthoTextureCylinders", "1"],
    ["--orthoTextureViews", "2"],
    ["--orthoTexture", "2"],
    ["--defectWindow", "3"],
    ["--orthoDefects", "1"],
    ["--orthoMap", "1", "--orthoDefects", "1"] + G2,
    ["--orthoMap", "1", "--orthoDefects", "1", "--defectRefine", "1"],
    ["--orthoMap", "1", "--orthoTexture", "2"] + G2,
    ["--orthoMap", "1", "--orthoTexture", "2", "--cull", "hpr"],
    ["--orthoMap", "1"] + G2,
    ["--geometryMaps", "1"] + G2,
    ["--crackMaps", "1"],
    M + ["--crackMaps", "1"] + G2,
    ["--crackWidth", "1"],
    M + ["--crackWidth", "1"] + G2,
    M + ["--crackWidth", "1", "--enableMLS", "1"],
    ["--crackLength", "1"],
    ["--crackSkeleton", "1"],
    ["--crackDirection", "1"],
    ["--crackBranches", "1"],
    ["--crackPrune", "-1"],
    FUSE + ["--crackBranches", "1", "--crackSkeletonStep", "17"],
    FUSE + ["--crackSkeleton", "1", "--crackSkeletonStep", "17"],
    ["--crackFuse", "1"],
    FUSE + G2,
    FUSE + ["--enableMLS", "1"],
    ["--geometryMaps", "1", "--enableMLS", "1"],
    ["--orthoFrame", "facets"],
    ["--facetCylinders", "1"],
    ["--facets", "1"] + G2,
    ["--facets", "1", "--streamColour", "1"],
    ["--facets", "1", "--enableMLS", "1"],
    ["--facets", "1", "--normalRadius", "0"],
    ["--registerStride", "2"],
    ["--compareRegister", "1"],
    CM + ["--compareRegister", "1"] + G2,
    CM + ["--compareRegister", "1", "--streamColour", "1"],
    CM + ["--compareRegister", "1", "--enableMLS", "1"],
    CM + ["--compareRegister", "1", "--registerMaxDistance", "0.2"],
    CM + G2,
    CM + ["--streamColour", "1"],
    CM + ["--enableMLS", "1"],
    CM + ["--normalRadius", "0"],
    ["--claheClip", "2"],
    ["--balanceExposure", "1"] + G2,
    ["--balanceExposure", "1", "--streamColour", "1"],
    ["--streamColour", "1"],
    ["--streamColour", "1", "--enableMLS", "1"],
    S + ["--enableNIDOptimize", "1"],
    S + ["--enableInitialGuessManual", "1"],
    S + G2,
    S + ["--cull", "hpr"],
    S + ["--matchBack", "radius"],
    S + ["--smoothColorsRadius", "0.1"],
    S + M,
    S + ["--mlsUpsampling", "slp"],
]
# rule k together with rule k + 1: the two command lines joined, except where joining them switches one of the two off
PAIRS = {
    9: ["--orthoDefects", "1"] + G2,
    16: ["--crackMaps", "1"] + G2,
    18: ["--crackWidth", "1"] + G2,
    27: ["--crackFuse", "1", "--crackSkeleton", "1", "--crackSkeletonStep", "17"],
    28: ["--crackFuse", "1"] + G2,
    39: ["--compareRegister", "1"] + G2,
    51: ["--streamColour", "1"],
    52: ["--streamColour", "1", "--enableMLS", "1", "--enableNIDOptimize", "1"],
}
FRAME9 = "1,2,3,4,5,6,7,8,9"
ODDITIES = [
    [], ["-h"], ["--help"], ["--help=1"],
    # a flag given twice: the last one counts
    ["--crackThreshold", "5", "--crackThreshold", "7"], ["--enableMLS", "1", "--enableMLS", "0"],
    ["--orthoFrame", FRAME9, "--orthoFrame", "auto"], ["--orthoFrame", "facets", "--orthoFrame", "auto"], ["--orthoFrame", "auto", "--orthoFrame", FRAME9],
    ["--crackPrune", "-1", "--crackPrune", "1"], ["--cull", "hpr", "--cull=zbuffer"], ["-p", "a", "--point_cloud_path", "b"],
    # two value flags of one group without their switch: the message names the first
    ["--balanceGamma", "1.1", "--claheClip", "2"], ["--claheTiles", "4,4", "--balanceGamma", "1.1"], ["--claheClip=2", "--claheTiles", "4,4"],
    ["--registerStride", "2", "--registerRadius", "0.1"], ["--registerIterations", "5", "--registerStride", "2"],
    ["--registerMaxDistance=0.01", "--registerIterations", "5"], ["--balanceImages", "0", "--balanceGamma", "1.1"],
    # -h with what is refused
    ["-h", "--crackFuse", "1"], ["--crackLength", "1", "-h"], ["-h", "--bogus"], ["-h", "--gpus"],
    # not an option
    ["--bogus"], ["--bogus=1"], ["--bogus", "1"], ["-x"], ["bare"], ["-p=x"], ["--", "x"], ["--crackthreshold", "1"], ["--=1"],
    # a value that looks like a flag is a value
    ["-p", "--gpus"], ["--compareMap", "-h"],
]


def _binary(name):
    from pointcloudprocessor_amd import _build, host_build

    _build.build()
    return host_build.build()[name]


def _probe():
    return _binary("options_probe")


def _rows():
    p = subprocess.run([_probe(), "--rows"], capture_output=True, text=True, check=True)
    rows = []
    for line in p.stdout.splitlines():
        name, short, kind, listed, marks, lo, hi, words = line.split("\t")
        rows.append(dict(name=name, short=short, kind=kind, listed=listed == "1", marks=marks == "1", lo=int(lo), hi=int(hi),
                         words=words.split(",") if words else []))
    return rows


def _values(row, rows):
    """The probe values of a flag, by its reader kind."""
    words = sorted({w for r in rows for w in r["words"]})
    bounds = sorted({str(b) for r in rows if r["kind"] in ("IntStrict", "Int64Strict", "IntPrefix") for b in (r["lo"] - 1, r["lo"], r["hi"], r["hi"] + 1)},
                    key=int)
    kind = row["kind"]
    if kind in ("BoolWord", "Bool01"):
        vals = BASIC + BOOLISH + ["0.5", "TRUE", "False", "no", "oN"]
    elif kind in ("IntStrict", "Int64Strict", "IntPrefix", "IntThrow"):
        vals = BASIC + ["true", "0.5", "1e9", "0x1p-3", "8,8", "+1", "0x10", "010"] + BIG + bounds
    elif kind in ("FloatStrict", "FloatStrictFinite", "DoubleNarrowed", "FloatPrefix", "FloatThrow", "DoubleThrow"):
        vals = BASIC + ["true", "8,8"] + REALS + BIG
    elif kind == "Word":
        vals = BASIC + words + ["HPR", "Both"]
    elif kind == "Text":
        vals = BASIC + ["a b"]
    elif kind == "Custom":
        vals = BASIC + BOOLISH + REALS + LISTS + BIG + words + FRAME_WORDS + ["16,16", "17,1", "1,17", "8;8", ",8", "0,nan,1", "0,0,1e-200", "1e200,1e200,1e200",
                                                                                       "1,2,3,4,5,6,7,8,x", "1,2,3,4,5,6,7,8,9,", "1,2,3,4,5,6,7,8,9,10"]
    else:
        raise AssertionError(f"reader kind {kind} of {row['name']}: say here which values it sees")
    return list(dict.fromkeys(vals))


def _valid(row):
    kind, name = row["kind"], row["name"]
    if kind in ("IntStrict", "Int64Strict", "IntPrefix"):
        return str(row["lo"])
    if kind == "Word":
        return row["words"][0]
    if kind == "Custom":
        return {"--claheTiles": "4,4", "--crackUp": "0,3,4", "--orthoFrame": "facets"}[name]
    return {"Text": "x", "BoolWord": "1", "Bool01": "1", "IntThrow": "1"}.get(kind, "0.01")


def _corpus():
    rows = _rows()
    lines = []
    for row in rows:
        name = row["name"]
        if row["marks"]:
            assert name in ENABLE or name in NO_SWITCH, f"{name} marks a value-flag group: name its switch in ENABLE"
        with_ = [[]] + ([ENABLE[name]] if name in ENABLE else [])
        if row["kind"] == "None":
            lines += [[name], [name + "=1"], [row["short"]]]
            continue
        for pre in with_:
            lines.append(pre + [name])                          # 1. the value is missing
            lines.append(pre + [name + "=" + _valid(row)])      # 2. --flag=value
            lines += [pre + [name, v] for v in _values(row, rows)]  # 3., 4. the probe list, alone and enabled
        lines.append([name + "="])
        if row["short"]:                                        # 7. each short form
            lines += [[row["short"]], [row["short"], "x"], [row["short"], ""]]
    lines += RULES                                              # 5. each rule alone
    lines += [PAIRS.get(k, RULES[k] + RULES[k + 1]) for k in range(len(RULES) - 1)]  # 6. neighbours: which one wins
    lines += ODDITIES
    for args in lines:
        assert not any("\t" in a or "\n" in a for a in args)
    return lines, rows


def _run(lines):
    p = subprocess.run([_probe()], input="".join("\t".join(a) + "\n" for a in lines), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.split("\n")
    assert out[-1] == "" and len(out) - 1 == len(lines), (len(out) - 1, len(lines))  # one answer per command line: none skipped
    return out[:-1]


def test_every_flag_answers_as_the_hand_written_parser_did():
    lines, rows = _corpus()
    got = _run(lines)
    path = os.path.join(GOLDEN, "cli_options.txt")
    assert os.path.getsize(path) < 256 * 1024
    with open(path) as f:
        want = f.read().split("\n")[:-1]
    assert len(want) == len(got), (len(want), len(got))
    bad = [(a, w, g) for a, w, g in zip(lines, want, got) if w != g]
    for a, w, g in bad[:20]:
        print("command line:", a, "\n  was:", w, "\n  is: ", g)
    assert not bad, f"{len(bad)} of {len(lines)} command lines answer differently"
    assert all(g[:2] in ("E\t", "O\t") for g in got)
    # the corpus reaches every flag, and every rule fires alone with a message of its own
    assert len(rows) > 80 and all(any(r["name"] in a for a in lines) for r in rows)
    alone = got[len(got) - len(ODDITIES) - (2 * len(RULES) - 1):][:len(RULES)]
    assert all(a.startswith("E\tthe ") for a in alone) and len(set(alone)) == len(RULES) - 1  # (--crackSkeletonStep: two rules, one text)


def test_help_text_is_unchanged():
    exe = _binary("PointCloudProcessor")
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert p.returncode == 1 and p.stderr == ""
    with open(os.path.join(GOLDEN, "cli_help.txt")) as f:
        assert p.stdout == f.read()
    # what the parser accepts without listing it stays unlisted
    listed = {r["name"] for r in _rows() if r["listed"]}
    for flag in ("--gpus", "--mlsVoxelSize", "--mlsDilationIterations", "--mlsUpsampling", "--mlsUpsamplingRadius", "--mlsUpsamplingStep", "--cull",
                 "--matchBack", "--smoothColorsRadius", "--fuseMasks", "--streamColour", "--streamChunk", "--skip_filtered_dumps"):
        assert flag not in listed and ("\n  " + flag + " ") not in p.stdout


# The refusals that the per-feature command-line tests (tests/test_cli_*_gpu.py: test_refusals_name_the_flags,
# test_flag_errors) check through the real binary on a GPU machine: the same flags behind the same fixed arguments, the same
# needles.  parse() refuses them before any device is touched, so they are checked here too.
PLAIN = ["-p", "scans.pcd", "-o", "odo.txt", "-i", "src/", "-t", "out/"]
MASKS = PLAIN + ["-m", "src/"]
NODUMPS = PLAIN + ["--skip_filtered_dumps", "1"]
CYL_NEEDLES = ("--orthoTextureCylinders 1", "--orthoTexture k", "--facetCylinders 1", "--orthoFrame facets")
REFUSALS = [
    # test_cli_compare_gpu
    (NODUMPS + CM, ("--gpus", "2"), ("--compareMap", "--gpus", "index shard", "not built")),
    (NODUMPS + CM, ("--enableMLS", "1"), ("--compareMap", "--enableMLS 1", "not built")),
    (NODUMPS + CM, ("--enableMLS", "1", "--streamColour", "1"), ("--compareMap", "--streamColour 1", "chunk")),
    (NODUMPS + CM, ("--normalRadius", "0"), ("--compareMap", "--normalRadius 0")),
    (NODUMPS + CM, ("--compareRadius", "0.004"), ("--compareRadius", "invalid")),
    (NODUMPS + CM, ("--compareMinPoints", "1"), ("--compareMinPoints", "invalid")),
    # test_cli_crack_branch_gpu
    (MASKS, ("--crackBranches", "1"), ("--crackBranches 1", "--crackFuse 1")),
    (MASKS, ("--crackFuse", "1", "--crackBranches", "1", "--crackPrune", "-0.5"), ("--crackPrune", "1024")),
    (MASKS, ("--crackFuse", "1", "--crackBranches", "1", "--crackPrune", "1025"), ("--crackPrune", "1024")),
    (MASKS, ("--crackFuse", "1", "--crackBranches", "1", "--crackPrune", "nan"), ("--crackPrune", "1024")),
    (MASKS, ("--crackFuse", "1", "--crackBranches", "1", "--crackSkeletonStep", "17"), ("--crackSkeletonStep",)),
    (PLAIN, ("--crackFuse", "1", "--crackBranches", "1"), ("--crackFuse 1", "--mask_image_folder")),
    (MASKS, ("--crackFuse", "1", "--crackBranches", "1", "--gpus", "2"), ("--crackFuse 1", "--gpus", "index shard", "not built")),
    # test_cli_crack_direction_gpu
    (MASKS, ("--crackDirection", "1"), ("--crackDirection 1", "--crackFuse 1")),
    (MASKS, ("--crackFuse", "1", "--crackDirection", "1", "--crackUp", "0,0,0"), ("--crackUp", "invalid", "not zero")),
    (MASKS, ("--crackFuse", "1", "--crackDirection", "1", "--crackUp", "0,1"), ("--crackUp", "invalid")),
    (MASKS, ("--crackFuse", "1", "--crackDirection", "1", "--crackUp", "0,nan,1"), ("--crackUp", "invalid")),
    (PLAIN, ("--crackFuse", "1", "--crackDirection", "1"), ("--crackFuse 1", "--mask_image_folder")),
    (MASKS, ("--crackFuse", "1", "--crackDirection", "1", "--gpus", "2"), ("--crackFuse 1", "--gpus", "index shard", "not built")),
    # test_cli_crack_fuse_gpu
    (PLAIN, ("--crackFuse", "1"), ("--crackFuse 1", "--mask_image_folder")),
    (MASKS, ("--crackFuse", "1", "--gpus", "2"), ("--crackFuse 1", "--gpus", "index shard", "not built")),
    (MASKS, ("--crackFuse", "1", "--enableMLS", "1"), ("--crackFuse 1", "--enableMLS 1", "smoothed cloud")),
    (MASKS, ("--crackFuse", "1", "--crackLinkRadius", "0.004"), ("--crackLinkRadius", "invalid")),
    (MASKS, ("--crackFuse", "1", "--crackMinViews", "0"), ("--crackMinViews", "invalid")),
    # test_cli_crack_length_gpu
    (MASKS, ("--crackLength", "1"), ("--crackLength 1", "--crackFuse 1")),
    (PLAIN, ("--crackFuse", "1", "--crackLength", "1"), ("--crackFuse 1", "--mask_image_folder")),
    (MASKS, ("--crackFuse", "1", "--crackLength", "1", "--gpus", "2"), ("--crackFuse 1", "--gpus", "index shard", "not built")),
    (MASKS, ("--crackFuse", "1", "--crackLength", "1", "--enableMLS", "1"), ("--crackFuse 1", "--enableMLS 1", "smoothed cloud")),
    # test_cli_crack_maps_gpu
    (PLAIN, ("--crackMaps", "1"), ("--crackMaps 1", "--mask_image_folder")),
    (MASKS, ("--crackMaps", "1", "--gpus", "2"), ("--crackMaps 1", "--gpus", "index shards")),
    (MASKS, ("--crackMaps", "1", "--crackThreshold", "256"), ("--crackThreshold", "invalid")),
    # test_cli_crack_skeleton_gpu
    (MASKS, ("--crackSkeleton", "1"), ("--crackSkeleton 1", "--crackFuse 1")),
    (MASKS, ("--crackFuse", "1", "--crackSkeleton", "1", "--crackSkeletonStep", "17"), ("--crackSkeletonStep", "16")),
    (PLAIN, ("--crackFuse", "1", "--crackSkeleton", "1"), ("--crackFuse 1", "--mask_image_folder")),
    (MASKS, ("--crackFuse", "1", "--crackSkeleton", "1", "--gpus", "2"), ("--crackFuse 1", "--gpus", "index shard", "not built")),
    (MASKS, ("--crackFuse", "1", "--crackSkeleton", "1", "--enableMLS", "1"), ("--crackFuse 1", "--enableMLS 1", "smoothed cloud")),
    # test_cli_crack_width_gpu
    (PLAIN, ("--crackWidth", "1"), ("--crackWidth 1", "--mask_image_folder")),
    (MASKS, ("--crackWidth", "1", "--gpus", "2"), ("--crackWidth 1", "--gpus", "index shard", "not built")),
    (MASKS, ("--crackWidth", "1", "--enableMLS", "1"), ("--crackWidth 1", "--enableMLS 1", "smoothed cloud")),
    (MASKS, ("--crackWidth", "1", "--crackPlaneRadius", "182"), ("--crackPlaneRadius", "invalid")),
    # test_cli_cylinders_gpu
    (PLAIN, ("--facetCylinders", "1"), ("--facetCylinders 1", "--facets 1")),
    (PLAIN, ("--facetCylinders", "1", "--facets", "0"), ("--facetCylinders 1", "--facets 1")),
    (PLAIN, ("--facetCylinders", "1", "--facets", "1", "--gpus", "2"), ("--facets 1", "--gpus", "index shard")),
    # test_cli_facets_gpu
    (PLAIN, ("--facets", "1", "--gpus", "2"), ("--facets 1", "--gpus", "index shard", "not built")),
    (PLAIN, ("--facets", "1", "--enableMLS", "1"), ("--facets 1", "--enableMLS 1", "not built")),
    (PLAIN, ("--facets", "1", "--enableMLS", "1", "--streamColour", "1"), ("--facets 1", "--streamColour 1", "chunk")),
    (PLAIN, ("--orthoMap", "1", "--orthoFrame", "facets"), ("--orthoFrame facets", "--facets 1")),
    (PLAIN, ("--facets", "1", "--normalRadius", "0"), ("--facets 1", "--normalRadius 0")),
    (PLAIN, ("--facets", "1", "--facetAngle", "60"), ("--facetAngle", "invalid")),
    (PLAIN, ("--facets", "1", "--facetMinPoints", "0"), ("--facetMinPoints", "invalid")),
    # test_cli_geometry_gpu
    (PLAIN, ("--geometryMaps", "1", "--gpus", "2"), ("--geometryMaps 1", "--gpus", "index shard", "not built")),
    (PLAIN, ("--geometryMaps", "1", "--normalRadius", "2"), ("--normalRadius", "invalid")),
    (PLAIN, ("--geometryMaps", "1", "--enableMLS", "1"), ("--geometryMaps 1", "--enableMLS 1", "smoothed cloud")),
    # test_cli_image_balance_gpu (test_flag_errors)
    (PLAIN, ("--balanceImages", "2"), ("'--balanceImages'", "is invalid (0, 1)")),
    (PLAIN, ("--balanceImages", "1", "--claheClip", "-1"), ("'--claheClip'", "is invalid")),
    (PLAIN, ("--balanceImages", "1", "--claheClip", "nan"), ("'--claheClip'", "is invalid")),
    (PLAIN, ("--balanceImages", "1", "--claheTiles", "8"), ("'--claheTiles'", "is invalid (x,y with 1..16 each)")),
    (PLAIN, ("--balanceImages", "1", "--claheTiles", "0,8"), ("'--claheTiles'", "is invalid")),
    (PLAIN, ("--balanceImages", "1", "--claheTiles", "8,17"), ("'--claheTiles'", "is invalid")),
    (PLAIN, ("--balanceImages", "1", "--balanceGamma", "0"), ("'--balanceGamma'", "is invalid")),
    (PLAIN, ("--claheClip", "3"), ("'--claheClip'", "needs '--balanceImages 1'")),
    (PLAIN, ("--claheTiles", "4,4", "--balanceImages", "0"), ("'--claheTiles'", "needs '--balanceImages 1'")),
    (PLAIN, ("--balanceGamma", "1.1"), ("'--balanceGamma'", "needs '--balanceImages 1'")),
    # test_cli_ortho_defects_gpu
    (PLAIN, ("--orthoDefects", "1"), ("--orthoDefects 1", "--orthoMap 1")),
    (PLAIN, ("--orthoMap", "1", "--defectWindow", "5"), ("--defectWindow", "--orthoDefects 1")),
    (PLAIN, ("--orthoMap", "1", "--defectClasses", "hollow"), ("--defectClasses", "--orthoDefects 1")),
    (PLAIN, ("--orthoMap", "1", "--orthoDefects", "1", "--defectRefine", "1"), ("--defectRefine 1", "--defectWindow")),
    (PLAIN, ("--orthoMap", "1", "--orthoDefects", "1", "--defectThreshold", "2"), ("--defectThreshold", "2^-20")),
    (PLAIN, ("--orthoMap", "1", "--orthoDefects", "1", "--defectWindow", "1025"), ("--defectWindow", "0..1024")),
    (PLAIN, ("--orthoMap", "1", "--orthoDefects", "1", "--defectMinPixels", "0"), ("--defectMinPixels", "1 or more")),
    (PLAIN, ("--orthoMap", "1", "--orthoDefects", "1", "--defectClasses", "dents"), ("--defectClasses", "hollow, bulge or both")),
    (PLAIN, ("--orthoMap", "1", "--orthoDefects", "1", "--gpus", "2"), ("--gpus",)),
    # test_cli_ortho_gpu
    (PLAIN, ("--orthoMap", "1", "--gpus", "2"), ("--orthoMap 1", "--gpus", "index shard", "not built")),
    (PLAIN, ("--orthoMap", "1", "--orthoGsd", "2"), ("--orthoGsd", "invalid")),
    (PLAIN, ("--orthoMap", "1", "--orthoFill", "2000"), ("--orthoFill", "invalid")),
    (PLAIN, ("--orthoMap", "1", "--orthoFrame", "1,2,3"), ("--orthoFrame", "invalid")),
    # test_cli_ortho_texture_gpu
    (PLAIN, ("--orthoTexture", "4"), ("--orthoTexture", "--orthoMap 1")),
    (PLAIN, ("--orthoMap", "1", "--orthoTexture", "4", "--gpus", "2"), ("--orthoTexture", "--gpus", "index shard")),
    (PLAIN, ("--orthoMap", "1", "--orthoTexture", "4", "--cull", "hpr"), ("--orthoTexture", "--cull hpr", "depth maps")),
    (PLAIN, ("--orthoMap", "1", "--orthoTexture", "17"), ("--orthoTexture", "invalid")),
    (PLAIN, ("--orthoMap", "1", "--orthoTexture", "4", "--orthoTextureViews", "6"), ("--orthoTextureViews", "invalid")),
    (PLAIN, ("--orthoMap", "1", "--orthoTexture", "4", "--orthoTextureStep", "0"), ("--orthoTextureStep", "invalid")),
    (PLAIN, ("--orthoMap", "1", "--orthoTextureViews", "5"), ("--orthoTextureViews", "--orthoTexture k")),
    # test_cli_register_gpu
    (NODUMPS, ("--compareRegister", "1"), ("--compareRegister 1", "needs '--compareMap'")),
    (NODUMPS, ("--compareMap", "B", "--registerStride", "3"), ("--registerStride", "needs '--compareRegister 1'")),
    (NODUMPS, ("--compareMap", "B", "--compareRegister", "1", "--gpus", "2"), ("--compareRegister 1", "--gpus", "index shard", "not built")),
    (NODUMPS, ("--compareMap", "B", "--compareRegister", "1", "--enableMLS", "1"), ("--compareRegister 1", "--enableMLS 1", "not built")),
    (NODUMPS, ("--compareMap", "B", "--compareRegister", "1", "--enableMLS", "1", "--streamColour", "1"), ("--compareRegister 1", "--streamColour 1", "chunk")),
    (NODUMPS, ("--compareMap", "B", "--compareRegister", "1", "--registerRadius", "0.004"), ("--registerRadius", "invalid")),
    (NODUMPS, ("--compareMap", "B", "--compareRegister", "1", "--registerMaxDistance", "0.2"), ("--registerMaxDistance", "invalid", "--registerRadius")),
    (NODUMPS, ("--compareMap", "B", "--compareRegister", "1", "--registerIterations", "0"), ("--registerIterations", "invalid")),
    # test_cli_voxel_output_gpu
    (NODUMPS, ("--outputLeaf", "0.05", "--gpus", "2"), ("--outputLeaf", "--gpus", "voxel sums", "not built")),
    (NODUMPS, ("--skip_full_cloud", "1"), ("--skip_full_cloud 1", "--outputLeaf")),
    (NODUMPS, ("--outputLeaf", "2"), ("--outputLeaf", "invalid")),
    # test_ortho_cyl_texture_pipeline_gpu
    (PLAIN, ("--orthoTextureCylinders", "1"), CYL_NEEDLES),
    (PLAIN, ("--orthoTextureCylinders", "1", "--facets", "1", "--facetCylinders", "1", "--orthoMap", "1", "--orthoFrame", "facets"), CYL_NEEDLES),
    (PLAIN, ("--orthoTextureCylinders", "1", "--facets", "1", "--orthoMap", "1", "--orthoFrame", "facets", "--orthoTexture", "2"), CYL_NEEDLES),
    (PLAIN, ("--orthoTextureCylinders", "1", "--facets", "1", "--facetCylinders", "1", "--orthoMap", "1", "--orthoTexture", "2"), CYL_NEEDLES),
]


def test_refusals_name_the_flags():
    got = _run([base + list(flags) for base, flags, _ in REFUSALS])
    for (base, flags, needles), answer in zip(REFUSALS, got):
        assert answer.startswith("E\t"), (flags, answer)  # (main() turns the exception into its exit code -2)
        for s in needles:
            assert s in answer, (flags, s, answer)


def test_an_exception_of_the_parser_is_exit_254():
    """What the probe reports as E is, in the program, main()'s "Unhandled Exception" and exit code -2 -- also beside -h."""
    exe = _binary("PointCloudProcessor")
    for args, text in ((PLAIN + ["--crackFuse", "1"], "the option '--crackFuse 1' needs the masks (--mask_image_folder)"),
                       (["-h", "--crackLength", "1"], "the option '--crackLength 1' needs the widths on the map (--crackFuse 1)")):
        p = subprocess.run([exe] + args, capture_output=True, text=True)
        assert p.returncode == 254 and p.stdout == "", (p.returncode, p.stdout[-300:])
        assert p.stderr == "Unhandled Exception reached the top of main: " + text + ", application will now exit\n"
