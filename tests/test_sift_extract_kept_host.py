"""The host half of K24 (pp_sift_extract_to_matcher) without a device and under the sanitizers: tests/sift_extract_kept_host_driver.cpp compiles with
g++ -fsanitize=address,undefined -ffp-contract=off and runs as its own program.  pp_sift_extract_to_matcher cuts BEFORE it computes an orientation or a
descriptor, from the keypoint counts of the levels; that cut (SelectKeptKeypoints) must select the level SelectLevels selects on the reference's
containers, its per-octave ranges must be the kept suffix, and the rows of the kept features in the matcher's store (KeptBlockRows) must be each
image's features in the reference's order.  The counts the call reports for the kept features only are printed here from ExtractOnHost's full result;
tests/test_gpu_sift_extract_to_matcher.py reads them through kept_lines()."""
import os
import subprocess

import pytest

import sift_extract_goldens as G

ROOT = G.ROOT
CUTS = (1, 5, 20, 36, 49, 8192)
# what max_num_features = 20 keeps (first feature, features), counted on the CPU from the `levels` of the recordings: of `odd` 42 of 101 - octave -1
# dropped whole, levels 1 and 2 of octave 0, octaves 1 and 2 whole; of `blobs` 28 of 225 - octaves -1 and 0 dropped
CUT_20 = {"odd": (59, 42), "blobs": (197, 28)}


def build_driver(directory, sanitize=True):
    """sanitize=False: the same program built plainly, for a test that runs beside a device"""
    exe = os.path.join(str(directory), "sift_extract_kept_host_driver")
    checks = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + checks + ["-ffp-contract=off", "-o", exe,
                                                                                          os.path.join(ROOT, "tests", "sift_extract_kept_host_driver.cpp")])
    return exe


def run_driver(exe, script):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    return out.stdout.splitlines()


def kept_command(image_file, width, height, options):
    return "kept %s %d %d %s" % (os.path.join(G.GOLDEN, image_file), width, height, G.option_words(options))


def parse_kept(line):
    """-> (verdict, {field: int or 'ok' / 'bad'}, [(first, count) per octave])"""
    words = line.split()
    at = words.index("octaves")
    fields = {k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in zip(words[1:at:2], words[2:at:2])}
    return words[0], fields, [tuple(int(v) for v in w.split(":")) for w in words[at + 1:]]


def kept_lines(exe, requests):
    """requests: [(image_file, width, height, options)] -> parse_kept() of each, in one run of the driver"""
    lines = run_driver(exe, [kept_command(*r) for r in requests])
    assert len(lines) == len(requests), lines
    return [parse_kept(line) for line in lines]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("sift_kept"))


@pytest.fixture(scope="module")
def cuts(driver):
    """every golden case under its own options, and `odd` and `blobs` under every max_num_features of CUTS: one run of the driver"""
    keys = [("case", c["name"]) for c in G.CASES] + [(name, m) for name in ("odd", "blobs") for m in CUTS]
    requests = [(c["image"], c["width"], c["height"], c["options"]) for c in G.CASES]
    for name in ("odd", "blobs"):
        c = G.case(name)
        requests += [(c["image"], c["width"], c["height"], dict(c["options"], max_num_features=m)) for m in CUTS]
    out = dict(zip(keys, kept_lines(driver, requests)))
    for key in keys:
        print(key, out[key])
    return out


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_the_cut_from_the_keypoint_counts_selects_the_level_of_select_levels(cuts, name):
    verdict, f, octaves = cuts[("case", name)]
    c = G.case(name)
    assert verdict == "same" and [f["first_level"], f["first_feature"], f["num_features"]] == c["cut"]      # (the cut recorded from the reference)
    assert f["ranges"] == f["membership"] == f["grouping"] == "ok" and len(octaves) == c["options"]["num_octaves"]


@pytest.mark.parametrize("name", ("odd", "blobs"))
@pytest.mark.parametrize("max_num_features", CUTS)
def test_the_cut_under_every_max_num_features(cuts, name, max_num_features):
    verdict, f, octaves = cuts[(name, max_num_features)]
    assert verdict == "same" and f["ranges"] == f["membership"] == f["grouping"] == "ok"
    total = G.case(name)["cut"][2]
    assert f["first_feature"] + f["num_features"] == total and f["found"] == f["num_features"]
    # the ranges are suffixes of their octaves and sum to the kept keypoints (the driver checked each against the octave's count)
    assert sum(count for _, count in octaves) == f["kept_keypoints"] <= f["keypoints"]
    kept = [q for q, (_, count) in enumerate(octaves) if count]
    assert kept and all(first == 0 for first, _ in octaves[kept[0] + 1:])
    assert f["kept_keypoints"] > max_num_features or f["first_level"] == 0      # the level that crosses the bound is kept whole
    if max_num_features == 8192:
        assert f["first_level"] == 0 and f["num_features"] == total and all(first == 0 for first, _ in octaves)
    if max_num_features == 20:
        assert (f["first_feature"], f["num_features"]) == CUT_20[name]
    if name == "odd" and max_num_features in (36, 49):
        recorded = G.case({36: "odd_cut_between_levels", 49: "odd_cut_at_level_boundary"}[max_num_features])["cut"]
        assert [f["first_level"], f["first_feature"], f["num_features"]] == recorded


def test_the_cases_the_cuts_cover(cuts):
    """from the driver's output, not by assumption: a whole octave dropped in front of a proper suffix of the next; a suffix inside the first octave; a
    count that lands exactly on a level boundary; images without a cut and without a feature"""
    _, f, octaves = cuts[("odd", 20)]
    assert octaves[0] == (37, 0) and octaves[1][0] > 0 and octaves[1][1] > 0 and octaves[2][0] == octaves[3][0] == 0 and f["two_orientations"] > 0
    _, f, octaves = cuts[("blobs", 20)]
    assert octaves[0][1] == octaves[1][1] == 0 and octaves[2] == (0, 21)
    assert cuts[("blobs", 36)][2][1][0] > 0 and cuts[("blobs", 36)][2][1][1] > 0 and cuts[("blobs", 36)][1]["num_features"] == 63
    _, f, octaves = cuts[("odd", 49)]
    assert octaves[0][0] > 0 and octaves[0][1] > 0 and f["num_features"] == 75
    # 49 keypoints are exactly the levels from 3 on: the running count does not EXCEED the bound there, so level 2 comes in as well
    assert cuts[("odd", 36)][1]["kept_keypoints"] == 49 and f["first_level"] == 2 and f["kept_keypoints"] == 62
    assert cuts[("case", "tiny")][1]["num_features"] == 2 and cuts[("case", "constant")][1]["keypoints"] == 0
    assert cuts[("case", "constant")][1]["levels"] == 0 and cuts[("case", "constant")][0] == "same"


def _rows(driver, num_octaves, counts_by_image, row0):
    """counts_by_image[i][q] -> the store row of every feature in launch order, with its image"""
    n = len(counts_by_image)
    counts = [counts_by_image[i][q] for q in range(num_octaves) for i in range(n)]
    line, = run_driver(driver, ["rows %d %d %s %s" % (num_octaves, n, " ".join(map(str, row0)), " ".join(map(str, counts)))])
    block_row = [int(v) for v in line.split()]
    assert len(block_row) == num_octaves * n
    return [(block_row[q * n + i] + c, i) for q in range(num_octaves) for i in range(n) for c in range(counts_by_image[i][q])]


def test_the_destination_rows_are_a_permutation_in_the_reference_order(driver):
    counts = [[0, 5, 7, 1], [3, 0, 0, 2], [0, 0, 0, 0], [4, 4, 4, 4], [0, 0, 9, 0]]      # features per octave; an image without any
    per_image = [sum(c) for c in counts]
    offsets = [sum(per_image[:i]) for i in range(len(counts) + 1)]
    rows = _rows(driver, 4, counts, offsets[:-1])
    assert sorted(r for r, _ in rows) == list(range(offsets[-1]))      # every row of 0 .. offsets[N], once
    for i in range(len(counts)):
        mine = [r for r, image in rows if image == i]      # launch order = octave by octave = the reference's order inside an image
        assert mine == list(range(offsets[i], offsets[i + 1]))
    # a later group of a split batch: its images' rows start behind those of the groups before
    rows = _rows(driver, 2, [[2, 1], [0, 3]], [100, 103])
    assert sorted(r for r, _ in rows) == list(range(100, 106)) and [r for r, i in rows if i == 1] == [103, 104, 105]
    assert _rows(driver, 3, [[0, 0, 0]], [7]) == []
