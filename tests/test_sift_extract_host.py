"""csrc/sift_core.hpp and csrc/sift_extract_replay.hpp - the arithmetic and the host rule of SIFT extraction (K21) - without a device and under the
sanitizers: tests/sift_extract_host_driver.cpp compiles with g++ -fsanitize=address,undefined -ffp-contract=off, runs as its own program and extracts
every golden image and option variant serially through the functions the kernels call.  Against the recording of the reference's CPU extractor
(tests/golden/sift) with NO tolerance: the digest of every Gaussian, DoG and gradient level, the candidates in order, the keypoints, angles and raw
descriptors by their bits, the range max_num_features keeps; the uint8 descriptors against the project's rule restated in
sift_extract_goldens.finish_descriptors.  A sanitizer report ends the driver with a non-zero status."""
import os
import subprocess

import numpy as np
import pytest

import sift_extract_goldens as G

ROOT = G.ROOT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sift_extract") / "sift_extract_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "sift_extract_host_driver.cpp")])
    return exe


def _run(exe, script):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    return out.stdout.splitlines()


@pytest.fixture(scope="module")
def dumps(driver, tmp_path_factory):
    """every case extracted once, in one run of the driver"""
    d = tmp_path_factory.mktemp("sift_dumps")
    script = ["extract %s %d %d %s 1 %s" % (os.path.join(G.GOLDEN, c["image"]), c["width"], c["height"], d / (c["name"] + ".dump"), G.option_words(c["options"]))
              for c in G.CASES]
    assert _run(driver, script) == ["ok"] * len(G.CASES)
    return {c["name"]: G.parse_dump(str(d / (c["name"] + ".dump"))) for c in G.CASES}


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_scale_space_levels_and_candidates(dumps, name):
    c, d = G.case(name), dumps[name]
    rec = G.recording(c)
    assert len(rec["stage_names"]) > 0
    for key, kind, o, s in G.stage_names(rec):
        w, h = np.frombuffer(d["dims %d" % o], np.int32)
        level = np.frombuffer(d[key], np.float32).reshape((h, w, 2) if kind == "grad" else (h, w))
        G.check_stage(rec, key, level, sampled=name in ("blobs", "odd", "tiny"))
    octaves = np.frombuffer(d["octaves"], np.int32).reshape(-1, 9)
    assert len(octaves) == len(rec["octave_counts"]) == c["options"]["num_octaves"]
    for (o, w, h, ncand, nkeys), got in zip(rec["octave_counts"], octaves):
        assert (got[0], got[1], got[2], got[3]) == (w, h, ncand, nkeys)
        G.assert_same_bits(np.frombuffer(d["cand %d" % o], np.int32).reshape(-1, 3), rec["cand_%d" % o], "candidates of octave %d" % o)


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_features_and_the_kept_range(dumps, name):
    c, d = G.case(name), dumps[name]
    cut = np.frombuffer(d["cut"], np.int64)
    assert list(cut[:3]) == c["cut"]
    start, count = int(cut[1]), int(cut[2])
    keypoints = np.frombuffer(d["keypoints"], np.float32).reshape(-1, 4)[start:start + count]
    descriptors = np.frombuffer(d["descriptors"], np.uint8).reshape(-1, 128)[start:start + count]
    G.check_result(c, keypoints, descriptors, np.frombuffer(d["raw"], np.float32), np.frombuffer(d["octave_level"], np.int32), np.frombuffer(d["angles"], np.float64),
                   int(cut[0]))
    G.assert_same_bits(np.frombuffer(d["levels"], np.int64).reshape(-1, 4), G.recording(c)["levels"], "level containers")


def test_the_cases_the_images_were_made_for(dumps):
    """from the reports, not by assumption: the 160 x 120 image has two-orientation keypoints, refinement moves, edge and peak rejections and windows the
    border cuts; the variants cut where their names say; the tiny image's filters are wider than its last octaves"""
    d = dumps["blobs"]
    octaves = np.frombuffer(d["octaves"], np.int32).reshape(-1, 9)
    cut = np.frombuffer(d["cut"], np.int64)
    assert len(np.frombuffer(d["angles"], np.float64)) >= 100
    assert cut[3] > 0 and cut[4] > 0                                        # two orientations, windows cut by the border
    assert octaves[:, 4].sum() > 0 and octaves[:, 5].sum() > 0 and octaves[:, 6].sum() > 0      # moved, rejected by peak value, by edge score
    assert len(np.frombuffer(dumps["constant"]["angles"], np.float64)) == 0
    levels = G.recording(G.case("odd"))["levels"]
    from_coarsest = np.cumsum(levels[::-1, 2])
    assert 49 in from_coarsest and 36 not in from_coarsest                  # 49 ends a level exactly, 36 falls inside one
    assert G.case("odd_cut_at_level_boundary")["cut"][0] == len(levels) - 1 - list(from_coarsest).index(49) - 1
    assert 0 < G.case("odd_cut_between_levels")["cut"][0] and G.case("odd_cut_between_levels")["cut"][2] < len(G.recording(G.case("odd"))["keypoints"])
    tiny = np.frombuffer(dumps["tiny"]["octaves"], np.int32).reshape(-1, 9)
    assert tuple(tiny[-1, :2]) == (5, 3)                                    # the widest filter has 27 taps
    assert np.all(G.recording(G.case("odd_upright"))["angles"] == 0.0)
    one = G.recording(G.case("odd_one_orientation"))["levels"]
    assert np.array_equal(one[:, 2] >= one[:, 3], np.ones(len(one), bool)) and np.any(levels[:, 3] > levels[:, 2])


DEFAULT = dict(max_num_features=8192, first_octave=-1, num_octaves=4, octave_resolution=3, peak_threshold=0.02 / 3, edge_threshold=10.0,
               max_num_orientations=2, upright=0, normalization=0)


def _check(driver, w, h, **kw):
    return _run(driver, ["check %d %d %s" % (w, h, G.option_words(dict(DEFAULT, **kw)))])[0]


def test_option_check(driver):
    assert _check(driver, 160, 120) == "ok" and _check(driver, 1, 1, first_octave=0, num_octaves=1) == "ok"
    assert _check(driver, 3200, 2400) == "ok" and _check(driver, 160, 120, max_num_orientations=4, normalization=1, octave_resolution=1) == "ok"
    for why, (w, h, kw) in (("size", (0, 10, {})), ("size", (10, -1, {})),
                            ("max_num_features", (64, 64, dict(max_num_features=0))), ("octave_resolution", (64, 64, dict(octave_resolution=0))),
                            ("peak_threshold", (64, 64, dict(peak_threshold=0.0))), ("peak_threshold", (64, 64, dict(peak_threshold=float("nan")))),
                            ("edge_threshold", (64, 64, dict(edge_threshold=-1.0))), ("edge_threshold", (64, 64, dict(edge_threshold=float("nan")))),
                            ("max_num_orientations must", (64, 64, dict(max_num_orientations=0))),
                            ("max_num_orientations above 4", (64, 64, dict(max_num_orientations=5))),
                            ("unknown normalization", (64, 64, dict(normalization=2))), ("unknown normalization", (64, 64, dict(normalization=-1))),
                            ("num_octaves", (64, 64, dict(num_octaves=0))), ("num_octaves", (64, 64, dict(num_octaves=-1))),
                            ("first_octave", (64, 64, dict(first_octave=-9))),
                            ("last octave", (20, 14, dict(first_octave=0, num_octaves=5))), ("last octave", (64, 64, dict(first_octave=7, num_octaves=1))),
                            ("int32", (20000, 14000, {})), ("int32", (2 ** 20, 4, {})), ("int32", (40000, 30000, dict(first_octave=0)))):
        line = _check(driver, w, h, **kw)
        assert line.startswith("refused") and why in line, (why, line)
    assert _check(driver, 20, 14, first_octave=0, num_octaves=4) == "ok"
