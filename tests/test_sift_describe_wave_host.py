"""The wavefront descriptor of K23 without a device and under the sanitizers: tests/sift_describe_wave_host_driver.cpp compiles with
g++ -fsanitize=address,undefined -ffp-contract=off and runs as its own program.  k_sift_describe_wave is DescriptorSample + DescriptorFold + the norms by
parts (csrc/sift_core.hpp) around LDS; ExtractOnHost's wave route runs the same functions with 64 "lanes" in a loop and an array in place of LDS.  Held
with NO tolerance to Descriptor() + FinishDescriptor(), the route tests/test_sift_extract_host.py holds to the recording of the reference: the bits of
every raw descriptor, every byte, every window flag, for every golden case; constructed pixels at the edges of the bin ranges through DescriptorFold
against the inner loop of Descriptor(); and the sub-batch planner."""
import os
import subprocess

import numpy as np
import pytest

import sift_extract_goldens as G

ROOT = G.ROOT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sift_wave") / "sift_describe_wave_host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "sift_describe_wave_host_driver.cpp")])
    return exe


def _run(exe, script):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    return out.stdout.splitlines()


def _fields(line):
    words = line.split()
    return words[0], {k: int(v) for k, v in zip(words[1::2], words[2::2])}


# No golden case has a descriptor window under 64 pixels (the smallest, in `tiny`, has 216: counted by the driver).  This one does: a 20 x 14 window of
# the `blobs` image from its first octave 0, whose second octave is 10 x 7 - windows of 40 pixels, and two keypoints with two orientations there.
SMALL = dict(name="blobs_window_20x14", x0=92, y0=0, width=20, height=14, options=dict(G.case("blobs")["options"], first_octave=0, num_octaves=2))


def small_image():
    return np.ascontiguousarray(G.image(G.case("blobs"))[SMALL["y0"]:SMALL["y0"] + SMALL["height"], SMALL["x0"]:SMALL["x0"] + SMALL["width"]])


@pytest.fixture(scope="module")
def compared(driver, tmp_path_factory):
    """both routes on every case and on the small window, in one run of the driver"""
    small = str(tmp_path_factory.mktemp("sift_wave_images") / "small.u8")
    small_image().tofile(small)
    script = ["wave %s %d %d %s" % (os.path.join(G.GOLDEN, c["image"]), c["width"], c["height"], G.option_words(c["options"])) for c in G.CASES]
    script.append("wave %s %d %d %s" % (small, SMALL["width"], SMALL["height"], G.option_words(SMALL["options"])))
    lines = _run(driver, script)
    names = G.CASE_NAMES + [SMALL["name"]]
    assert len(lines) == len(names)
    for name, line in zip(names, lines):
        print(name, line)
    return {name: _fields(line) for name, line in zip(names, lines)}


@pytest.mark.parametrize("name", G.CASE_NAMES)
def test_the_wave_route_equals_the_lane_route(compared, name):
    verdict, f = compared[name]
    assert verdict == "same" and (f["raw"], f["bytes"], f["windows"]) == (0, 0, 0), compared[name]
    assert f["features"] == len(G.recording(G.case(name))["keypoints"])      # every feature before the cut was compared


def test_the_compared_set_holds_the_cases_that_matter(compared):
    """from the driver's counts, not by assumption: a ragged last chunk, a window smaller than one chunk, windows the border cuts, keypoints with two
    features (two windows over the same pixels with different rotations)"""
    _, blobs = compared["blobs"]
    _, tiny = compared["tiny"]
    assert blobs["not_multiple_of_64"] > 0 and blobs["cut"] == 116 and blobs["two_orientations"] == 24 and blobs["max_pixels"] > 64
    assert tiny["features"] == 2 and tiny["cut"] == 2 and tiny["max_pixels"] == 216      # the smallest windows of the golden cases
    assert compared["constant"][1]["features"] == 0
    verdict, small = compared[SMALL["name"]]
    assert verdict == "same" and (small["raw"], small["bytes"], small["windows"]) == (0, 0, 0)
    assert small["features"] == 4 and small["below_64"] == 2 and small["min_pixels"] == 40 and small["two_orientations"] == 2


FOLD = {      # binx biny bint rbinx rbiny rbint win mod -> bins that receive an addition
    "the orientation wraps from 7 to 0": ("0 -1 7 0.25 0.5 0.75 0.5 0.25", 8),
    "bint == 8 (theta of exactly 2 pi)": ("-1 0 8 0.125 0.375 0.0 0.75 1.5", 8),
    "binx == -3: only dbinx 1 is in range": ("-3 0 2 0.9 0.1 0.3 0.5 0.5", 4),
    "binx == 1: only dbinx 0 is in range": ("1 -2 3 0.2 0.6 0.4 0.5 0.5", 4),
    "biny == -3: only dbiny 1 is in range": ("-1 -3 5 0.3 0.8 0.6 0.25 2.0", 4),
    "biny == 1: only dbiny 0 is in range": ("-2 1 6 0.7 0.2 0.1 0.25 2.0", 4),
    "both at the corner": ("1 1 7 0.4 0.4 0.9 1.0 1.0", 2),
    "wholly out of range in x": ("2 0 1 0.5 0.5 0.5 1.0 1.0", 0),
    "wholly out of range in y": ("0 -4 1 0.5 0.5 0.5 1.0 1.0", 0),
    "a zero modulus still adds": ("0 0 0 0.5 0.5 0.5 1.0 0.0", 8),
}


@pytest.mark.parametrize("what", sorted(FOLD))
def test_a_constructed_pixel_through_the_fold(driver, what):
    words, touched = FOLD[what]
    assert _run(driver, ["fold " + words]) == ["same touched %d" % touched]


def test_an_empty_window_and_a_keypoint_outside(driver):
    """width height x y sigma level: a window the two-row level leaves empty (y1 < y0) is normalised from zeros; a keypoint that fails the bounds check -
    outside the level, or at a level without a gradient - gives 128 zeros and computed == 0; an ordinary and a cut window for comparison"""
    lines = _run(driver, ["frame 8 2 3.0 0.2 1.6 0", "frame 40 30 100.0 5.0 1.6 0", "frame 40 30 20.0 15.0 1.6 3", "frame 40 30 20.0 29.0 1.6 0",
                          "frame 40 30 20.0 15.0 1.6 0", "frame 40 30 2.0 3.0 1.6 1", "frame 9 8 4.0 4.0 1.6 0", "frame 10 10 5.0 5.0 1.6 0"])
    assert lines[0] == "same computed 1 pixels 0 nonzero 0"
    assert lines[1] == lines[2] == lines[3] == "same computed 0 pixels 0 nonzero 0"
    for line in lines[4:6]:
        verdict, f = _fields(line)
        assert verdict == "same" and f["computed"] == 1 and f["pixels"] > 64 and f["nonzero"] > 0, line
    assert _fields(lines[6])[0] == "same" and _fields(lines[6])[1]["pixels"] == 42      # less than one chunk
    assert _fields(lines[7])[0] == "same" and _fields(lines[7])[1]["pixels"] == 64      # exactly one


def test_the_sub_batch_planner(driver):
    plans = _run(driver, ["plan 1 10 20 30", "plan 1000 10 20 30", "plan 50 10 20 500 5 5", "plan 30 10 20 10 20 30 1", "plan 8 9", "plan 100"])
    assert plans[0] == "0 1 2 3"            # a target of one byte: every image alone
    assert plans[1] == "0 3"                # one sub-batch
    assert plans[2] == "0 2 3 5"            # the oversized image in the middle runs alone, its neighbours keep their order
    assert plans[3] == "0 2 4 5 6"          # greedy: a sum equal to the target still fits
    assert plans[4] == "0 1" and plans[5] == "0"
    for plan, n in zip(plans, (3, 3, 5, 6, 1, 0)):
        first = [int(v) for v in plan.split()]
        assert first[0] == 0 and first[-1] == n and all(a < b for a, b in zip(first, first[1:]))      # nothing dropped, nothing twice, in order
