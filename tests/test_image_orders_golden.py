"""The image orders of pp_ba_plan_ordering, held to tests/golden/image_orders.json: for every case of tests/golden/gen_image_orders.py's corpus - the scenes of
tests/test_image_ordering.py, every ordering switch, constant poses, the co-visibility matrix, per-image and shared intrinsics, shuffled ids, rings, stars
and chains of clusters, both sides of the candidate threshold, more block columns than the one-launch factorisation holds, the dense early exit, the
iterative hand-off - the info[8] and the whole old_of_new (length + FNV-1a digest) the library computed before the ordering moved from
csrc/image_ordering.hip into the stages of csrc/image_ordering.hpp.  Host only."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_image_orders", os.path.join(ROOT, "tests", "golden", "gen_image_orders.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def planned():
    seconds = {}
    return gen.run(seconds=seconds), seconds


def test_every_order_is_what_it_was_before_the_split(planned):
    got, seconds = planned
    with open(gen.GOLDEN) as f:
        golden = json.load(f)
    assert sorted(got) == sorted(golden) == sorted(name for name, _, _, _ in gen.corpus())
    for name, want in golden.items():
        assert got[name] == want, name
    assert max(seconds.values()) < 1.0, max(seconds.items(), key=lambda kv: kv[1])      # (the slowest plans in ~0.01 s; the first call also loads the library)


def test_the_corpus_reaches_every_path(planned):
    info = {name: dict(zip(gen.INFO_KEYS, case["info"])) for name, case in planned[0].items()}
    digest = {name: case["old_of_new"][1] for name, case in planned[0].items()}
    for name in ("seq300", "seq500_shuffled", "ring500", "seq1000_shuffled", "star5", "chain4", "star8", "seq300_constant", "seq300_matrix", "seq500_private8"):
        assert info[name]["reordered"] and info[name]["chains"] >= 2 and info[name]["block_sparse"], name
    # the switches: natural keeps the caller's order without looking (nnz_natural -1), rcm and band are one chain, the graph's separators win where asked for
    assert (info["seq300/ordering=natural"]["reordered"], info["seq300/ordering=natural"]["nnz_natural"], info["seq300/ordering=1"]["nnz_natural"]) == (0, -1, -1)
    assert info["seq300/ordering=rcm"]["reordered"] and info["star5/ordering=band"]["reordered"] and info["star5/ordering=band"]["chains"] == 1
    assert info["dense120/ordering=rcm"]["reordered"] and not info["dense120"]["reordered"] and info["dense120"]["nnz_natural"] == -1      # forced / the dense early exit
    assert digest["seq500_private8/graph_nd=1"] != digest["seq500_private8/graph_nd=0"] == digest["seq500_private8"]
    # 8 columns per image against the tail; an odd count falls back to the tail
    assert info["seq500_private8"]["block_columns"] == (8 * 500 + 1 + 63) // 64 and info["seq500_private8"]["chain_steps"] < info["seq500_private8/intr_layout=tail"]["chain_steps"]
    assert planned[0]["seq500_private_odd"] == planned[0]["seq500_private_odd/intr_layout=tail"] and info["seq500_private_odd"]["intrinsics_columns"] == 500
    assert info["seq300_shared_intrinsics"]["intrinsics_columns"] == 2 and digest["seq300_shared_intrinsics"] == digest["seq300"]
    # constant poses change the graph; the matrix of a scene gives its order; unsorted observations and a point seen twice by an image change nothing
    assert digest["seq300_constant"] != digest["seq300"] and digest["seq300_constant_matrix"] == digest["seq300_constant"] and digest["seq300_matrix"] == digest["seq300_shuffled"]
    assert digest["seq300_unsorted"] == digest["seq300_twice"] == digest["seq300"]
    # 7 block columns: no candidate; 8: looked at (nnz_natural is known); 132: a band at most, one chain of all block columns; above 1000 images: not looked at
    assert (info["seq70"]["block_columns"], info["seq70"]["nnz_natural"], info["seq75"]["block_columns"]) == (7, -1, 8) and info["seq75"]["nnz_natural"] > 0
    big = info["seq1400/linear_solver=1"]
    assert (big["block_columns"], big["chains"], big["chain_steps"]) == (132, 1, 132) and big["nnz_natural"] > 0
    assert info["seq1100"]["nnz_natural"] == -1 and not info["seq1100"]["reordered"] and info["seq1100/linear_solver=1"]["chains"] >= 8
