"""Plain-Python restatement of the image-set search of IncrementalMapper::RegisterInitialLineImages (sfm/incremental_mapper.cc:199-423) - TEST
INFRASTRUCTURE, written from the semantics: dicts of sets do what the std::map of std::sets does there.

A scene (initial_sets_scenes.py) is a flat correspondence graph: `line_image` [L] (lines numbered image by image), `line_aligned` [L], `corr` [L] lists of
line numbers, `check_images`, `subset` (image indices or None = all).  Within one image set the order of the line numbers equals the reference's order on
its FeatureIdxs, because an image's lines are numbered in ascending line_idx.

PINNED where the reference is unspecified (std::sort is not stable): equal aligned counts are ordered by ascending image set."""
from itertools import combinations

ON_CHIP_LIST = 64      # the device keeps a filtered neighbour list of up to this many entries on chip (pp_init_sets_report.overflow_lines counts the longer ones)


def find_initial_sets(scene, min_num_aligned_tracks=20, min_num_random_tracks=20, max_num_sets=10):
    line_image, aligned, corr = scene["line_image"], scene["line_aligned"], scene["corr"]
    num_images = scene["num_images"]
    subset = set(range(num_images)) if scene.get("subset") is None else set(scene["subset"])
    check = set(scene["check_images"])
    assert check <= subset and len(check) == len(scene["check_images"])
    tracks = {True: {}, False: {}}      # class -> {image set: {track}}
    num_candidates = work_lines = overflow_lines = 0
    for r in range(len(line_image)):
        if line_image[r] not in check:
            continue
        nbrs = [n for n in corr[r] if bool(aligned[n]) == bool(aligned[r]) and line_image[n] in subset]
        if len(nbrs) < 3:
            continue
        work_lines += 1
        overflow_lines += len(nbrs) > ON_CHIP_LIST
        for i, j, k in combinations(range(len(nbrs)), 3):
            members = {}
            for l in (r, nbrs[i], nbrs[j], nbrs[k]):
                members.setdefault(line_image[l], l)
            if len(members) != 4:
                continue
            num_candidates += 1
            images = tuple(sorted(members))
            tracks[bool(aligned[r])].setdefault(images, set()).add(tuple(members[c] for c in images))
    al, rnd = tracks[True], tracks[False]
    qualified = [images for images in sorted(al) if len(al[images]) >= min_num_aligned_tracks and images in rnd and len(rnd[images]) >= min_num_random_tracks]
    ranked = sorted(qualified, key=lambda images: (-len(al[images]), images))
    sets = [dict(images=list(images), num_aligned=len(al[images]), num_random=len(rnd[images]), aligned=sorted(al[images]), random=sorted(rnd[images]))
            for images in ranked[:max_num_sets]]
    return dict(sets=sets, num_candidates=num_candidates, num_aligned_tracks=sum(len(t) for t in al.values()), num_random_tracks=sum(len(t) for t in rnd.values()),
                num_aligned_sets=len(al), num_random_sets=len(rnd), num_qualified=len(qualified), work_lines=work_lines, overflow_lines=overflow_lines,
                counts={images: (len(al.get(images, ())), len(rnd.get(images, ()))) for images in set(al) | set(rnd)})
