"""Records what the reference's non_max_suppression_fast returns (utils/bounding_box/bbox.py) into tests/golden/bbox_nms.npz.

    python tests/golden/make_bbox_nms.py PATH/TO/utils/bounding_box/bbox.py

Run once where the reference is at hand; the tests only read the .npz.  The module itself imports SimpleITK and matplotlib and cannot
be imported: the file is parsed with `ast`, that one FunctionDef is compiled with `np` in scope, nothing else of it runs.
Cases: hand-made sets (nested, disjoint, chained overlaps) and at least 200 random sets of 1 .. 39 boxes, x, y in 0 .. 39 and w, h in
1 .. 19.  NO set has two boxes with the same y + h: the reference sorts them with NumPy's default unstable sort, so its answer on such
a set depends on the NumPy build; only about a fifth of the random draws qualify, so the generator draws until enough do.
Arrays: boxes_<k> int64 [m, 4] (x, y, w, h), picks_<k> int64 [p, 4], thresh float64 (one for all), count."""
import ast
import os
import sys

import numpy as np

THRESH = 0.5
RANDOM_SETS = 240

HAND = [
    [[2, 2, 10, 10], [4, 4, 3, 3]],                                            # nested: the small one lies inside the large one
    [[4, 4, 3, 3], [2, 2, 10, 10], [5, 5, 1, 1]],                              # nested twice, another order
    [[0, 0, 4, 4], [10, 1, 4, 4], [20, 2, 4, 4], [0, 20, 3, 3]],               # disjoint
    [[0, 0, 10, 10], [4, 1, 10, 10], [8, 2, 10, 10], [12, 3, 10, 10]],         # a chain: each overlaps the next by more than half
    [[0, 0, 10, 10], [6, 1, 10, 10], [12, 2, 10, 10]],                         # a chain with overlaps below the threshold
    [[3, 3, 1, 1]],                                                            # one box
    [[0, 0, 10, 4], [0, 1, 10, 4], [0, 2, 10, 4], [0, 3, 10, 4], [0, 4, 10, 4]],   # a ladder
]


def load_reference(path):
    tree = ast.parse(open(path).read(), filename=path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "non_max_suppression_fast"]
    assert len(fn) == 1, "non_max_suppression_fast not found in %s" % path
    scope = {"np": np}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), scope)
    return scope["non_max_suppression_fast"]


def untied(boxes):
    bottom = boxes[:, 1] + boxes[:, 3]
    return len(set(bottom.tolist())) == len(bottom)


def main(argv):
    nms = load_reference(argv[1])
    rng = np.random.default_rng(20240607)
    sets = [np.asarray(h, dtype=np.int64) for h in HAND]
    draws = 0
    while len(sets) < len(HAND) + RANDOM_SETS:
        draws += 1
        m = int(rng.integers(1, 40))
        b = np.concatenate([rng.integers(0, 40, (m, 2)), rng.integers(1, 20, (m, 2))], axis=1).astype(np.int64)
        if untied(b):
            sets.append(b)
    out = {"thresh": np.float64(THRESH), "count": np.int64(len(sets))}
    for k, b in enumerate(sets):
        assert untied(b), k
        picks = np.asarray(nms(b.copy(), THRESH), dtype=np.int64).reshape(-1, 4)
        out["boxes_%d" % k], out["picks_%d" % k] = b, picks
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bbox_nms.npz")
    np.savez_compressed(path, **out)
    print("%d sets (%d random draws for %d kept) -> %s" % (len(sets), draws, RANDOM_SETS, path))


if __name__ == "__main__":
    main(sys.argv)
