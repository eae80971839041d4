"""Writes diversity_tree6.json beside this file: known answers of the per-sample diversity measures (include/rappas_place.h, the
diversity block) on a tree of six nodes whose lengths are dyadic, worked out by hand below -- no library call, no logarithm: every
D is 1 or 1/2, where rk_log2 and rk_exp2 are exact by definition, so every value is a dyadic number or a dyadic multiple of RK_LN2.

    node    0     1     2     3     4     5          leaves 3 and 4 are a cherry under node 1 (the stem), leaf 5 hangs under node 2
    parent -1     0     0     1     1     2
    length  -     1     2    0.5    4    0.25        h = length / 2: a branch's mass sits at the midpoint of its edge

Run: python tests/golden/diversity/make_diversity_tree6.py"""
import json
import os

LN2 = float.fromhex("0x1.62e42fefa39efp-1")  # RK_LN2
THETA = [0.0, 1.0, 2.0]
NAN = "nan:0x7ff8000000000000"

h = [0.0, 0.5, 1.0, 0.25, 2.0, 0.125]

# A: all mass on leaf 4.  Proximal half of 4 and both halves of the stem have a = T: rooted, not split, D = 1, lg D = +0.0,
# pw(1, theta) = rk_exp2(theta * 0) = 1.  rooted_pd = the path from the midpoint of edge 4 to the root.  The entropy terms are
# h * (-(1 * 0) * LN2) = -0.0, and +0.0 + -0.0 = +0.0.
path_a = h[4] + (h[1] + h[1])
A = [path_a, 0.0, 0.0, 0.0, 0.0] + [path_a, 0.0] * len(THETA)

# B: leaves 3 and 4 with 512 each, T = 1024.  Proximal halves of 3 and 4: D = E = 1/2, M = 1, split.  Stem: D = 1, rooted only.
path_b = h[3] + h[4]          # between the two midpoints: pd, and bwpd since M = 1
stem = h[1] + h[1]
B = [path_b + stem, path_b, path_b, h[3] * 0.25 + h[4] * 0.25,
     # lane 4 holds h[4] * (0.5 * LN2) = LN2, lane 3 holds h[3] * (0.5 * LN2) = LN2 / 8, the other lanes +0.0; the fold adds lane 4
     # into lane 0 at stride 4, lane 3 into lane 1 at stride 2, lane 1 into lane 0 at stride 1: one rounding, of 1.125 * LN2
     h[4] * (0.5 * LN2) + h[3] * (0.5 * LN2)]
for th in THETA:
    half_pow = {0.0: 1.0, 1.0: 0.5, 2.0: 0.25}[th]  # rk_exp2(-theta) at an integer: the scale alone, exact
    B += [h[4] * half_pow + (stem + h[3] * half_pow), path_b]  # (the fold: lane 4 + lane 0, then + (lane 1 + lane 3))

# C: mass on the root only: the root's h is 0, every other a is 0.
C = [0.0] * (5 + 2 * len(THETA))

doc = {
    "about": "diversity known answers, exact in binary64 (include/rappas_place.h, the diversity block): a tree of six nodes, four samples; "
             "values are C99 hex floats, the row of the sample without mass is the quiet NaN",
    "n_branches": 6,
    "parent": [-1, 0, 0, 1, 1, 2],
    "branch_len": [0, 1, 2, 0.5, 4, 0.25],
    "theta": THETA,
    "columns": ["rooted_pd", "pd", "bwpd", "quadratic", "phylo_entropy"] + [c + "_%g" % t for t in THETA for c in ("rooted_pd", "bwpd")],
    "samples": [
        {"name": "A one leaf", "mass": [0, 0, 0, 0, 1000, 0], "row": [v.hex() for v in A]},
        {"name": "B cherry", "mass": [0, 0, 0, 512, 512, 0], "row": [v.hex() for v in B]},
        {"name": "C root only", "mass": [77, 0, 0, 0, 0, 0], "row": [v.hex() for v in C]},
        {"name": "D empty", "mass": [0, 0, 0, 0, 0, 0], "row": [NAN] * len(C)},
    ],
}

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "diversity_tree6.json"), "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
