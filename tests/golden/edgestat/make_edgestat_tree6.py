"""Writes edgestat_tree6.json beside this file: known answers of the edge statistics (include/rappas_place.h, the edge dispersion and
correlation block) on the tree of six nodes of the diversity fixture, five samples of which one is empty, two metadata columns.

    node    0     1     2     3     4     5          leaves 3 and 4 are a cherry under node 1, leaf 5 hangs under node 2
    parent -1     0     0     1     1     2

The integer words are worked out by hand below: the mid-ranks of every row are written down as they are read off the values (and
checked against a count over exact rationals, so that a slip of the pen fails here and not in a test).  The finished values come
from exact rational arithmetic (fractions) and one square root at the end; the library's differ from them by the rounding of its
sums, at most 5 * 2^-53 relative on these values, which lie well apart: the tests compare at 1e-12.  No library call.

Run: python tests/golden/edgestat/make_edgestat_tree6.py"""
import json
import math
import os
from fractions import Fraction as Fr

PARENT = [-1, 0, 0, 1, 1, 2]
#            node 0    1    2    3    4    5
MASS = [[0, 100, 200, 300, 400, 0],      # s0
        [0, 0, 500, 100, 150, 250],      # s1
        [100, 200, 50, 0, 600, 50],      # s2
        [0, 0, 0, 0, 0, 0],              # s3: no mass, takes no part
        [0, 50, 50, 200, 100, 600]]      # s4
NAMES = ["pH", "depth"]
# (the values of the empty sample are never used: a NaN there leaves the column usable)
META = [[5.5, 7.0, 6.25, 99.0, 8.0],
        [-10.0, 20.0, -10.0, float("nan"), 40.0]]
ACTIVE = [0, 1, 2, 4]
N = len(ACTIVE)
B, S, F = 6, 5, 2

clade = [[m[0] + sum(m[1:]), m[1] + m[3] + m[4], m[2] + m[5], m[3], m[4], m[5]] for m in MASS]
T = [c[0] for c in clade]
assert [T[s] for s in ACTIVE] == [1000] * 4 and T[3] == 0

# the profiles of the active samples, exact: P0 = m / T, P1 = (c + (c - m)) / T - 1; the root's row is zeros
P = [[[Fr(0)] * N if x == 0 else [Fr(MASS[s][x], T[s]) for s in ACTIVE] for x in range(B)],
     [[Fr(0)] * N if x == 0 else [Fr(2 * clade[s][x] - MASS[s][x], T[s]) - 1 for s in ACTIVE] for x in range(B)]]

# Twice the mid-ranks, by hand, over the active samples s0 s1 s2 s4.
#   P0 (mass share)   node 1: .1 0 .2 .05      node 2: .2 .5 .05 .05 (s2 and s4 tie for ranks 1 and 2: 1.5 each)
#                     node 3: .3 .1 0 .2       node 4: .4 .15 .6 .1         node 5: 0 .25 .05 .6
#   P1 (imbalance)    node 1: .5 -.5 .4 -.35   node 2: -.8 0 -.85 .25       a leaf's is its share minus one: the ranks of P0
#   the root: four zeros, all tied at mid-rank 2.5
RANK2 = [[[5, 5, 5, 5], [6, 2, 8, 4], [6, 8, 3, 3], [8, 4, 2, 6], [6, 4, 8, 2], [2, 6, 4, 8]],
         [[5, 5, 5, 5], [8, 2, 6, 4], [4, 6, 2, 8], [8, 4, 2, 6], [6, 4, 8, 2], [2, 6, 4, 8]]]
#   pH: 5.5 7 6.25 8                depth: -10 20 -10 40 (s0 and s2 tie)
GRANK2 = [[2, 6, 4, 8], [3, 6, 3, 8]]


def count_rank2(v):
    return [2 * sum(1 for b in v if b < a) + sum(1 for b in v if b == a) + 1 for a in v]


G = [[Fr(META[f][s]) for s in ACTIVE] for f in range(F)]
for q in range(2):
    for x in range(B):
        assert RANK2[q][x] == count_rank2(P[q][x]), (q, x)
for f in range(F):
    assert GRANK2[f] == count_rank2(G[f]), f

dev = lambda r2: [r - (N + 1) for r in r2]
gd = [dev(r) for r in GRANK2]
grss = [sum(d * d for d in g) for g in gd]
rss = [[sum(d * d for d in dev(RANK2[q][x])) for x in range(B)] for q in range(2)]
rcross = [[[sum(a * b for a, b in zip(dev(RANK2[q][x]), gd[f])) for f in range(F)] for x in range(B)] for q in range(2)]
assert grss == [20, 18] and rss[0] == [0, 20, 18, 20, 20, 20]
assert rcross[0][5] == [20, 18] and rcross[1][5][0] == rss[1][5] == grss[0]   # node 5 rises with the pH: Spearman is exactly 1


def moments(v):
    mean = sum(v) / N
    return mean, sum((a - mean) ** 2 for a in v)


def ratio(num, den2):
    """num / sqrt(den2) for exact num and den2; None (0 / 0, NaN) for a constant row"""
    return None if den2 == 0 else float(num) / math.sqrt(den2)


gmom = [moments(g) for g in G]
table = []
for x in range(B):
    row = []
    for q in range(2):
        mean, ss = moments(P[q][x])
        var = ss / N
        row += [float(mean), float(var), math.sqrt(var)]
        if q == 0:
            row += [None if mean == 0 else math.sqrt(var) / float(mean), None if mean == 0 else float(var / mean)]
    for f in range(F):
        for q in range(2):
            mean, ss = moments(P[q][x])
            cross = sum((a - mean) * (g - gmom[f][0]) for a, g in zip(P[q][x], G[f]))
            row += [ratio(cross, ss * gmom[f][1]), ratio(Fr(rcross[q][x][f]), Fr(rss[q][x] * grss[f]))]
    table.append(row)
assert table[5][8 + 1] == 1.0 and table[5][8 + 3] == 1.0   # mass_spearman_pH and imb_spearman_pH of node 5

columns = ["mass_mean", "mass_var", "mass_sd", "mass_cv", "mass_vmr", "imb_mean", "imb_var", "imb_sd"]
for name in NAMES:
    columns += [c + "_" + name for c in ("mass_pearson", "mass_spearman", "imb_pearson", "imb_spearman")]

doc = {
    "about": "edge statistics known answers (include/rappas_place.h, the edge dispersion and correlation block): a tree of six nodes, five "
             "samples (s3 empty), two metadata columns; integer words exact, finished values from exact rationals (null = NaN), to be "
             "compared at relative 1e-12",
    "n_branches": B,
    "parent": PARENT,
    "mass": MASS,
    "feature_names": NAMES,
    "meta": [[None if v != v else v for v in row] for row in META],
    "n_active": N,
    "unusable": 0,
    "rss": rss,
    "rcross": rcross,
    "grss": grss,
    "columns": columns,
    "table": table,
    "feature_table": [[float(m), float(ss / N)] for m, ss in gmom],
}

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "edgestat_tree6.json"), "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
