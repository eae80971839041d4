"""The EDPL of include/rappas_place.h restated in plain Python (a Python float is a binary64, and *, + and - on it round once: no
contraction) and in exact rationals.  The lowest common ancestor is found by walking parents, deliberately not the engine's sparse
table; the pair sum runs in a Python loop in the order the header fixes.  Also the result sets the EDPL tests share."""
from fractions import Fraction

import numpy as np

from tests import kr_ref as R


class Tree:
    """D, h, pos and depth of every node of (parent, branch_len), as the header defines them"""

    def __init__(self, parent, bl):
        self.parent = [int(p) for p in parent]
        self.B = len(self.parent)
        self.root, order = R.preorder(self.parent)
        bl = np.asarray(bl, np.float32)
        self.len = [float(np.float64(bl[x])) for x in range(self.B)]  # (double)branch_len[x]
        self.D = [0.0] * self.B
        self.h = [0.0] * self.B
        self.pos = [0.0] * self.B
        self.depth = [0] * self.B
        for x in order[1:]:  # a parent comes before its children
            p = self.parent[x]
            self.D[x] = self.D[p] + self.len[x]
            self.h[x] = self.len[x] * 0.5
            self.pos[x] = self.D[x] - self.h[x]
            self.depth[x] = self.depth[p] + 1

    def lca(self, a, b):
        while self.depth[a] > self.depth[b]:
            a = self.parent[a]
        while self.depth[b] > self.depth[a]:
            b = self.parent[b]
        while a != b:
            a, b = self.parent[a], self.parent[b]
        return a

    def distance(self, a, b):
        if a == b:
            return 0.0
        l = self.lca(a, b)
        if l == a:
            return self.pos[b] - self.pos[a]
        if l == b:
            return self.pos[a] - self.pos[b]
        return (self.pos[a] - self.D[l]) + (self.pos[b] - self.D[l])

    # the same in exact rationals: no rounding anywhere
    def exact(self):
        D = [Fraction(0)] * self.B
        pos = [Fraction(0)] * self.B
        _, order = R.preorder(self.parent)
        for x in order[1:]:
            D[x] = D[self.parent[x]] + Fraction(self.len[x])
            pos[x] = D[x] - Fraction(self.len[x]) / 2
        return D, pos

    def distance_exact(self, a, b, D, pos):
        if a == b:
            return Fraction(0)
        l = self.lca(a, b)
        if l == a:
            return pos[b] - pos[a]
        if l == b:
            return pos[a] - pos[b]
        return (pos[a] - D[l]) + (pos[b] - D[l])


def shuffled(tree, seed):
    """the same tree with its ids relabelled at random: in no pre-order, the root anywhere"""
    parent, bl = tree
    B = len(parent)
    perm = np.random.default_rng(seed).permutation(B)  # old id -> new id
    new_parent = np.full(B, -1, np.int32)
    new_parent[perm] = np.where(parent >= 0, perm[np.maximum(parent, 0)], -1)
    new_bl = np.zeros(B, np.float32)
    new_bl[perm] = bl
    return new_parent, new_bl


def trees(sizes):
    for B in sizes:
        yield f"star-{B}", shuffled(R.star(B, B), B)
        yield f"caterpillar-{B}", shuffled(R.caterpillar(B, B), B + 1)
        yield f"random-{B}", R.random_tree(B, 60 + B)


def golden():
    """tests/golden/edpl/edpl_tree6.json (a directory of its own: every *.json directly under tests/golden is a placement vector of
    tests/golden_util.py), with its reads as the arrays the calls take"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edpl", "edpl_tree6.json")) as f:
        g = json.load(f)
    reads = g["reads"]
    g["n_rows"] = np.array([r["n_rows"] for r in reads], np.uint8)
    g["branch"] = np.array([r["branch"] for r in reads], np.uint16)
    g["lwr"] = np.array([r["lwr"] for r in reads], np.float64)
    g["edpl"] = np.array([r["edpl"] for r in reads], np.float64)
    g["parent"] = np.array(g["parent"], np.int32)
    g["branch_len"] = np.array(g["branch_len"], np.float32)
    return g


def edpl_ref(parent, bl, K, n_rows, branch, lwr):
    """float64 [n]: the definition, read after read and pair after pair"""
    t = Tree(parent, bl)
    n = len(n_rows)
    branch = np.asarray(branch).reshape(n, K)
    lwr = np.asarray(lwr, np.float64).reshape(n, K)
    out = np.zeros(n, np.float64)
    for r in range(n):
        rows = [(int(branch[r, e]), float(lwr[r, e])) for e in range(min(int(n_rows[r]), K))]
        rows = [(b, w) for b, w in rows if b < t.B and w > 0.0]  # (NaN > 0.0 is False)
        acc = 0.0
        for i in range(len(rows)):
            for j in range(i + 1, len(rows)):
                acc = acc + ((rows[i][1] * rows[j][1]) * t.distance(rows[i][0], rows[j][0]))
        out[r] = 2.0 * acc
    return out


def result_set(B, K, n, seed, plant=True):
    """(n_rows u8 [n], branch u16 [n, K], lwr f64 [n, K]): rows with distinct branches, n_rows from 0 to K, weights from a Dirichlet
    draw; plant: in about a tenth of the reads one row becomes a branch >= B, a weight 0, a negative weight or a NaN.  The rows behind
    n_rows are the engine's fillers (branch 0xFFFF, lwr 0)."""
    rng = np.random.default_rng(seed)
    n_rows = np.minimum(rng.integers(0, K + 1, n), B).astype(np.uint8)  # (distinct branches: no more rows than the tree has nodes)
    live = np.arange(K)[None, :] < n_rows[:, None]
    draw = rng.integers(0, B, (n, K))
    srt = np.sort(np.where(live, draw, -1 - np.arange(K)[None, :]), axis=1)
    for r in np.nonzero((srt[:, 1:] == srt[:, :-1]).any(axis=1))[0]:  # the reads that drew a branch twice: drawn again, without replacement
        draw[r, :n_rows[r]] = rng.choice(B, n_rows[r], replace=False)
    branch = np.where(live, draw, 0xFFFF).astype(np.uint16)
    g = np.where(live, rng.gamma(0.7, size=(n, K)) + 1e-12, 0.0)
    lwr = g / np.maximum(g.sum(axis=1, keepdims=True), 1e-300)  # a Dirichlet draw over the live rows
    if plant:
        for r in np.nonzero((rng.random(n) < 0.1) & (n_rows > 0))[0]:
            e, what = rng.integers(0, n_rows[r]), rng.integers(0, 4)
            if what == 0 and B < 65536:
                branch[r, e] = rng.integers(B, 65536)
            else:
                lwr[r, e] = (0.0, -0.25, np.nan)[max(what, 1) - 1]
    return n_rows, branch, lwr


def spread_rows(B, K, n, seed):
    """rows spread over the whole id range (on a caterpillar: over the whole chain, every pair far apart)"""
    rng = np.random.default_rng(seed)
    n_rows = np.full(n, K, np.uint8)
    width = B // K  # row e of a read lies in the e-th of K stretches of the id range: distinct, and spread over all of it
    branch = rng.permuted(np.arange(K)[None, :] * width + rng.integers(0, width, (n, K)), axis=1).astype(np.uint16)
    lwr = rng.dirichlet(np.ones(K), n)
    return n_rows, branch, lwr


def lca_bytes(B):
    """the bytes of the distance tables of a tree of B nodes: dpar (8 B) and depth (2 B) per position and levels =
    floor(log2(B - 1)) + 1 rows of 2 B, rounded up to 8-byte words -- what EdgeTree.edpl_lds_bytes reports for a tree in the LDS form"""
    levels = (B - 1).bit_length() if B >= 2 else 0
    return 8 * (B + (B * 2 * (1 + levels) + 7) // 8)


def same(a, b):
    return a.shape == b.shape and bool((R.bits(a) == R.bits(b)).all())


if __name__ == "__main__":
    # python -m tests.edpl_ref KIND B: the device against the host twin on rows spread over the whole tree (tests/test_gpu_edpl.py
    # runs it under a time limit); exit status 0 when the bits agree
    import sys

    import rappas_amd as ra
    import torch
    kind, B = sys.argv[1], int(sys.argv[2])
    parent, bl = R.caterpillar(B, 3) if kind == "caterpillar" else R.random_tree(B, 3)
    n_rows, branch, lwr = spread_rows(B, 16, 4096, 11)
    et = ra.EdgeTree(parent, bl)
    out = {"n_rows": torch.from_numpy(n_rows).cuda(), "branch": torch.from_numpy(branch.view(np.int16)).cuda(), "lwr": torch.from_numpy(lwr).cuda()}
    got = et.edpl(out, 16)
    torch.cuda.synchronize()
    sys.exit(0 if same(got.cpu().numpy(), ra.edpl_host(parent, bl, 16, n_rows, branch, lwr)) else 1)
