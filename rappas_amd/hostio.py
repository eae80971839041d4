"""Host-side callers / data formats either side of the placement hot path.

These are the pieces RAPPAS keeps in Java around the native call; they are restated here so that the engine can be
driven end-to-end without a JVM (`python -m rappas_amd.tools.place`).  No placement compute happens in this module.
Reference lines (paths relative to the reference root):

* N3  FASTA ingest   src/inputs/FASTAPointer.java:66-149 (multi-line records, blank and '#' lines skipped, no gap
                     stripping for placement: Main_PLACEMENT_v07.java:195), src/inputs/Fasta.java
      dedup          src/core/algos/PlacementProcess.java:591-629 (MD5 of the sequence without '-', case-sensitive; the first
                     occurrence keeps its FULL header, later duplicates are listed by the header cut at the first space)
* N2  --jsondb       src/main_v2/SessionNext_v2.java:214-270 (json-simple dump; `states` / `align` are bare toString() tokens,
                     so the file is not strictly JSON; only DNA dumps are usable: AAStates.expandMer ignores its argument)
* N1  jplace         src/main_v2/Main_PLACEMENT_v07.java:224-315, src/core/algos/PlacementProcess.java:1005-1046,
                     src/tree/NewickReader.java:46-160 (node ids in order of appearance = pre-order, root 0),
                     src/tree/PhyloTree.java:408-439 (jplace edge ids, post-order), src/tree/NewickWriter.java:116-212
"""
import hashlib
import json
import math
import re
import struct
from dataclasses import dataclass, field
from decimal import Decimal

import numpy as np

# ------------------------------------------------------------------------------------------------
# N3: FASTA + dedup
# ------------------------------------------------------------------------------------------------


def read_fasta(text):
    """-> list of (header, sequence).  `text`: str or bytes of a whole FASTA file.
    FASTAPointer.nextSequenceAsFasta: empty lines and lines starting with '#' are skipped, a line starting with '>'
    opens a record, sequence lines are concatenated as they are (gaps kept) and the result is trim()-med."""
    if isinstance(text, bytes):
        text = text.decode("utf-8", "replace")
    records, header, parts = [], None, []
    for line in text.splitlines():
        if not line or line.startswith("#"):
            continue
        if line[0] == ">":
            if header is not None:
                records.append((header, "".join(parts).strip()))
            header, parts = line[1:], []
        elif header is not None:
            parts.append(line)
    if header is not None:
        records.append((header, "".join(parts).strip()))
    return records


def dedup_reads(records):
    """PlacementProcess.java:591-629.  -> (unique [(header, sequence)], names [[str, ...]]) where names[i][0] is the full header
    of the first occurrence and names[i][1:] the space-cut headers of its duplicates, in file order."""
    index, unique, names = {}, [], []
    for header, seq in records:
        key = hashlib.md5(seq.replace("-", "").encode()).digest()
        if key in index:
            cut = header.find(" ")
            names[index[key]].append(header if cut < 0 else header[:cut])
        else:
            index[key] = len(unique)
            unique.append((header, seq))
            names.append([header])
    return unique, names


def notplaced_log(records, unique, placed):
    """Text of `notplaced_<query>.tsv` (Main_PLACEMENT_v07.java:214, PlacementProcess.java:797-806): the FULL header of every
    read none of whose k-mers is in the database, one per line, in file order.  The reference registers a checksum only for reads
    that produce a jplace record (:1046), so every later copy of an unplaced read is placed again, fails again and is logged
    again: all occurrences are listed, not just the first.  `placed[i]`: unique read i has RK_FLAG_PLACED."""
    index = {hashlib.md5(seq.replace("-", "").encode()).digest(): i for i, (_, seq) in enumerate(unique)}
    lines = [header for header, seq in records if not placed[index[hashlib.md5(seq.replace("-", "").encode()).digest()]]]
    return "".join(h + "\n" for h in lines)


def reversed_log(records, unique, flags):
    """Text of `reversed_<query>.tsv` (written next to the not-placed log when reads are placed on the reverse or on both strands):
    the FULL header of every read whose reported result comes from its reverse complement (RK_FLAG_REVERSE, bit 32 of the unique
    read's flags), one per line, in file order, every occurrence -- the not-placed log's rules."""
    return notplaced_log(records, unique, (np.asarray(flags) & 32) == 0)


def frames_log(records, unique, frame):
    """Text of `frames_<query>.tsv` (written next to the not-placed log by --translate): one line `header<TAB>frame` for every read
    with a jplace record, in file order, every occurrence (a duplicate follows its representative, the reversed log's rules).
    `frame[i]`: the reading frame unique read i's result comes from (0..5, 0xFF = none), written +1 +2 +3 for the read as given
    from base 0, 1, 2 and -1 -2 -3 for its reverse complement."""
    index = {hashlib.md5(seq.replace("-", "").encode()).digest(): i for i, (_, seq) in enumerate(unique)}
    out = []
    for header, seq in records:
        f = int(frame[index[hashlib.md5(seq.replace("-", "").encode()).digest()]])
        if f <= 5:
            out.append(f"{header}\t{'+' if f < 3 else '-'}{f % 3 + 1}\n")
    return "".join(out)


# The standard genetic code (NCBI table 1) over the engine's states: index = b0 | b1 << 2 | b2 << 4 with A=0 T=1 C=2 G=3, value =
# residue state in the order R H K D E S T N Q C G P A I L M F W Y V, 31 = stop.  Spelled from the textbook TCAG table here (the
# engine holds the same table as numbers, rappas_amd/csrc/rk_translate.h).
CODON_STOP = 31
_AA_ORDER = "RHKDESTNQCGPAILMFWYV"
_TCAG_TABLE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
CODON_TABLE = np.zeros(64, np.uint8)
for _i, _aa in enumerate(_TCAG_TABLE):
    _b = ["ATCG".index("TCAG"[(_i >> s) & 3]) for s in (4, 2, 0)]
    CODON_TABLE[_b[0] | _b[1] << 2 | _b[2] << 4] = CODON_STOP if _aa == "*" else _AA_ORDER.index(_aa)


def translate_frames(dna, lens=None, fixed_len=0, aa_words=None):
    """The numpy twin of rk_translate_packed_device over all six reading frames: 2-bit DNA records u32 [n, dna_words] (A=0 T=1 C=2
    G=3, base i at bits [2i, 2i+2)) -> (aa u32 [6, n, aa_words], aa_lens u32 [6, n]).  Frame f < 3 reads the record from base f,
    frame 3 + o its reverse complement (base i of that = base R-1-i, state ^ 1) from base o; per read and frame the longest stop-free
    run of residues (the first of equal ones), 5 bits a residue from bit 0, zero beyond."""
    dna = np.ascontiguousarray(dna, dtype=np.uint32)
    n, dna_words = dna.shape
    cap = dna_words * 16
    R = np.minimum(np.asarray(lens, np.int64), cap) if lens is not None else np.full(n, min(int(fixed_len), cap), np.int64)
    if aa_words is None:
        aa_words = max(1, ((cap if lens is not None else int(fixed_len)) // 3 * 5 + 31) // 32)
    pos = np.arange(cap)
    states = ((dna[:, pos >> 4] >> (2 * (pos & 15)).astype(np.uint32)) & 3).astype(np.int64)  # [n, cap]
    aa = np.zeros((6, n, aa_words), np.uint32)
    aa_lens = np.zeros((6, n), np.uint32)
    rows = np.arange(n)
    max_codons = cap // 3
    for f in range(6):
        o = f % 3
        n_codons = np.where(R >= o + 3, (R - o) // 3, 0)
        j = np.arange(max_codons)
        code = np.zeros((n, max_codons), np.int64)
        for t in range(3):
            i = o + 3 * j[None, :] + t  # base of the frame's strand
            src = i if f < 3 else R[:, None] - 1 - i
            b = states[rows[:, None], np.clip(src, 0, max(cap - 1, 0))] if cap else np.zeros((n, max_codons), np.int64)
            code |= (b ^ (1 if f >= 3 else 0)) << (2 * t)
        res = CODON_TABLE[code].astype(np.int64)
        ok = (j[None, :] < n_codons[:, None]) & (res != CODON_STOP)
        run = np.zeros((n, max_codons + 1), np.int64)  # run[:, j + 1] = residues of the stop-free run that ends at codon j
        for c in range(max_codons):
            run[:, c + 1] = np.where(ok[:, c], run[:, c] + 1, 0)
        end = np.argmax(run, axis=1)  # (the first maximum: of runs of equal length the first)
        length = run[rows, end]
        start = end - length
        for i in range(int(length.max()) if n else 0):
            st = np.where(i < length, res[rows, np.minimum(start + i, max(max_codons - 1, 0))], 0).astype(np.uint64)
            w, sh = (5 * i) >> 5, (5 * i) & 31
            if w < aa_words:
                aa[f, :, w] |= ((st << np.uint64(sh)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            if sh > 27 and w + 1 < aa_words:
                aa[f, :, w + 1] |= (st >> np.uint64(32 - sh)).astype(np.uint32)
        aa_lens[f] = length
    return aa, aa_lens


_COMPLEMENT = np.arange(256, dtype=np.uint8)
for _a, _b in ("AT", "TA", "UA", "CG", "GC", "RY", "YR", "KM", "MK", "BV", "VB", "DH", "HD"):
    _COMPLEMENT[ord(_a)] = ord(_b)
    _COMPLEMENT[ord(_a.lower())] = ord(_b.lower())


def revcomp(seq_bytes):
    """Reverse complement of one DNA read (bytes / str / uint8 array -> the same type), the numpy twin of rk_revcomp_ascii_device:
    A<->T, U->A, C<->G, R<->Y, K<->M, B<->V, D<->H; S, W, N, '.' and '-' are their own complements; case is kept; every other byte
    is copied as it is."""
    if isinstance(seq_bytes, str):
        return revcomp(seq_bytes.encode("latin-1")).decode("latin-1")
    if isinstance(seq_bytes, (bytes, bytearray)):
        return _COMPLEMENT[np.frombuffer(bytes(seq_bytes), np.uint8)[::-1]].tobytes()
    return _COMPLEMENT[np.asarray(seq_bytes, np.uint8)[::-1]]


def revcomp_batch(seq, seq_off):
    """revcomp of every read of a batch (uint8 concatenation, uint64 offsets [n + 1]) -> uint8 array under the same offsets"""
    seq = np.asarray(seq, np.uint8)
    off = np.asarray(seq_off).astype(np.int64)
    lens = np.diff(off)
    # output byte i of read r (at off[r] + i) comes from off[r + 1] - 1 - i
    src = np.repeat(off[1:] - 1 + off[:-1], lens) - np.arange(int(off[-1]) - int(off[0]), dtype=np.int64) - int(off[0])
    return _COMPLEMENT[seq[src]] if len(src) else np.zeros(0, np.uint8)


def pack_batch(seqs):
    """list of str -> (uint8 concatenation, uint64 offsets) as rk_place_batch takes them."""
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    buf = np.frombuffer("".join(seqs).encode("latin-1"), np.uint8) if off[-1] else np.zeros(0, np.uint8)
    return np.ascontiguousarray(buf), off


# ------------------------------------------------------------------------------------------------
# N1: tree (Newick) with the reference's node ids and jplace edge ids
# ------------------------------------------------------------------------------------------------
@dataclass
class Node:
    id: int
    label: str = ""
    bl: np.float32 = np.float32(0.0)
    children: list = field(default_factory=list)
    parent: "Node" = None
    jplace_edge: int = -1


@dataclass
class Tree:
    root: Node
    nodes: list  # by id

    @property
    def rooted(self):
        return len(self.root.children) == 2  # NewickReader.java:209-220

    def jplace_newick(self):
        return write_newick(self, True, True, True)


def tree_to_blob(tree):
    """the reference tree as the `user` blob of a database image (rk_db_save): exact, line based -- the twin of rkh::tree_to_blob
    (rappas_amd/csrc/host/rk_fastio.hpp):  RKTREE 1 <nodes> <root> / <id> <parent> <jplace edge> <float32 bits, hex> <n children> <ids...> TAB <label>"""
    out = [f"RKTREE 1 {len(tree.nodes)} {tree.root.id}\n"]
    for n in tree.nodes:
        bits = int(np.float32(n.bl).view(np.uint32))
        kids = "".join(f" {c.id}" for c in n.children)
        out.append(f"{n.id} {n.parent.id if n.parent is not None else -1} {n.jplace_edge} {bits:08x} {len(n.children)}{kids}\t{n.label}\n")
    return "".join(out).encode("utf-8")


def tree_from_blob(blob):
    text = blob.decode("utf-8")
    lines = text.split("\n")
    head = lines[0].split()
    if len(head) != 4 or head[0] != "RKTREE" or head[1] != "1":
        raise ValueError("database image carries no reference tree (RKTREE blob)")
    n_nodes, root = int(head[2]), int(head[3])
    nodes = [Node(i) for i in range(n_nodes)]
    for i in range(n_nodes):
        nums, label = lines[1 + i].split("\t", 1)
        f = nums.split()
        if int(f[0]) != i:
            raise ValueError("database image: malformed tree line")
        n = nodes[i]
        n.parent = nodes[int(f[1])] if int(f[1]) >= 0 else None
        n.jplace_edge = int(f[2])
        n.bl = np.array([int(f[3], 16)], dtype=np.uint32).view(np.float32)[0]
        n.children = [nodes[int(c)] for c in f[5:5 + int(f[4])]]
        n.label = label
    return Tree(nodes[root], nodes)


def parse_newick(s):
    """NewickReader.java:46-200: an internal node gets its id when its '(' is read, a leaf when its text ends; ids are
    therefore the pre-order numbering with the root = 0.  `label:length` is split at ':' (float32 length)."""
    s = s.strip()
    nodes, stack, cur_children = [], [], [[]]
    token, last_closed = [], None

    def fill(node, text):
        if not text:
            return
        data = text.split(":")
        node.label = data[0]
        if len(data) > 1 and data[1]:
            node.bl = np.float32(float(data[1].split("{")[0]))

    def new_node():
        n = Node(len(nodes))
        nodes.append(n)
        return n

    for ch in s:
        if ch == "(":
            stack.append(new_node())
            cur_children.append([])
            token, last_closed = [], None
        elif ch in ",);":
            text = "".join(token).strip()
            token = []
            if last_closed is not None:
                fill(last_closed, text)
                last_closed = None
            elif text or ch != ";":
                leaf = new_node()
                fill(leaf, text)
                cur_children[-1].append(leaf)
            if ch == ")":
                parent = stack.pop()
                for c in cur_children.pop():
                    c.parent = parent
                    parent.children.append(c)
                cur_children[-1].append(parent)
                last_closed = parent
            elif ch == ";":
                break
        else:
            token.append(ch)
    root = cur_children[0][0]
    tree = Tree(root, nodes)
    reset_jplace_edge_ids(tree)
    return tree


def reset_jplace_edge_ids(tree):
    """PhyloTree.java:408-439: depth-first; a leaf child gets the next id when met, an internal node after all of its
    children (the root last)."""
    counter = [-1]

    def dfs(node):
        for c in node.children:
            if not c.children:
                counter[0] += 1
                c.jplace_edge = counter[0]
            else:
                dfs(c)
        counter[0] += 1
        node.jplace_edge = counter[0]

    dfs(tree.root)


def masses_table(tree, masses):
    """the per-edge table of a mass buffer (include/rappas_place.h: mass_q30[B] | best[B] | four totals, B = the tree's nodes), the
    text `--masses FILE` writes -- the twin of rkh::masses_table (rappas_amd/csrc/host/rk_hostio.hpp), byte-identical: tab-separated,
    one header line, one line per node in id order, a last line `#total` with the four totals.  edge_num is the node's jplace edge
    (-1 for the root); mass = mass_q30 / 2^30 with nine decimals; the clade columns are the integer sums (modulo 2^64, as the words
    themselves) over the node's subtree, the node included."""
    B = len(tree.nodes)
    m = [int(x) for x in np.asarray(masses, dtype=np.uint64).reshape(-1)]
    if len(m) != 2 * B + 4:
        raise ValueError(f"masses_table: the buffer holds {len(m)} words, the tree's {B} nodes need {2 * B + 4}")
    cm, cb = m[:B], m[B:2 * B]
    order, stack = [], [tree.root]
    while stack:
        n = stack.pop()
        order.append(n)
        stack.extend(n.children)
    for n in reversed(order[1:]):  # children before parents: every node hands its subtree's sums up
        if n.parent is not None:
            cm[n.parent.id] = (cm[n.parent.id] + cm[n.id]) & 0xFFFFFFFFFFFFFFFF
            cb[n.parent.id] = (cb[n.parent.id] + cb[n.id]) & 0xFFFFFFFFFFFFFFFF
    out = ["node_id\tedge_num\tlabel\tbest_reads\tmass_q30\tmass\tclade_best_reads\tclade_mass_q30\tclade_mass\n"]
    for n in tree.nodes:
        i = n.id
        edge = -1 if n is tree.root else n.jplace_edge
        out.append("%d\t%d\t%s\t%d\t%d\t%.9f\t%d\t%d\t%.9f\n" % (i, edge, n.label, m[B + i], m[i], float(m[i]) / 1073741824.0, cb[i], cm[i],
                                                               float(cm[i]) / 1073741824.0))
    out.append("#total\t%d\t%d\t%d\t%d\n" % tuple(m[2 * B:]))
    return "".join(out)


def sample_name(header, sep):
    """`--sample-sep C`: a record's sample is its header up to the first C; a header without C is an error that names it"""
    cut = header.find(sep)
    if cut < 0:
        raise ValueError(f"--sample-sep: the header '{header}' does not contain the separator '{sep}'")
    return header[:cut]


def sample_members(records, unique, sep):
    """the per-sample membership of the unique reads -- the twin of rkh::sample_members (rappas_amd/csrc/host/rk_hostio.hpp).
    -> (names, member_off u64 [n + 1], member_sample u32, member_weight u32): the samples in byte-wise order of their names; unique
    read i owns the entries member_off[i] .. member_off[i + 1], one per distinct sample among its records, the number of those records
    as its weight, in sample order -- the CSR rk_place_batch_masses_samples takes."""
    rec_names = [sample_name(header, sep) for header, _ in records]
    names = sorted(set(rec_names), key=lambda s: s.encode("utf-8", "surrogatepass"))
    rank = {s: i for i, s in enumerate(names)}
    index = {hashlib.md5(seq.replace("-", "").encode()).digest(): i for i, (_, seq) in enumerate(unique)}
    per_read = [{} for _ in unique]
    for (_, seq), s in zip(records, rec_names):
        d = per_read[index[hashlib.md5(seq.replace("-", "").encode()).digest()]]
        d[rank[s]] = d.get(rank[s], 0) + 1
    off, sample, weight = [0], [], []
    for d in per_read:
        for s in sorted(d):
            sample.append(s)
            weight.append(d[s])
        off.append(len(sample))
    return names, np.array(off, np.uint64), np.array(sample, np.uint32), np.array(weight, np.uint32)


def masses_samples_table(tree, names, masses):
    """the text `--masses FILE` / `--masses-only FILE` write with `--sample-sep`: for each sample in order a line
    `#sample<TAB>name<TAB>index` and masses_table of its words, then a line `#skipped_entries<TAB>n` (the last word of the sample mass
    buffer).  The twin of rkh::masses_samples_table, byte-identical."""
    W = 2 * len(tree.nodes) + 4
    m = np.asarray(masses, dtype=np.uint64).reshape(-1)
    if len(m) != len(names) * W + 1:
        raise ValueError(f"masses_samples_table: the buffer holds {len(m)} words, {len(names)} samples on the tree's {len(tree.nodes)} nodes need {len(names) * W + 1}")
    out = []
    for s, name in enumerate(names):
        out.append(f"#sample\t{name}\t{s}\n")
        out.append(masses_table(tree, m[s * W:(s + 1) * W]))
    out.append(f"#skipped_entries\t{int(m[-1])}\n")
    return "".join(out)


def kr_table(names, D):
    """the text `--kr FILE` writes: a line `#kr<TAB>S`, one line per sample in sample order -- its name and the S distances of its row,
    `%.17g` (a NaN as `nan`), tab-separated --, and a last line `#samples_without_mass<TAB>n`, n the samples whose diagonal is NaN.
    The twin of rkh::kr_table (rappas_amd/csrc/host/rk_hostio.hpp), byte-identical."""
    S = len(names)
    D = np.asarray(D, dtype=np.float64).reshape(S, S)
    out = [f"#kr\t{S}\n"]
    for s, name in enumerate(names):
        out.append(name + "".join("\tnan" if np.isnan(d) else "\t%.17g" % d for d in D[s]) + "\n")
    out.append(f"#samples_without_mass\t{int(np.isnan(np.diagonal(D)).sum())}\n")
    return "".join(out)


def epca_table(names, n_branches, k, iters, n_active, k_eff, eigenvalue, share, residual, projection, loading):
    """the text `--epca FILE` writes, every double as `%.17g`: a line `#epca<TAB>S<TAB>B<TAB>k<TAB>n_active<TAB>k_eff<TAB>iters`; the
    lines `#eigenvalue`, `#share`, `#residual` with k values each; `#projections` and a line per sample (its name and k values);
    `#loadings` and a line per node id (the id and k values); `#samples_without_mass<TAB>n`.  The arrays are what placement.epca_finish
    gives: eigenvalue, share, residual [k], projection [S, k], loading [B, k].  The twin of rkh::epca_table, byte-identical."""
    S = len(names)
    projection = np.asarray(projection, np.float64).reshape(S, k)
    loading = np.asarray(loading, np.float64).reshape(n_branches, k)

    def row(head, v):
        return head + "".join("\t%.17g" % float(v[j]) for j in range(k)) + "\n"

    out = [f"#epca\t{S}\t{n_branches}\t{k}\t{n_active}\t{k_eff}\t{iters}\n", row("#eigenvalue", eigenvalue), row("#share", share),
           row("#residual", residual), "#projections\n"]
    out.extend(row(names[s], projection[s]) for s in range(S))
    out.append("#loadings\n")
    out.extend(row(str(x), loading[x]) for x in range(n_branches))
    out.append(f"#samples_without_mass\t{S - n_active}\n")
    return "".join(out)


def edpl_table(records, unique, n_rows, edpl):
    """the text `--edpl FILE` writes: a line `#edpl<TAB>n_lines`, then `header<TAB>edpl` (`%.17g`) with the FULL header of every FASTA
    record that has a placement, in file order, every occurrence (a duplicate follows its representative, the frames log's rules).
    n_rows[i], edpl[i]: the rows and the EDPL of unique read i.  The twin of rkh::edpl_table, byte-identical."""
    index = {hashlib.md5(seq.replace("-", "").encode()).digest(): i for i, (_, seq) in enumerate(unique)}
    lines = []
    for header, seq in records:
        u = index[hashlib.md5(seq.replace("-", "").encode()).digest()]
        if n_rows[u]:
            lines.append("%s\t%.17g\n" % (header, float(edpl[u])))
    return f"#edpl\t{len(lines)}\n" + "".join(lines)


def _squash_leaf(name):
    """a sample name as a Newick leaf: single-quoted, a quote doubled, when it holds any of ()[]':;, or white space"""
    if any(c in "()[]':;, \t\n\r\v\f" for c in name):
        return "'" + name.replace("'", "''") + "'"
    return name


def squash_table(names, merges, n_merges, with_mass=None):
    """the text `--squash FILE` writes: a line `#squash<TAB>S<TAB>n_merges`; one line per merge, `k<TAB>a<TAB>b<TAB>distance<TAB>size`
    (`%.17g`); a line `#newick<TAB>tree;` -- leaves named by sample (quoted where Newick needs it), an inner node at height
    distance / 2, a leaf at height 0, an edge length height(parent) - height(child) as `%.17g` (negative where the clustering is not
    monotone), children in the order a, b, no length on the root; one sample with mass gives `name;`, none gives `;` --; a line
    `#inversions<TAB>n`, the number of negative edge lengths; and a last line `#samples_without_mass<TAB>n`.
    merges: rows of placement.SQUASH_MERGE (or anything with a, b, size, distance per row).  with_mass: one flag per sample; None: the
    samples the merges name (which cannot tell one sample with mass from none).  The twin of rkh::squash_table, byte-identical."""
    S = len(names)
    out = [f"#squash\t{S}\t{n_merges}\n"]
    sub, height = {}, {}  # per slot: the subtree's text and its height
    if with_mass is None:
        with_mass = [False] * S
        for k in range(n_merges):
            with_mass[int(merges[k]["a"])] = with_mass[int(merges[k]["b"])] = True
    for s in range(S):
        if with_mass[s]:
            sub[s], height[s] = _squash_leaf(names[s]), 0.0
    inversions, root = 0, None
    for k in range(n_merges):
        a, b, d, size = int(merges[k]["a"]), int(merges[k]["b"]), float(merges[k]["distance"]), int(merges[k]["size"])
        out.append("%d\t%d\t%d\t%.17g\t%d\n" % (k, a, b, d, size))
        h = d / 2
        la, lb = h - height[a], h - height[b]
        inversions += (la < 0) + (lb < 0)
        sub[a] = "(%s:%.17g,%s:%.17g)" % (sub[a], la, sub.pop(b), lb)
        height[a] = h
        root = a
    if root is None and len(sub) == 1:
        root = next(iter(sub))
    out.append("#newick\t" + (sub[root] if root is not None else "") + ";\n")
    out.append(f"#inversions\t{inversions}\n")
    out.append(f"#samples_without_mass\t{S - sum(1 for f in with_mass if f)}\n")
    return "".join(out)


def kmeans_table(names, k, assign, dist, sizes, within, info):
    """the text `--kmeans FILE` writes: a line `#kmeans<TAB>S<TAB>k<TAB>k_eff<TAB>n_active<TAB>rounds<TAB>converged`; `#clusters` and a
    line `j<TAB>size<TAB>within` (`%.17g`) per cluster j < k; `#samples` and a line `name<TAB>cluster<TAB>distance` per sample in sample
    order, a sample without mass with the cluster `-` and the distance `0`; a last line `#samples_without_mass<TAB>n`.  The arrays are
    what kmeans_host and EdgeTree.kmeans_batch give.  The twin of rkh::kmeans_table, byte-identical."""
    S = len(names)
    info = [int(w) for w in info]
    out = ["#kmeans\t%d\t%d\t%d\t%d\t%d\t%d\n" % (S, k, info[0], info[1], info[2], info[3] & 1), "#clusters\n"]
    out.extend("%d\t%d\t%.17g\n" % (j, int(sizes[j]), float(within[j])) for j in range(k))
    out.append("#samples\n")
    for s in range(S):
        a = int(assign[s])
        out.append("%s\t-\t0\n" % names[s] if a == 0xFFFFFFFF else "%s\t%d\t%.17g\n" % (names[s], a, float(dist[s])))
    out.append(f"#samples_without_mass\t{S - info[1]}\n")
    return "".join(out)


def diversity_table(names, theta, values):
    """the text `--diversity FILE` writes: a line `#diversity<TAB>S<TAB>n_theta`; a line `#columns` with rooted_pd, pd, bwpd, quadratic,
    phylo_entropy and, per theta, rooted_pd_<theta> and bwpd_<theta> (theta as `%.17g`); one line per sample in sample order -- its
    name and its values, `%.17g` (a NaN as `nan`), tab-separated --; a last line `#samples_without_mass<TAB>n`, n the samples whose
    row is NaN.  `values` [S, 5 + 2 n_theta] is what diversity_host and EdgeTree.diversity_batch give.  The twin of
    rkh::diversity_table, byte-identical."""
    S, theta = len(names), [float(t) for t in theta]
    values = np.asarray(values, dtype=np.float64).reshape(S, 5 + 2 * len(theta))
    out = ["#diversity\t%d\t%d\n" % (S, len(theta)), "#columns\trooted_pd\tpd\tbwpd\tquadratic\tphylo_entropy"]
    out.extend("\trooted_pd_%.17g\tbwpd_%.17g" % (t, t) for t in theta)
    out.append("\n")
    for s, name in enumerate(names):
        out.append(name + "".join("\tnan" if np.isnan(v) else "\t%.17g" % v for v in values[s]) + "\n")
    out.append(f"#samples_without_mass\t{int(np.isnan(values[:, 0]).sum())}\n")
    return "".join(out)


def _metadata_number(text):
    """a number of a --metadata file: [+-] digits with an optional point and fraction, an optional exponent; None for anything else or
    for a value that is not finite (what strtod and float() accept beyond that -- inf, nan, hex, blanks -- is no number here)"""
    if not re.fullmatch(r"[+-]?(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?", text):
        return None
    v = float(text)
    return v if math.isfinite(v) else None


def parse_metadata(text):
    """the sample metadata of `--metadata TSV` -- the twin of rkh::parse_metadata (rappas_amd/csrc/host/rk_hostio.hpp), the same
    sentences.  A first line `sample<TAB>name_1<TAB>...<TAB>name_F` with F <= 8, then one line per sample: its name and F finite
    numbers; empty lines are skipped.  -> (feature names, {sample name: [F values]}).  ValueError("--metadata: ...") for a header
    that is none, a line with another number of fields, a field that is no finite number, a sample named twice."""
    if isinstance(text, bytes):
        text = text.decode("utf-8", "replace")
    lines = [(i + 1, ln) for i, ln in enumerate(text.split("\n")) if ln.rstrip("\r") != ""]
    head = lines[0][1].rstrip("\r").split("\t") if lines else []
    if not head or head[0] != "sample" or len(head) - 1 > 8 or any(n == "" for n in head[1:]):
        raise ValueError("--metadata: the first line must be sample<TAB>name_1<TAB>...<TAB>name_F with at most 8 column names")
    rows = {}
    for no, ln in lines[1:]:
        f = ln.rstrip("\r").split("\t")
        if len(f) != len(head):
            raise ValueError(f"--metadata: line {no} has {len(f)} fields, the first line has {len(head)}")
        values = [_metadata_number(v) for v in f[1:]]
        for v, field in zip(values, f[1:]):
            if v is None:
                raise ValueError(f"--metadata: line {no}: '{field}' is not a finite number")
        if f[0] in rows:
            raise ValueError(f"--metadata: line {no}: the sample '{f[0]}' has a line already")
        rows[f[0]] = values
    return head[1:], rows


def metadata_of_samples(sample_names, parsed):
    """float64 [F, S]: the metadata of the samples of a run, in sample order, from parse_metadata's answer (None: no file, F = 0);
    ValueError for more than 4096 samples and for a sample of the run without a line -- lines of other samples are ignored"""
    if len(sample_names) > 4096:
        raise ValueError(f"--edge-stats: the run has {len(sample_names)} samples, at most 4096")
    names, rows = parsed if parsed is not None else ([], {})
    for s in sample_names:
        if parsed is not None and s not in rows:
            raise ValueError(f"--metadata: the sample '{s}' of the run has no line")
    return np.array([[rows[s][f] for s in sample_names] for f in range(len(names))], np.float64).reshape(len(names), len(sample_names))


def edge_stats_table(names, feature_names, n_active, table, feature_table):
    """the text `--edge-stats FILE` writes, every double as `%.17g` (a NaN as `nan`): a line
    `#edge_stats<TAB>S<TAB>B<TAB>F<TAB>n_active`; a line `#columns` with node, the eight fixed columns and, per metadata column,
    mass_pearson_<name>, mass_spearman_<name>, imb_pearson_<name>, imb_spearman_<name>; a line per node id (the id and its values);
    `#features` and a line per metadata column (its name, its mean and its population variance over the samples with mass);
    `#samples_without_mass<TAB>n`.  table [B, 8 + 4F] and feature_table [F, 2] are what edgestats.edgestat_finish gives.  The twin of
    rkh::edge_stats_table, byte-identical."""
    S, F = len(names), len(feature_names)
    table = np.asarray(table, np.float64)
    B = table.shape[0]
    table = table.reshape(B, 8 + 4 * F)
    feature_table = np.asarray(feature_table, np.float64).reshape(F, 2)
    num = lambda v: "\tnan" if np.isnan(v) else "\t%.17g" % v
    out = [f"#edge_stats\t{S}\t{B}\t{F}\t{n_active}\n", "#columns\tnode\tmass_mean\tmass_var\tmass_sd\tmass_cv\tmass_vmr\timb_mean\timb_var\timb_sd"]
    out.extend(f"\tmass_pearson_{n}\tmass_spearman_{n}\timb_pearson_{n}\timb_spearman_{n}" for n in feature_names)
    out.append("\n")
    out.extend(str(x) + "".join(num(v) for v in table[x]) + "\n" for x in range(B))
    out.append("#features\n")
    out.extend(feature_names[f] + num(feature_table[f, 0]) + num(feature_table[f, 1]) + "\n" for f in range(F))
    out.append(f"#samples_without_mass\t{S - n_active}\n")
    return "".join(out)


def _fmt12(x):
    """NumberFormat.getNumberInstance(Locale.UK) with exactly 12 fraction digits (NewickWriter.java:61-64): grouping commas,
    HALF_EVEN on the exact binary value."""
    return f"{Decimal(float(x)):,.12f}"


def write_newick(tree, with_bl, with_internal_names, with_jplace_labels):
    """NewickWriter.java:116-212 (no node-id prefix).  At an unrooted top level (3 sons) the root carries neither length
    nor edge label."""
    out = []

    def dfs(node, level):
        out.append("(")
        n = len(node.children)
        for i, c in enumerate(node.children):
            if not c.children:
                out.append(c.label)
                if with_bl:
                    out.append(":" + _fmt12(c.bl))
                if with_jplace_labels:
                    out.append("{%d}" % c.jplace_edge)
            else:
                dfs(c, level + 1)
            if i < n - 1:
                out.append(",")
            else:
                out.append(")")
                if with_internal_names:
                    out.append(node.label)
                if with_bl and level > -1:
                    out.append(":" + _fmt12(node.bl))
                if with_jplace_labels and level > -1:
                    out.append("{%d}" % node.jplace_edge)
        if node.parent is None:
            out.append(";")

    dfs(tree.root, 0 if tree.rooted else -1)
    return "".join(out)


# ------------------------------------------------------------------------------------------------
# N1: numbers the way json-simple prints them (Number.toString())
# ------------------------------------------------------------------------------------------------
def _java_float_repr(shortest, value):
    """Float.toString / Double.toString layout from the shortest uniquely-identifying decimal digits:
    plain decimal for 1e-3 <= |x| < 1e7, otherwise d.dddE[-]n; always at least one digit after the point.
    (JDK >= 19 digits.  Older JDKs print a few values with one digit more than the shortest form, e.g. 2.0E23 as
    1.9999999999999998E23 and Float.MIN_VALUE as 1.4E-45; both spellings parse to the same number.)"""
    if value != value or value in (float("inf"), float("-inf")):
        return "null"  # JSONValue.toJSONString: non-finite numbers become null
    d = Decimal(shortest)
    sign, digits, exp = d.as_tuple()
    digits = list(digits)
    while len(digits) > 1 and digits[-1] == 0:
        digits.pop()
        exp += 1
    neg = "-" if (sign or (value == 0 and math.copysign(1.0, value) < 0)) else ""
    if all(x == 0 for x in digits):
        return neg + "0.0"
    ds = "".join(map(str, digits))
    e10 = len(ds) + exp  # value = 0.ds * 10^e10
    a = abs(value)
    if 1e-3 <= a < 1e7:
        if e10 <= 0:
            body = "0." + "0" * (-e10) + ds
        elif e10 >= len(ds):
            body = ds + "0" * (e10 - len(ds)) + ".0"
        else:
            body = ds[:e10] + "." + ds[e10:]
    else:
        body = ds[0] + "." + (ds[1:] or "0") + "E" + str(e10 - 1)
    return neg + body


def java_double_to_string(x):
    return _java_float_repr(repr(float(x)), float(x))


def java_float_to_string(x):
    x = np.float32(x)
    return _java_float_repr(np.format_float_scientific(x, unique=True, trim="0") if np.isfinite(x) else "nan", float(x))


# ------------------------------------------------------------------------------------------------
# N1: jplace document
# ------------------------------------------------------------------------------------------------
def jplace_placements(tree, names, n_rows, branch, score, lwr, guppy=False):
    """One placement object per placed unique read, rows [edge_num, likelihood, like_weight_ratio, distal_length,
    pendant_length] (PlacementProcess.java:1005-1046); `names[i]` from dedup_reads."""
    out = []
    for i in range(len(n_rows)):
        if n_rows[i] == 0:
            continue
        rows = []
        for j in range(int(n_rows[i])):
            node = tree.nodes[int(branch[i, j])]
            edge = str(node.jplace_edge)
            like = java_float_to_string(score[i, j])
            ratio = java_double_to_string(lwr[i, j])
            distal = java_float_to_string(np.float32(node.bl) / np.float32(2))
            rows.append([distal, edge, ratio, like, "0.0"] if guppy else [edge, like, ratio, distal, "0.0"])
        out.append((rows, names[i]))
    return out


_SHORT_ESC = {'"': '\\"', "\\": "\\\\", "\b": "\\b", "\f": "\\f", "\n": "\\n", "\r": "\\r", "\t": "\\t", "/": "\\/"}


def _jstr(s):
    """JSONValue.escape of json-simple 1.1 (the reference's lib/json_simple-1.1.jar): the short escapes incl. '\\/', and
    \\uXXXX (upper-case hex) for U+0000-001F, U+007F-009F and U+2000-20FF; everything else verbatim."""
    out = ['"']
    for ch in s:
        if ch in _SHORT_ESC:
            out.append(_SHORT_ESC[ch])
        elif ch <= "\u001f" or "\u007f" <= ch <= "\u009f" or "\u2000" <= ch <= "\u20ff":
            out.append("\\u%04X" % ord(ch))
        else:
            out.append(ch)
    out.append('"')
    return "".join(out)


def jplace_document(tree, placements, call_string="", guppy=False):
    """Main_PLACEMENT_v07.java:224-315.  Key order follows json-simple's JSONObject (a java.util.HashMap): top level
    metadata, tree, placements, fields, version; a placement is p, nm.  The regex prettifier of :304-310 is applied."""
    fields = ["distal_length", "edge_num", "like_weight_ratio", "likelihood", "pendant_length"] if guppy else \
             ["edge_num", "likelihood", "like_weight_ratio", "distal_length", "pendant_length"]
    pl = []
    for rows, nm in placements:
        p = ",".join("[" + ",".join(r) + "]" for r in rows)
        n = ",".join("[" + _jstr(name) + ",1]" for name in nm)
        pl.append('{"p":[' + p + '],"nm":[' + n + "]}")
    out = ('{"metadata":{"invocation":' + _jstr("viromeplacer" + call_string) + '},"tree":' + _jstr(tree.jplace_newick()) +
           ',"placements":[' + ",".join(pl) + '],"fields":[' + ",".join(_jstr(f) for f in fields) + '],"version":3}')
    out = out.replace("},{", "\n},{\n\t")
    out = out.replace('],"', '],\n\t"')
    out = out.replace("]}],", "]\n}\n],\n")
    out = out.replace(',"placements":[{"p"', ',\n"placements":\n[\n{\n\t"p"')
    out = out.replace("],[", "],\n\t[")
    out = out.replace('"p":[[', '"p":\n\t[[')
    out = out.replace('"nm":[[', '"nm":\n\t[[')
    return out


# ------------------------------------------------------------------------------------------------
# N2: --jsondb dumps
# ------------------------------------------------------------------------------------------------
DNA_STATE = {"A": 0, "T": 1, "C": 2, "G": 3}


def load_jsondb(text):
    """SessionNext_v2.saveToJSON dump -> dict(alphabet, k, n_branches, thr, thr_log10, key_codes, row_offsets, branch_ids,
    scores, tree, calibration).  The bare `states` / `align` tokens are replaced by null before parsing."""
    if isinstance(text, bytes):
        text = text.decode("utf-8", "replace")
    text = re.sub(r'"(states|align)"\s*:\s*(?!["{\[\-\dntf])[^,}]+', r'"\1":null', text)
    doc = json.loads(text)
    k = int(doc["k"])
    tree = parse_newick(doc["originalTree"])
    codes, off, br, sc = [], [0], [], []
    for kmer, row in doc["hash"].items():
        if len(kmer) != k or any(c not in DNA_STATE for c in kmer):
            raise ValueError(f"jsondb: k-mer {kmer!r} is not a DNA {k}-mer (amino-acid dumps are unusable: "
                             "AAStates.expandMer ignores its argument)")
        codes.append(sum(DNA_STATE[c] << (2 * i) for i, c in enumerate(kmer)))
        for node, v in row.items():
            br.append(int(node))
            sc.append(v)
        off.append(len(br))
    return dict(alphabet=4, k=k, n_branches=len(tree.nodes), thr=np.float32(doc["PPStarThreshold"]),
                thr_log10=np.float32(doc["PPStarThresholdAsLog10"]), key_codes=np.array(codes, np.uint64),
                row_offsets=np.array(off, np.uint64), branch_ids=np.array(br, np.uint16), scores=np.array(sc, np.float32),
                tree=tree, calibration=doc.get("calibrationNormScore"), omega=doc.get("omega"))


def load_uniondb(data):
    """A `.union` database (SessionNext_v2.storeHash, src/main_v2/SessionNext_v2.java:109-147; read back by load, :158-207):
    a Java serialization stream holding, in this order, block data {int k, int minK, float omega, int branchPerEdge, float
    stateThreshold, float PPStarThreshold, float PPStarThresholdAsLog10}, the objects states, align, originalTree, extendedTree,
    ARTree, nodeMapping, block data {float calibrationNormScore, boolean onlyFakes} and the CustomHash_v4_FastUtil81.
    Same result dict as load_jsondb.  What is taken from the object graph:

    * alphabet: the class of `states` (core.DNAStatesShifted / core.AAStates; --convertUO shows as 'U' in AAStates' char map);
    * tree: PhyloTree.indexById (HashMap<Integer, PhyloNode>, src/tree/PhyloTree.java:39) -> per node id, label, branch length,
      jplace edge id (src/tree/PhyloNode.java:30-37) and, from its DefaultMutableTreeNode part, parent and ordered children;
    * rows: CustomHash_v4_FastUtil81.hash, an Object2ObjectOpenCustomHashMap<byte[], Char2FloatOpenHashMap>
      (src/core/hash/CustomHash_v4_FastUtil81.java:36): fastutil writes its open-hash maps as defaultWriteObject() followed by
      the entries -- writeObject(key), writeObject(value) for the outer map, writeChar(key), writeFloat(value) for a row -- `size`
      of them.  DNA keys are compressMer bytes (DNAStatesShifted.java:115-143: little-endian 2-bit codes), AA keys one state
      per byte.
    PARITY UNPINNED (rappas_amd/javaser.py): never run against a file written by a JVM."""
    from . import javaser
    recs = javaser.parse(data)
    blocks = b"".join(v for t, v in recs if t == "block")
    objs = [v for t, v in recs if t == "object"]
    if len(blocks) < 33 or len(objs) < 7:
        raise ValueError(f"union: expected 33 bytes of scalars and 7 objects, found {len(blocks)} and {len(objs)} (a database stored "
                         "without its hash?)")
    k, mink, omega, bpe, st_thr, thr, thr_log10 = struct.unpack(">iififff", blocks[:28])
    calib, only_fakes = struct.unpack(">f?", blocks[28:33])
    states, _align, otree, _etree, _artree, _nodemap, chash = objs[:7]
    if states.classname == "core.DNAStatesShifted":
        alphabet, convert_uo = 4, False
    elif states.classname == "core.AAStates":
        alphabet = 20
        b = states.get("b")
        convert_uo = b is not None and any(javaser.boxed(key) in (ord("U"), "U") for key, _ in javaser.hashmap_items(b))
    else:
        raise ValueError(f"union: unknown States class {states.classname}")
    # ---- original tree ----
    index = otree.get("indexById")
    if index is None:
        raise ValueError("union: originalTree has no indexById map")
    jn = {int(javaser.boxed(key)): val for key, val in javaser.hashmap_items(index)}
    nodes = [None] * len(jn)
    for i, o in jn.items():
        if not 0 <= i < len(nodes):
            raise ValueError(f"union: node id {i} outside 0..{len(nodes) - 1}")
        n = Node(i)
        n.label = o.get("label") or ""
        n.bl = np.float32(o.get("branchLengthToAncestor"))
        n.jplace_edge = int(o.get("jplaceEdgeId"))
        nodes[i] = n
    ident = {id(o): i for i, o in jn.items()}
    root = None
    for i, o in jn.items():
        ch = o.get("children")
        for c in (javaser.arraylist_items(ch) if ch is not None else []):
            nodes[i].children.append(nodes[ident[id(c)]])
            nodes[ident[id(c)]].parent = nodes[i]
    for n in nodes:
        if n.parent is None:
            root = n if root is None or n.id < root.id else root
    tree = Tree(root, nodes)
    # ---- hash ----
    outer = chash.get("hash")
    if outer is None:
        raise ValueError("union: CustomHash_v4_FastUtil81 without its map")
    oname = "it.unimi.dsi.fastutil.objects.Object2ObjectOpenCustomHashMap"
    rname = "it.unimi.dsi.fastutil.chars.Char2FloatOpenHashMap"
    kv = outer.objects(oname)
    n_keys = int(outer.get("size"))
    if len(kv) != 2 * n_keys:
        raise ValueError(f"union: outer map announces {n_keys} entries, stream holds {len(kv) // 2}")
    codes, off, br, sc = [], [0], [], []
    for key, row in zip(kv[0::2], kv[1::2]):
        raw = key.raw
        if alphabet == 4:
            code = int.from_bytes(raw, "little")  # compressMer bytes: base i at bits 2*(i%4) of byte i/4
            if code >> (2 * k):
                raise ValueError("union: DNA key has bits beyond 2k")
        else:
            code = sum((b & 0xFF) << (5 * i) for i, b in enumerate(raw))
        codes.append(code)
        m = int(row.get("size"))
        blob = row.block(rname)
        if len(blob) != 6 * m:
            raise ValueError(f"union: row announces {m} entries, stream holds {len(blob)} bytes")
        for e in range(m):
            node, v = struct.unpack_from(">Hf", blob, 6 * e)
            br.append(node)
            sc.append(v)
        off.append(len(br))
    return dict(alphabet=alphabet, convert_uo=convert_uo, k=k, n_branches=len(nodes), thr=np.float32(thr), thr_log10=np.float32(thr_log10),
                key_codes=np.array(codes, np.uint64), row_offsets=np.array(off, np.uint64), branch_ids=np.array(br, np.uint16),
                scores=np.array(sc, np.float32), tree=tree, calibration=calib, omega=omega, only_fakes=only_fakes)


def dump_jsondb(db, newick, omega=1.5):
    """Writer with the layout json-simple gives saveToJSON (for tests and for exchanging synthetic DBs): HashMap key order
    is not reproduced (irrelevant to any reader), floats are printed like Float.toString."""
    letters = "ATCG"
    rows = []
    for r in range(len(db.key_codes)):
        code = int(db.key_codes[r])
        kmer = "".join(letters[(code >> (2 * i)) & 3] for i in range(db.k))
        a, b = int(db.row_offsets[r]), int(db.row_offsets[r + 1])
        ent = ",".join(f'"{int(db.branch_ids[e])}":{java_float_to_string(db.scores[e])}' for e in range(a, b))
        rows.append(f'"{kmer}":{{{ent}}}')
    head = (f'"k":{db.k},"mink":{db.k},"omega":{java_float_to_string(omega)},"branchPerEdge":1,"stateThreshold":1.4E-45,'
            f'"PPStarThreshold":{java_float_to_string(db.thr)},"PPStarThresholdAsLog10":{java_float_to_string(db.thr_log10)},'
            f'"states":core.DNAStatesShifted@6d06d69c,"align":alignement.Alignment@7852e922,"originalTree":{_jstr(newick)},'
            f'"calibrationNormScore":null')
    return "{" + head + ',"hash":{' + ",".join(rows) + "}}"
