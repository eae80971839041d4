"""`--edge-stats FILE [--metadata TSV]` of the two placement drivers, `rk_place` and `python -m rappas_amd.tools.place`, as far as no
GPU is needed: the two option rules exit 2 with their sentences before any file is opened; a metadata file that breaks its syntax
ends both drivers with the same sentence before the database is read; neither writes anything.  And the parser and the table writer
of rappas_amd/hostio.py on their own."""
import os
import subprocess
import sys

import numpy as np
import pytest

from rappas_amd import build, edgestats as ES, hostio
from rappas_amd.tools import place as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = "--metadata: the first line must be sample<TAB>name_1<TAB>...<TAB>name_F with at most 8 column names"

# (id, the file's text, the sentence)
BAD_FILES = [
    ("empty", "", HEAD),
    ("no_sample_word", "name\tpH\na\t1\n", HEAD),
    ("nine_columns", "sample" + "".join(f"\tc{i}" for i in range(9)) + "\n", HEAD),
    ("unnamed_column", "sample\tpH\t\n", HEAD),
    ("short_line", "sample\tpH\tdepth\na\t1\t2\n\nb\t1\n", "--metadata: line 4 has 2 fields, the first line has 3"),
    ("long_line", "sample\tpH\na\t1\t2\n", "--metadata: line 2 has 3 fields, the first line has 2"),
    ("nan", "sample\tpH\na\tnan\n", "--metadata: line 2: 'nan' is not a finite number"),
    ("infinity", "sample\tpH\r\na\t1\r\nb\t-inf\r\n", "--metadata: line 3: '-inf' is not a finite number"),
    ("overflow", "sample\tpH\na\t1e999\n", "--metadata: line 2: '1e999' is not a finite number"),
    ("hex", "sample\tpH\na\t0x10\n", "--metadata: line 2: '0x10' is not a finite number"),
    ("blank_in_number", "sample\tpH\na\t 1\n", "--metadata: line 2: ' 1' is not a finite number"),
    ("empty_number", "sample\tpH\na\t\n", "--metadata: line 2: '' is not a finite number"),
    ("duplicate", "sample\tpH\na\t1\nb\t2\na\t3\n", "--metadata: line 4: the sample 'a' has a line already"),
]


@pytest.fixture(scope="module")
def rk_place():
    return build.build_host_tools()


def drivers(rk_place):
    return (("cpp", [rk_place]), ("py", [sys.executable, "-m", "rappas_amd.tools.place"]))


def run(cmd, args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(cmd + args, capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)


@pytest.mark.parametrize("args,sentence", [
    (["--masses-only", "{t}", "--edge-stats", "{e}"], P.EDGE_STATS_NEEDS_SAMPLE_SEP),
    (["--masses-only", "{t}", "--sample-sep", "_", "--metadata", "{m}"], P.METADATA_NEEDS_EDGE_STATS),
    (["--out", "{o}", "--masses", "{t}", "--sample-sep", "_", "--kr", "{r}", "--metadata", "{m}"], P.METADATA_NEEDS_EDGE_STATS),
], ids=["edge_stats_without_sample_sep", "metadata_without_edge_stats", "metadata_without_edge_stats_placing"])
def test_a_broken_rule_exits_2_with_its_sentence_and_writes_nothing(rk_place, tmp_path, args, sentence):
    for name, cmd in drivers(rk_place):
        d = tmp_path / name
        d.mkdir()
        paths = {x: str(d / x) for x in "temor"}
        r = run(cmd, ["--jsondb", str(d / "no_such_db.json"), "--fasta", str(d / "no_such.fasta")] + [a.format(**paths) for a in args])
        assert r.returncode == 2 and sentence in r.stderr, (name, r.returncode, r.stderr[-2000:])
        assert os.listdir(d) == [], name


@pytest.mark.parametrize("text,sentence", [b[1:] for b in BAD_FILES], ids=[b[0] for b in BAD_FILES])
def test_a_bad_metadata_file_ends_both_drivers_before_the_database_is_read(rk_place, tmp_path, text, sentence):
    """the database named here is no database: a driver that read it before the metadata would say so"""
    with pytest.raises(ValueError) as e:
        hostio.parse_metadata(text.encode())
    assert str(e.value) == sentence
    (tmp_path / "db.json").write_text("no database")
    (tmp_path / "q.fasta").write_text(">a_1\nACGT\n")
    (tmp_path / "meta.tsv").write_bytes(text.encode())
    for name, cmd in drivers(rk_place):
        d = tmp_path / name
        d.mkdir()
        r = run(cmd, ["--jsondb", str(tmp_path / "db.json"), "--fasta", str(tmp_path / "q.fasta"), "--masses-only", str(d / "t"), "--sample-sep", "_",
                      "--edge-stats", str(d / "es"), "--metadata", str(tmp_path / "meta.tsv"), "--logs", str(d / "logs")])
        assert r.returncode == 1 and r.stderr.strip().endswith(sentence), (name, r.returncode, r.stderr[-2000:])
        assert os.listdir(d) == [], name


def test_parse_metadata_and_the_samples_of_a_run():
    names, rows = hostio.parse_metadata(b"sample\tpH\tdepth\r\n\r\nsoil\t6.5\t-1e2\ngut\t+7.\t.5\nsea\t8\t3E+1\n")
    assert names == ["pH", "depth"] and rows == {"soil": [6.5, -100.0], "gut": [7.0, 0.5], "sea": [8.0, 30.0]}
    meta = hostio.metadata_of_samples(["gut", "soil"], (names, rows))  # the line of `sea`, which the run does not have, is ignored
    assert meta.dtype == np.float64 and meta.tolist() == [[7.0, 6.5], [0.5, -100.0]]
    assert hostio.metadata_of_samples(["gut", "soil"], None).shape == (0, 2)
    assert hostio.parse_metadata("sample\n") == ([], {}) and hostio.metadata_of_samples(["x"], ([], {"x": []})).shape == (0, 1)
    with pytest.raises(ValueError, match="--metadata: the sample 'void' of the run has no line"):
        hostio.metadata_of_samples(["gut", "void"], (names, rows))
    with pytest.raises(ValueError, match="--edge-stats: the run has 4097 samples, at most 4096"):
        hostio.metadata_of_samples([str(i) for i in range(4097)], None)


def test_the_table_text_of_the_known_answers():
    from tests.test_edgestat_host import golden_case
    g, parent, m, S, meta = golden_case()
    r = ES.edgestat_finish(len(parent), S, *ES.edgestat_host(parent, m, S, meta), g["feature_names"])
    names = ["s%d" % s for s in range(S)]
    lines = hostio.edge_stats_table(names, g["feature_names"], r.n_active, r.table, r.feature_table).split("\n")
    assert lines[0] == "#edge_stats\t5\t6\t2\t4" and lines[1] == "#columns\tnode\t" + "\t".join(g["columns"])
    assert lines[2] == "0\t0\t0\t0\tnan\tnan\t0\t0\t0" + "\tnan" * 8   # the root: all ties
    row5 = lines[7].split("\t")
    assert row5[0] == "5" and row5[10] == "1" and row5[12] == "1" and len(row5) == 17 and row5[1] == "%.17g" % r.table[5, 0]
    assert lines[8] == "#features" and lines[9] == "pH\t6.6875\t%.17g" % r.feature_table[0, 1] and lines[10].startswith("depth\t10\t")
    assert lines[11] == "#samples_without_mass\t1" and lines[12] == "" and len(lines) == 13
