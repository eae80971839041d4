"""The two placement drivers, `rk_place` and `python -m rappas_amd.tools.place`, with every sample report asked for at once: each file of
one driver is the other's byte for byte, a report is the same whether the sample masses were summed on the device (--masses-only) or on
the host (--out --masses), and the same whether it is asked for alone or with the other four."""
import os
import subprocess
import sys

import pytest

from rappas_amd import hostio, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300

# the five reports: file name -> its options (the file's path follows the first)
REPORTS = {
    "kr": ["--kr"],
    "sq": ["--squash"],
    "ep": ["--epca", "--epca-components", "3", "--epca-iters", "50"],
    "km": ["--kmeans", "--kmeans-k", "{k}", "--kmeans-rounds", "60"],
    "dv": ["--diversity", "--diversity-theta", "0.5,1"],
}


def report_args(names, k):
    out = []
    for name in names:
        opt = [o.format(k=k) for o in REPORTS[name]]
        out += [opt[0], name] + opt[1:]
    return out


def make_inputs(d):
    """the shapes of test_drivers_kmeans (a tree of 75 nodes, k = 8; 700 records in four samples and one sample without mass) as
    d/db.json and d/q.fasta, and the 700 records in one sample as d/one.fasta"""
    n_nodes = 75
    sdb, genome = synth.make_clade_db(k=8, n_branches=n_nodes, genome_len=12_000, mean_row=6, seed=13)
    nwk = synth.make_newick(n_nodes, seed=6)
    fs, _ = synth.make_clade_reads(genome, 300, 120, seed=10)
    read = lambda i: fs[i * 120:(i + 1) * 120].tobytes().decode()
    records = [(f"{('gut', 'soil', 'sea', 'a,b')[(i * 7 + i // 100) % 4]}_{i}", read(i % 300)) for i in range(700)]
    (d / "one.fasta").write_text("".join(f">gut_{i}\n{s}\n" for i, (_, s) in enumerate(records)))
    records.append(("void_1", "ACG"))  # a sample whose only read is too short to be placed: no mass
    (d / "db.json").write_text(hostio.dump_jsondb(sdb, nwk))
    (d / "q.fasta").write_text("".join(f">{h}\n{s}\n" for h, s in records))


def run(cmd, d, fasta, args):
    """one child in a directory of its own, every path relative to it (the jplace quotes the command line): -> {file name: bytes}.
    A child that fails ends the test: nothing is started after it."""
    d.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd + ["--jsondb", "../db.json", "--fasta", "../" + fasta, "--logs", "."] + args, capture_output=True, text=True, timeout=CHILD_TIMEOUT,
                       cwd=d, env=env)
    assert r.returncode == 0, (cmd, args, r.stderr[-3000:])
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d))}


def three_runs(cmd, d, name):
    """(a) masses-only, (b) placing with --masses, both strands and --edpl, (c) one sample only: all five reports each time"""
    a = run(cmd, d / (name + "_a"), "q.fasta", ["--masses-only", "t", "--sample-sep", "_"] + report_args(REPORTS, 3))
    b = run(cmd, d / (name + "_b"), "q.fasta", ["--out", "o.jplace", "--masses", "t", "--sample-sep", "_", "--strand", "both", "--edpl", "ed"] + report_args(REPORTS, 3))
    c = run(cmd, d / (name + "_c"), "one.fasta", ["--masses-only", "t", "--sample-sep", "_"] + report_args(REPORTS, 1))
    assert sorted(a) == sorted(["t", "notplaced_q.fasta.tsv"] + list(REPORTS))
    assert sorted(b) == sorted(["t", "o.jplace", "ed", "notplaced_q.fasta.tsv", "reversed_q.fasta.tsv"] + list(REPORTS))
    assert sorted(c) == sorted(["t", "notplaced_one.fasta.tsv"] + list(REPORTS))
    return a, b, c


def test_all_reports_at_once_from_both_drivers(tmp_path):
    from rappas_amd import build
    exe = build.build_host_tools()
    make_inputs(tmp_path)
    cpp = three_runs([exe], tmp_path, "cpp")
    py = three_runs([sys.executable, "-m", "rappas_amd.tools.place"], tmp_path, "py")
    for which, c, p in zip("abc", cpp, py):
        for f in c:
            assert c[f] == p[f], (which, f)
    for a, b, _ in (cpp, py):
        for f in REPORTS:  # summed on the device and left there, or summed on the host and uploaded (forward strand or the better one:
            assert a[f] == b[f], f  # these reads are placed from the strand they are given on)
    assert cpp[0]["sq"].startswith(b"#squash\t5\t") and cpp[2]["sq"].startswith(b"#squash\t1\t0\n") and cpp[2]["ep"].startswith(b"#epca\t1\t75\t3\t1\t0\t50\n")
    for f in REPORTS:
        alone = run([exe], tmp_path / ("alone_" + f), "q.fasta", ["--masses-only", "t", "--sample-sep", "_"] + report_args([f], 3))
        assert alone[f] == cpp[0][f] and alone["t"] == cpp[0]["t"], f
