"""The option rules of the two placement drivers, `rk_place` and `python -m rappas_amd.tools.place`: a command line that breaks a rule
exits 2 with the rule's sentence before any file or the device is opened (the database and the FASTA named here do not exist), and
writes none of the files it names.  One table of command lines serves both drivers."""
import os
import subprocess
import sys

import pytest

from rappas_amd import build
from rappas_amd.tools import place as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONLY = ["--masses-only", "{t}", "--sample-sep", "_"]

# (id, arguments after --jsondb / --fasta -- "{x}" is a path under the test's directory --, the sentence)
RULES = [
    ("masses_only_with_masses", ["--masses-only", "{t}", "--masses", "{m}"], P.MASSES_ONLY_WITH_MASSES),
    ("masses_only_with_out", ["--masses-only", "{t}", "--out", "{o}"], P.MASSES_ONLY_WITH_OUT),
    ("edpl_without_out", ["--masses-only", "{t}", "--edpl", "{e}"], P.EDPL_NEEDS_OUT),
    ("sample_sep_without_masses", ["--out", "{o}", "--sample-sep", "_"], P.SAMPLE_SEP_NEEDS_MASSES),
    ("sample_sep_of_two", ["--masses-only", "{t}", "--sample-sep", "__"], "--sample-sep takes one character"),
    ("kr_without_sample_sep", ["--masses-only", "{t}", "--kr", "{r}"], P.KR_NEEDS_SAMPLE_SEP),
    ("squash_without_sample_sep", ["--masses-only", "{t}", "--squash", "{r}"], P.SQUASH_NEEDS_SAMPLE_SEP),
    ("epca_without_sample_sep", ["--masses-only", "{t}", "--epca", "{r}"], P.EPCA_NEEDS_SAMPLE_SEP),
    ("kmeans_without_sample_sep", ["--masses-only", "{t}", "--kmeans", "{r}", "--kmeans-k", "3"], P.KMEANS_NEEDS_SAMPLE_SEP),
    ("diversity_without_sample_sep", ["--masses-only", "{t}", "--diversity", "{r}"], P.DIVERSITY_NEEDS_SAMPLE_SEP),
    ("epca_components_0", ONLY + ["--epca", "{r}", "--epca-components", "0"], P.EPCA_RANGES),
    ("epca_components_9", ONLY + ["--epca", "{r}", "--epca-components", "9"], P.EPCA_RANGES),
    ("epca_iters_0", ONLY + ["--epca", "{r}", "--epca-iters", "0"], P.EPCA_RANGES),
    ("kmeans_without_k", ONLY + ["--kmeans", "{r}"], P.KMEANS_RANGES),
    ("kmeans_k_65", ONLY + ["--kmeans", "{r}", "--kmeans-k", "65"], P.KMEANS_RANGES),
    ("kmeans_rounds_0", ONLY + ["--kmeans", "{r}", "--kmeans-k", "3", "--kmeans-rounds", "0"], P.KMEANS_RANGES),
    ("nine_thetas", ONLY + ["--diversity", "{r}", "--diversity-theta", "0,1,2,3,4,5,6,7,8"], P.DIVERSITY_RANGES),
    ("theta_8_5", ONLY + ["--diversity", "{r}", "--diversity-theta", "1,8.5"], P.DIVERSITY_RANGES),
    ("empty_theta_item", ONLY + ["--diversity", "{r}", "--diversity-theta", "1,,2"], P.DIVERSITY_RANGES),
    ("translate_with_strand_rev", ["--out", "{o}", "--translate", "--strand", "rev"], P.TRANSLATE_WITH_STRAND),
]

# two rules broken at once: (id, arguments, the sentence rk_place reports, the sentence the Python tool reports) -- each driver runs
# its checks in an order of its own, and the first rule that fires is the one reported
TWO_RULES = [
    ("kr_without_sample_sep_and_edpl_without_out", ["--masses-only", "{t}", "--kr", "{r}", "--edpl", "{e}"], P.EDPL_NEEDS_OUT, P.KR_NEEDS_SAMPLE_SEP),
    ("translate_with_strand_and_masses_only_with_out", ["--masses-only", "{t}", "--out", "{o}", "--translate", "--strand", "both"],
     P.MASSES_ONLY_WITH_OUT, P.TRANSLATE_WITH_STRAND),
]

CASES = [(i, a, s, s) for i, a, s in RULES] + TWO_RULES


@pytest.fixture(scope="module")
def rk_place():
    return build.build_host_tools()


@pytest.mark.parametrize("args,cpp_sentence,py_sentence", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_a_broken_rule_exits_2_with_its_sentence_and_writes_nothing(rk_place, tmp_path, args, cpp_sentence, py_sentence):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for name, cmd, sentence in (("cpp", [rk_place], cpp_sentence), ("py", [sys.executable, "-m", "rappas_amd.tools.place"], py_sentence)):
        d = tmp_path / name
        d.mkdir()
        paths = {x: str(d / x) for x in "tmoer"}
        r = subprocess.run(cmd + ["--jsondb", str(d / "no_such_db.json"), "--fasta", str(d / "no_such.fasta")] + [a.format(**paths) for a in args],
                           capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
        assert r.returncode == 2, (name, r.returncode, r.stderr[-2000:])
        assert sentence in r.stderr, (name, r.stderr[-2000:])
        assert os.listdir(d) == [], name  # neither an output file nor a logs directory
