"""GPU (-m gpu): rk_kernel_name of one small handle per launch family, compared byte for byte with tests/golden/kernel_names.json -- the
strings the library gave on the MI355X before the launch geometry moved into rappas_amd/csrc/rk_geometry.h.  They carry lds/wave, cap,
waves/CU, main, work, windows and passes as the engine computes them from the LDS size the device reports, so they pin the geometry on the
device the way tests/test_geometry_grid.py pins it on the host.  A case is a handle build and a string compare."""
import json
import os

import pytest

import rappas_amd as ra
from rappas_amd import synth

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_names.json")) as f:
    GOLDEN = json.load(f)

C1 = lambda: synth.make_config_db("C1")                                     # 99 branches: the dense 16-lane kernel on the dense-row view
C2 = lambda: synth.make_config_db("C2", scale=0.2)                          # 999 branches, rows too sparse for the view
C4 = lambda: synth.make_config_db("C4", scale=0.2)                          # amino acids
MID = lambda: synth.make_db(4, 8, 4001, 30000, 400000, seed=2)              # windowed, below the sorted-stream kernel's 4 500 branches
T8K = lambda: synth.make_db(4, 8, 7999, 40000, 520000, seed=7999)           # windowed, short rows: the sorted-stream kernel first
T40K = lambda: synth.make_db(4, 8, 40001, 50000, 650000, seed=40002)        # ... beyond the uniform crossing: the hash kernel first
P3K = lambda: synth.make_db(20, 3, 3100, 6000, 60000, seed=6)               # amino acids, windowed
P20K = lambda: synth.make_db(20, 3, 20001, 7000, 80000, seed=20002)         # ... a larger tree (the hash kernel by RK_HASH_ALWAYS)
WG = lambda: synth.make_db(4, 6, 19999, 3000, 1_200_000, seed=5)            # rows of ~400 entries: the workgroup-per-read kernel
PWG = lambda: synth.make_db(20, 3, 19999, 3000, 1_200_000, seed=5)          # ... amino acids

# name -> (database, lanes_per_read, developer knobs, what the family's string starts with)
CASES = {
    "dense16_row24": (C1, 0, {}, "place_packed16_kernel<G=16,BITS=2,DIRECT4,ROW24,"),
    "dense16_canonical": (C1, 0, {"RK_NO_DENSE_UNITS": "1"}, "place_packed16_kernel<G=16,BITS=2,DIRECT4,ITEM32"),
    "dense16_sparse_rows": (C2, 0, {}, "place_packed16_kernel<G=16,BITS=2,DIRECT,ITEM32"),
    "dense16_protein": (C4, 0, {}, "place_packed16_kernel<G=16,BITS=5"),
    "lanes8": (C2, 8, {}, "place_packed_kernel<G=8,"),
    "lanes32": (C2, 32, {}, "place_packed_kernel<G=32,"),
    "lanes64": (C2, 64, {}, "place_packed_kernel<G=64,"),
    "lanes32_windowed_tree": (T8K, 32, {}, "place_packed_kernel<G=32,"),
    "windowed16w": (MID, 0, {}, "place_packed16w_kernel<BITS=2"),
    "windowed16w_large": (T40K, 0, {"RK_NO_WSTREAM": "1"}, "place_packed16w_kernel<BITS=2"),
    "sorted": (T8K, 0, {}, "place_packed16s_kernel<BITS=2"),
    "sorted_protein": (P3K, 0, {}, "place_packed16s_kernel<BITS=5"),
    "hash_big": (T40K, 0, {}, "place_hash64_kernel<BITS=2"),
    "hash_small": (T40K, 0, {"RK_HASH_SMALL_TABLE": "1"}, "place_hash64_kernel<BITS=2"),
    "hash_protein": (P20K, 0, {"RK_HASH_ALWAYS": "1"}, "place_hash64_kernel<BITS=5"),
    "wg": (WG, 0, {}, "place_wg_kernel<BITS=2"),
    "wg_passes2": (WG, 0, {"RK_WG_PASSES": "2"}, "place_wg_kernel<BITS=2"),
    "wg_protein": (PWG, 0, {}, "place_wg_kernel<BITS=5"),
}


def name_of(case):
    make, lanes, _, _ = CASES[case]
    db = ra.PhyloKmerDB.from_synth(make())
    try:
        if lanes:
            db.set_lanes_per_read(lanes)
        return db.kernel_name()
    finally:
        db.close()


def check(case):
    got = name_of(case)
    assert got.startswith(CASES[case][3]), got   # (the case still selects the family it is here for)
    assert got == GOLDEN[case], (got, GOLDEN[case])


@pytest.mark.parametrize("case", [c for c in CASES if not CASES[c][2]])
def test_kernel_name_is_the_recorded_one(case):
    check(case)


@pytest.mark.parametrize("case", [c for c in CASES if CASES[c][2]])
def test_kernel_name_under_a_developer_knob_is_the_recorded_one(case, monkeypatch, dev_lib):
    for knob, value in CASES[case][2].items():
        monkeypatch.setenv(knob, value)
    check(case)
