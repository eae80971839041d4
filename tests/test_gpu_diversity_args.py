"""The cases of test_diversity_args.py that need a tree handle: what rk_diversity_device, rk_diversity_batch and
rk_diversity_work_bytes answer to one bad argument -- return code and the whole text --, and the workspace size item
by item.  Every refused call fails before anything is launched; the sizes launch and allocate nothing."""
import numpy as np
import pytest

import rappas_amd as ra
from rappas_amd import _lib, synth
from rappas_amd._lib import RK_ERR_INVALID
from tests import kr_ref as R
from tests import test_diversity_args as D
from tests import test_samples_args as A

pytestmark = pytest.mark.gpu


def work_bytes(B, S, n_theta):
    """The workspace of rk_diversity_device, item by item:
        clade     S * B 64-bit words, the clade sums of every sample, sample-major
        partials  S * ceil(B / 2048) * (5 + 2 n_theta) doubles, a row of columns for every (sample, chunk)
    both 8-byte items laid end to end, the whole rounded up to 16 bytes."""
    clade = S * B * 8
    partials = S * -(-B // 2048) * (5 + 2 * n_theta) * 8
    return -(-(clade + partials) // 16) * 16


def test_workspace_sizes_item_by_item():
    lib = _lib.load()
    for B in (1, 2049, 65535):
        et = ra.EdgeTree(*R.random_tree(B, B))
        try:
            for S in (1, 65, 65535):
                for n_theta in (0, 8):
                    assert int(lib.rk_diversity_work_bytes(et.handle, S, n_theta)) == work_bytes(B, S, n_theta) == et.diversity_work_bytes(S, n_theta), (B, S, n_theta)
        finally:
            et.close()


class Device:
    """a valid device call's arguments: the tree of test_samples_args.py and one of six nodes, a database of five branches, the arrays
    on the device as addresses, the exact workspace"""

    def __init__(self):
        import torch
        v = D.values()
        self.tree = ra.EdgeTree(v["parent"], v["bl"])
        self.tree6 = ra.EdgeTree(np.array([-1, 0, 0, 2, 2, 1], np.int32), np.array([0, 1, 3, 2, 4, 1], np.float32))
        self.db = ra.PhyloKmerDB.from_synth(synth.make_db(4, 6, A.B, 40, 80, seed=1), device=0)
        self.masses = torch.from_numpy(v["masses"].view(np.int64)).cuda()
        self.out = torch.full((D.S * 9,), 7.0, dtype=torch.float64, device="cuda")
        self.work = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda")
        self.need = work_bytes(A.B, D.S, D.N_THETA)

    def base(self, call):
        if call.endswith("_batch"):
            return dict(db=self.db.handle, tree=self.tree.handle)
        return dict(tree=self.tree.handle, masses=self.masses.data_ptr(), out=self.out.data_ptr(), work=self.work.data_ptr(), work_bytes=self.need)

    def close(self):
        self.tree.close()
        self.tree6.close()
        self.db.close()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


def refused(d):
    thetas = [(c, t) for c, t in D.BAD_THETAS if "out" not in c] + [(dict(n_theta=9, theta=np.zeros(9)), D.N_THETA_RANGE)]
    sizer = "rk_diversity_work_bytes"
    return {
        "rk_diversity_device": [
            (dict(tree=None), "null tree"), (dict(S=0), D.SAMPLES % 0), (dict(S=65536), D.SAMPLES % 65536),
            (dict(masses=None), "null mass buffer"), (dict(out=None), "null output"), (dict(out=d.out.data_ptr() + 4), "the doubles must be 8-byte aligned"),
            (dict(work=None), f"workspace of 0 bytes, {d.need} needed ({sizer})"),
            (dict(work_bytes=d.need - 1), f"workspace of {d.need - 1} bytes, {d.need} needed ({sizer})"),
            (dict(work=d.work.data_ptr() + 8), "the workspace must be 16-byte aligned")] + thetas,
        "rk_diversity_batch": [
            (dict(db=None), "null handle"), (dict(tree=None), "null tree"), (dict(S=0), D.SAMPLES % 0), (dict(S=65536), D.SAMPLES % 65536),
            (dict(out=None), "null output"), (dict(tree=d.tree6.handle), "the tree has 6 branches on device 0, the database 5 on device 0"),
            (dict(masses=None), "the handle holds the buffer of 0 samples, not of 3 (the last per-sample profile-only call leaves it)")] + thetas,
    }


@pytest.mark.parametrize("call", ["rk_diversity_device", "rk_diversity_batch"])
def test_one_bad_argument_is_refused_with_its_text(dev, call):
    import torch
    for i, (change, text) in enumerate(refused(dev)[call]):
        rc, msg, v = D.run(_lib.load(), call, change, dev.base(call))
        assert (rc, msg) == (RK_ERR_INVALID, f"{call}: {text}"), (i, change)
        if call.endswith("_batch") and isinstance(v["out"], np.ndarray):
            assert (v["out"] == 7.0).all(), (i, change)
    torch.cuda.synchronize()
    assert (dev.out == 7.0).all() and (dev.work == 0x5A).all()  # nothing was launched, nothing written


def test_the_valid_calls_the_cases_start_from_are_accepted(dev):
    import torch
    want = ra.diversity_host(D.values()["parent"], D.values()["bl"], D.values()["masses"], D.S, (0.25, 1.0)).values
    rc, msg, v = D.run(_lib.load(), "rk_diversity_batch", {}, dev.base("rk_diversity_batch"))
    assert rc == _lib.RK_OK and (R.bits(v["out"].reshape(D.S, 9)) == R.bits(want)).all()
    out = torch.full((D.S * 9,), 7.0, dtype=torch.float64, device="cuda")
    rc, msg, _ = D.run(_lib.load(), "rk_diversity_device", dict(out=out.data_ptr()), dev.base("rk_diversity_device"))
    torch.cuda.synchronize()
    assert rc == _lib.RK_OK and (R.bits(out.cpu().numpy().reshape(D.S, 9)) == R.bits(want)).all()


def test_a_size_out_of_range_is_zero_with_its_text(dev):
    call = "rk_diversity_work_bytes"
    for change, text in ((dict(S=0), D.SAMPLES % 0), (dict(S=65536), D.SAMPLES % 65536), (dict(n_theta=9), D.N_THETA_RANGE)):
        assert D.run(_lib.load(), call, change, dict(tree=dev.tree.handle))[:2] == (0, f"{call}: {text}"), change
    assert D.run(_lib.load(), call, {}, dict(tree=dev.tree.handle))[0] == dev.need
