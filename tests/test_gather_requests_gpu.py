"""The gathering walk's row requests (csrc/kernels_prune.h: gather_walk_kernel, issue_rows): list after list, every wave from its first
piece of a list on, the tables' descriptors made once per class of the model.  What can go wrong there is a list's first and last piece
(lists start at any even slot, a wave may have no piece of a list, a list may be one piece) and the change of class between a
workgroup's work items.  PAML_AMD_GATHER_R moves the lists' edges: small R gives tiles of one to a few pieces, R = 70 tiles whose lists
end at other slots than those of the default R = 128 that tests/test_gather_walk_gpu.py runs.  Every case compares the BITS of lnL and of
every per-pattern log f_h with PAML_AMD_GATHER_WALK=0 (the generated walk), computed once per data set in an environment of its own."""
import functools

import numpy as np
import pytest

from test_gather_walk_gpu import case, run

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(name):
    """the generated walk on this data set: its own environment (nothing a test has set reaches it), computed once, read-only"""
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("PAML_AMD_GATHER_R", raising=False)
        off, _, gw0 = run(case(name), mp, "0")
    assert not gw0["in_use"]
    off["lnf"].setflags(write=False)
    return off


def same_bits(name, monkeypatch, R):
    off = reference(name)
    monkeypatch.setenv("PAML_AMD_GATHER_R", str(R))
    got, _, gw = run(case(name), monkeypatch, "1")
    assert gw["in_use"] and gw["R"] == R and gw["tiles"] * 128 >= case(name).n_patt
    assert got["lnL"].hex() == off["lnL"].hex()
    bad = np.flatnonzero(got["lnf"].view(np.uint64) != off["lnf"].view(np.uint64))
    assert bad.size == 0, "log f_h differs at patterns %r" % bad[:10].tolist()
    return gw


@pytest.mark.parametrize("name,R", [("t16", 8), ("t16", 24), ("t16", 70), ("t8_root2", 8), ("t12_root4", 10), ("t12_root4", 70),
                                    ("n60", 24), ("t16_zero_weights", 24)])
def test_same_bits_as_the_generated_walk(monkeypatch, name, R):
    same_bits(name, monkeypatch, R)


@pytest.mark.parametrize("R", [24, 128])
def test_class_changes_between_the_work_items_of_a_workgroup(monkeypatch, R):
    """K = 3, work items (tile, class) class-major, one workgroup per CU, a workgroup's items a whole grid apart.  More items than any GPU
    has CUs (304 at most), so the grid is the CU count and workgroups walk several.  With no more tiles than CUs, two items a grid apart
    are never of one class: the cached table descriptors change at every step of a workgroup.  With more tiles than CUs every workgroup
    has an item in each class's run of tiles and changes class twice, with items of one class between the changes (the small R)."""
    gw = same_bits("t16_m2a", monkeypatch, R)
    assert 3 * gw["tiles"] > 304
