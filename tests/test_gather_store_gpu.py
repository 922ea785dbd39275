"""The gathering walk's deferred result store (csrc/kernels_prune.h: gather_walk_kernel, store_out): a tile's value leaves the workgroup at
the head of the NEXT stage, the last one behind the loop, with its own pattern, class and predicate carried across the barrier.  What can
go wrong there is a store that is missed or goes out with another tile's index or class.  Every case therefore evaluates ONE engine twice
— first at branch lengths scaled by 1.3, then at the case's own — and compares the BITS of the second evaluation's lnL and of every
per-pattern log f_h with PAML_AMD_GATHER_WALK=0 (the generated walk) on the same data: a slot the second evaluation did not write, or
wrote elsewhere, still holds the first one's value.  The reference is computed once per data set in an environment of its own."""
import functools

import numpy as np
import pytest

from paml_amd.engine import engine_for
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


def twice_same_bits(name, monkeypatch, R=None):
    off = reference(name)
    pb = case(name)
    if R is None:
        monkeypatch.delenv("PAML_AMD_GATHER_R", raising=False)
    else:
        monkeypatch.setenv("PAML_AMD_GATHER_R", str(R))
    monkeypatch.setenv("PAML_AMD_JIT", "1")
    monkeypatch.setenv("PAML_AMD_CHERRY_TABLES", "1")
    monkeypatch.setenv("PAML_AMD_SUBTREE_TABLES", "1")
    monkeypatch.setenv("PAML_AMD_GATHER_WALK", "1")
    eng = engine_for(pb)
    first = eng.eval(pb.tree.branch * 1.3, pb.gene_rate, want_lnf=True)
    got = eng.eval(pb.tree.branch, pb.gene_rate, want_lnf=True)
    gw, kname = eng.gather_walk(), eng.kernel_name
    eng.close()
    assert kname == "mfma64_jit" and gw["in_use"] and gw["n_computed"] == 1 and gw["R"] == (128 if R is None else R)
    assert np.isfinite(first["lnL"]) and first["lnL"].hex() != off["lnL"].hex()      # (the first evaluation really left other values)
    assert got["lnL"].hex() == off["lnL"].hex()
    bad = np.flatnonzero(got["lnf"].view(np.uint64) != off["lnf"].view(np.uint64))
    assert bad.size == 0, "log f_h differs at patterns %r" % bad[:10].tolist()
    return gw


def test_one_work_item_per_workgroup_the_store_behind_the_loop(monkeypatch):
    """two tiles, two workgroups of one item each: the only store is the one behind the loop; the last tile holds one pattern, so seven of
    its eight waves have nothing to store and the predicate has to travel with the value"""
    gw = twice_same_bits("t16_129", monkeypatch)
    assert gw["tiles"] == 2


@pytest.mark.parametrize("R", [24, 128])
def test_class_changes_between_consecutive_items(monkeypatch, R):
    """K = 3, more (tile, class) items than any GPU has CUs: the store of an item of class k goes out while the registers already describe an
    item of class k + 1"""
    gw = twice_same_bits("t16_m2a", monkeypatch, R)
    assert 3 * gw["tiles"] > 304


@pytest.mark.parametrize("name,R", [("t16", 8),                  # many stages per workgroup, tiles of one to four pieces
                                    ("t16_zero_weights", 24),    # the flag travels with the value
                                    ("n60", 24),                 # 60 states
                                    ("t8_root2", 8),             # two lookups
                                    ("t12_root4", 10)])          # four lookups
def test_same_bits_on_the_second_evaluation(monkeypatch, name, R):
    twice_same_bits(name, monkeypatch, R)
