"""The gathering walk, the host side (csrc/gather_tiles.h): the tiles with their distinct rows, through paml_amd_debug_gather_tiles, against a
brute-force recount in numpy — every position once and in order, at most 128 patterns and R rows per tile, every slot at the pattern's own
row, no row twice in a list, the greedy cut —, and the generated walk's sources, which the switch must leave what they were."""
import hashlib

import numpy as np
import pytest

from paml_amd import engine
from paml_amd.problem import balanced_tree
from test_subtree_order_cpu import PARENT_TABLE_FORM, skewed_keys


@pytest.fixture(scope="module")
def lib_path():
    return engine.build()


def recount(keys, order, wflag, R, tiles, n_rows):
    nk, n_patt = keys.shape
    order = np.arange(n_patt) if order is None else order
    nxt, total = 0, 0
    for t in tiles:
        assert t["first"] == nxt and 1 <= t["count"] <= 128
        patt = order[nxt:nxt + t["count"]]
        assert np.array_equal(t["patt"], patt)
        assert np.array_equal(t["flag"], wflag[patt]) and not t["flag_tail"].any()
        distinct = 0
        for k in range(nk):
            own = keys[k][patt]
            n = int(t["slot"][k].max()) + 1
            lst = np.array(t["rows"][k])
            assert len(lst) == (n + 1) // 2 * 2 and (n % 2 == 0 or lst[n] == lst[n - 1])      # an odd list: its last row once more
            lst = lst[:n]
            assert len(set(lst.tolist())) == n and set(lst.tolist()) == set(own.tolist())       # no row twice, nothing but the tile's rows
            assert t["slot"][k].min() >= 0 and np.array_equal(lst[t["slot"][k]], own)           # every slot at the pattern's own row
            assert np.all(t["slot_tail"][k] == t["start"][k])
            distinct += n
        assert distinct <= R
        nxt += t["count"]
        total += distinct
        if nxt < n_patt and t["count"] < 128:      # greedy: the next pattern would have taken the tile past R
            fresh = sum(int(keys[k][order[nxt]] not in set(keys[k][patt].tolist())) for k in range(nk))
            assert distinct + fresh > R
    assert nxt == n_patt and total == n_rows


@pytest.mark.parametrize("n_patt", [1, 127, 128, 129, 128 * 5 + 37])
@pytest.mark.parametrize("R", [128, 96, 8])
def test_tiles_against_a_recount(lib_path, n_patt, R):
    bounds = [700, 9, 61 * 61]
    keys = skewed_keys(n_patt, bounds, seed=n_patt + R)
    rng = np.random.default_rng(n_patt)
    wflag = (rng.random(n_patt) < 0.8).astype(np.uint8)
    order = engine.debug_subtree_order(keys, bounds)
    for o in (order, None):
        tiles, n_rows = engine.debug_gather_tiles(keys, bounds, order=o, wflag=wflag, R=R)
        recount(keys, o, wflag, R, tiles, n_rows)


def test_a_table_with_one_row_and_all_rows_distinct(lib_path):
    n = 128 * 5 + 37
    one = np.stack([np.zeros(n, dtype=np.uint32), skewed_keys(n, [50], seed=1)[0]])
    tiles, n_rows = engine.debug_gather_tiles(one, [1, 50])
    recount(one, None, np.ones(n, dtype=np.uint8), 128, tiles, n_rows)
    assert [t["count"] for t in tiles] == [128] * 5 + [37] and all(t["rows"][0] == [0, 0] for t in tiles)
    every = np.stack([np.arange(n, dtype=np.uint32)] * 3)      # three rows per pattern: R = 128 cuts after 42 patterns
    tiles, n_rows = engine.debug_gather_tiles(every, [n, n, n])
    recount(every, None, np.ones(n, dtype=np.uint8), 128, tiles, n_rows)
    assert n_rows == 3 * n and [t["count"] for t in tiles] == [42] * 16 + [n - 42 * 16]


def test_bad_arguments_are_refused(lib_path):
    keys = np.zeros((2, 10), dtype=np.uint32)
    for kw in (dict(R=1), dict(R=161), dict(order=np.zeros(10, dtype=np.uint32))):
        with pytest.raises(engine.EngineError):
            engine.debug_gather_tiles(keys, [1, 1], **kw)
    with pytest.raises(engine.EngineError):
        engine.debug_gather_tiles(keys + 1, [1, 1])


@pytest.mark.parametrize("shape", sorted(PARENT_TABLE_FORM))
def test_generated_walk_with_the_switch_off_is_the_parents(lib_path, shape, monkeypatch):
    """with PAML_AMD_GATHER_WALK=0 and the alignment's order the table form's source hashes to the values test_subtree_order_cpu.py holds:
    this change did not touch the generator.  (The generator does not read the switch, so this cannot show that the engine acquires the
    fallback unchanged; test_gather_walk_gpu.py's flip test, which runs both kernels on one engine, does.)"""
    n_tips, nodes, n, want = PARENT_TABLE_FORM[shape]
    monkeypatch.setenv("PAML_AMD_GATHER_WALK", "0")
    monkeypatch.setenv("PAML_AMD_SUBTREE_ORDER", "0")
    src, _ = engine.debug_jit_subtree(balanced_tree(n_tips), nodes, n, n, compile=False)
    assert hashlib.sha256(src.encode()).hexdigest()[:16] == want
