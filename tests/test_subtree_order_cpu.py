"""The pattern order of the walk with subtree tables, the host side (csrc/subtree_classes.h: subtree_pattern_order): a permutation, the
lexicographic sort of the patterns by their classes with ties in pattern order, the same in processes started with different host
thread counts; and the generated
sources — with PAML_AMD_SUBTREE_ORDER=0 the table form is the parent commit's, with PAML_AMD_SUBTREE_TABLES=0 nothing changes."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from paml_amd import engine
from paml_amd.problem import balanced_tree
from test_subtree_tables_cpu import PARENT_SOURCES, _shape


@pytest.fixture(scope="module")
def lib_path():
    return engine.build()


def skewed_keys(n_patt, bounds, seed):
    """class arrays with a few large classes and many small ones, as tabulated nodes have them"""
    rng = np.random.default_rng(seed)
    return np.stack([np.minimum((b * rng.random(n_patt) ** 3).astype(np.uint32), b - 1) for b in bounds])


def brute(keys, seq):
    """sorted() over (key tuple, pattern): what the counting sorts must reproduce"""
    n_patt = keys.shape[1]
    return np.array(sorted(range(n_patt), key=lambda h: tuple(int(keys[k][h]) for k in seq) + (h,)), dtype=np.uint32)


@pytest.mark.parametrize("n_patt", [1, 37, 128 * 3 + 37, 5000])
def test_order_is_the_lexicographic_sort_and_a_permutation(lib_path, n_patt):
    bounds = [700, 9, 61 * 61]
    keys = skewed_keys(n_patt, bounds, seed=n_patt)
    got = engine.debug_subtree_order(keys, bounds)
    assert np.array_equal(np.sort(got), np.arange(n_patt))
    assert np.array_equal(got, brute(keys, [1, 0, 2]))      # smallest table first
    assert np.array_equal(engine.debug_subtree_order(keys, bounds, largest_first=True), brute(keys, [2, 0, 1]))
    assert np.array_equal(engine.debug_subtree_order(keys, bounds, as_given=True), brute(keys, [0, 1, 2]))
    assert np.array_equal(engine.debug_subtree_order(keys, bounds), got)      # deterministic


def test_order_does_not_depend_on_the_host_thread_count(lib_path):
    """Child processes started with OMP_NUM_THREADS = 1 and 7 (the variable has to be there before the library's runtime starts)."""
    code = ("import hashlib, numpy as np\nfrom paml_amd import engine\nrng = np.random.default_rng(3)\n"
            "keys = np.stack([rng.integers(0, b, 20000).astype(np.uint32) for b in (700, 9, 3721)])\n"
            "print(hashlib.sha256(engine.debug_subtree_order(keys, [700, 9, 3721]).tobytes()).hexdigest())")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = [subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, OMP_NUM_THREADS=n), capture_output=True, text=True, timeout=120)
           for n in ("1", "7")]
    assert all(g.returncode == 0 for g in got), got[0].stderr[-2000:] + got[1].stderr[-2000:]
    assert got[0].stdout == got[1].stdout and len(got[0].stdout.strip()) == 64


def test_ties_keep_the_pattern_order(lib_path):
    keys = np.array([[2, 0, 2, 0, 1, 2, 0]], dtype=np.uint32)
    assert engine.debug_subtree_order(keys, [3]).tolist() == [1, 3, 6, 4, 0, 2, 5]
    same = np.zeros((2, 50), dtype=np.uint32)
    assert engine.debug_subtree_order(same, [1, 4]).tolist() == list(range(50))
    # equal table sizes: the keys in the order given
    keys = skewed_keys(300, [20, 20], seed=2)
    assert np.array_equal(engine.debug_subtree_order(keys, [20, 20]), brute(keys, [0, 1]))
    assert np.array_equal(engine.debug_subtree_order(keys, [20, 20], largest_first=True), brute(keys, [0, 1]))


def test_single_key_is_a_stable_argsort(lib_path):
    key = skewed_keys(4000, [300], seed=11)
    assert np.array_equal(engine.debug_subtree_order(key, [300]), np.argsort(key[0], kind="stable").astype(np.uint32))
    assert engine.debug_subtree_order(np.zeros((0, 5), dtype=np.uint32), []).tolist() == [0, 1, 2, 3, 4]      # no key: the identity


def test_a_class_beyond_its_bound_is_refused(lib_path):
    with pytest.raises(engine.EngineError):
        engine.debug_subtree_order(np.array([[0, 3, 1]], dtype=np.uint32), [3])


# sha256 (first 16 hex digits) of the table form's source as the parent commit generates it (engine.debug_jit_subtree of a parent build):
# the alignment's order must give these very kernels
PARENT_TABLE_FORM = {
    "none_left": (16, [18, 21, 24, 27, 17], 61, "dac1232a0023cd56"),
    "one_left": (32, [35, 38, 42, 45, 49, 52, 56, 59, 34, 41, 48, 55], 61, "4a67f3345f591ee6"),
    "five_left": (32, [35, 38, 42, 45, 49, 52, 56, 59], 61, "d7d9f2297bbdd41b"),
    "level1_60": (16, [18, 21, 24, 27], 60, "cf5c95895f7346ba"),
    "none_left_64": (16, [18, 21, 24, 27, 17], 64, "c181068524272dd8"),
}


@pytest.mark.parametrize("shape", sorted(PARENT_TABLE_FORM))
def test_table_form_without_the_order_is_the_parents(lib_path, shape, monkeypatch):
    n_tips, nodes, n, want = PARENT_TABLE_FORM[shape]
    monkeypatch.setenv("PAML_AMD_SUBTREE_ORDER", "0")
    off, _ = engine.debug_jit_subtree(balanced_tree(n_tips), nodes, n, n, compile=False)
    assert hashlib.sha256(off.encode()).hexdigest()[:16] == want
    monkeypatch.setenv("PAML_AMD_SUBTREE_ORDER", "1")
    on, _ = engine.debug_jit_subtree(balanced_tree(n_tips), nodes, n, n, compile=False)
    # with the order: the position -> pattern load at the tile's head, and the root stores there; nothing else differs
    assert on.count("JIT2_ORDER()") == 1 and on.count(", hs, valid);") == 1
    assert on.replace("   JIT2_ORDER()\n", "").replace(", hs, valid);", ", h, valid);") == off


@pytest.mark.parametrize("shape", ["balanced16", "hiv", "random23"])
@pytest.mark.parametrize("order", ["0", "1"])
def test_sources_without_subtree_tables_do_not_depend_on_the_order(lib_path, shape, order, monkeypatch):
    monkeypatch.setenv("PAML_AMD_SUBTREE_TABLES", "0")
    monkeypatch.setenv("PAML_AMD_SUBTREE_ORDER", order)
    tree, scale = _shape(shape)
    plain = engine.debug_jit(tree, scale_node=scale, compile=False)
    tables = engine.debug_jit_tables(tree, scale_node=scale)[0]
    got = (hashlib.sha256(plain.encode()).hexdigest()[:16], hashlib.sha256(tables.encode()).hexdigest()[:16])
    assert got == PARENT_SOURCES[shape]


def test_table_form_with_the_order_compiles_for_gfx950(lib_path):
    src, left = engine.debug_jit_subtree(balanced_tree(32), [35, 38, 42, 45, 49, 52, 56, 59], compile=True)      # the ring form
    assert left == 5 and "#error" not in src and "JIT2_ORDER()" in src
