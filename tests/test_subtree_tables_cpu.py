"""Subtree tables, the host side (csrc/subtree_classes.h, jit.h: SubtreeProgram): the classes of the patterns below every internal node
against numpy.unique, the table form's generated source for no, one and five operand blocks left per tile (compiled for gfx950), and
the source without subtree tables, which must stay what it was."""
import hashlib
import re

import numpy as np
import pytest

import helpers
from paml_amd import engine, synth
from paml_amd.problem import balanced_tree, parse_newick


@pytest.fixture(scope="module")
def lib_path():
    return engine.build()


def tips_below(tree):
    ptr, flat = tree.csr()
    below = {}

    def walk(v):
        if v < tree.n_tips and v != tree.root:
            below[v] = [v]
        else:
            below[v] = [t for s in flat[ptr[v]:ptr[v + 1]] for t in walk(int(s))]
        return below[v]
    walk(tree.root)
    return below


def numpy_counts(pb):
    """node -> number of distinct columns of the tips below it, for every internal node below the root"""
    below = tips_below(pb.tree)
    return {v: len(np.unique(pb.z[below[v]], axis=1).T) for v in range(pb.tree.n_tips, pb.tree.n_nodes) if v != pb.tree.root}


# (the counts the issue lists for these shapes: the seeded data of synth.codon_m0_problem)
LISTED = {(16, 40000): {18: 5465, 21: 5410, 24: 5393, 27: 5334, 17: 16494}, (32, 40000): {}, (12, 40000): {13: 10890}}


@pytest.mark.parametrize("shape", sorted(LISTED))
def test_class_counts_match_numpy_unique(lib_path, shape):
    pb = synth.codon_m0_problem(n_tips=shape[0], n_patt=shape[1])
    u, cls = engine.debug_subtree_classes(pb.tree, pb.z, pb.n_codes, want_classes=True)
    want = numpy_counts(pb)
    got = {v: int(u[v]) for v in want}
    assert got == want
    assert all(u[v] == 0 for v in range(pb.tree.n_nodes) if v not in want)
    for v, n in LISTED[shape].items():
        assert got[v] == n
    if shape[0] == 32:
        assert all(15000 < got[v] < 18000 for v in (34, 41, 48, 55))
    if shape[0] == 12:
        assert all(2500 < got[v] < 3300 for v in (14, 16, 18, 20))
    # the classes themselves: two patterns share a class at v exactly when their columns below v agree, and the classes of a node that is
    # not a cherry are dense ranks in order of first occurrence
    below = tips_below(pb.tree)
    ptr, flat = pb.tree.csr()
    for v in want:
        _, inv = np.unique(pb.z[below[v]], axis=1, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        pairs = np.unique(np.stack([inv, cls[v].astype(np.int64)]), axis=1)
        assert pairs.shape[1] == want[v]
        sons = flat[ptr[v]:ptr[v + 1]]
        if len(sons) == 2 and all(s < pb.tree.n_tips for s in sons):
            assert np.array_equal(cls[v], pb.z[sons[0]].astype(np.uint32) * pb.n_codes + pb.z[sons[1]])
        else:
            _, first = np.unique(cls[v], return_index=True)
            assert np.array_equal(cls[v][np.sort(first)], np.arange(want[v]))


@pytest.mark.parametrize("case", ["none_left", "one_left", "five_left"])
def test_table_form_compiles_for_gfx950(lib_path, case):
    """The generated source with 0, 1 and 5 operand blocks left per tile: the short forms (no ring traffic at all; the ring never more than
    a tile ahead) and the ring form."""
    if case == "none_left":
        tree, nodes, left = balanced_tree(16), [18, 21, 24, 27, 17], 0
    elif case == "one_left":
        tree, nodes, left = balanced_tree(32), [35, 38, 42, 45, 49, 52, 56, 59, 34, 41, 48, 55], 1
    else:
        tree, nodes, left = balanced_tree(32), [35, 38, 42, 45, 49, 52, 56, 59], 5
    src, got = engine.debug_jit_subtree(tree, nodes, compile=True)
    assert got == left and "#error" not in src
    loop = src[src.index("for (;; ptile = 0)"):]
    n_top = loop.count("jit_lookup_row(")
    assert n_top == {"none_left": 3, "one_left": 4, "five_left": 8}[case]
    assert loop.count("jit_matvec") == {"none_left": 0, "one_left": 1, "five_left": 5}[case]
    assert "jit_lookup(" not in loop      # every cherry lies below a tabulated node
    if left == 0:
        assert "JIT2_PIECE" not in src and "JIT_SYNC" not in src
    # the class indices are rows of the code block behind the weight flags, three per lookup
    rows = [int(m) for m in re.findall(r"JIT2_N?IDX\(\d+, (\d+)\)", loop)]
    assert sorted(set(rows)) == [tree.n_tips + 1 + 3 * k for k in range(n_top)]


def test_a_node_that_cannot_be_tabulated_is_refused(lib_path):
    tree = balanced_tree(16)
    assert engine.debug_jit_subtree(tree, [17], compile=False) == ("", None)          # its sons are not tabulated
    assert engine.debug_jit_subtree(tree, [18, 16], compile=False) == ("", None)      # the root
    assert engine.debug_jit_subtree(tree, [19], compile=False) == ("", None)          # a cherry: the cherry tables' business
    t9 = helpers.random_problem(61, 9, 10, seed=309).tree      # four cherries, of which the cherry tables take three (four operand blocks must stay)
    ptr, flat = t9.csr()
    left_out = [v for v in range(9, t9.n_nodes) if v != t9.root and all(x < 9 for x in flat[ptr[v]:ptr[v + 1]]) and ptr[v + 1] - ptr[v] == 2
                and v not in [c[2] for c in engine.debug_jit_tables(t9)[2]]]
    assert left_out == [15]
    assert engine.debug_jit_subtree(t9, [15], compile=False) == ("", None)
    scale = np.zeros(tree.n_nodes, dtype=np.uint8)
    scale[18] = 1
    assert engine.debug_jit_subtree(tree, [18], compile=False, scale_node=scale) == ("", None)      # a rescaled node stays a product
    src, left = engine.debug_jit_subtree(tree, [21], compile=False, scale_node=scale)
    assert left == 4 and "jit_scale(" in src      # (five with cherry tables alone)


# sha256 (first 16 hex digits) of the sources of the per-tree kernel without tables and with cherry tables only, as generated before the
# subtree tables existed: switching them off must give these very kernels
PARENT_SOURCES = {
    "balanced16": ("df3f4fab7e61a04f", "a27dbc11cab39dac"),
    "balanced8": ("bfc0d7ebea4e50df", "801aa8ae05968745"),
    "hiv": ("0cb3c8691e244fec", "1fe9944bab86aa3e"),
    "caterpillar": ("178039f21b221fae", "9eb4d6cc1ce3eb66"),
    "random23": ("2c22abfe4a84cc1c", "abe5e623b2b61411"),
    "scaled": ("a8dc72c5516279ef", "0201b80b56a18efb"),
    "random120": ("d4a1e941aafaaaa4", "e3b0c44298fc1c14"),
    "random200": ("2135a103f5d3c4d1", "e3b0c44298fc1c14"),
    "balanced128": ("02ac2922342a9cca", "e3b0c44298fc1c14"),
}


def _shape(shape):
    scale = None
    if shape.startswith("balanced"):
        tree = balanced_tree(int(shape[8:]))
    elif shape == "hiv":
        tree = helpers.problem_from_golden(helpers.load_golden("hiv_m0")).tree
    elif shape == "caterpillar":
        s = "(t1:0.1,t2:0.1)"
        for i in range(3, 12):
            s = "(%s:0.05,t%d:0.1)" % (s, i)
        tree = parse_newick("(%s:0.05,t12:0.1,t13:0.1);" % s)
    elif shape in ("random120", "random200"):
        tree = helpers.random_problem(61, int(shape[6:]), 10, seed=7).tree
    else:
        pb = helpers.random_problem(61, 23, 10, seed=5, scale_every=6 if shape == "scaled" else None)
        tree, scale = pb.tree, pb.scale_node
    return tree, scale


@pytest.mark.parametrize("shape", sorted(PARENT_SOURCES))
def test_sources_without_subtree_tables_are_unchanged(lib_path, shape):
    tree, scale = _shape(shape)
    plain = engine.debug_jit(tree, scale_node=scale, compile=False)
    tables = engine.debug_jit_tables(tree, scale_node=scale)[0]
    got = (hashlib.sha256(plain.encode()).hexdigest()[:16], hashlib.sha256(tables.encode()).hexdigest()[:16])
    assert got == PARENT_SOURCES[shape]
