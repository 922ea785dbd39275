"""The cherry-table form of the per-tree 61-state kernel (jit.h: jit_cherry_program, OP_LOOKUP), without a GPU: the generator closes
its schedule on the shapes of test_jit_schedule_is_consistent, and the blocks of a tabulated cherry leave the operand stream."""
import pytest

import helpers
from paml_amd import engine


@pytest.fixture(scope="module")
def lib_path():
    return engine.build()


def _tree(shape):
    from paml_amd.problem import balanced_tree, parse_newick
    if shape.startswith("balanced"):
        return balanced_tree(int(shape[8:])), None
    if shape == "hiv":
        return helpers.problem_from_golden(helpers.load_golden("hiv_m0")).tree, None
    if shape == "caterpillar":
        s = "(t1:0.1,t2:0.1)"
        for i in range(3, 12):
            s = "(%s:0.05,t%d:0.1)" % (s, i)
        return parse_newick("(%s:0.05,t12:0.1,t13:0.1);" % s), None
    if shape in ("random120", "random200"):
        return helpers.random_problem(61, int(shape[6:]), 10, seed=7).tree, None
    pb = helpers.random_problem(61, 23, 10, seed=5, scale_every=6 if shape == "scaled" else None)
    return pb.tree, pb.scale_node


@pytest.mark.parametrize("shape", ["balanced16", "balanced32", "balanced128", "hiv", "caterpillar", "random23", "scaled", "random120", "random200"])
def test_table_form_closes_and_drops_the_cherries_blocks(lib_path, shape):
    tree, scale = _tree(shape)
    src, stream, tabs = engine.debug_jit_tables(tree, scale_node=scale)
    if tree.n_tips > 95:      # one tip-code block, replaced between tiles: no tables
        assert tabs == [] and src == ""
        return
    assert len(tabs) >= 1
    assert "prune_jit" in src and "#error" not in src
    # one lookup per tabulated cherry in the loop body, plus the requests for the first tile in front of it
    body = src[src.index("for (;; ptile = 0)"):]
    assert src.count("#define JIT_NC 61") == 1
    for c in range(len(tabs)):
        assert body.count("JIT_CTAB(iclass, %d)" % c) + body.count("JIT_CTAB(n_iclass, %d)" % c) == 1
    # a tabulated cherry's P block and its two tip tables are no operand blocks any more; everything else still is, once
    gone = set()
    for a, b, node in tabs:
        gone |= {(1, a), (1, b), (0, node)}
    assert not gone & set(stream)
    plain = engine.debug_jit(tree, scale_node=scale, compile=False)
    n_blocks = tree.n_tips + (tree.n_nodes - tree.n_tips - 1)
    assert len(stream) == n_blocks - 3 * len(tabs) and len(set(stream)) == len(stream) and len(stream) >= 4
    assert "jit_lookup" not in plain and "JIT_NC" not in plain


def test_table_cap_takes_cherries_in_program_order(lib_path):
    from paml_amd.problem import balanced_tree
    tree = balanced_tree(16)
    _, _, all_tabs = engine.debug_jit_tables(tree)
    src, stream, tabs = engine.debug_jit_tables(tree, max_tabs=3)
    assert len(all_tabs) == 8 and tabs == all_tabs[:3] and "#error" not in src
    assert len(stream) == 16 + 13 - 9


def test_next_tiles_lookups_wait_for_this_tiles(lib_path):
    """A cherry that is a son of the root is looked up AFTER the tile's last product.  The next tile's first lookups go into the same
    arrays (AL0, AL1) as this tile's: they may be requested only once this tile has copied its own out."""
    import re
    from paml_amd.problem import parse_newick
    tree = parse_newick("((((t1:0.1,t2:0.1):0.1,t3:0.1):0.1,t4:0.1):0.1,(t5:0.1,t6:0.1):0.1,(t7:0.1,t8:0.1):0.1);")
    src, stream, tabs = engine.debug_jit_tables(tree)
    assert len(tabs) == 3 and "#error" not in src
    body = src[src.index("for (;; ptile = 0)"):]
    for k in range(2):
        req = body.index("jit_lookup(AL%d, JIT_CTAB(n_iclass" % k)
        use = [m.start() for m in re.finditer(r"jit_copy\(A\d+, AL%d\)" % k, body)]
        assert len(use) == 1 and use[0] < req
    for shape in ("balanced16", "balanced32", "hiv", "caterpillar", "random23", "scaled"):      # ... and so on every other shape
        t, sc = _tree(shape)
        b = engine.debug_jit_tables(t, scale_node=sc)[0]
        b = b[b.index("for (;; ptile = 0)"):]
        for k in range(2):
            if "jit_lookup(AL%d, JIT_CTAB(n_iclass" % k in b:
                assert re.search(r"jit_copy\(A\d+, AL%d\)" % k, b).start() < b.index("jit_lookup(AL%d, JIT_CTAB(n_iclass" % k)
