"""Cherry tables of the per-tree 61-state kernel (jit.h: OP_LOOKUP; kernels_pmat.h: cherry_table_kernel): the product
P(t) . (tipA o tipB) of a cherry comes from a table of all n_codes^2 such products instead of a matrix product per pattern.
Every case is held to the oracle as in test_engine_gpu.check (lnL 1e-10 relative, every log f_h 1e-9, fhK) and must have the BITS
of the same evaluation without tables: the builder forms a table entry with the walk's own functions in the walk's order."""
import numpy as np
import pytest

import helpers
from paml_amd import synth
from paml_amd.engine import KEEP_PARTIALS, engine_for
from paml_amd.problem import parse_newick
from test_engine_gpu import check

pytestmark = pytest.mark.gpu


def _n_cherries(tree):
    ptr, flat = tree.csr()
    return sum(1 for v in range(tree.n_tips, tree.n_nodes)
               if ptr[v + 1] - ptr[v] == 2 and all(s < tree.n_tips for s in flat[ptr[v]:ptr[v + 1]]))


def on_off(pb, monkeypatch, flags=0, **kw):
    """check() with tables forced on, then off; the two must agree bit for bit.  Returns what cherry_tables() reported with them on."""
    monkeypatch.setenv("PAML_AMD_JIT", "1")
    monkeypatch.setenv("PAML_AMD_CHERRY_TABLES", "1")
    eng, out, _ = check(pb, flags=flags, **kw)
    used = eng.cherry_tables()
    name = eng.kernel_name
    eng.close()
    monkeypatch.setenv("PAML_AMD_CHERRY_TABLES", "0")
    eng0, out0, _ = check(pb, flags=flags, **kw)
    assert eng0.cherry_tables() == (0, 0)
    assert name == eng0.kernel_name
    eng0.close()
    assert out["lnL"] == out0["lnL"]
    assert np.array_equal(out["lnf"], out0["lnf"])
    assert np.array_equal(out["fhK"], out0["fhK"])
    return used, name


@pytest.mark.parametrize("n_patt", [421, 40000])
def test_every_tip_in_a_cherry(monkeypatch, n_patt):
    """16 taxa, all in cherries: five operand blocks are left per tile; 421 patterns end in a ragged tile, 40 000 are more tiles than
    CUs (the tile loop, the next tile's lookups under this tile's last product)."""
    pb = synth.codon_m0_problem(n_tips=16, n_patt=n_patt)
    used, name = on_off(pb, monkeypatch)
    assert name == "mfma64_jit"
    assert used == (8, 8 * pb.n_codes ** 2 * 512)


@pytest.mark.parametrize("n_tips", [6, 9, 23])
def test_random_trees_three_classes(monkeypatch, n_tips):
    """((a,b),c): a lookup, then a tip factor; nodes of two cherries; a cherry right under the root."""
    pb = helpers.random_problem(61, n_tips, 700, K=3, seed=300 + n_tips)
    used, name = on_off(pb, monkeypatch)
    assert name == "mfma64_jit"
    assert 1 <= used[0] <= _n_cherries(pb.tree) and used[1] == 3 * used[0] * pb.n_codes ** 2 * 512


def test_caterpillar(monkeypatch):
    """13 tips, one cherry at the bottom of a deep stack."""
    s = "(t1:0.1,t2:0.1)"
    for i in range(3, 12):
        s = "(%s:0.05,t%d:0.1)" % (s, i)
    pb = helpers.random_problem(61, 13, 300, seed=41)
    pb.tree = parse_newick("(%s:0.05,t12:0.1,t13:0.1);" % s)
    used, name = on_off(pb, monkeypatch)
    assert name == "mfma64_jit" and used[0] == 1


def test_scaled_cherries_stay_products(monkeypatch):
    """A cherry whose node is rescaled (SCALE between the tip step and the product) is not tabulated."""
    pb = helpers.random_problem(61, 23, 500, seed=5, scale_every=4)
    n_ch = _n_cherries(pb.tree)
    ptr, flat = pb.tree.csr()
    cherry = next(v for v in range(pb.tree.n_tips, pb.tree.n_nodes)
                  if v != pb.tree.root and ptr[v + 1] - ptr[v] == 2 and all(x < pb.tree.n_tips for x in flat[ptr[v]:ptr[v + 1]]))
    pb.scale_node = pb.scale_node.copy()
    pb.scale_node[cherry] = 1      # (every fourth internal node rescales; make sure a cherry is among them)
    used, _ = on_off(pb, monkeypatch)
    assert used[0] < n_ch


ROOT_CHERRIES = "((((t1:0.1,t2:0.1):0.1,t3:0.1):0.1,t4:0.1):0.1,(t5:0.1,t6:0.1):0.1,(t7:0.1,t8:0.1):0.1);"


def _several_tiles(shape):
    if shape == "root_cherries":      # two cherry sons of the root, visited after the tile's last product
        pb = helpers.random_problem(61, 8, 70001, seed=51)
        pb.tree = parse_newick(ROOT_CHERRIES)
    elif shape == "caterpillar":
        s = "(t1:0.1,t2:0.1)"
        for i in range(3, 12):
            s = "(%s:0.05,t%d:0.1)" % (s, i)
        pb = helpers.random_problem(61, 13, 40000, seed=41)
        pb.tree = parse_newick("(%s:0.05,t12:0.1,t13:0.1);" % s)
    elif shape == "polytomy":
        pb = helpers.random_problem(61, 11, 40000, seed=21, polytomy=True)
    elif shape == "scaled":
        pb = helpers.random_problem(61, 23, 40000, seed=5, scale_every=4)
    elif shape == "codes64":
        pb = helpers.with_code_table(helpers.random_problem(61, 9, 40000, seed=12), 64)
    elif shape == "classes3":
        pb = helpers.random_problem(61, 9, 30000, K=3, seed=309)
    else:
        n_tips = int(shape[6:])
        pb = helpers.random_problem(61, n_tips, 70001 if n_tips < 10 else 40000, seed=300 + n_tips)
    return pb


@pytest.mark.parametrize("shape", ["root_cherries", "random6", "random9", "random23", "caterpillar", "polytomy", "scaled", "codes64", "classes3"])
def test_tree_shapes_over_several_tiles_per_workgroup(monkeypatch, shape):
    """The tree shapes again with more 128-pattern tiles (x classes) than the 256 CUs of an MI355X — 313 to 704 — so that workgroups walk
    two or three tiles: the next tile's first lookups are requested by its predecessor, into arrays the predecessor may itself still
    be using, and the static wait counts run over the loop edge.  A kernel that mixes up tiles is right on a workgroup's last tile
    only, so it takes several to see it."""
    pb = _several_tiles(shape)
    assert (pb.n_patt + 127) // 128 * pb.K > 256
    used, name = on_off(pb, monkeypatch)
    assert name == "mfma64_jit" and used[0] >= 1


def test_tables_are_on_by_default_from_the_pattern_threshold(monkeypatch):
    """No switch: per-tree kernels by size (65 536 pattern-classes), tables from 32 768 patterns of the engine on."""
    monkeypatch.delenv("PAML_AMD_CHERRY_TABLES", raising=False)
    monkeypatch.delenv("PAML_AMD_JIT", raising=False)
    pb = _several_tiles("root_cherries")
    eng, _, _ = check(pb)
    assert eng.kernel_name == "mfma64_jit" and eng.cherry_tables()[0] == 3
    eng.close()
    pb = helpers.random_problem(61, 9, 30000, K=3, seed=309)      # per-tree kernel by size, fewer patterns than the threshold
    eng = engine_for(pb)
    eng.eval(pb.tree.branch, pb.gene_rate)
    assert eng.kernel_name == "mfma64_jit" and eng.cherry_tables() == (0, 0)


def test_polytomy(monkeypatch):
    pb = helpers.random_problem(61, 11, 500, K=2, seed=21, polytomy=True)
    on_off(pb, monkeypatch)


def test_ambiguous_codes_within_64(monkeypatch):
    pb = helpers.with_code_table(helpers.random_problem(61, 9, 600, seed=12), 64)
    used, name = on_off(pb, monkeypatch)
    assert name == "mfma64_jit" and used[0] >= 1 and used[1] == used[0] * 64 * 64 * 512


def test_more_than_64_codes_and_keep_partials_run_without(monkeypatch):
    monkeypatch.setenv("PAML_AMD_JIT", "1")
    monkeypatch.setenv("PAML_AMD_CHERRY_TABLES", "1")
    pb = helpers.with_code_table(helpers.random_problem(61, 9, 600, seed=13), 80)
    eng, _, _ = check(pb)
    assert eng.kernel_name == "mfma64_jit" and eng.cherry_tables() == (0, 0)
    eng.close()
    pb = synth.codon_m0_problem(n_tips=16, n_patt=421)
    eng, _, _ = check(pb, flags=KEEP_PARTIALS)
    assert eng.kernel_name == "mfma64_jit" and eng.cherry_tables() == (0, 0)


def test_lanes_never_share_a_table(monkeypatch):
    """Eight eval_device calls back to back, each with its own branch lengths and result slot, then one fence: a pruning kernel that
    read tables the builder of a later evaluation was already rewriting would not reproduce eval() of its own lengths."""
    import torch
    monkeypatch.setenv("PAML_AMD_JIT", "1")
    monkeypatch.setenv("PAML_AMD_CHERRY_TABLES", "1")
    pb = synth.codon_m0_problem(n_tips=16, n_patt=40000)
    rng = np.random.default_rng(3)
    brs = [pb.tree.branch * rng.uniform(0.5, 1.5, pb.tree.n_nodes) for _ in range(8)]
    ref = engine_for(pb)
    want = [ref.eval(b, pb.gene_rate)["lnL"] for b in brs]
    assert ref.cherry_tables()[0] == 8 and len(set(want)) == 8
    eng = engine_for(pb)
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    for i, b in enumerate(brs):
        eng.eval_device(b, out.data_ptr() + 8 * i, pb.gene_rate)
    eng.flush()
    torch.cuda.synchronize()
    assert eng.cherry_tables()[0] == 8
    assert out.cpu().numpy().tolist() == want
