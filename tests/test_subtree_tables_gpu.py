"""Subtree tables of the per-tree 60..64-state kernel (jit.h: SubtreeProgram; kernels_pmat.h: subtree_table_kernel): above the cherries
the product of a node comes from a table with one row per class of patterns below the node, and the walk looks the row up by the
pattern's class.  Every case is held to the oracle as in test_engine_gpu.check (lnL 1e-10 relative, every log f_h 1e-9, fhK) with the
tables on and with PAML_AMD_SUBTREE_TABLES=0, the two runs must have the same BITS (the builder forms a row with the walk's own
functions), and the set of tabulated nodes and their class counts are held against a numpy count, so that a silently disabled path
fails.  The data are synth.codon_m0_problem's, which repeat in shallow subtrees (helpers.random_problem's do not); all shapes have
more 128-pattern tiles than CUs and a ragged last tile (40000 = 312 x 128 + 64)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import oracle
from paml_amd import models, synth
from paml_amd.engine import engine_for
from paml_amd.problem import balanced_tree
from test_engine_gpu import check

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
M2A = [0.6, 0.3, 0.1, 2.5]      # the M2a classes of bench.py's SWEEP
ORACLE_EVALUATE = oracle.evaluate


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, oracle's result), made once and left unchanged"""
    if name == "t16":
        pb = synth.codon_m0_problem(n_tips=16, n_patt=40000)
    elif name == "t32":
        pb = synth.codon_m0_problem(n_tips=32, n_patt=40000)
    elif name == "t12":
        pb = synth.codon_m0_problem(n_tips=12, n_patt=40000)
    elif name == "t8":
        pb = synth.codon_m0_problem(n_tips=8, n_patt=40000)
    elif name == "t16_421":
        pb = synth.codon_m0_problem(n_tips=16, n_patt=421)
    elif name == "t16_m2a":
        freqs, omegas = models.nssites_classes(2, M2A, 3)
        pb = synth.codon_nssites_problem(case("t16")[0], 2.0, omegas, freqs)
    elif name == "t16_scaled":
        import copy
        pb = copy.copy(case("t16")[0])
        pb.scale_node = np.zeros(pb.tree.n_nodes, dtype=np.uint8)
        pb.scale_node[18] = 1
    elif name in ("pool60", "pool64"):
        # each 4-tip clade's columns drawn from a pool of 500 random columns: 500 classes per 4-tip node, nearly all patterns distinct above
        n = int(name[4:])
        pb = helpers.random_problem(n, 16, 40000, seed=700 + n)
        pb.tree = balanced_tree(16)
        rng = np.random.default_rng(n)
        z = np.zeros((16, 40000), dtype=np.uint8)
        for c in range(4):
            pool = rng.integers(0, n, size=(4, 500)).astype(np.uint8)
            z[4 * c:4 * c + 4] = pool[:, rng.integers(0, 500, size=40000)]
        pb.z = z
    else:
        raise KeyError(name)
    return pb, ORACLE_EVALUATE(pb, want_fhk=True)


def tips_below(tree):
    ptr, flat = tree.csr()
    below = {}

    def walk(v):
        below[v] = [v] if v < tree.n_tips else [t for s in flat[ptr[v]:ptr[v + 1]] for t in walk(int(s))]
        return below[v]
    walk(tree.root)
    return below


def numpy_u(pb, nodes):
    below = tips_below(pb.tree)
    return {v: np.unique(pb.z[below[v]], axis=1).shape[1] for v in nodes}


def held_to_oracle(pb, ref, monkeypatch):
    """test_engine_gpu.check itself — its bounds — with the oracle's result for this problem taken from the one computed once"""
    def evaluate(p, want_fhk=False):
        assert p is pb and want_fhk
        return ref
    monkeypatch.setattr(oracle, "evaluate", evaluate)
    try:
        eng, out, _ = check(pb)
    finally:
        monkeypatch.setattr(oracle, "evaluate", ORACLE_EVALUATE)
    return eng, out


def on_off(name, monkeypatch, frac, nodes, blocks_left, cap_mb=None, cherries_left_out=0):
    """Tables on, then off: both held to the oracle, the same bits, the same kernel name; with them on, exactly `nodes` are tabulated,
    with the class counts numpy finds, sons before fathers.  Returns the report of the run with tables."""
    pb, ref = case(name)
    monkeypatch.setenv("PAML_AMD_JIT", "1")
    monkeypatch.setenv("PAML_AMD_CHERRY_TABLES", "1")
    monkeypatch.setenv("PAML_AMD_SUBTREE_MAX_FRAC", str(frac))
    monkeypatch.setenv("PAML_AMD_SUBTREE_TABLES", "1")
    if cap_mb is not None:
        monkeypatch.setenv("PAML_AMD_SUBTREE_CAP_MB", str(cap_mb))
    eng, out = held_to_oracle(pb, ref, monkeypatch)
    rep, cherries, kname = eng.subtree_tables(), eng.cherry_tables(), eng.kernel_name
    eng.close()
    monkeypatch.setenv("PAML_AMD_SUBTREE_TABLES", "0")
    eng0, out0 = held_to_oracle(pb, ref, monkeypatch)
    rep0 = eng0.subtree_tables()
    assert rep0["nodes"] == [] and rep0["bytes"] == 0 and rep0["blocks_left"] == -1 and rep0["n_computed"] == 0
    assert eng0.cherry_tables() == cherries and eng0.kernel_name == kname == "mfma64_jit"
    eng0.close()
    assert out["lnL"] == out0["lnL"]
    assert np.array_equal(out["lnf"], out0["lnf"])
    assert np.array_equal(out["fhK"], out0["fhK"])
    want = numpy_u(pb, nodes)
    assert sorted(rep["nodes"]) == sorted(nodes)
    assert dict(zip(rep["nodes"], rep["u"])) == want
    assert rep["u"] == sorted(rep["u"])
    assert rep["bytes"] == pb.K * sum(want.values()) * 512 and rep["blocks_left"] == (blocks_left if nodes else -1)
    assert rep["n_computed"] == 1
    n_cherries = sum(1 for v, t in tips_below(pb.tree).items() if len(t) == 2) - cherries_left_out
    assert cherries == (n_cherries, pb.K * n_cherries * pb.n_codes ** 2 * 512)      # (all cherries are still built: the level above reads them)
    return rep


def test_no_block_left(monkeypatch):
    """The headline's shape: every node below the root is tabulated, the walk is three lookups and the root, no operand ring traffic."""
    on_off("t16", monkeypatch, 0.5, [18, 21, 24, 27, 17], 0)


def test_one_block_left(monkeypatch):
    """32 taxa: 8 four-tip and 4 eight-tip nodes; node 33 (16 tips, 0.80 of the patterns distinct) stays a product — one operand block per
    tile, the ring never more than a tile ahead."""
    pb = case("t32")[0]
    assert numpy_u(pb, [33])[33] > 0.5 * pb.n_patt
    on_off("t32", monkeypatch, 0.5, [35, 38, 42, 45, 49, 52, 56, 59, 34, 41, 48, 55], 1)


def test_five_blocks_left_ring_form(monkeypatch):
    """frac 0.2: the four-tip nodes only (0.134), the eight-tip nodes (0.41) stay products: five blocks, the ring across tiles, the next
    tile's first lookups requested by its predecessor."""
    pb = case("t32")[0]
    u = numpy_u(pb, [35, 34])
    assert u[35] < 0.2 * pb.n_patt < u[34]
    on_off("t32", monkeypatch, 0.2, [35, 38, 42, 45, 49, 52, 56, 59], 5)


def test_son_is_a_tip(monkeypatch):
    """12 taxa: nodes 14, 16, 18, 20 are a cherry and a tip (the builder takes the tip's column from its table in LDS), 13 two of them."""
    on_off("t12", monkeypatch, 0.5, [14, 16, 18, 20, 13], 0)


def test_nothing_qualifies(monkeypatch):
    """421 patterns: more than half of them are distinct at every four-tip node — cherry tables as before, no subtree table."""
    pb = case("t16_421")[0]
    assert min(numpy_u(pb, [18, 21, 24, 27]).values()) > 0.5 * pb.n_patt
    on_off("t16_421", monkeypatch, 0.5, [], -1)


def test_three_classes_class_change_between_tiles(monkeypatch):
    """M2a's three classes: a table set per class; a workgroup's next tile can belong to the next class."""
    rep = on_off("t16_m2a", monkeypatch, 0.5, [18, 21, 24, 27, 17], 0)
    assert rep["bytes"] == 3 * sum(rep["u"]) * 512


@pytest.mark.parametrize("n", [60, 64])
def test_60_and_64_states(monkeypatch, n):
    """subtree_table_kernel<false, 15> (60 states: the walk's products run 15 k-blocks) and <false>; the four-tip clades repeat, nothing
    above them does."""
    pb = case("pool%d" % n)[0]
    assert numpy_u(pb, [17])[17] > 0.5 * pb.n_patt
    rep = on_off("pool%d" % n, monkeypatch, 0.5, [18, 21, 24, 27], 1)
    assert max(rep["u"]) <= 500


def test_a_rescaled_node_stays_a_product(monkeypatch):
    """scale_node on the four-tip node 18: it is not tabulated, and neither is its father 17, one of whose sons has no table."""
    on_off("t16_scaled", monkeypatch, 0.5, [21, 24, 27], 2)


def test_a_cherry_the_cherry_tables_leave_out_is_never_tabulated(monkeypatch):
    """8 taxa: the cherry tables take three of the four cherries (four operand blocks must stay for their form); the fourth, node 13, is
    no candidate here either — it has no dense classes and no son rows — and stays a tip step and a product: three blocks left, the
    short form with a cherry's two tip tables in the ring.  Node 9 (two tabulated cherries) is tabulated."""
    on_off("t8", monkeypatch, 0.5, [9], 3, cherries_left_out=1)


def test_cap_drops_the_largest_node(monkeypatch):
    """15 MB hold the four-tip nodes' 11.1 MB and not node 17's 8.4 MB beside them."""
    on_off("t16", monkeypatch, 0.5, [18, 21, 24, 27], 1, cap_mb=15)


def _table_env(monkeypatch, frac=0.5):
    monkeypatch.setenv("PAML_AMD_JIT", "1")
    monkeypatch.setenv("PAML_AMD_CHERRY_TABLES", "1")
    monkeypatch.setenv("PAML_AMD_SUBTREE_TABLES", "1")
    monkeypatch.setenv("PAML_AMD_SUBTREE_MAX_FRAC", str(frac))


def test_lanes_never_share_a_table(monkeypatch):
    """test_cherry_tables_gpu's lifetime test with subtree tables: eight eval_device calls back to back, each with its own branch lengths
    and result slot, reproduce eval() of their own lengths — the tables rotate with the P set they were built from."""
    import torch
    _table_env(monkeypatch)
    pb = case("t16")[0]
    rng = np.random.default_rng(3)
    brs = [pb.tree.branch * rng.uniform(0.5, 1.5, pb.tree.n_nodes) for _ in range(8)]
    ref = engine_for(pb)
    want = [ref.eval(b, pb.gene_rate)["lnL"] for b in brs]
    assert len(ref.subtree_tables()["nodes"]) == 5 and len(set(want)) == 8
    ref.close()
    eng = engine_for(pb)
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    for i, b in enumerate(brs):
        eng.eval_device(b, out.data_ptr() + 8 * i, pb.gene_rate)
    eng.flush()
    torch.cuda.synchronize()
    assert len(eng.subtree_tables()["nodes"]) == 5
    assert out.cpu().numpy().tolist() == want
    eng.close()


def test_classes_are_computed_once_per_data_set_and_tree(monkeypatch):
    """Ten evaluations: one class computation; set_tree of an NNI neighbour and one more: two — and the neighbour's tables are its own."""
    _table_env(monkeypatch)
    pb = case("t16")[0]
    eng = engine_for(pb)
    assert eng.subtree_tables() == dict(nodes=[], u=[], bytes=0, blocks_left=-1, n_computed=0)      # (nothing evaluated yet)
    rng = np.random.default_rng(5)
    for _ in range(10):
        eng.eval(pb.tree.branch * rng.uniform(0.8, 1.2, pb.tree.n_nodes), pb.gene_rate)
    rep = eng.subtree_tables()
    assert rep["n_computed"] == 1 and sorted(rep["nodes"]) == [17, 18, 21, 24, 27]
    import copy
    nb = copy.copy(pb)
    nb.tree = pb.tree.nni(18, 19, 21)      # node 18 = (21's clade, cherry 20), node 17 = (18, cherry 19)
    eng.set_tree(nb.tree)
    got = eng.eval(nb.tree.branch, nb.gene_rate)["lnL"]
    rep = eng.subtree_tables()
    assert rep["n_computed"] == 2
    assert dict(zip(rep["nodes"], rep["u"])) == numpy_u(nb, rep["nodes"]) and 21 in rep["nodes"] and 18 in rep["nodes"]
    eng.close()
    monkeypatch.setenv("PAML_AMD_SUBTREE_TABLES", "0")
    eng0 = engine_for(nb)
    assert eng0.eval(nb.tree.branch, nb.gene_rate)["lnL"] == got
    eng0.close()


def test_two_ranks_on_one_gpu(monkeypatch, tmp_path):
    """Pattern shards through the shared-memory stand-in for RCCL, as tests/test_multirank_gpu.py: every rank computes the classes of its
    own patterns and builds its own tables; lnL has the bits of the one-rank run."""
    from test_multirank_gpu import shim_env
    worker = os.path.join(HERE, "shim", "subtree_rank_worker.py")

    def ranks(world):
        xdir = tmp_path / ("w%d" % world)
        xdir.mkdir()
        env = shim_env(PAML_AMD_JIT="1", PAML_AMD_CHERRY_TABLES="1", PAML_AMD_SUBTREE_TABLES="1", PAML_AMD_SUBTREE_MAX_FRAC="0.5")
        procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(xdir), "subtree16"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
                 for r in range(world)]
        outs = []
        try:
            for p in procs:
                outs.append(p.communicate(timeout=300)[0].decode())
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
        for r, p in enumerate(procs):
            assert p.returncode == 0, "rank %d of %d failed:\n%s" % (r, world, outs[r][-3000:])
        return [json.load(open(xdir / ("out%d.json" % r))) for r in range(world)]

    one = ranks(1)[0]
    two = ranks(2)
    pb = case("t16")[0]
    for r in two:
        assert r["lnL"] == one["lnL"] and r["lnL_device"] == one["lnL_device"] and r["kernel"] == one["kernel"] == "mfma64_jit"
        lo, hi = r["shard"]
        shard = pb.slice_patterns(lo, hi)
        assert dict(zip(r["nodes"], r["u"])) == numpy_u(shard, [18, 21, 24, 27, 17])
    assert sorted(one["nodes"]) == [17, 18, 21, 24, 27]
