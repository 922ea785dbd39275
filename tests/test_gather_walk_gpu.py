"""The gathering walk (csrc/kernels_prune.h: gather_walk_kernel; csrc/gather_tiles.h): a table form that is lookups and the root only runs on
a kernel that fetches every distinct table row of a tile once into LDS.  Every case runs with the switch on, with PAML_AMD_GATHER_WALK=0
(the generated walk) and with PAML_AMD_SUBTREE_TABLES=0, and compares the BITS of lnL and of every per-pattern log f_h.  Tables are forced on
(PAML_AMD_JIT=1 PAML_AMD_CHERRY_TABLES=1); the columns come from small pools (test_subtree_order_gpu.py: pooled) so that classes repeat.
Shapes are the smallest that take each path: 128 x 5 + 37 patterns, with a stretch of one column (one row per table for whole tiles) and a
stretch of columns that are all different (three fresh rows per pattern: R = 128 cuts those tiles after 42 patterns)."""
import copy
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from paml_amd import models, synth
from paml_amd.engine import engine_for
from paml_amd.problem import balanced_tree, parse_newick
from test_subtree_order_gpu import pooled

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NP = 128 * 5 + 37
T16_CLADES = [list(range(8)), list(range(8, 12)), list(range(12, 16))]
# one subtree table (node 9, above the cherry 11 and two tips) and the cherry tables 12 and 13 at the root; two subtree tables at a two-son root
T8_ROOT3 = "((((t1,t2),t3),t4),(t5,t6),(t7,t8));"
T8_ROOT2 = "((((t1,t2),t3),t4),(((t5,t6),t7),t8));"
# four sons at the root, each a subtree table above a cherry and a tip: four lookups
T12_ROOT4 = "(((t1,t2),t3),((t4,t5),t6),((t7,t8),t9),((t10,t11),t12));"


def stretches(pb, seed, n_codes):
    """positions 100 .. 299 hold one column, 300 .. 449 columns that differ from each other at every tabulated node"""
    rng = np.random.default_rng(seed)
    z = pb.z.copy()
    z[:, 100:300] = z[:, 100:101]
    fresh = rng.integers(0, n_codes, size=(pb.tree.n_tips, 150)).astype(np.uint8)
    fresh[0::4] = (np.arange(150) % n_codes).astype(np.uint8)      # (tips 0, 4, 8, 12: one in every clade of four)
    fresh[1::4] = (np.arange(150) // n_codes).astype(np.uint8)
    z[:, 300:450] = fresh
    out = copy.copy(pb)
    out.z = z
    return out


def with_tree(pb, newick):
    out = copy.copy(pb)
    out.tree = parse_newick(newick)
    out.tree.branch[:] = np.where(np.arange(out.tree.n_nodes) < out.tree.n_tips, 0.1, 0.05)
    out.tree.branch[out.tree.root] = 0
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    if name in ("t16", "t16_zero_weights"):
        pb = stretches(pooled(synth.codon_m0_problem(n_tips=16, n_patt=NP), T16_CLADES, [50, 12, 20], NP, 3, 61), 7, 61)
        if name == "t16_zero_weights":
            pb.weights = pb.weights.copy()
            pb.weights[[0, 5, 127, 128, 200, 383, 384, 450, NP - 1]] = 0
    elif name == "t16_129":      # few rows: the tiles are cut by their 128 patterns, the last one holds a single pattern
        pb = pooled(synth.codon_m0_problem(n_tips=16, n_patt=129), T16_CLADES, [20, 5, 8], 129, 11, 61)
    elif name == "t8_root3":
        pb = pooled(with_tree(synth.codon_m0_problem(n_tips=8, n_patt=NP), T8_ROOT3), [list(range(4)), [4, 5], [6, 7]], [40, 30, 30], NP, 12, 61)
    elif name == "t8_root2":
        pb = pooled(with_tree(synth.codon_m0_problem(n_tips=8, n_patt=NP), T8_ROOT2), [list(range(4)), list(range(4, 8))], [40, 60], NP, 13, 61)
    elif name == "t12_root4":
        pb = pooled(with_tree(synth.codon_m0_problem(n_tips=12, n_patt=NP), T12_ROOT4), [list(range(3 * c, 3 * c + 3)) for c in range(4)], [30, 40, 20, 50], NP, 14, 61)
    elif name == "t16_m2a":      # more (tile, class) work items than any GPU has CUs: a workgroup's next tile belongs to another class
        n_patt = 128 * 120 + 37
        base = pooled(synth.codon_m0_problem(n_tips=16, n_patt=NP), T16_CLADES, [900, 40, 70], n_patt, 4, 61)
        freqs, omegas = models.nssites_classes(2, [0.6, 0.3, 0.1, 2.5], 3)
        pb = synth.codon_nssites_problem(base, 2.0, omegas, freqs)
    elif name == "t32":          # five operand blocks left: the ring form, which stays on the generated walk
        pb = pooled(synth.codon_m0_problem(n_tips=32, n_patt=NP), [list(range(4 * c, 4 * c + 4)) for c in range(8)], [30] * 8, NP, 5, 61, skew=1.0)
    elif name in ("n60", "n64"):
        n = int(name[1:])
        pb = helpers.random_problem(n, 16, NP, seed=900 + n)
        pb.tree = balanced_tree(16)
        pb = stretches(pooled(pb, T16_CLADES, [50, 12, 20], NP, n, n), n, n)
    else:
        raise KeyError(name)
    return pb


def run(pb, monkeypatch, gather, tables="1"):
    monkeypatch.setenv("PAML_AMD_JIT", "1")
    monkeypatch.setenv("PAML_AMD_CHERRY_TABLES", "1")
    monkeypatch.setenv("PAML_AMD_SUBTREE_TABLES", tables)
    monkeypatch.setenv("PAML_AMD_GATHER_WALK", gather)
    eng = engine_for(pb)
    out = eng.eval(pb.tree.branch, pb.gene_rate, want_lnf=True)
    rep, gw, kname = eng.subtree_tables(), eng.gather_walk(), eng.kernel_name
    eng.close()
    assert kname == "mfma64_jit" and np.isfinite(out["lnL"])
    return out, rep, gw


def three_ways(name, monkeypatch, n_nodes, in_use=True, blocks_left=0):
    """switch on, switch off, no subtree tables: the same bits; the kernel is really in use where it should be"""
    pb = case(name)
    on, rep, gw = run(pb, monkeypatch, "1")
    assert len(rep["nodes"]) == n_nodes and rep["blocks_left"] == blocks_left
    assert gw["in_use"] == in_use and gw["n_computed"] == (1 if in_use else 0)
    off, rep0, gw0 = run(pb, monkeypatch, "0")
    assert rep0["nodes"] == rep["nodes"] and not gw0["in_use"] and gw0["n_computed"] == 0
    plain, rep1, gw1 = run(pb, monkeypatch, "1", tables="0")
    assert rep1["nodes"] == [] and not gw1["in_use"]
    for other in (off, plain):
        assert on["lnL"].hex() == other["lnL"].hex()
        bad = np.flatnonzero(on["lnf"].view(np.uint64) != other["lnf"].view(np.uint64))
        assert bad.size == 0, "log f_h differs at patterns %r" % bad[:10].tolist()
    return pb, on, gw


def test_three_lookups_one_row_stretch_and_r_cuts(monkeypatch):
    pb, _, gw = three_ways("t16", monkeypatch, 5)
    assert gw["R"] == 128 and gw["tiles"] > (NP + 127) // 128      # the stretch of distinct columns: tiles cut by R
    assert gw["rows"] >= 3 * 150


def test_one_subtree_table_and_two_cherry_tables_at_the_root(monkeypatch):
    three_ways("t8_root3", monkeypatch, 2)


def test_two_son_root(monkeypatch):
    three_ways("t8_root2", monkeypatch, 4)


def test_four_son_root_four_lookups(monkeypatch):
    three_ways("t12_root4", monkeypatch, 4)


def test_three_classes_class_change_between_work_items(monkeypatch):
    _, _, gw = three_ways("t16_m2a", monkeypatch, 5)
    assert 3 * gw["tiles"] > 304      # (more work items than an MI355X has CUs)


def test_zero_weights(monkeypatch):
    pb, on, _ = three_ways("t16_zero_weights", monkeypatch, 5)
    zero = pb.weights == 0
    assert zero.sum() == 9 and np.all(on["lnf"][~zero] < 0)
    full = run(case("t16"), monkeypatch, "1")[0]      # the same columns, every weight 1: the other patterns' values do not move
    assert np.array_equal(on["lnf"][~zero], full["lnf"][~zero])


@pytest.mark.parametrize("n", [60, 64])
def test_60_and_64_states(monkeypatch, n):
    three_ways("n%d" % n, monkeypatch, 5)


def test_last_tile_of_one_pattern(monkeypatch):
    _, _, gw = three_ways("t16_129", monkeypatch, 5)
    assert gw["tiles"] == 2


def test_operand_block_left_stays_on_the_generated_walk(monkeypatch):
    three_ways("t32", monkeypatch, 8, in_use=False, blocks_left=5)


def test_switch_flips_between_evaluations_of_one_engine(monkeypatch):
    pb = case("t16")
    monkeypatch.setenv("PAML_AMD_JIT", "1")
    monkeypatch.setenv("PAML_AMD_CHERRY_TABLES", "1")
    monkeypatch.setenv("PAML_AMD_GATHER_WALK", "0")
    eng = engine_for(pb)
    a = eng.eval(pb.tree.branch, pb.gene_rate, want_lnf=True)
    assert not eng.gather_walk()["in_use"] and eng.gather_walk()["n_computed"] == 0
    monkeypatch.setenv("PAML_AMD_GATHER_WALK", "1")
    b = eng.eval(pb.tree.branch, pb.gene_rate, want_lnf=True)
    assert eng.gather_walk()["in_use"] and eng.gather_walk()["n_computed"] == 1
    monkeypatch.setenv("PAML_AMD_GATHER_WALK", "0")
    c = eng.eval(pb.tree.branch, pb.gene_rate, want_lnf=True)
    assert not eng.gather_walk()["in_use"] and eng.gather_walk()["n_computed"] == 1
    eng.close()
    assert a["lnL"].hex() == b["lnL"].hex() == c["lnL"].hex() and np.array_equal(a["lnf"], b["lnf"]) and np.array_equal(a["lnf"], c["lnf"])


def test_tiles_are_rebuilt_after_set_tips_and_set_tree_only(monkeypatch):
    monkeypatch.setenv("PAML_AMD_JIT", "1")
    monkeypatch.setenv("PAML_AMD_CHERRY_TABLES", "1")
    pb = case("t16")
    eng = engine_for(pb)
    assert eng.gather_walk() == dict(in_use=False, tiles=0, rows=0, R=0, n_computed=0, host_seconds=0.0)
    rng = np.random.default_rng(5)
    first = eng.eval(pb.tree.branch, pb.gene_rate, want_lnf=True)
    for _ in range(5):
        eng.eval(pb.tree.branch * rng.uniform(0.8, 1.2, pb.tree.n_nodes), pb.gene_rate)
    assert eng.gather_walk()["n_computed"] == 1 and eng.gather_walk()["in_use"]
    perm = rng.permutation(pb.n_patt)      # the same columns in another order: other tiles, every pattern's value moves with it
    eng.set_tips(pb.z[:, perm], pb.weights[perm])
    moved = eng.eval(pb.tree.branch, pb.gene_rate, want_lnf=True)
    assert eng.gather_walk()["n_computed"] == 2
    assert np.array_equal(moved["lnf"], first["lnf"][perm])
    eng.eval(pb.tree.branch, pb.gene_rate)
    assert eng.gather_walk()["n_computed"] == 2
    nb = pb.tree.nni(18, 19, 21)
    eng.set_tree(nb)
    got = eng.eval(nb.branch, pb.gene_rate, want_lnf=True)
    eng.eval(nb.branch * 1.1, pb.gene_rate)
    assert eng.gather_walk()["n_computed"] == 3 and eng.gather_walk()["in_use"]
    eng.close()
    monkeypatch.setenv("PAML_AMD_SUBTREE_TABLES", "0")
    pn = copy.copy(pb)
    pn.tree, pn.z, pn.weights = nb, pb.z[:, perm], pb.weights[perm]
    eng0 = engine_for(pn)
    want = eng0.eval(nb.branch, pb.gene_rate, want_lnf=True)
    eng0.close()
    assert got["lnL"].hex() == want["lnL"].hex() and np.array_equal(got["lnf"], want["lnf"])


def test_two_ranks_on_one_gpu(monkeypatch, tmp_path):
    """Pattern shards through the shared-memory stand-in for RCCL (tests/shim/gather_rank_worker.py: subtree_rank_worker.py's run, and what
    Engine.gather_walk() says after it): every rank cuts its own tiles and really runs on the kernel, inside the communicator and in a run of
    eval_device calls; lnL has the bits of one rank on the generated walk."""
    from test_multirank_gpu import shim_env
    worker = os.path.join(HERE, "shim", "gather_rank_worker.py")

    def ranks(world, gather):
        xdir = tmp_path / ("w%d_%s" % (world, gather))
        xdir.mkdir()
        env = shim_env(PAML_AMD_JIT="1", PAML_AMD_CHERRY_TABLES="1", PAML_AMD_SUBTREE_TABLES="1", PAML_AMD_SUBTREE_MAX_FRAC="0.5", PAML_AMD_GATHER_WALK=gather)
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

    one = ranks(1, "0")[0]
    assert not one["gather_walk"]["in_use"] and one["gather_walk"]["tiles"] == 0
    for r in ranks(2, "1"):
        assert r["gather_walk"]["in_use"] and r["gather_walk"]["tiles"] > 0 and r["gather_walk"]["n_computed"] == 1
        assert r["lnL"] == one["lnL"] and r["lnL_device"] == one["lnL_device"] and r["kernel"] == one["kernel"] == "mfma64_jit"
        assert sorted(r["nodes"]) == sorted(one["nodes"]) == [17, 18, 21, 24, 27]
