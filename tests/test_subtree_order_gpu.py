"""The pattern order of the walk with subtree tables (csrc/subtree_classes.h: subtree_pattern_order; kernels_prune.h: sztile_kernel; jit.h:
the table form's root stores at order[position]) and the table builder's two LDS layouts (kernels_pmat.h: subtree_table_kernel).  Every
case runs with the order, with PAML_AMD_SUBTREE_ORDER=0 and with PAML_AMD_SUBTREE_TABLES=0 and compares the BITS of lnL and of every
per-pattern log f_h — a value stored at a wrong pattern shows there and nowhere else.  The tables-off run is the one the other test
files hold to the oracle.  Shapes are the smallest that take each path: 128 x 3 + 37 patterns (a partial last tile) whose columns come
from small pools, so that classes repeat, are skewed, and their runs in the sorted order cross tile borders."""
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
from paml_amd.problem import balanced_tree

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NP = 128 * 3 + 37


def pooled(pb, clades, pools, n_patt, seed, n_codes, skew=2.0):
    """pb with n_patt columns: the tips of clades[i] take their codes together from a pool of pools[i] random columns, low pool members
    much more often than high ones"""
    rng = np.random.default_rng(seed)
    z = np.zeros((pb.tree.n_tips, n_patt), dtype=np.uint8)
    for tips, size in zip(clades, pools):
        pool = rng.integers(0, n_codes, size=(len(tips), size)).astype(np.uint8)
        z[tips] = pool[:, np.minimum((size * rng.random(n_patt) ** skew).astype(np.int64), size - 1)]
    out = copy.copy(pb)
    out.z, out.weights, out.gene_off = z, np.ones(n_patt), np.array([0, n_patt], dtype=np.int32)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    if name in ("t8", "t8_zero_weights"):
        pb = pooled(synth.codon_m0_problem(n_tips=8, n_patt=NP), [list(range(8))], [40], NP, 1, 61)
        if name == "t8_zero_weights":
            pb.weights = pb.weights.copy()
            pb.weights[[0, 5, 127, 128, 200, 383, 384, NP - 1]] = 0
    elif name == "t12":
        pb = pooled(synth.codon_m0_problem(n_tips=12, n_patt=NP), [list(range(12))], [60], NP, 2, 61)
    elif name == "t16":
        pb = pooled(synth.codon_m0_problem(n_tips=16, n_patt=NP), [list(range(8)), list(range(8, 12)), list(range(12, 16))], [50, 12, 20], NP, 3, 61)
    elif name == "t16_m2a":      # more (tile, class) pairs than any GPU has CUs: the next tile of a workgroup of the WALK (prune_jit is persistent) belongs to another class
        n_patt = 128 * 120 + 37
        base = pooled(synth.codon_m0_problem(n_tips=16, n_patt=NP), [list(range(8)), list(range(8, 12)), list(range(12, 16))], [900, 40, 70], n_patt, 4, 61)
        freqs, omegas = models.nssites_classes(2, [0.6, 0.3, 0.1, 2.5], 3)
        pb = synth.codon_nssites_problem(base, 2.0, omegas, freqs)
    elif name == "t32":          # the four-tip clades repeat, nothing above them does: five operand blocks left
        pb = pooled(synth.codon_m0_problem(n_tips=32, n_patt=NP), [list(range(4 * c, 4 * c + 4)) for c in range(8)], [30] * 8, NP, 5, 61, skew=1.0)
    elif name in ("n60", "n64"):
        n = int(name[1:])
        pb = helpers.random_problem(n, 16, NP, seed=900 + n)
        pb.tree = balanced_tree(16)
        pb = pooled(pb, [list(range(4 * c, 4 * c + 4)) for c in range(4)], [30] * 4, NP, n, n, skew=1.0)
    else:
        raise KeyError(name)
    return pb


def table_env(monkeypatch, order="1", tables="1", **more):
    monkeypatch.setenv("PAML_AMD_JIT", "1")
    monkeypatch.setenv("PAML_AMD_CHERRY_TABLES", "1")
    monkeypatch.setenv("PAML_AMD_SUBTREE_TABLES", tables)
    monkeypatch.setenv("PAML_AMD_SUBTREE_ORDER", order)
    for k, v in more.items():
        monkeypatch.setenv(k, v)


def run(pb, monkeypatch, order, tables="1", **more):
    table_env(monkeypatch, order, tables, **more)
    eng = engine_for(pb)
    out = eng.eval(pb.tree.branch, pb.gene_rate, want_lnf=True)
    rep, ordr, kname = eng.subtree_tables(), eng.subtree_order(), eng.kernel_name
    eng.close()
    assert kname == "mfma64_jit" and np.isfinite(out["lnL"])
    return out, rep, ordr


def three_ways(name, monkeypatch, nodes, blocks_left, **more):
    """with the order, without it, without subtree tables: the same bits; the tables and the order are really in use where they should be"""
    pb = case(name)
    on, rep, ordr = run(pb, monkeypatch, "1", **more)
    assert sorted(rep["nodes"]) == sorted(nodes) and rep["blocks_left"] == blocks_left
    assert ordr["in_use"] and ordr["n_computed"] == 1
    off, rep0, ordr0 = run(pb, monkeypatch, "0", **more)
    assert rep0["nodes"] == rep["nodes"] and rep0["u"] == rep["u"] and not ordr0["in_use"] and ordr0["n_computed"] == 0
    plain, rep1, ordr1 = run(pb, monkeypatch, "1", tables="0")
    assert rep1["nodes"] == [] and not ordr1["in_use"] and ordr1["n_computed"] == 0
    for other in (off, plain):
        assert on["lnL"].hex() == other["lnL"].hex()
        bad = np.flatnonzero(on["lnf"].view(np.uint64) != other["lnf"].view(np.uint64))
        assert bad.size == 0, "log f_h differs at patterns %r" % bad[:10].tolist()
    return pb, on, rep


def test_last_tile_partial(monkeypatch):
    pb, on, rep = three_ways("t8", monkeypatch, [9], 3)
    # the other sequence of the keys: another order, the same bits
    other, _, ordr = run(pb, monkeypatch, "2")
    assert ordr["in_use"] and other["lnL"].hex() == on["lnL"].hex() and np.array_equal(other["lnf"], on["lnf"])


def test_zero_weights(monkeypatch):
    pb, on, _ = three_ways("t8_zero_weights", monkeypatch, [9], 3)
    zero = pb.weights == 0
    assert zero.sum() == 8 and np.all(on["lnf"][~zero] < 0)
    full = run(case("t8"), monkeypatch, "1")[0]      # the same columns, every weight 1: the other patterns' values do not move
    assert np.array_equal(on["lnf"][~zero], full["lnf"][~zero])


def test_three_classes_class_change_between_tiles(monkeypatch):
    pb, _, rep = three_ways("t16_m2a", monkeypatch, [18, 21, 24, 27, 17], 0)
    assert rep["bytes"] == 3 * sum(rep["u"]) * 512


def test_tip_son_full_lds_layout(monkeypatch):
    three_ways("t12", monkeypatch, [14, 16, 18, 20, 13], 0)


def test_two_levels_small_lds_layout(monkeypatch):
    three_ways("t16", monkeypatch, [18, 21, 24, 27, 17], 0)


def test_operand_blocks_left_ring_form(monkeypatch):
    three_ways("t32", monkeypatch, [35, 38, 42, 45, 49, 52, 56, 59], 5)


@pytest.mark.parametrize("n", [60, 64])
def test_60_and_64_states(monkeypatch, n):
    three_ways("n%d" % n, monkeypatch, [18, 21, 24, 27], 1)


def test_order_is_rebuilt_after_set_tips_and_set_tree_only(monkeypatch):
    table_env(monkeypatch)
    pb = case("t16")
    eng = engine_for(pb)
    assert eng.subtree_order() == dict(in_use=False, n_computed=0, host_seconds=0.0)
    rng = np.random.default_rng(5)
    first = eng.eval(pb.tree.branch, pb.gene_rate, want_lnf=True)
    for _ in range(5):
        eng.eval(pb.tree.branch * rng.uniform(0.8, 1.2, pb.tree.n_nodes), pb.gene_rate)
    assert eng.subtree_order()["n_computed"] == 1 and eng.subtree_order()["in_use"]
    perm = rng.permutation(pb.n_patt)      # the same columns in another order: another permutation, every pattern's value moves with it
    eng.set_tips(pb.z[:, perm], pb.weights[perm])
    moved = eng.eval(pb.tree.branch, pb.gene_rate, want_lnf=True)
    assert eng.subtree_order()["n_computed"] == 2
    assert np.array_equal(moved["lnf"], first["lnf"][perm])
    eng.eval(pb.tree.branch, pb.gene_rate)
    assert eng.subtree_order()["n_computed"] == 2
    nb = pb.tree.nni(18, 19, 21)
    eng.set_tree(nb)
    got = eng.eval(nb.branch, pb.gene_rate, want_lnf=True)
    eng.eval(nb.branch * 1.1, pb.gene_rate)
    assert eng.subtree_order()["n_computed"] == 3 and eng.subtree_tables()["n_computed"] == 3
    eng.close()
    monkeypatch.setenv("PAML_AMD_SUBTREE_TABLES", "0")
    pn = copy.copy(pb)
    pn.tree, pn.z, pn.weights = nb, pb.z[:, perm], pb.weights[perm]
    eng0 = engine_for(pn)
    want = eng0.eval(nb.branch, pb.gene_rate, want_lnf=True)
    eng0.close()
    assert got["lnL"].hex() == want["lnL"].hex() and np.array_equal(got["lnf"], want["lnf"])


def test_two_ranks_on_one_gpu(monkeypatch, tmp_path):
    """Pattern shards through the shared-memory stand-in for RCCL (tests/shim/subtree_rank_worker.py as it is): every rank sorts its own
    patterns; lnL has the bits of one rank without the order.  (The worker does not report subtree_order(): that the ranks really ran with
    the order follows from the environment they are given and the default, not from an assertion here; the one-process cases above
    assert in_use.)"""
    from test_multirank_gpu import shim_env
    worker = os.path.join(HERE, "shim", "subtree_rank_worker.py")

    def ranks(world, order):
        xdir = tmp_path / ("w%d_%s" % (world, order))
        xdir.mkdir()
        env = shim_env(PAML_AMD_JIT="1", PAML_AMD_CHERRY_TABLES="1", PAML_AMD_SUBTREE_TABLES="1", PAML_AMD_SUBTREE_MAX_FRAC="0.5", PAML_AMD_SUBTREE_ORDER=order)
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
    for r in ranks(2, "1"):
        assert r["lnL"] == one["lnL"] and r["lnL_device"] == one["lnL_device"] and r["kernel"] == one["kernel"] == "mfma64_jit"
        assert sorted(r["nodes"]) == sorted(one["nodes"]) == [17, 18, 21, 24, 27]
