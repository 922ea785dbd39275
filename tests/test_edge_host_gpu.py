"""Branch supports in the C host (pamlh_edge_optimize, pamlh_branch_supports, pamlh_branch_supports_from_replicates) and the driver
(pamlh_lnl --branch-supports), on brown.nuc under HKY85.  The yardsticks: the screened lnL of paml_amd_nni_scores from below, the fully
maximised lnL of the topology (tests/golden/brown_spr_all15.json, the reference's runmode = 0 on all 15 trees) from above with the four
decimals the searches use (1e-4), and the numpy coordinate ascent of tests/edge_ref.py run to 1e-9 on the same problem (1e-4; pinned on
the CPU in tests/test_edge_cpu.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import ancestral_ref as ar
import edge_ref as er
from paml_amd import engine, hostlib
from test_edge_cpu import supports_restated
from test_nni_host_gpu import _analysis, _bipartitions

pytestmark = pytest.mark.gpu


def _maximised(tmp_path, name, newick):
    a = _analysis(tmp_path, name, newick)
    opt = a.optimize(a.default_x())
    assert opt["converged"]
    return a, np.array(opt["x"]), opt["lnL"]


def _numpy_ascent(a, x):
    """l[n_edges][3] of edge_ref.coordinate_ascent on the analysis's problem at x."""
    pb = a.problem(x)
    P = ar.matrices_from_oracle(pb)
    passes = er.tree_passes(pb, P)
    edges, five = pb.tree.edge_configs()
    return np.array([[er.coordinate_ascent(pb, P, cfg, five[e], passes=passes)[1] for cfg in edges[e]] for e in range(len(edges))])


def test_every_configuration_is_maximised_over_its_five_branches(tmp_path):
    g = helpers.load_golden("brown_spr_all15")
    best = max(g["trees"], key=lambda t: t["lnL"])
    by_topology = {tuple(tuple(b) for b in t["bipartitions"]): t["lnL"] for t in g["trees"]}
    a, x, mle = _maximised(tmp_path, "best", best["newick"])
    assert abs(mle - best["lnL"]) <= 1e-4
    names = a.seq_names()
    t = a.problem(x).tree
    edges, five = a.edge_list()
    ref_edges, ref_five = t.edge_configs()
    assert np.array_equal(edges, ref_edges) and np.array_equal(five, ref_five) and len(edges) == a.n_tips - 3
    nni = a.nni_scores(x)
    screened = {tuple(int(c) for c in sw): l for sw, l in zip(nni["swaps"], nni["lnL"])}
    got = a.edge_optimize(x)
    sup = a.branch_supports(x, n_rep=1000, seed=1)
    ascent = _numpy_ascent(a, x)
    print("edge_optimize: %d sweeps, %d engine calls, %d rows at a bound" % (got["sweeps"], got["calls"], got["rows_at_bound"]))
    assert np.array_equal(sup["edge_node"], edges[:, 0, 0])
    assert np.max(np.abs(sup["lnL"] - got["lnL"])) <= 1e-8 * abs(mle)      # (the last call's lnL of the same lengths)
    order = list(a.branch_order())
    for e in range(len(edges)):
        for i, (v, s, xx) in enumerate(tuple(int(c) for c in cfg) for cfg in edges[e]):
            l = got["lnL"][e][i]
            low = nni["lnL0"] if i == 0 else screened[(v, s, xx)]
            tree_i = t if i == 0 else t.nni(v, s, xx)
            top = by_topology[tuple(tuple(b) for b in _bipartitions(tree_i.newick(names), names))]
            print("edge %d configuration %d: screened %.6f <= %.6f <= fully maximised %.6f; numpy ascent %.6f" % (e, i, low, l, top, ascent[e][i]))
            assert low - 1e-9 <= l
            assert l <= top + 1e-4
            assert abs(l - ascent[e][i]) <= 1e-4
            # the swap applied, the five lengths written into x: the analysis's own lnL
            if i:
                a.apply_nni(v, s, xx)
            x5 = x.copy()
            for c, tc in zip(five[e], got["t5"][e][i]):
                x5[order.index(int(c))] = tc
            own = a.lnL(x5)
            if i:
                a.apply_nni(v, xx, s)
            assert abs(own - l) <= 1e-8 * abs(l), (e, i, own, l)
        assert abs(got["lnL"][e][0] - mle) <= 1e-6
    assert (sup["delta"] > 0).all() and ((sup["support"] >= 0) & (sup["support"] <= 1)).all()
    assert np.allclose(sup["delta"], 2 * (sup["lnL"][:, 0] - sup["lnL"][:, 1:].max(axis=1)), rtol=0, atol=1e-12 * abs(mle))
    print("delta %s support %s" % (sup["delta"], sup["support"]))


def test_an_edge_with_a_better_neighbour_gets_support_zero(tmp_path):
    g = helpers.load_golden("brown_nni_search")
    a, x, mle = _maximised(tmp_path, "start", g["runs"][0]["start"])
    ascent = _numpy_ascent(a, x)
    delta_ref = 2 * (ascent[:, 0] - ascent[:, 1:].max(axis=1))
    assert (delta_ref <= 0).any() and np.abs(delta_ref).min() > 1e-3      # (the start is no NNI-local optimum; no edge is near a tie)
    sup = a.branch_supports(x, n_rep=1000, seed=3)
    assert np.array_equal(sup["delta"] <= 0, delta_ref <= 0)
    assert (sup["support"][delta_ref <= 0] == 0).all()
    assert np.max(np.abs(sup["delta"] - delta_ref)) <= 4e-4      # (four values, each within 1e-4 of the ascent's)


def test_supports_equal_the_table_of_the_same_replicates_and_repeat(tmp_path):
    a = hostlib.Analysis(os.path.join(helpers.GOLDEN, "ctl", "brown_hky85.ctl"), "baseml")
    x = np.array(a.default_x())
    pb = a.problem(x)
    for seed in (1, 17):
        sup = a.branch_supports(x, n_rep=500, seed=seed)
        got = a.edge_optimize(x)
        l3, lnf = a.edge_lnf(x, got["edges"], got["five"], got["t5"])
        assert np.array_equal(l3, sup["lnL"])
        rep = engine.rell_replicates(lnf.reshape(-1, a.n_patt), pb.weights, pb.gene_off, n_rep=500, seed=seed)
        delta, support = hostlib.branch_supports_from_replicates(rep, l3)
        assert np.array_equal(delta, sup["delta"]) and np.array_equal(support, sup["support"])
        assert np.array_equal(support, supports_restated(rep, l3)[1])
        again = a.branch_supports(x, n_rep=500, seed=seed)
        assert all(np.array_equal(again[k], sup[k]) for k in ("edge_node", "delta", "support", "lnL")) and again["newick"] == sup["newick"]


def test_driver_prints_the_table_and_a_tree_that_reads_back(tmp_path):
    ctl = os.path.join(helpers.GOLDEN, "ctl", "brown_hky85.ctl")
    out = subprocess.run([hostlib.DRIVER_PATH, "baseml", ctl, "--branch-supports", "--replicates", "200", "--seed", "5"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    head = next(i for i, ln in enumerate(lines) if ln.startswith("Branch supports (SH-like aLRT, 200 replicates, seed 5)"))
    a = hostlib.Analysis(ctl, "baseml")
    x = np.array(a.default_x())
    sup = a.branch_supports(x, n_rep=200, seed=5)
    f = a.problem(x).tree.father()
    rows = lines[head + 2:head + 2 + len(sup["edge_node"])]
    for e, ln in enumerate(rows):
        m = re.match(r"\s*(\d+)\.\.(\d+)\s+(-?[\d.]+)\s+(-?[\d.]+)\s+(-?[\d.]+)\s+(-?[\d.]+)\s+([\d.]+)\s*$", ln)
        assert m, ln
        v = int(sup["edge_node"][e])
        assert (int(m.group(1)), int(m.group(2))) == (int(f[v]) + 1, v + 1)
        assert np.allclose([float(m.group(k)) for k in (3, 4, 5)], sup["lnL"][e], rtol=0, atol=6e-7)
        assert abs(float(m.group(6)) - sup["delta"][e]) <= 6e-7 and abs(float(m.group(7)) - sup["support"][e]) <= 6e-4
    newick = lines[head + 2 + len(rows)]
    assert newick == sup["newick"] and newick.endswith(";") and len(re.findall(r"\)[01]\.\d{3}", newick)) == len(rows)
    b = _analysis(tmp_path, "back", newick)      # the host reads the labelled tree back: the same topology
    names = a.seq_names()
    assert _bipartitions(re.sub(r"\)[01]\.\d{3}", ")", b.problem(np.array(b.default_x())).tree.newick(names)), names) == \
        _bipartitions(a.problem(x).tree.newick(names), names)
