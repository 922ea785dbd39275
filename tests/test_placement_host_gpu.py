"""Placement in the C host (pamlh_load_placement, pamlh_placement_scores, pamlh_place, pamlh_placement_newick) and the driver (pamlh_lnl
--place), on brown.nuc under K80 with kappa fixed: nothing is estimated from frequencies, so the four-sequence tree and the
five-sequence trees share every parameter.  The query, Gorilla, is the third of the file's five sequences: the rows of the tips are not
the rows of the file.  The lnL of every (branch, pendant length) is held against an ordinary analysis loaded with the tree that
pamlh_placement_newick writes, evaluated by the CPU oracle and once by its own engine (1e-8: both are one evaluation of a 5-tip tree at
the same lengths, lnL ~ -3.2e3)."""
import re
import subprocess

import numpy as np
import pytest

import oracle
from paml_amd import hostlib
from test_nni_host_gpu import _bipartitions
from test_placement_cpu import TREE4, _analysis

pytestmark = pytest.mark.gpu
PENDANT, PHI = (0.05, 0.3), 0.4
NAMES = ["Human", "Chimpanzee", "Gorilla", "Orangutan", "Gibbon"]


def test_scores_equal_the_analyses_of_the_enlarged_trees(tmp_path):
    a = _analysis(tmp_path, "place", TREE4, placement=True)
    assert a.n_tips == 4 and a.query_names() == ["Gorilla"]
    x = np.array(a.default_x())
    got = a.placement_scores(x, PENDANT, PHI)
    base = a.eval_gpu(x, want_lnf=False)[0]
    assert abs(got["lnL0"] - base) <= 1e-10 * abs(base)
    assert got["lnL"].shape == (1, 5, 2) and np.array_equal(got["edges"], a.branch_order())
    for b in range(5):
        for j, tau in enumerate(PENDANT):
            # (the loaded analysis is evaluated by the CPU oracle: an engine per tree would cost a second each)
            five = _analysis(tmp_path, "five%d_%d" % (b, j), a.placement_newick(0, b, PHI, tau), n_tips=5)
            ref = oracle.evaluate(five.problem(np.array(five.default_x())))["lnL"]
            print("branch %d, pendant %.2f: one call %.9f, loaded %.9f" % (b, tau, got["lnL"][0, b, j], ref))
            assert abs(got["lnL"][0, b, j] - ref) <= 1e-8, (b, j, got["lnL"][0, b, j], ref)
    # ... and one of them on the GPU, through the host's own evaluation
    five = _analysis(tmp_path, "five_gpu", a.placement_newick(0, 1, PHI, PENDANT[1]), n_tips=5)
    assert abs(got["lnL"][0, 1, 1] - five.eval_gpu(np.array(five.default_x()), want_lnf=False)[0]) <= 1e-8
    # place: the argmax of that table and the likelihood weight ratios of the branches
    pl = a.place(x, PENDANT, PHI)
    le = got["lnL"][0].max(axis=1)
    be = int(np.argmax(le))
    assert pl["best_edge"][0] == be and pl["best_pendant"][0] == PENDANT[int(np.argmax(got["lnL"][0, be]))] and pl["best_lnL"][0] == le[be]
    assert abs(pl["lwr"][0].sum() - 1) <= 1e-12 and int(np.argmax(pl["lwr"][0])) == be
    assert np.allclose(pl["lwr"][0], np.exp(le - le[be]) / np.exp(le - le[be]).sum(), rtol=1e-12, atol=0)
    # the analysis itself is as it was
    assert a.eval_gpu(x, want_lnf=False)[0] == base


def test_driver_prints_the_table_and_the_best_tree(tmp_path):
    a = _analysis(tmp_path, "drv", TREE4, placement=True)
    x = np.array(a.default_x())
    ref, pl = a.placement_scores(x, PENDANT, PHI), a.place(x, PENDANT, PHI)
    out = subprocess.run([hostlib.DRIVER_PATH, "baseml", str(tmp_path / "drv.ctl"), "--place", "--pendant", ",".join("%g" % t for t in PENDANT), "--split", "%g" % PHI],
                         cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert any(ln.startswith("query 1 (Gorilla)") for ln in lines)
    rows = [ln.split() for ln in lines if re.fullmatch(r"\s*\d+\.\.\d+\s+[0-9.]+\s+-?[0-9.]+\s+-?[0-9.]+\s+[0-9.]+(\s+\*)?\s*", ln)]
    assert len(rows) == 5
    t = a.problem(x).tree
    f = t.father()
    for b, row in enumerate(rows):
        v = int(ref["edges"][b])
        lb = ref["lnL"][0, b]
        assert row[0] == "%d..%d" % (f[v] + 1, v + 1)
        assert abs(float(row[1]) - PENDANT[int(np.argmax(lb))]) <= 1e-6 and abs(float(row[2]) - lb.max()) <= 1e-6
        assert abs(float(row[3]) - (lb.max() - ref["lnL0"])) <= 1e-6 and abs(float(row[4]) - pl["lwr"][0, b]) <= 1e-6
        assert (row[-1] == "*") == (b == pl["best_edge"][0])
    nw = next(ln for ln in lines if ln.startswith("(") and ln.rstrip().endswith(";"))
    want = a.placement_newick(0, int(pl["best_edge"][0]), PHI, float(pl["best_pendant"][0]))
    assert _bipartitions(nw, NAMES) == _bipartitions(want, NAMES) and len(_bipartitions(nw, NAMES)) == 2
