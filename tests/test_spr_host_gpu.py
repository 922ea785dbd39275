"""SPR in the C host (pamlh_spr_scores, pamlh_apply_spr, pamlh_spr_search) and the driver (pamlh_lnl --spr-scores, --spr-search), on
brown.nuc under HKY85.  The screened lnL of a move is held against the analysis itself after pamlh_apply_spr, evaluated at the x the
move rewrites (1e-8: both are one evaluation of a 5-tip tree at the same lengths, lnL ~ -2.7e3); the search against the maximised lnL of
all 15 unrooted topologies of the five sequences from the unmodified reference (tests/golden/brown_spr_all15.json, runmode = 0, one
tree per run) and against the reference's NNI search from the same starting trees (tests/golden/brown_nni_search.json)."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
from paml_amd import hostlib
from paml_amd.problem import parse_newick
from test_nni_host_gpu import _analysis, _bipartitions

pytestmark = pytest.mark.gpu
CTL = os.path.join(helpers.GOLDEN, "ctl")


def _sons(a, x):
    return [[int(c) for c in u] for u in a.problem(x).tree.sons]


def test_scores_equal_the_analysis_after_the_move_is_applied():
    a = hostlib.Analysis(os.path.join(CTL, "brown_hky85.ctl"), "baseml")
    x = np.array(a.default_x())
    got = a.spr_scores(x, phi=0.3)
    base = a.eval_gpu(x, want_lnf=False)[0]
    assert abs(got["lnL0"] - base) <= 1e-10 * abs(base)
    t = a.problem(x).tree
    assert np.array_equal(got["moves"], t.spr_moves()) and len(got["moves"]) >= 3
    assert np.array_equal(a.spr_scores(x, radius=1)["moves"], t.spr_moves(1))
    fa = t.father()
    for i in (0, len(got["moves"]) // 2, len(got["moves"]) - 1):
        s, xx = (int(c) for c in got["moves"][i])
        b = hostlib.Analysis(os.path.join(CTL, "brown_hky85.ctl"), "baseml")
        x2 = b.apply_spr(s, xx, 0.3, x)
        q = t.spr(s, xx, 0.3)
        assert _sons(b, x2) == [list(u) for u in q.sons]
        assert np.allclose(b.problem(x2).tree.branch, q.branch, rtol=0, atol=1e-15) and abs(x2[:b.ntime].sum() - x[:b.ntime].sum()) <= 1e-12
        ref = b.eval_gpu(x2, want_lnf=False)[0]
        print("move (%d, %d): screened %.9f, applied %.9f" % (s, xx, got["lnL"][i], ref))
        assert abs(got["lnL"][i] - ref) <= 1e-8, (i, got["lnL"][i], ref)
    with pytest.raises(RuntimeError, match="sibling"):
        a.apply_spr(s, next(int(c) for c in t.sons[fa[s]] if c != s), 0.5, x)
    with pytest.raises(RuntimeError, match="phi"):
        a.apply_spr(s, xx, 1.5, x)
    assert _sons(a, x) == [list(u) for u in t.sons]      # (a refused move leaves the tree alone)


def test_the_inverse_move_restores_the_son_lists():
    a = hostlib.Analysis(os.path.join(CTL, "brown_hky85.ctl"), "baseml")
    x = np.array(a.default_x())
    t = a.problem(x).tree
    fa = t.father()
    base = a.eval_gpu(x, want_lnf=False)[0]
    # an s that is its father's second son: the move leaves sons[f] = (x, s), the inverse (c, s), which is where they were
    s, xx = next((int(s), int(xx)) for s, xx in t.spr_moves() if t.sons[fa[s]][1] == s)
    f = int(fa[s])
    c = int(t.sons[f][0])
    nodes = list(a.problem(x).tree.branch)
    x1 = a.apply_spr(s, xx, 0.5, x)
    assert _sons(a, x1) != [list(u) for u in t.sons]
    x2 = a.apply_spr(s, c, t.branch[c] / (t.branch[c] + t.branch[f]), x1)
    assert _sons(a, x2) == [[int(v) for v in u] for u in t.sons]
    assert np.allclose(x2, x, rtol=0, atol=1e-15) and np.allclose(a.problem(x2).tree.branch, nodes, rtol=0, atol=1e-15)
    assert abs(a.eval_gpu(x2, want_lnf=False)[0] - base) <= 1e-10 * abs(base)


@pytest.mark.parametrize("run", [0, 1])
def test_search_ends_at_a_tree_no_move_improves(tmp_path, run):
    g, all15 = helpers.load_golden("brown_nni_search"), helpers.load_golden("brown_spr_all15")
    golden = dict((tuple(tuple(b) for b in t["bipartitions"]), t["lnL"]) for t in all15["trees"])
    assert len(golden) == 15
    r = g["runs"][run]
    a = _analysis(tmp_path, "start", r["start"])
    out = a.spr_search(a.default_x())
    print("start %s: %d moves, %d screening calls, %d optimisations, lnL %.6f (the NNI search's %.4f)\n%s" %
          (r["start"], out["moves"], out["screening_calls"], out["optimisations"], out["lnL"], r["best_lnL"], out["newick"]))
    assert out["lnL"] >= r["best_lnL"] - 1e-4
    assert out["moves"] >= 1 and out["screening_calls"] == out["moves"] + 1
    names = g["names"]
    found = tuple(_bipartitions(out["newick"], names))
    assert abs(out["lnL"] - golden[found]) <= 2e-4, (out["lnL"], golden[found])
    # no move of the tree found leads to a topology the golden ranks higher
    t = parse_newick(out["newick"], names)
    assert len(t.spr_moves()) >= 1
    for s, x in t.spr_moves():
        other = tuple(_bipartitions(t.spr(s, x).newick(names, lengths=False), names))
        assert golden[other] <= golden[found] + 1e-4, (s, x, golden[other], golden[found])
    # the estimates belong to the tree found: one evaluation of the analysis as it stands gives the search's lnL
    assert abs(a.eval_gpu(out["x"], want_lnf=False)[0] - out["lnL"]) <= 1e-8 * abs(out["lnL"])


def test_driver_prints_the_table_and_the_search(tmp_path):
    g = helpers.load_golden("brown_nni_search")
    a = _analysis(tmp_path, "drv", g["runs"][0]["start"])
    ref = a.spr_scores(np.array(a.default_x()), radius=2, phi=0.4)
    out = subprocess.run([hostlib.DRIVER_PATH, "baseml", str(tmp_path / "drv.ctl"), "--spr-scores", "--radius", "2", "--split", "0.4", "--spr-search", "--top", "6"],
                         cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    rows = [ln.split() for ln in lines if re.fullmatch(r"\s*\d+\s+\d+\s+-?[0-9.]+\s+-?[0-9.]+\s*", ln)]
    assert len(rows) == len(ref["moves"]) >= 1
    for row, mv, l in zip(rows, ref["moves"], ref["lnL"]):
        assert [int(c) - 1 for c in row[:2]] == list(mv)
        assert abs(float(row[2]) - l) <= 1e-6 and abs(float(row[3]) - (l - ref["lnL0"])) <= 1e-6
    assert sum(ln.startswith("move ") for ln in lines) >= 1
    nw = next(ln for ln in lines if ln.startswith("(") and ln.rstrip().endswith(";"))
    assert _bipartitions(nw, g["names"]) == [tuple(b) for b in g["runs"][0]["best_bipartitions"]]
    lnl = float(next(ln for ln in lines if ln.startswith("lnL  =")).split("=")[1])
    assert abs(lnl - g["runs"][0]["best_lnL"]) <= 2e-4
