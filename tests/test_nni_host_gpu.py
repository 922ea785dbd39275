"""NNI in the C host (pamlh_nni_scores, pamlh_apply_nni, pamlh_nni_search) and the driver (pamlh_lnl --nni-scores, --nni-search), on
brown.nuc under HKY85.  The screened lnL of every neighbour is held against an analysis loaded with the rearranged tree from a tree file
(1e-8: both are one evaluation of a 5-tip tree at the same lengths, lnL ~ -2.7e3); the search against the unmodified reference's
runmode = 5 from the same starting trees (tests/golden/brown_nni_search.json: the same unrooted topology, lnL within 1e-4, the four
decimals it prints)."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
from paml_amd import hostlib

pytestmark = pytest.mark.gpu
CTL = os.path.join(helpers.GOLDEN, "ctl")
CTL_TEXT = ("seqfile = %s\ntreefile = %s\nmodel = 4\nfix_kappa = 0\nkappa = 5\nfix_alpha = 1\nalpha = 0\nncatG = 1\ncleandata = 1\n")


def _analysis(tmp_path, name, newick, n_tips=5):
    tree = tmp_path / (name + ".trees")
    tree.write_text("%d 1\n%s\n" % (n_tips, newick))
    ctl = tmp_path / (name + ".ctl")
    ctl.write_text(CTL_TEXT % (os.path.join(helpers.GOLDEN, "data", "brown.nuc"), tree))
    return hostlib.Analysis(str(ctl), "baseml")


def _bipartitions(newick, names):
    """The non-trivial splits of the unrooted tree, each as the sorted names of the side without names[0]."""
    s = re.sub(r"[:#]\s*[0-9.eE+-]+", "", newick).replace(" ", "").rstrip(";")
    stack, splits = [], set()
    for tok in re.findall(r"[(),]|[^(),]+", s):
        if tok == "(":
            stack.append(set())
        elif tok == ")":
            clade = stack.pop()
            if stack:
                stack[-1] |= clade
                side = clade if names[0] not in clade else set(names) - clade
                if 1 < len(side) < len(names) - 1:
                    splits.add(tuple(sorted(side)))
        elif tok != ",":
            stack[-1].add(tok)
    return sorted(splits)


def test_scores_equal_the_analyses_of_the_rearranged_trees(tmp_path):
    a = hostlib.Analysis(os.path.join(CTL, "brown_hky85.ctl"), "baseml")
    x = np.array(a.default_x())
    got = a.nni_scores(x)
    base = a.eval_gpu(x, want_lnf=False)[0]
    assert abs(got["lnL0"] - base) <= 1e-10 * abs(base)
    t = a.problem(x).tree
    assert np.array_equal(got["swaps"], t.nni_swaps()) and len(got["swaps"]) == 2 * (a.n_tips - 3)
    names = a.seq_names()
    for i, (v, s, xx) in enumerate(got["swaps"]):
        b = _analysis(tmp_path, "swap%d" % i, t.nni(v, s, xx).newick(names))
        ref = b.eval_gpu(np.array(b.default_x()), want_lnf=False)[0]
        print("swap (%d, %d, %d): screened %.9f, loaded %.9f" % (v, s, xx, got["lnL"][i], ref))
        assert abs(got["lnL"][i] - ref) <= 1e-8, (i, got["lnL"][i], ref)
    # apply_nni: the analysis itself on the rearranged tree, and back
    v, s, xx = (int(c) for c in got["swaps"][1])
    a.apply_nni(v, s, xx)
    assert abs(a.eval_gpu(x, want_lnf=False)[0] - got["lnL"][1]) <= 1e-8
    assert [[int(c) for c in u] for u in a.problem(x).tree.sons] == [[int(c) for c in u] for u in t.nni(v, s, xx).sons]
    a.apply_nni(v, xx, s)
    assert a.eval_gpu(x, want_lnf=False)[0] == base
    with pytest.raises(RuntimeError, match="is not a son of"):
        a.apply_nni(v, xx, s)


@pytest.mark.parametrize("run", [0, 1])
def test_search_ends_at_the_references_tree(tmp_path, run):
    g = helpers.load_golden("brown_nni_search")
    r = g["runs"][run]
    a = _analysis(tmp_path, "start", r["start"])
    n_swaps = len(a.nni_scores(np.array(a.default_x()))["swaps"])
    out = a.nni_search(a.default_x())
    print("start %s: %d moves, %d screening calls, %d optimisations, lnL %.6f (reference %.4f)\n%s" %
          (r["start"], out["moves"], out["screening_calls"], out["optimisations"], out["lnL"], r["best_lnL"], out["newick"]))
    assert _bipartitions(r["start"], g["names"]) != [tuple(b) for b in r["best_bipartitions"]]
    assert _bipartitions(out["newick"], g["names"]) == [tuple(b) for b in r["best_bipartitions"]]
    assert abs(out["lnL"] - r["best_lnL"]) <= 1e-4, (out["lnL"], r["best_lnL"])
    assert out["moves"] >= 1 and out["screening_calls"] == out["moves"] + 1
    assert out["optimisations"] <= (out["moves"] + 1) * n_swaps
    # the estimates belong to the tree found: one evaluation of the analysis as it stands gives the search's lnL
    assert abs(a.eval_gpu(out["x"], want_lnf=False)[0] - out["lnL"]) <= 1e-8 * abs(out["lnL"])


def test_driver_prints_the_table_and_the_search(tmp_path):
    g = helpers.load_golden("brown_nni_search")
    a = _analysis(tmp_path, "drv", g["runs"][0]["start"])
    ref = a.nni_scores(np.array(a.default_x()))
    out = subprocess.run([hostlib.DRIVER_PATH, "baseml", str(tmp_path / "drv.ctl"), "--nni-scores", "--nni-search"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    rows = [ln.split() for ln in lines if re.fullmatch(r"\s*\d+\s+\d+\s+\d+\s+-?[0-9.]+\s+-?[0-9.]+\s*", ln)]
    assert len(rows) == len(ref["swaps"])
    for row, sw, l in zip(rows, ref["swaps"], ref["lnL"]):
        assert [int(c) - 1 for c in row[:3]] == list(sw)
        assert abs(float(row[3]) - l) <= 1e-6 and abs(float(row[4]) - (l - ref["lnL0"])) <= 1e-6
    assert sum(ln.startswith("move ") for ln in lines) >= 1
    nw = next(ln for ln in lines if ln.startswith("(") and ln.rstrip().endswith(";"))
    assert _bipartitions(nw, g["names"]) == [tuple(b) for b in g["runs"][0]["best_bipartitions"]]
    lnl = float(next(ln for ln in lines if ln.startswith("lnL  =")).split("=")[1])
    assert abs(lnl - g["runs"][0]["best_lnL"]) <= 1e-4
