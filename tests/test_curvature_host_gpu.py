"""The lock-step Newton optimiser over all branch lengths in the C host (pamlh_curvature, pamlh_newton_branches, pamlh_optimize_newton)
and the driver (pamlh_lnl --optimize --newton-branches).  The host's branch block is held against Engine.curvature on the problem the
host exports — that checks the mapping and the gene rates, not the derivatives, whose references are in tests/test_curvature_gpu.py;
the optimiser against pamlh_optimize's maxima and the reference's MLEs at the host optimiser tests' bound (5e-6 in lnL)."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
from paml_amd import hostlib
from paml_amd.engine import engine_for
from test_host_c import CASES

pytestmark = pytest.mark.gpu
CTL = os.path.join(helpers.GOLDEN, "ctl")
MAX_SWEEPS = 50
_cache = {}


def _maximum(prog, ctl):
    """(analysis, x*, lnL*) of optimize(default_x), computed once per control file and left unchanged."""
    if ctl not in _cache:
        a = hostlib.Analysis(os.path.join(CTL, ctl), prog)
        r = a.optimize(a.default_x())
        assert r["converged"]
        _cache[ctl] = (a, r["x"].copy(), r["lnL"])
    a, x, l = _cache[ctl]
    return a, x.copy(), l


@pytest.mark.parametrize("prog,ctl", [("codeml", "hiv_ns0.ctl"), ("codeml", "lyso_bsa.ctl"), ("baseml", "brown_hky85_g4.ctl"), ("baseml", "horai_mg4.ctl")])
def test_host_curvature_branch_block_is_the_engines(prog, ctl):
    """hiv_ns0 (61 states), lyso_bsa (branch labels, four classes, polytomies), brown_hky85_g4 (Cijk + gamma), horai_mg4 (several genes
    with their own models and rates): g and h equal Engine.curvature on the exported problem, mapped by branch_order."""
    a = hostlib.Analysis(os.path.join(CTL, ctl), prog)
    x = np.array(a.default_x())
    got = a.curvature(x)
    pb = a.problem(x)
    ref = engine_for(pb).curvature(pb.tree.branch, pb.gene_rate)
    order = a.branch_order()[:a.ntime]
    assert a.ntime == pb.tree.n_nodes - 1 and len(got["curv"]) == a.ntime
    assert np.allclose(got["curv"], ref["curv"][order], rtol=1e-9, atol=1e-8)
    assert np.allclose(got["grad"], ref["grad"][order], rtol=1e-9, atol=1e-8)
    assert abs(got["lnL"] - ref["lnL"]) <= 1e-10 * abs(ref["lnL"])
    assert np.all(np.isfinite(got["curv"])) and (got["curv"] != 0).any()


def _trace(err):
    """lnL of the accepted sweeps of a verbose pamlh_newton_branches run (its lines on stderr), sweep 0 = the start."""
    return [float(m.group(1)) for m in re.finditer(r"newton sweep +\d+: lnL (-?[\d.]+)", err)]


def _newton_from(a, start, l_star, capfd, what):
    nt = a.ntime
    lo, hi = a.bounds()
    capfd.readouterr()
    r = a.newton_branches(start, e=1e-8, max_sweeps=MAX_SWEEPS, verbose=1)
    trace = _trace(capfd.readouterr().err)
    base = a.optimize(start)
    print("%s: newton_branches %d sweeps, %d engine calls, %d rejected, lnL %.6f (lnL* %.6f); optimize from the same start: %d evaluations, lnL %.6f"
          % (what, r["sweeps"], r["calls"], r["rejected"], r["lnL"], l_star, base["n_eval"], base["lnL"]))
    assert abs(r["lnL"] - l_star) <= 5e-6, (r["lnL"], l_star)
    assert r["sweeps"] <= MAX_SWEEPS and r["calls"] == r["sweeps"] + 1 and r["rejected"] <= r["sweeps"]
    assert len(trace) == r["sweeps"] - r["rejected"] + 1 and all(b >= c for b, c in zip(trace[1:], trace[:-1])), trace
    assert abs(trace[-1] - r["lnL"]) <= 1e-6 and trace[0] <= r["lnL"]
    assert np.array_equal(r["x"][nt:], start[nt:])
    assert ((r["x"][:nt] >= lo[:nt]) & (r["x"][:nt] <= hi[:nt])).all()
    assert abs(a.eval_gpu(r["x"], want_lnf=False)[0] - r["lnL"]) <= 1e-8 * abs(r["lnL"])
    assert r["calls"] < base["n_eval"], (r["calls"], base["n_eval"])
    return r


@pytest.mark.parametrize("prog,ctl", [("codeml", "hiv_ns0.ctl"), ("baseml", "brown_hky85_g4.ctl")])
def test_newton_branches_returns_to_the_maximum(prog, ctl, capfd):
    """From x* = optimize(default_x) with the branch block multiplied alternately by 1.6 and 0.5 (clipped to the bounds), the rest of x
    at x*: back to within 5e-6 of lnL(x*) in at most 50 sweeps, lnL monotone over the trace, the other entries untouched, and fewer
    engine calls than pamlh_optimize spends evaluations from the same start."""
    a, xs, l_star = _maximum(prog, ctl)
    nt = a.ntime
    lo, hi = a.bounds()
    start = xs.copy()
    start[:nt] = np.clip(xs[:nt] * np.where(np.arange(nt) % 2 == 0, 1.6, 0.5), lo[:nt], hi[:nt])
    _newton_from(a, start, l_star, capfd, ctl + " x1.6 / x0.5")


@pytest.mark.parametrize("prog,ctl", [("codeml", "hiv_ns0.ctl"), ("baseml", "brown_hky85_g4.ctl")])
def test_newton_branches_from_saturated_branches(prog, ctl, capfd):
    """Every branch at 3.0, where curvatures can be non-negative: the steps of the gradient's sign bring it inside the box and to the
    same maximum."""
    a, xs, l_star = _maximum(prog, ctl)
    start = xs.copy()
    start[:a.ntime] = 3.0
    _newton_from(a, start, l_star, capfd, ctl + " all 3.0")


@pytest.mark.parametrize("gname,prog,ctl", [CASES[0], CASES[1], CASES[2], CASES[4]])
def test_optimize_newton_finds_the_reference_mle(gname, prog, ctl):
    """The four cases of test_optimiser_with_the_analytic_gradient_finds_the_reference_mle through the alternation: same bound on lnL."""
    g = helpers.load_golden(gname)
    a = hostlib.Analysis(os.path.join(CTL, ctl), prog)
    r = a.optimize_newton(a.default_x())
    print("%s: optimize_newton n_eval %d, lnL %.6f (golden %.6f)" % (gname, r["n_eval"], r["lnL"], g["lnL"]))
    assert r["converged"]
    assert abs(r["lnL"] - g["lnL"]) <= 5e-6, (r["lnL"], g["lnL"])
    lo, hi = a.bounds()
    assert ((r["x"] >= lo) & (r["x"] <= hi)).all()


def _driver(tmp_path, ctl_name, prog, *flags):
    ctl = tmp_path / ctl_name
    ctl.write_text(open(os.path.join(CTL, ctl_name)).read().replace("../data/", os.path.join(helpers.GOLDEN, "data") + "/"))
    return subprocess.run([hostlib.DRIVER_PATH, prog, str(ctl)] + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=300)


def _printed_lnl(out):
    return float(next(ln for ln in out.stdout.splitlines() if ln.startswith("lnL  =")).split("=")[1])


def test_a_clock_is_refused_by_name(tmp_path):
    """brown_hky85_clock.ctl: x holds node ages — refused by the library's three entry points and by the driver."""
    ctl = "brown_hky85_clock.ctl"
    a = hostlib.Analysis(os.path.join(CTL, ctl), "baseml")
    x = np.array(a.default_x())
    for call in (a.curvature, a.newton_branches, a.optimize_newton):
        with pytest.raises(RuntimeError, match=r"clock = 1: x holds node ages"):
            call(x)
    out = _driver(tmp_path, ctl, "baseml", "--optimize", "--newton-branches")
    assert out.returncode != 0 and "clock = 1: x holds node ages" in out.stderr


def test_driver_newton_branches(tmp_path):
    """pamlh_lnl --optimize --newton-branches exits 0, prints its sweeps, and prints the lnL of the default --optimize run to 1e-5."""
    plain = _driver(tmp_path, "brown_hky85.ctl", "baseml", "--optimize")
    newton = _driver(tmp_path, "brown_hky85.ctl", "baseml", "--optimize", "--newton-branches")
    assert plain.returncode == 0, plain.stderr
    assert newton.returncode == 0, newton.stderr
    assert "newton sweep" in newton.stderr and "newton sweep" not in plain.stderr
    print("driver: lnL %.6f with --newton-branches, %.6f without" % (_printed_lnl(newton), _printed_lnl(plain)))
    assert abs(_printed_lnl(newton) - _printed_lnl(plain)) <= 1e-5
