"""The gradient over every parameter from one engine call in the C host (pamlh_gradient_full, pamlh_rate_matrix,
pamlh_use_analytic_gradient(p, 2)): against Richardson-extrapolated central differences of pamlh_eval_batch_gpu, against pamlh_gradient
on the branch lengths, and in the optimiser against the reference's MLEs."""
import os

import numpy as np
import pytest

import helpers
import modelgrad_ref as mr
from paml_amd import hostlib

pytestmark = pytest.mark.gpu
CTL = os.path.join(helpers.GOLDEN, "ctl")
# HIV M0 (kappa, omega), NSsites M2a (proportions), brown HKY85 + gamma (kappa, alpha; Cijk), FMutSel with estimated codon frequencies
FULL_CASES = [("codeml", "hiv_ns0.ctl"), ("codeml", "hiv_ns2.ctl"), ("baseml", "brown_hky85_g4.ctl"), ("codeml", "hiv_fmutsel_est.ctl")]


@pytest.mark.parametrize("prog,ctl", FULL_CASES)
def test_full_gradient_against_richardson_differences(prog, ctl):
    """Every parameter that is not a branch length, at the control file's initial values: Richardson extrapolation of central differences
    at h = 1e-3 (1 + |x_i|) and h / 2; the bound is 10 |D(h) - D(h/2)| (the differences' own truncation estimate) + 1e-12 |lnL| / h (the
    rounding of a difference quotient of a sum evaluated to ~1e-12 relative).  The branch entries equal pamlh_gradient's to 1e-9."""
    a = hostlib.Analysis(os.path.join(CTL, ctl), prog)
    x = np.array(a.default_x())
    full = a.gradient_full(x)
    assert full is not None and len(full["grad"]) == a.np and np.all(np.isfinite(full["grad"]))
    part = a.gradient(x)
    scale = np.max(np.abs(part["grad"][:a.ntime]))
    assert np.max(np.abs(full["grad"][:a.ntime] - part["grad"][:a.ntime])) <= 1e-9 * scale
    assert abs(full["lnL"] - part["lnL"]) <= 1e-10 * abs(part["lnL"])
    lo, hi = a.bounds()
    checked = 0
    for i in range(a.ntime, a.np):
        h = 1e-3 * (1 + abs(x[i]))
        if x[i] + h > hi[i] or x[i] - h < lo[i]:
            continue      # (one-sided in the host: not restated here)
        rows = np.tile(x, (4, 1))
        rows[0, i] += h; rows[1, i] -= h; rows[2, i] += h / 2; rows[3, i] -= h / 2
        l = a.eval_batch_gpu(rows)
        d1, d2 = (l[0] - l[1]) / (2 * h), (l[2] - l[3]) / h
        R, bound = (4 * d2 - d1) / 3, 10 * abs(d1 - d2) + 1e-12 * abs(full["lnL"]) / h
        print("%s parameter %d: chain rule %.10g, Richardson %.10g, deviation %.3e, bound %.3e" % (ctl, i, full["grad"][i], R, abs(full["grad"][i] - R), bound))
        assert abs(full["grad"][i] - R) <= bound, (i, full["grad"][i], R, bound)
        checked += 1
    assert checked >= 2
    again = a.gradient_full(x)      # (the state was left at x: the same bytes)
    assert again["grad"].tobytes() == full["grad"].tobytes()


def test_rate_matrix_is_what_the_exported_problem_exponentiates():
    for prog, ctl in FULL_CASES:
        a = hostlib.Analysis(os.path.join(CTL, ctl), prog)
        x = np.array(a.default_x())
        pb = a.problem(x)
        for s, es in enumerate(pb.eigen):
            A, B = a.rate_matrix(s), mr.rate_matrix(es, pb.n)
            assert np.max(np.abs(A - B)) <= 1e-10 * np.max(np.abs(B)), (ctl, s)


def test_full_gradient_is_declined_where_the_branch_gradient_is():
    for prog, ctl in (("baseml", "brown_hky85_clock.ctl"), ("baseml", "brown_unrest.ctl"), ("baseml", "brown_hky85_adg.ctl")):
        a = hostlib.Analysis(os.path.join(CTL, ctl), prog)
        assert a.gradient_full(np.array(a.default_x())) is None, ctl


@pytest.mark.parametrize("gname,prog,ctl", [("hiv_m0", "codeml", "hiv_ns0.ctl"), ("brown_hky85", "baseml", "brown_hky85.ctl")])
def test_optimiser_with_the_full_gradient_finds_the_reference_mle(gname, prog, ctl):
    """As test_c_host_optimiser_finds_the_reference_mle (bound on lnL 5e-6, x inside the box), with fewer evaluations than mode 0."""
    g = helpers.load_golden(gname)
    a = hostlib.Analysis(os.path.join(CTL, ctl), prog)
    base = a.optimize(a.default_x())
    r = a.optimize(a.default_x(), analytic_gradient=2)
    print("%s: n_eval %d with the full gradient, %d without; lnL %.6f / %.6f" % (gname, r["n_eval"], base["n_eval"], r["lnL"], base["lnL"]))
    assert r["converged"]
    assert abs(r["lnL"] - g["lnL"]) <= 5e-6, (r["lnL"], g["lnL"])
    lo, hi = a.bounds()
    assert ((r["x"] >= lo) & (r["x"] <= hi)).all()
    assert r["n_eval"] < base["n_eval"]
