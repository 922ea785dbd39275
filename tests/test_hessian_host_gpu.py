"""The exact Hessian of the branch lengths in the C host (pamlh_branch_hessian_exact, pamlh_write_bv_exact, pamlh_standard_errors_exact,
pamlh_newton_full) and the driver's --exact-hessian, --se-exact and --newton-full, on HIV M0 and on brown.nuc HKY85 at their maxima.
The Hessian's own references are in tests/test_hessian_gpu.py; here the host's block is held against Richardson central differences of
Analysis.gradient's branch block, the standard errors against the inverse of the full Hessian by differences of gradient_full, and the
optimiser against pamlh_newton_branches."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
from paml_amd import hostlib
from paml_amd.engine import engine_for

pytestmark = pytest.mark.gpu
CTL = os.path.join(helpers.GOLDEN, "ctl")
CASES = [("codeml", "hiv_ns0.ctl"), ("baseml", "brown_hky85.ctl")]
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


def _richardson_columns(grad, x, idx, h_of):
    """(R, bound_trunc): column i of the Jacobian of grad by the Richardson pair of central differences at h_of(i) and half of it, and
    10 |D(h) - D(h/2)|, the differences' own truncation estimate."""
    R, T = [], []
    for i in idx:
        h = h_of(i)

        def D(s):
            xp, xm = x.copy(), x.copy()
            xp[i] += s
            xm[i] -= s
            return (grad(xp) - grad(xm)) / (2 * s)
        d1, d2 = D(h), D(h / 2)
        R.append((4 * d2 - d1) / 3)
        T.append(10 * np.abs(d1 - d2))
    return np.array(R).T, np.array(T).T


@pytest.mark.parametrize("prog,ctl", CASES)
def test_branch_hessian_exact_equals_differences_of_the_gradient(prog, ctl):
    """H[:, j] against the Richardson pair of central differences (h = 1e-4 (1 + t_j) and half of it) of Analysis.gradient's branch block
    in t_j.  The bound per entry, derived as in tests/test_hessian_cpu.py: 10 |D(h) - D(h/2)| + 1e-12 S_i / h with S_i = sum_h w_h
    |s_i(h)| from Engine.gradient's scores on the exported problem (the rounding of a difference quotient of a sum of that magnitude
    evaluated to ~1e-12 relative)."""
    a, xs, l_star = _maximum(prog, ctl)
    nt = a.ntime
    lo, hi = a.bounds()
    got = a.branch_hessian_exact(xs)
    assert got["H"].shape == (nt, nt) and got["H"].tobytes() == got["H"].T.tobytes()
    assert abs(got["lnL"] - l_star) <= 1e-8 * abs(l_star)
    plain = a.gradient(xs)
    assert np.allclose(got["grad"], plain["grad"][:nt], rtol=1e-9, atol=1e-8)
    assert np.allclose(np.diag(got["H"]), a.curvature(xs)["curv"], rtol=1e-12, atol=0)
    pb = a.problem(xs)
    order = a.branch_order()[:nt]
    S = (np.abs(engine_for(pb).gradient(pb.tree.branch, pb.gene_rate, want_scores=True)["scores"]) @ pb.weights)[order]
    free = [j for j in range(nt) if xs[j] - 1e-4 * (1 + xs[j]) > lo[j] and xs[j] + 1e-4 * (1 + xs[j]) < hi[j]]
    assert len(free) >= nt // 2
    R, T = _richardson_columns(lambda x: a.gradient(x)["grad"][:nt], xs, free, lambda j: 1e-4 * (1 + xs[j]))
    bound = T + 1e-12 * S[:, None] / np.array([1e-4 * (1 + xs[j]) for j in free])[None, :]
    dev = np.abs(got["H"][:, free] - R)
    print("%s: largest deviation of H from differences of the gradient %.3e (|H| max %.3e), largest share of its bound %.3f"
          % (ctl, dev.max(), np.abs(got["H"]).max(), (dev / bound).max()))
    assert (dev <= bound).all()
    sk = a.branch_hessian(xs)["H"]      # the outer product of scores is another matrix
    assert not np.allclose(sk, got["H"], rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("prog,ctl", CASES)
def test_write_bv_exact_writes_write_bvs_block_with_the_exact_matrix(prog, ctl, tmp_path):
    a, xs, _ = _maximum(prog, ctl)
    nt = a.ntime
    a.write_bv(xs, tmp_path / "skt.BV")
    a.write_bv_exact(xs, tmp_path / "exact.BV")
    skt, exact = open(tmp_path / "skt.BV").read(), open(tmp_path / "exact.BV").read()
    assert skt.split("Hessian")[0] == exact.split("Hessian")[0] and exact.count("Hessian") == 1
    rows = [ln.split() for ln in exact.split("Hessian")[1].strip().splitlines()]
    assert len(rows) == nt and all(len(r) == nt for r in rows)
    H = a.branch_hessian_exact(xs)["H"]
    want = [[(" %10.4g" % v).split()[0] for v in row] for row in H]
    assert rows == want
    assert skt.split("Hessian")[1] != exact.split("Hessian")[1]


@pytest.mark.parametrize("prog,ctl", CASES)
def test_standard_errors_exact_are_no_farther_from_the_full_hessians_than_method_1s(prog, ctl):
    """The reference: the inverse of minus the full Hessian by Richardson central differences (h = 1e-4 (1 + |x_i|) and half of it) of
    gradient_full over the parameters method 1 keeps.  se's largest relative deviation from it is no larger than method 1's; the
    parameters given -1 are those method 1 gives -1."""
    a, xs, _ = _maximum(prog, ctl)
    se1, _ = a.standard_errors(xs, method=1)
    r = a.standard_errors_exact(xs)
    se = r["se"]
    assert np.array_equal(se == -1, se1 == -1)
    free = [i for i in range(a.np) if se1[i] != -1]
    assert len(free) >= 2
    J, _ = _richardson_columns(lambda x: a.gradient_full(x)["grad"], xs, free, lambda i: 1e-4 * (1 + abs(xs[i])))
    Hf = J[free, :]
    Hf = -(Hf + Hf.T) / 2
    ref = np.sqrt(np.diag(np.linalg.inv(Hf)))
    d_exact = float(np.max(np.abs(se[free] - ref) / ref))
    d_m1 = float(np.max(np.abs(se1[free] - ref) / ref))
    print("%s: largest relative deviation of se from the full Hessian's: exact %.3e, method 1 %.3e" % (ctl, d_exact, d_m1))
    assert np.allclose(r["hess"], r["hess"].T, rtol=0, atol=0)
    assert d_exact <= d_m1


def _trace(err, tag):
    return [float(m.group(1)) for m in re.finditer(tag + r" sweep +\d+: lnL (-?[\d.]+)", err)]


@pytest.mark.parametrize("prog,ctl", CASES)
def test_newton_full_reaches_newton_branches_maximum_in_no_more_sweeps(prog, ctl, capfd):
    """From x* with the branch block multiplied alternately by 1.6 and 0.5 (the curvature tests' perturbed start), e = 1e-8: within 1e-6
    of newton_branches' lnL, lnL monotone over the verbose trace, no more sweeps than newton_branches, the other entries untouched."""
    a, xs, l_star = _maximum(prog, ctl)
    nt = a.ntime
    lo, hi = a.bounds()
    start = xs.copy()
    start[:nt] = np.clip(xs[:nt] * np.where(np.arange(nt) % 2 == 0, 1.6, 0.5), lo[:nt], hi[:nt])
    nb = a.newton_branches(start, e=1e-8, max_sweeps=50)
    capfd.readouterr()
    r = a.newton_full(start, e=1e-8, max_sweeps=50, verbose=1)
    trace = _trace(capfd.readouterr().err, "newton-full")
    print("%s: newton_full %d sweeps (%d calls, %d rejected), lnL %.8f; newton_branches %d sweeps (%d rejected), lnL %.8f; lnL* %.8f"
          % (ctl, r["sweeps"], r["calls"], r["rejected"], r["lnL"], nb["sweeps"], nb["rejected"], nb["lnL"], l_star))
    assert abs(r["lnL"] - nb["lnL"]) <= 1e-6, (r["lnL"], nb["lnL"])
    assert len(trace) == r["sweeps"] - r["rejected"] + 1 and all(b >= c for b, c in zip(trace[1:], trace[:-1])), trace
    assert abs(trace[-1] - r["lnL"]) <= 1e-6 and trace[0] <= r["lnL"]
    assert r["sweeps"] <= nb["sweeps"], (r["sweeps"], nb["sweeps"])
    assert r["calls"] == r["sweeps"] + 1
    assert np.array_equal(r["x"][nt:], start[nt:])
    assert ((r["x"][:nt] >= lo[:nt]) & (r["x"][:nt] <= hi[:nt])).all()
    assert abs(a.eval_gpu(r["x"], want_lnf=False)[0] - r["lnL"]) <= 1e-8 * abs(r["lnL"])


def _calls(a):
    return [("pamlh_branch_hessian_exact", a.branch_hessian_exact), ("pamlh_write_bv_exact", lambda x: a.write_bv_exact(x, os.devnull)),
            ("pamlh_standard_errors_exact", a.standard_errors_exact), ("pamlh_newton_full", a.newton_full)]


@pytest.mark.parametrize("prog,ctl,text", [("baseml", "brown_hky85_clock.ctl", r"clock = 1: x holds node ages"),
                                            ("codeml", "mhc_m0.ctl", r"fix_blength = 2: the branch lengths are not parameters"),
                                            ("codeml", "mhc_m0_prop.ctl", r"fix_blength = 3: the branch lengths are not parameters"),
                                            ("baseml", "brown_hky85_adg.ctl", r"rho models \(auto-discrete-gamma\)"),
                                            ("baseml", "brown_unrest.ctl", r"a rate-matrix \(UNREST\) model")])
def test_what_pamlh_curvature_refuses_is_refused_by_name(prog, ctl, text):
    a = hostlib.Analysis(os.path.join(CTL, ctl), prog)
    x = np.array(a.default_x())
    with pytest.raises(RuntimeError, match=text):
        a.curvature(x)
    for name, call in _calls(a):
        with pytest.raises(RuntimeError, match=name + ": " + text):
            call(x)


def test_a_pattern_shard_is_refused_by_name():
    a = hostlib.Analysis(os.path.join(CTL, "horai_mg4.ctl"), "baseml")      # (enough site patterns for two ranks)
    a.set_shard(0, 2)
    x = np.array(a.default_x())
    for name, call in _calls(a):
        with pytest.raises(RuntimeError, match=name + r": a pattern shard \(2 ranks\)"):
            call(x)


def _driver(tmp_path, ctl_name, prog, *flags):
    ctl = tmp_path / ctl_name
    ctl.write_text(open(os.path.join(CTL, ctl_name)).read().replace("../data/", os.path.join(helpers.GOLDEN, "data") + "/"))
    return subprocess.run([hostlib.DRIVER_PATH, prog, str(ctl)] + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=300)


def test_driver_flags(tmp_path):
    """pamlh_lnl --optimize --newton-full --bv FILE --exact-hessian --se-exact: exits 0, prints the sweeps and the standard errors,
    writes the block, and ends at the lnL of the plain --optimize run to 1e-5; a clock is refused by name."""
    plain = _driver(tmp_path, "brown_hky85.ctl", "baseml", "--optimize", "--bv", "skt.BV")
    out = _driver(tmp_path, "brown_hky85.ctl", "baseml", "--optimize", "--newton-full", "--bv", "exact.BV", "--exact-hessian", "--se-exact")
    assert plain.returncode == 0, plain.stderr
    assert out.returncode == 0, out.stderr
    assert "newton-full sweep" in out.stderr and "newton-full sweep" not in plain.stderr
    assert "newton-full: lnL" in out.stdout and "SEs for parameters (observed information, exact branch block):" in out.stdout
    lnl = lambda o: float(next(ln for ln in o.stdout.splitlines() if ln.startswith("lnL  =")).split("=")[1])
    assert abs(lnl(out) - lnl(plain)) <= 1e-5
    skt, exact = open(tmp_path / "skt.BV").read(), open(tmp_path / "exact.BV").read()
    assert "Hessian" in exact and skt.split("Hessian")[1] != exact.split("Hessian")[1]
    refused = _driver(tmp_path, "brown_hky85_clock.ctl", "baseml", "--se-exact")
    assert refused.returncode != 0 and "clock = 1: x holds node ages" in refused.stderr
