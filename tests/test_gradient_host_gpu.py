"""The analytic branch-length gradient in the C host (pamlh_gradient, pamlh_use_analytic_gradient, pamlh_branch_hessian) and the driver
(pamlh_lnl --optimize --analytic-gradient, --bv FILE).  The host's branch block is held against Engine.gradient on the problem the host
exports — that checks the mapping, the signs and the gene rates, not the derivative itself, whose references are in
tests/test_gradient_gpu.py — the optimiser against the reference's MLEs, the --bv block against pamlh_branch_hessian and the restatement."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import ancestral_ref as ar
import gradient_ref as gr
from paml_amd import hostlib
from paml_amd.engine import Engine, engine_for
from test_host_c import CASES

pytestmark = pytest.mark.gpu
CTL = os.path.join(helpers.GOLDEN, "ctl")


@pytest.mark.parametrize("prog,ctl", [("codeml", "hiv_ns0.ctl"), ("codeml", "lyso_bsa.ctl"), ("baseml", "brown_hky85_g4.ctl"), ("baseml", "horai_mg4.ctl")])
def test_host_gradient_branch_block_is_the_engines(prog, ctl):
    """hiv_ns0 (61 states), lyso_bsa (branch labels, four classes, polytomies), brown_hky85_g4 (Cijk + gamma), horai_mg4 (several genes
    with their own models and rates): the leading ntime entries equal Engine.gradient on the exported problem, mapped by branch_order;
    the other entries are central differences and agree with the same differences of single evaluations taken here (step 1e-6 (|x| + 1);
    allowance 1e-3 of max(1, |g|): the rounding of an lnL of ~1e3, ~1e-10, over a step of 2e-6 is ~5e-5 already)."""
    a = hostlib.Analysis(os.path.join(CTL, ctl), prog)
    x = np.array(a.default_x())
    got = a.gradient(x)
    pb = a.problem(x)
    eng = engine_for(pb)
    ref = eng.gradient(pb.tree.branch, pb.gene_rate)
    order = a.branch_order()[:a.ntime]
    assert a.ntime == pb.tree.n_nodes - 1
    assert np.allclose(got["grad"][:a.ntime], ref["grad"][order], rtol=1e-9, atol=1e-9)
    assert abs(got["lnL"] - ref["lnL"]) <= 1e-10 * abs(ref["lnL"])
    assert np.all(np.isfinite(got["grad"])) and len(got["grad"]) == a.np
    lo, hi = a.bounds()
    for i in range(a.ntime, a.np):
        h = 1e-6 * (abs(x[i]) + 1)
        if x[i] + h > hi[i] or x[i] - h < lo[i]:
            continue      # (one-sided in the host: not restated here)
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        fd = (a.eval_gpu(xp, want_lnf=False)[0] - a.eval_gpu(xm, want_lnf=False)[0]) / (2 * h)
        assert abs(got["grad"][i] - fd) <= 1e-3 * max(1.0, abs(fd)), (i, got["grad"][i], fd)


@pytest.mark.parametrize("gname,prog,ctl", [CASES[0], CASES[1], CASES[2], CASES[4]])
def test_optimiser_with_the_analytic_gradient_finds_the_reference_mle(gname, prog, ctl):
    """The four cases of test_c_host_optimiser_finds_the_reference_mle with the branch lengths' derivatives from paml_amd_gradient: same
    bound on lnL (5e-6), x inside the box, and fewer likelihood evaluations than the default run next to it."""
    g = helpers.load_golden(gname)
    a = hostlib.Analysis(os.path.join(CTL, ctl), prog)
    base = a.optimize(a.default_x())
    r = a.optimize(a.default_x(), analytic_gradient=True)
    print("%s: n_eval %d with the analytic gradient, %d without; lnL %.6f / %.6f" % (gname, r["n_eval"], base["n_eval"], r["lnL"], base["lnL"]))
    assert r["converged"]
    assert abs(r["lnL"] - g["lnL"]) <= 5e-6, (r["lnL"], g["lnL"])
    lo, hi = a.bounds()
    assert ((r["x"] >= lo) & (r["x"] <= hi)).all()
    assert r["n_eval"] < base["n_eval"]


def test_optimiser_with_the_analytic_gradient_on_branch_site_model_a():
    """lyso_bsa.ctl (labels, four classes): started as test_c_host_optimiser_on_branch_site_and_clade_models starts it, near the
    reference's optimum, the search comes back to the golden lnL within that test's 5e-5."""
    g = helpers.load_golden("lyso_bsa")
    a = hostlib.Analysis(os.path.join(CTL, "lyso_bsa.ctl"), "codeml")
    x0 = np.array(g["x"])
    x0[a.ntime:] *= 1.1
    lo, hi = a.bounds()
    r = a.optimize(np.clip(x0, lo, hi), analytic_gradient=True)
    assert r["converged"] and abs(r["lnL"] - g["mle_lnL"]) < 5e-5, (r["lnL"], g["mle_lnL"])


def _driver(tmp_path, ctl_name, prog, *flags):
    ctl = tmp_path / ctl_name
    ctl.write_text(open(os.path.join(CTL, ctl_name)).read().replace("../data/", os.path.join(helpers.GOLDEN, "data") + "/"))
    return subprocess.run([hostlib.DRIVER_PATH, prog, str(ctl)] + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=300)


def test_driver_writes_the_bv_block(tmp_path):
    out = _driver(tmp_path, "brown_hky85.ctl", "baseml", "--optimize", "--analytic-gradient", "--bv", "out.BV")
    assert out.returncode == 0, out.stderr
    xline = next(ln for ln in out.stdout.splitlines() if ln.startswith("x:"))
    x = np.array([float(v) for v in xline.split()[1:]])
    a = hostlib.Analysis(os.path.join(CTL, "brown_hky85.ctl"), "baseml")
    nt = a.ntime
    lines = [ln for ln in (tmp_path / "out.BV").read_text().splitlines() if ln.strip()]
    assert int(lines[0]) == a.n_tips
    assert lines[1].lstrip().startswith("(") and lines[1].rstrip().endswith(";") and lines[1].count(":") == nt
    t = np.array([float(v) for v in lines[2].split()])
    g = np.array([float(v) for v in lines[3].split()])
    assert len(t) == nt and len(g) == nt and np.allclose(t, x[:nt], atol=5e-7)
    assert not np.any((t > 0.0004) & (np.abs(g) < 0.005) & (g != 0))
    assert lines[4].strip() == "Hessian"
    H = np.array([[float(v) for v in ln.split()] for ln in lines[5:5 + nt]])
    assert H.shape == (nt, nt) and np.array_equal(H, H.T)
    assert np.linalg.eigvalsh(H).max() <= 1e-6 * np.abs(H).max()      # (negative semi-definite to the four printed digits)
    # the block written at a known x (pamlh_write_bv through the host library; the driver's x above is its printed, rounded form): every
    # number is pamlh_branch_hessian's to the printed digits, the gradient after the reference's zeroing rule
    bh = a.branch_hessian(x)
    a.write_bv(x, tmp_path / "known.BV")
    known = [ln for ln in (tmp_path / "known.BV").read_text().splitlines() if ln.strip()]
    gk = np.array([float(v) for v in known[3].split()])
    Hk = np.array([[float(v) for v in ln.split()] for ln in known[5:5 + nt]])
    gz = np.where((x[:nt] > 0.0004) & (np.abs(bh["grad"]) < 0.005), 0.0, bh["grad"])
    assert np.array_equal(gk, [float("%9.6f" % v) for v in gz])
    assert np.array_equal(Hk, [[float("%10.4g" % v) for v in row] for row in bh["H"]])
    assert np.allclose(H, Hk, rtol=1e-2)      # (the driver's own vector differs from its printed x in the seventh decimal)
    # ... and pamlh_branch_hessian against the restatement's scores
    pb = a.problem(x)
    eng = engine_for(pb)
    eng.eval(pb.tree.branch, pb.gene_rate)
    rs = gr.gradient_of(pb, ar.matrices_from_engine(eng, pb))
    s = rs["scores"][a.branch_order()[:nt]]
    assert np.allclose(bh["H"], -(s * pb.weights[None, :]) @ s.T, rtol=1e-9)
    assert np.allclose(bh["grad"], rs["grad"][a.branch_order()[:nt]], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("over", [None, "clock = 0"])
def test_driver_refuses_bv_with_a_clock_or_a_rooted_tree(tmp_path, over):
    """brown_hky85_clock.ctl (a rooted tree under the clock) as it is, and with the clock switched off: then only the root's two sons
    stand in the way (the committed clock-free control files all read unrooted trees; nhomo = 3 .. 5 keep the three-son root too).
    Both are refused with the message, by the driver and by pamlh_write_bv, and no file is written."""
    ctl = "brown_hky85_clock.ctl"
    a = hostlib.Analysis(os.path.join(CTL, ctl), "baseml", overrides=over)
    assert len(a.problem(np.array(a.default_x())).tree.sons[a.root]) == 2
    assert a.ntime == (a.n_nodes - 1 if over else a.n_tips - 1)      # (branch lengths without the clock, node ages with it)
    out = _driver(tmp_path, ctl, "baseml", "--bv", "out.BV", *(["--set", over] if over else []))
    assert out.returncode != 0 and "unrooted tree" in out.stderr and "clock" in out.stderr
    assert not (tmp_path / "out.BV").exists()
    with pytest.raises(RuntimeError, match="unrooted tree"):
        a.write_bv(a.default_x(), tmp_path / "lib.BV")
    assert not (tmp_path / "lib.BV").exists()
