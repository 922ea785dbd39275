"""Posterior expected substitution counts in the C host (pamlh_count_labels, pamlh_subst_counts) and the driver's --subst-counts, on HIV M0
(codons: synonymous / nonsynonymous) and brown.nuc HKY85 (nucleotides: transitions / transversions) at the control files' initial values.
The engine call's own references are in tests/test_counts_gpu.py; here the host's label sets, its branch order, its expansion from
patterns to sites and the driver's table are held against the restatement (tests/counts_ref.py) on the exported problem, at the family's
rtol 1e-9 / atol 1e-8."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import ancestral_ref as ar
import counts_ref as cref
from paml_amd import hostlib
from paml_amd.engine import engine_for

pytestmark = pytest.mark.gpu
CTL = os.path.join(helpers.GOLDEN, "ctl")
TOL = dict(rtol=1e-9, atol=1e-8)
_cache = {}


def _analysis(prog, ctl):
    """(analysis, x) at the control file's initial values, loaded once and left unchanged."""
    if ctl not in _cache:
        a = hostlib.Analysis(os.path.join(CTL, ctl), prog)
        _cache[ctl] = (a, np.array(a.default_x(), dtype=np.float64))
    a, x = _cache[ctl]
    return a, x.copy()


def _sums_to_total_and_dwell(a, x, want_names):
    nt = a.ntime
    got = a.subst_counts(x, per_site=True)
    assert got["names"] == want_names and got["counts"].shape == (2, nt) and got["site_counts"].shape == (2, nt, len(a.pose()))
    _, total = a.count_labels("total")
    _, dwell = a.count_labels("dwell")
    both = a.subst_counts(x, labels=np.concatenate([total, dwell]), per_site=True)
    assert np.allclose(got["counts"].sum(axis=0), both["counts"][0], **TOL)
    assert np.allclose(got["site_counts"].sum(axis=0), both["site_counts"][0], **TOL)
    # the dwell row is the branch-length block of x: at every site, and times the number of sites in total
    assert np.allclose(both["site_counts"][1], np.broadcast_to(x[:nt, None], both["site_counts"][1].shape), **TOL)
    assert np.allclose(both["counts"][1], x[:nt] * len(a.pose()), **TOL)
    # the per-site table summed over the sites is the total
    assert np.allclose(got["site_counts"].sum(axis=2), got["counts"], **TOL)
    assert (got["counts"] > 0).all()
    return got


def test_hiv_m0_synonymous_and_nonsynonymous_counts():
    a, x = _analysis("codeml", "hiv_ns0.ctl")
    got = _sums_to_total_and_dwell(a, x, ["synonymous", "nonsynonymous"])
    names, M = a.count_labels()
    n = a.n
    assert M.shape == (2, n, n) and not M[:, np.arange(n), np.arange(n)].any()
    off = 1.0 - np.eye(n)
    assert np.array_equal(M[0] + M[1], off) and np.array_equal(M[0], M[0].T) and 0 < M[0].sum() < M[1].sum()
    # the totals are the restatement's on the analysis's engine inputs
    pb = a.problem(x)
    eng = engine_for(pb)
    eng.eval(pb.tree.branch, pb.gene_rate)
    ref = cref.subst_counts_of(pb, ar.matrices_from_engine(eng, pb), M)
    order = a.branch_order()[:a.ntime]
    print("largest deviation from the restatement %.3e of %.3e" % (float(np.max(np.abs(got["counts"] - ref["counts"][:, order]))), float(np.max(ref["counts"]))))
    assert np.allclose(got["counts"], ref["counts"][:, order], **TOL)
    assert np.allclose(got["site_counts"], ref["site_counts"][:, order][:, :, a.pose()], **TOL)


def test_brown_hky85_transitions_and_transversions():
    a, x = _analysis("baseml", "brown_hky85.ctl")
    _sums_to_total_and_dwell(a, x, ["transitions", "transversions"])
    names, M = a.count_labels()
    ts = np.zeros((4, 4))
    ts[0, 1] = ts[1, 0] = ts[2, 3] = ts[3, 2] = 1      # T <-> C, A <-> G
    assert np.array_equal(M[0], ts) and np.array_equal(M[0] + M[1], 1.0 - np.eye(4))
    with pytest.raises(RuntimeError, match="pamlh_count_labels: kind \"other\""):
        a.count_labels("other")


def _driver(tmp_path, ctl_name, prog, *flags):
    ctl = tmp_path / ctl_name
    ctl.write_text(open(os.path.join(CTL, ctl_name)).read().replace("../data/", os.path.join(helpers.GOLDEN, "data") + "/"))
    return subprocess.run([hostlib.DRIVER_PATH, prog, str(ctl)] + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=300)


def test_the_driver_prints_the_same_numbers(tmp_path):
    a, x = _analysis("baseml", "brown_hky85.ctl")
    nt = a.ntime
    got = a.subst_counts(x, per_site=True)
    _, total = a.count_labels("total")
    tot = a.subst_counts(x, labels=total)["counts"][0]
    out = _driver(tmp_path, "brown_hky85.ctl", "baseml", "--subst-counts", "--per-site")
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    head = next(i for i, ln in enumerate(lines) if ln.startswith("Expected numbers of substitutions for each branch"))
    assert lines[head + 2].split() == ["branch", "t", "transitions", "transversions", "total"]
    rows = [ln.split() for ln in lines[head + 4:head + 4 + nt]]
    assert all(".." in r[0] and len(r) == 5 for r in rows)
    table = np.array([[float(v) for v in r[1:]] for r in rows])
    assert np.allclose(table[:, 0], x[:nt], rtol=0, atol=5e-7)
    assert np.allclose(table[:, 1:3], got["counts"].T, rtol=0, atol=5e-7) and np.allclose(table[:, 3], tot, rtol=0, atol=5e-7)
    site = next(i for i, ln in enumerate(lines) if ln.startswith("Expected transitions substitutions: site"))
    n_sites = len(a.pose())
    per = np.array([[float(v) for v in ln.split()[1:]] for ln in lines[site + 1:site + 1 + n_sites]])
    assert per.shape == (n_sites, nt) and np.allclose(per, got["site_counts"][0].T, rtol=0, atol=5e-7)
    plain = _driver(tmp_path, "brown_hky85.ctl", "baseml")
    assert plain.returncode == 0 and "Expected numbers of substitutions" not in plain.stdout


@pytest.mark.parametrize("prog,ctl,text", [("baseml", "brown_hky85_clock.ctl", r"clock = 1: x holds node ages"),
                                            ("baseml", "brown_hky85_adg.ctl", r"rho models \(auto-discrete-gamma\)"),
                                            ("baseml", "brown_unrest.ctl", r"a rate-matrix \(UNREST\) model")])
def test_what_pamlh_curvature_refuses_is_refused_by_name(prog, ctl, text, tmp_path):
    a = hostlib.Analysis(os.path.join(CTL, ctl), prog)
    x = np.array(a.default_x())
    with pytest.raises(RuntimeError, match="pamlh_subst_counts: " + text):
        a.subst_counts(x)
    if "clock" in ctl:
        refused = _driver(tmp_path, ctl, prog, "--subst-counts")
        assert refused.returncode != 0 and "clock = 1: x holds node ages" in refused.stderr


def test_a_pattern_shard_is_refused_by_name():
    a = hostlib.Analysis(os.path.join(CTL, "horai_mg4.ctl"), "baseml")      # (enough site patterns for two ranks)
    a.set_shard(0, 2)
    with pytest.raises(RuntimeError, match=r"pamlh_subst_counts: a pattern shard \(2 ranks\)"):
        a.subst_counts(np.array(a.default_x()))
