"""paml_amd_subst_counts: posterior expected labelled substitution counts and dwell times on every branch, per pattern and summed, in one
engine call.  Reference: the numpy + scipy restatement tests/counts_ref.py (label integrals by Van Loan's block exponential, not by the
kernel's spectral formula; pinned on the CPU by tests/test_counts_cpu.py) fed with the matrices paml_amd_get_pmat returns after the call.
Tolerance: rtol 1e-9 / atol 1e-8, the family's, per pattern and on the totals; lnL against eval within 1e-10 |lnL| and byte-equal to
Engine.model_gradient's, whose passes the call reuses."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import ancestral_ref as ar
import counts_ref as cref
import curvature_ref as cr
import gradient_ref as gr
import modelgrad_ref as mr
from paml_amd import engine
from paml_amd.engine import engine_for
from paml_amd.problem import EIGEN_QMAT
from test_ancestral_gpu import _rooted_at_tip0
from test_engine_gpu import _branch_model_problem
from test_multirank_gpu import shim_env
from test_oracle_golden import _closed_form

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-9, atol=1e-8)


def _same_bytes(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def _branches(pb):
    t = pb.tree
    return np.where(np.arange(t.n_nodes) == t.root, 0.0, t.branch)


def _check_identities(pb, got):
    """What holds without a reference: the root's entries and the patterns of weight 0 are 0; the identity (the last label) returns the
    branch length at every live pattern and branch[v] sum w in total."""
    t = pb.tree
    live = pb.weights > 0
    assert not got["counts"][:, t.root].any() and not got["site_counts"][:, t.root].any() and not got["site_counts"][:, :, ~live].any()
    dwell = got["site_counts"][-1][:, live]
    print("dwell: largest deviation from the branch length %.3e" % float(np.max(np.abs(dwell - _branches(pb)[:, None]))))
    assert np.allclose(dwell, np.broadcast_to(_branches(pb)[:, None], dwell.shape), **TOL)
    assert np.allclose(got["counts"][-1], _branches(pb) * pb.weights.sum(), **TOL)


def _check(pb, eng=None, restatement=True, seed=5):
    """One subst_counts call on pb (a random 0 / 1 mask, its complement, the identity) against its references; returns (engine, result)."""
    eng = eng or engine_for(pb)
    t = pb.tree
    labels = cref.mask_labels(pb.n, seed)
    base = eng.eval(t.branch, pb.gene_rate)["lnL"]
    got = eng.subst_counts(t.branch, pb.gene_rate, labels=labels, want_sites=True, want_lnf=True)
    assert abs(got["lnL"] - base) <= 1e-10 * abs(base), (got["lnL"], base)
    assert got["counts"].shape == (3, t.n_nodes) and got["site_counts"].shape == (3, t.n_nodes, pb.n_patt)
    _check_identities(pb, got)
    # additivity: mask + complement = every change
    total = eng.subst_counts(t.branch, pb.gene_rate, labels=(labels[0] + labels[1])[None], want_sites=True)
    assert np.allclose(total["counts"][0], got["counts"][0] + got["counts"][1], **TOL)
    assert np.allclose(total["site_counts"][0], got["site_counts"][0] + got["site_counts"][1], **TOL)
    mgd = eng.model_gradient(t.branch, pb.gene_rate)
    assert _same_bytes(got["lnL"], mgd["lnL"])
    if restatement:
        ref = cref.subst_counts_of(pb, ar.matrices_from_engine(eng, pb), labels)      # (the matrices of the call just made)
        print("site_counts: max abs error %.3e of magnitude %.3e; counts: %.3e of %.3e" % (
            float(np.max(np.abs(got["site_counts"] - ref["site_counts"]))), float(np.max(np.abs(ref["site_counts"]))),
            float(np.max(np.abs(got["counts"] - ref["counts"]))), float(np.max(np.abs(ref["counts"])))))
        assert np.allclose(got["site_counts"], ref["site_counts"], **TOL)
        assert np.allclose(got["counts"], ref["counts"], **TOL)
        live = pb.weights > 0
        assert np.max(np.abs(got["lnf"] - ref["lnf"])[live]) <= 1e-9
    return eng, got


# ---- parity with the restatement ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [s[0] for s in gr.REVERSIBLE_SHAPES])
def test_subst_counts_match_the_restatement(name):
    _check(gr.reversible_problem(name))


@pytest.mark.parametrize("n", [64, 21])
def test_subst_counts_at_the_ends_of_the_matrix_core_range(n):
    _check(helpers.random_problem(n, 9, 150, K=1, seed=300 + n))


def test_subst_counts_on_the_one_pattern_per_lane_kernel_at_20_states():
    """A keep-partials engine runs 20 states on the one-pattern-per-lane kernels (the other path of the product kernels' split)."""
    pb = helpers.random_problem(20, 9, 150, K=2, seed=71)
    _check(pb, engine_for(pb, flags=engine.KEEP_PARTIALS))


@pytest.mark.parametrize("n,K,genes", [(4, 2, 1), (61, 2, 2)])
def test_subst_counts_with_eigen_systems_of_different_pi_per_label(n, K, genes):
    _check(_branch_model_problem(n, K, 300 + n + K, n_genes=genes))


@pytest.mark.parametrize("n", [4, 61])
def test_subst_counts_with_a_model_and_pi_per_gene(n):
    _check(helpers.give_genes_their_own_models(mr.small_problem(n, tips=6, n_genes=3), seed=n))


@pytest.mark.parametrize("n", [4, 61])
def test_subst_counts_on_a_tree_rooted_at_a_tip(n):
    """Plain states only, as the gradient's test of a tip root (the evaluation has no value for a tip root on an alignment with ambiguity
    codes, so its lnL is no reference there; tools/counts_host_check.py holds that case against the restatement)."""
    _check(_rooted_at_tip0(mr.small_problem(n, tips=7, seed=1, ambiguity=False)))


@pytest.mark.parametrize("n,K,kind", [(4, 2, "k80"), (20, 1, "jc")])
def test_subst_counts_of_the_closed_form_kinds(n, K, kind):
    """Repeated eigenvalues: the tau e^{lambda tau} branch of Psi."""
    _check(_closed_form(mr.small_problem(n, tips=8, K=K, ambiguity=(n == 4)), kind))


def test_subst_counts_of_the_cijk_kind_on_the_brown_golden():
    _check(helpers.problem_from_golden(helpers.load_golden("brown_hky85")))


# ---- against the model-gradient call on the same engine --------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 61])
def test_subst_counts_against_the_model_gradient(n):
    """One eigen set.  With the label E_ab (a != b): sum_v counts[l][v] = A_ab g_A[0][a][b], because d exp(A tau) / d A_ab is the
    integral of e^{Au} E_ab e^{A(tau-u)}; and counts[l][v] = sum_{g,k} <W_gkv, I_lkv> with I from the restatement."""
    pb = mr.small_problem(n, tips=6)
    t = pb.tree
    assert len(pb.eigen) == 1
    eng = engine_for(pb)
    pairs = [(0, 1), (2, 0), (n - 1, n - 2)]
    labels = np.zeros((3, n, n))
    for l, (a, b) in enumerate(pairs):
        labels[l, a, b] = 1
    got = eng.subst_counts(t.branch, pb.gene_rate, labels=labels)
    mgd = eng.model_gradient(t.branch, pb.gene_rate, want_pairs=True)
    A = mr.rate_matrix(pb.eigen[0], n)
    for l, (a, b) in enumerate(pairs):
        want = A[a, b] * mgd["g_A"][0][a, b]
        assert np.isclose(got["counts"][l].sum(), want, **TOL), (l, got["counts"][l].sum(), want)
    I = cref.label_integrals(pb, labels)
    want = np.einsum("gkvyx,gkvlyx->lv", mgd["W"], I)
    assert np.allclose(got["counts"], want, **TOL)


# ---- deep trees: the rescaled outer chain ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,tips,K,every", [(20, 40, 1, 8), (61, 30, 2, 5)])
def test_subst_counts_deep_tree_with_rescaling(n, tips, K, every):
    """The dwell identity and additivity only: the linear-domain restatement underflows here."""
    _check(helpers.random_problem(n, tips, 70, K=K, seed=77 + n, scale_every=every), restatement=False)


# ---- batches, sub-lists, repeated calls ------------------------------------------------------------------------------------------------

def test_subst_counts_batches_have_the_same_bytes(monkeypatch):
    """PAML_AMD_COUNTS_ARENA_MB=1 cannot hold 3000 patterns of 61 states x 9 tips (test_counts_cpu.py): several batches, equal bytes."""
    c = cr.BATCHING_CASE
    pb = helpers.random_problem(c["n"], c["tips"], c["patterns"], K=c["K"], seed=13)
    t = pb.tree
    labels = cref.mask_labels(pb.n, 2)
    eng = engine_for(pb)
    one = eng.subst_counts(t.branch, pb.gene_rate, labels=labels, want_sites=True, want_lnf=True)
    assert engine.subst_counts_info()["last_batches"] == 1
    monkeypatch.setenv("PAML_AMD_COUNTS_ARENA_MB", "1")
    many = eng.subst_counts(t.branch, pb.gene_rate, labels=labels, want_sites=True, want_lnf=True)
    info = engine.subst_counts_info()
    assert info["last_batches"] > 1 and info["last_kernel_ms"] > 0, info
    for key in ("lnL", "counts", "site_counts", "lnf"):
        assert _same_bytes(one[key], many[key]), key
    _check_identities(pb, many)


@pytest.mark.parametrize("n", [4, 61])
def test_sub_lists_and_repeated_calls_have_the_same_bytes(n):
    pb = mr.small_problem(n, tips=7)
    t = pb.tree
    eng = engine_for(pb)
    labels = cref.mask_labels(n, 9)
    full = eng.subst_counts(t.branch, pb.gene_rate, labels=labels, want_sites=True, want_lnf=True)
    again = eng.subst_counts(t.branch, pb.gene_rate, labels=labels, want_sites=True, want_lnf=True)
    for key in ("lnL", "counts", "site_counts", "lnf"):
        assert _same_bytes(full[key], again[key]), key
    nodes = [v for v in range(t.n_nodes) if v != t.root][::-1][1::2]
    lab_ix = [2, 0]
    part = eng.subst_counts(t.branch, pb.gene_rate, labels=labels[lab_ix], nodes=nodes, want_sites=True, want_lnf=True)
    assert part["counts"].shape == (2, len(nodes)) and part["site_counts"].shape == (2, len(nodes), pb.n_patt)
    assert _same_bytes(part["lnL"], full["lnL"]) and _same_bytes(part["lnf"], full["lnf"])
    for i, l in enumerate(lab_ix):
        for j, v in enumerate(nodes):
            assert _same_bytes(part["counts"][i, j], full["counts"][l, v]), (l, v)
            assert _same_bytes(part["site_counts"][i, j], full["site_counts"][l, v]), (l, v)
    # without the per-pattern arrays: the same totals
    plain = eng.subst_counts(t.branch, pb.gene_rate, labels=labels)
    assert plain["site_counts"] is None and plain["lnf"] is None and _same_bytes(plain["counts"], full["counts"])


@pytest.mark.parametrize("n", [4, 61])
def test_the_other_calls_return_what_they_returned_before(n):
    pb = mr.small_problem(n, tips=7)
    t = pb.tree
    eng = engine_for(pb)

    def snapshot():
        ev = eng.eval(t.branch, pb.gene_rate, want_lnf=True)
        g = eng.gradient(t.branch, pb.gene_rate, want_lnf=True, want_scores=True)
        cv = eng.curvature(t.branch, pb.gene_rate)
        mgd = eng.model_gradient(t.branch, pb.gene_rate)
        return [np.float64(ev["lnL"]).tobytes(), ev["lnf"].tobytes(), np.float64(g["lnL"]).tobytes(), g["grad"].tobytes(), g["scores"].tobytes(),
                cv["curv"].tobytes(), mgd["g_A"].tobytes(), mgd["g_eff"].tobytes()]
    before = snapshot()
    eng.subst_counts(t.branch, pb.gene_rate, labels=cref.mask_labels(n, 1), want_sites=True)
    assert snapshot() == before


@pytest.mark.parametrize("n", [4, 61])
def test_patterns_of_weight_zero_contribute_nothing(n):
    pb = mr.small_problem(n, tips=7)
    live = pb.weights > 0
    assert not live.all()
    labels = cref.mask_labels(n, 5)
    eng, got = _check(pb)
    # the same alignment without those patterns
    q = pb.slice_patterns(0, pb.n_patt)
    q.z = np.ascontiguousarray(pb.z[:, live])
    q.weights = pb.weights[live].copy()
    q.gene_off = np.array([0, int(live.sum())], dtype=np.int32)
    dropped = engine_for(q).subst_counts(q.tree.branch, q.gene_rate, labels=labels, want_sites=True)
    assert np.allclose(got["counts"], dropped["counts"], **TOL)
    assert np.allclose(got["site_counts"][:, :, live], dropped["site_counts"], **TOL)
    # and with other characters in them
    r = pb.slice_patterns(0, pb.n_patt)
    r.z = pb.z.copy()
    r.z[:, ~live] = (r.z[:, ~live] + 1) % n
    other = engine_for(r).subst_counts(r.tree.branch, r.gene_rate, labels=labels, want_sites=True)
    assert _same_bytes(got["counts"], other["counts"]) and _same_bytes(got["site_counts"], other["site_counts"])


# ---- arguments --------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_engine_as_it_was():
    pb = mr.small_problem(4, tips=7)
    t = pb.tree
    eng = engine_for(pb)
    L = eng._L
    base = eng.eval(t.branch, pb.gene_rate)["lnL"]
    L.paml_amd_subst_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    br, lnl = np.ascontiguousarray(t.branch), np.zeros(1)
    cap = 16      # COUNTS_MAX_LABELS
    labels, counts = np.ascontiguousarray(np.tile(np.eye(4), (cap + 1, 1, 1))), np.zeros((cap + 1, t.n_nodes))
    EINVAL, EUNSUPPORTED = -1, -4

    def bad(e, rc, code, text):
        assert rc == code, rc
        msg = L.paml_amd_last_error(e._h).decode()
        assert msg.startswith("subst_counts") and text in msg, msg

    def call(e=eng, branch=br, n_lab=1, lab=labels, nodes=None, lnl_=lnl, counts_=counts):
        nd = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.int32)
        return L.paml_amd_subst_counts(e._h, p(branch), None, n_lab, p(lab), 0 if nd is None else len(nd), p(nd), p(lnl_), p(counts_), None, None)
    assert call() == 0
    bad(eng, call(branch=None), EINVAL, "null argument")
    bad(eng, call(lab=None), EINVAL, "null argument")
    bad(eng, call(lnl_=None), EINVAL, "null argument")
    bad(eng, call(counts_=None), EINVAL, "null argument")
    bad(eng, call(n_lab=0), EINVAL, "n_lab = 0")
    bad(eng, call(n_lab=cap + 1), EINVAL, "n_lab = %d" % (cap + 1))
    assert call(n_lab=cap) == 0
    for poison in (np.nan, np.inf):
        broken = labels.copy()
        broken[1, 2, 3] = poison
        bad(eng, call(n_lab=2, lab=broken), EINVAL, "not finite")
    bad(eng, call(nodes=[1, t.root]), EINVAL, "is the root")
    bad(eng, call(nodes=[1, t.n_nodes]), EINVAL, "out of range")
    bad(eng, call(nodes=[-1]), EINVAL, "out of range")
    bad(eng, call(nodes=[1, 2, 1]), EINVAL, "listed twice")
    fresh = engine.Engine(4, 7, 70)      # a model that is not set yet
    bad(fresh, call(e=fresh), EINVAL, "before set_tips/set_tree/set_pi/set_classes/set_eigen")
    pq = helpers.random_problem(4, 7, 70, seed=5)
    Q = pq.eigen[0]["U"] @ np.diag(pq.eigen[0]["Root"]) @ pq.eigen[0]["V"]
    pq.eigen = [dict(kind=EIGEN_QMAT, Q=np.ascontiguousarray(Q))]
    eq = engine_for(pq)
    bad(eq, call(e=eq, branch=np.ascontiguousarray(pq.tree.branch)), EUNSUPPORTED, "rate-matrix (UNREST)")
    with pytest.raises(engine.EngineError, match=r"subst_counts.*rate-matrix \(UNREST\)"):
        eq.subst_counts(pq.tree.branch, labels=np.eye(4))
    # the engines still evaluate, and count, as before
    assert eng.eval(t.branch, pb.gene_rate)["lnL"] == base
    assert abs(eq.eval(pq.tree.branch, pq.gene_rate)["lnL"] - engine_for(pq).eval(pq.tree.branch, pq.gene_rate)["lnL"]) == 0
    _check(pb, eng)


def test_subst_counts_refuses_an_engine_of_two_ranks(tmp_path):
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim", "counts_rank_worker.py")
    world = 2
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), str(tmp_path)], env=shim_env(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(world)]
    outs = []
    try:
        for pr in procs:
            outs.append(pr.communicate(timeout=300)[0].decode())
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    for r, pr in enumerate(procs):
        assert pr.returncode == 0, "rank %d failed:\n%s" % (r, outs[r][-3000:])
    for r in range(world):
        res = json.load(open(tmp_path / ("out%d.json" % r)))
        assert res["rc"] == -4 and res["msg"].startswith("subst_counts: one rank only") and "2" in res["msg"] and res["untouched"], res
