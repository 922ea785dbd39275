"""paml_amd_model_gradient: the derivative of lnL with respect to every input of the engine (effective lengths, rate matrices, freqK,
root frequencies) and the weighted outer products W they are pulled back from, in one engine call.  Reference: the numpy restatement
tests/modelgrad_ref.py (pinned on the CPU by tests/test_modelgrad_cpu.py) fed with the matrices paml_amd_get_pmat returns after the call.
Every tolerance is 1e-9 of the largest magnitude of the array compared, the project's parity bar; lnL against eval within 1e-10 |lnL|."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import ancestral_ref as ar
import gradient_ref as gr
import modelgrad_ref as mr
from paml_amd import engine, models
from paml_amd.engine import engine_for
from paml_amd.problem import EIGEN_QMAT, EIGEN_UVROOT
from test_ancestral_gpu import _rooted_at_tip0
from test_engine_gpu import _branch_model_problem
from test_multirank_gpu import shim_env
from test_oracle_golden import _closed_form

pytestmark = pytest.mark.gpu
OUTPUTS = ("g_eff", "g_freqK", "g_pi", "g_A", "W")
RTOL = 1e-9


def _close(name, got, want):
    scale = float(np.max(np.abs(want)))
    err = float(np.max(np.abs(got - want)))
    print("%s: largest error %.3e of magnitude %.3e" % (name, err, scale))
    assert got.shape == want.shape and err <= RTOL * scale, (name, err, scale)


def _check(pb, eng=None, outputs=OUTPUTS):
    """One model_gradient call on pb against the restatement; returns (engine, result)."""
    eng = eng or engine_for(pb)
    t = pb.tree
    base = eng.eval(t.branch, pb.gene_rate)["lnL"]
    got = eng.model_gradient(t.branch, pb.gene_rate, want_pairs=True)
    assert abs(got["lnL"] - base) <= 1e-10 * abs(base), (got["lnL"], base)
    ref = mr.model_gradient_of(pb, ar.matrices_from_engine(eng, pb))      # (the matrices of the call just made)
    for key in outputs:
        _close(key, got[key], ref[key])
    assert not got["g_eff"][:, :, t.root].any() and not got["W"][:, :, t.root].any()
    # sum_{g,k} g_eff d tau / d branch[v] is the branch gradient
    grad = eng.gradient(t.branch, pb.gene_rate)["grad"]
    _, dtau = mr.eff_lengths(pb)
    _close("grad", (got["g_eff"] * dtau).sum(axis=(0, 1)), grad)
    return eng, got


# ---- parity with the restatement ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [s[0] for s in gr.REVERSIBLE_SHAPES])
def test_model_gradient_matches_the_restatement(name):
    _check(gr.reversible_problem(name))


@pytest.mark.parametrize("n", [21, 64])
def test_model_gradient_at_the_ends_of_the_matrix_core_range(n):
    _check(mr.small_problem(n, K=1))


def test_model_gradient_on_the_lane_kernel_at_20_states():
    """A keep-partials engine runs 20 states on the one-pattern-per-lane kernels; the default engine takes them to the matrix cores."""
    pb = mr.small_problem(20)
    _check(pb, engine_for(pb, flags=engine.KEEP_PARTIALS))
    _check(pb)


def test_model_gradient_at_4_states_and_61_states_with_two_genes():
    _check(mr.small_problem(4, tips=9))
    _check(mr.small_problem(61, tips=6, n_genes=2))


# ---- kinds and configurations ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,K,kind", [(4, 2, "k80"), (20, 1, "jc")])
def test_model_gradient_of_the_closed_form_kinds(n, K, kind):
    _check(_closed_form(mr.small_problem(n, tips=8, K=K, ambiguity=(n == 4)), kind))


def test_model_gradient_of_the_cijk_kind_on_the_brown_golden():
    _check(helpers.problem_from_golden(helpers.load_golden("brown_hky85")))


@pytest.mark.parametrize("n,K,genes", [(4, 2, 1), (61, 2, 2)])
def test_model_gradient_with_eigen_systems_of_different_pi_per_label(n, K, genes):
    _check(_branch_model_problem(n, K, 300 + n + K, n_genes=genes))


@pytest.mark.parametrize("n", [4, 61])
def test_model_gradient_with_a_model_and_pi_per_gene(n):
    _check(helpers.give_genes_their_own_models(mr.small_problem(n, tips=6, n_genes=3), seed=n))


@pytest.mark.parametrize("n", [4, 61])
def test_model_gradient_on_a_tree_rooted_at_a_tip(n):
    """Plain states only, as the gradient's test of a tip root: on an alignment with ambiguity codes the evaluation (as the oracle) has
    no value for a tree rooted at a tip, so its lnL is no reference there (tools/modelgrad_host_check.py holds that case against the
    restatement)."""
    _check(_rooted_at_tip0(mr.small_problem(n, tips=7, seed=1, ambiguity=False)))


def test_model_gradient_on_a_polytomy():
    _check(mr.small_problem(5, tips=9, polytomy=True))
    _check(mr.small_problem(61, tips=8, polytomy=True, K=1))


# ---- deep trees: the rescaled chains ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,tips,K,every", [(20, 40, 1, 8), (61, 30, 2, 5)])
def test_model_gradient_deep_tree_with_rescaling(n, tips, K, every):
    _check(helpers.random_problem(n, tips, 70, K=K, seed=77 + n, scale_every=every))


# ---- repeated eigenvalues: what the series of Psi is for ------------------------------------------------------------------------------

def test_model_gradient_with_repeated_eigenvalues_jc_like_61_states():
    _check(_closed_form(mr.small_problem(61, tips=6, K=1), "jc"), outputs=("g_A", "g_eff", "W"))


def test_model_gradient_with_repeated_eigenvalues_equal_frequency_codons():
    pb = mr.small_problem(61, tips=6, K=1, seed=2)
    pb.pi = np.full_like(pb.pi, 1.0 / 61)
    U, V, root, _ = models.codon_m0_eigen(2.0, 1.0, pb.pi[0])      # (omega = 1: the equal-frequency matrix keeps its symmetries)
    gaps = np.abs(np.diff(np.sort(root)))
    assert (gaps < 1e-9).sum() >= 10      # (whole blocks of equal eigenvalues, to rounding)
    pb.eigen = [dict(kind=EIGEN_UVROOT, U=U, V=V, Root=root)]
    _check(pb, outputs=("g_A", "g_eff", "W"))


# ---- same bytes across workspace sizes and calls --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,arena_mb", [(4, "0.25"), (61, "4")])
def test_model_gradient_has_the_same_bytes_whatever_the_workspace(n, arena_mb, monkeypatch):
    """The pattern count is just past one summation segment of W (61 states, one gene) or two (4 states, two genes: one of them is longer
    than a segment wherever the cut falls); the small workspace walks three or more batches per gene, which cut the segments: a cut
    segment is carried across the borders in the same accumulator."""
    seg = engine.model_gradient_info()["segment"]
    genes = 2 if n == 4 else 1
    pb = helpers.random_problem(n, 7, genes * seg + 70, K=2 if n == 4 else 1, seed=31 + n, n_genes=genes, ambiguity=True)
    pb.weights[5::13] = 0
    t = pb.tree
    eng = engine_for(pb)
    one = eng.model_gradient(t.branch, pb.gene_rate, want_pairs=True)
    assert engine.model_gradient_info()["last_batches"] == genes
    again = eng.model_gradient(t.branch, pb.gene_rate, want_pairs=True)
    monkeypatch.setenv("PAML_AMD_MODELGRAD_ARENA_MB", arena_mb)
    many = eng.model_gradient(t.branch, pb.gene_rate, want_pairs=True)
    info = engine.model_gradient_info()
    assert info["last_batches"] >= 3 + genes and info["last_kernel_ms"] > 0, info      # (three or more in the gene longer than a segment)
    for other in (again, many):
        assert np.float64(one["lnL"]).tobytes() == np.float64(other["lnL"]).tobytes()
        for key in OUTPUTS:
            assert one[key].tobytes() == other[key].tobytes(), key
    ref = mr.model_gradient_of(pb, ar.matrices_from_engine(eng, pb))
    for key in OUTPUTS:
        _close(key, many[key], ref[key])


# ---- state ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 61])
def test_the_other_calls_return_what_they_returned_before(n):
    pb = mr.small_problem(n, tips=7)
    t = pb.tree
    eng = engine_for(pb)

    def snapshot():
        ev = eng.eval(t.branch, pb.gene_rate, want_lnf=True)
        g = eng.gradient(t.branch, pb.gene_rate, want_lnf=True, want_scores=True)
        nni = eng.nni_scores(t.branch, pb.gene_rate)
        return [np.float64(ev["lnL"]).tobytes(), ev["lnf"].tobytes(), np.float64(g["lnL"]).tobytes(), g["grad"].tobytes(), g["scores"].tobytes(),
                np.float64(nni["lnL0"]).tobytes(), nni["lnL"].tobytes()]
    before = snapshot()
    eng.model_gradient(t.branch, pb.gene_rate, want_pairs=True)
    assert snapshot() == before


@pytest.mark.parametrize("n", [4, 61])
def test_patterns_of_weight_zero_change_nothing(n):
    pb = mr.small_problem(n, tips=7)
    live = pb.weights > 0
    assert not live.all()
    eng, got = _check(pb)
    # the same alignment without those patterns
    q = pb.slice_patterns(0, pb.n_patt)
    q.z = np.ascontiguousarray(pb.z[:, live])
    q.weights = pb.weights[live].copy()
    q.gene_off = np.array([0, int(live.sum())], dtype=np.int32)
    dropped = engine_for(q).model_gradient(q.tree.branch, q.gene_rate, want_pairs=True)
    for key in OUTPUTS:
        _close(key, got[key], dropped[key])
    # and with other characters in them
    r = pb.slice_patterns(0, pb.n_patt)
    r.z = pb.z.copy()
    r.z[:, ~live] = (r.z[:, ~live] + 1) % n
    other = engine_for(r).model_gradient(r.tree.branch, r.gene_rate, want_pairs=True)
    for key in OUTPUTS:
        assert got[key].tobytes() == other[key].tobytes(), key


# ---- arguments --------------------------------------------------------------------------------------------------------------------------

def test_argument_errors_and_null_outputs():
    pb = mr.small_problem(4, tips=7)
    t = pb.tree
    eng = engine_for(pb)
    L = eng._L
    full = eng.model_gradient(t.branch, pb.gene_rate, want_pairs=True)
    L.paml_amd_model_gradient.argtypes = [C.c_void_p] * 9
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    br, gr_, lnl = np.ascontiguousarray(t.branch), np.ascontiguousarray(pb.gene_rate), np.zeros(1)
    EINVAL, EUNSUPPORTED = -1, -4

    def bad(e, rc, code, text):
        assert rc == code, rc
        msg = L.paml_amd_last_error(e._h).decode()
        assert msg.startswith("model_gradient") and text in msg, msg
    bad(eng, L.paml_amd_model_gradient(eng._h, None, None, p(lnl), None, None, None, None, None), EINVAL, "null argument")
    bad(eng, L.paml_amd_model_gradient(eng._h, p(br), None, None, None, None, None, None, None), EINVAL, "null argument")
    fresh = engine.Engine(4, 7, 70)
    bad(fresh, L.paml_amd_model_gradient(fresh._h, p(br), None, p(lnl), None, None, None, None, None), EINVAL, "before set_tips/set_tree/set_pi/set_classes/set_eigen")
    # every output by itself, the others NULL: the same bytes as together
    for i, key in enumerate(OUTPUTS):
        out = np.zeros_like(full[key])
        args = [None] * 5
        args[i] = p(out)
        assert L.paml_amd_model_gradient(eng._h, p(br), p(gr_), p(lnl), *args) == 0, L.paml_amd_last_error(eng._h).decode()
        assert out.tobytes() == full[key].tobytes() and np.float64(lnl[0]).tobytes() == np.float64(full["lnL"]).tobytes(), key
    pq = helpers.random_problem(4, 7, 70, seed=5)
    Q = pq.eigen[0]["U"] @ np.diag(pq.eigen[0]["Root"]) @ pq.eigen[0]["V"]
    pq.eigen = [dict(kind=EIGEN_QMAT, Q=np.ascontiguousarray(Q))]
    eq = engine_for(pq)
    bad(eq, L.paml_amd_model_gradient(eq._h, p(np.ascontiguousarray(pq.tree.branch)), None, p(lnl), None, None, None, None, None), EUNSUPPORTED, "rate-matrix (UNREST)")


def test_model_gradient_refuses_an_engine_of_two_ranks(tmp_path):
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim", "modelgrad_rank_worker.py")
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
        assert res["rc"] == -4 and res["msg"].startswith("model_gradient: one rank only") and "2" in res["msg"] and res["untouched"], res
