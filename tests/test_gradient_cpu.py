"""The yardstick of the gradient tests (tests/gradient_ref.py) pinned on the CPU, before any GPU run.  On exactly reversible models
(helpers.random_problem) the restatement's grad equals the oracle's branch-local dlnL at every branch to the tolerances
test_eval_branch_matches_oracle uses (rtol 1e-9, atol 1e-9) and its lnf the oracle's to 1e-9.  On models that are NOT reversible with
respect to the gene's pi (eigen systems with their own pi per branch label; trees rooted at a tip are here for the tip root's own code
path) the branch-local form, which re-roots the tree, is no reference: there the restatement is held against central differences of
oracle.evaluate."""
import copy

import numpy as np
import pytest

import helpers
import ancestral_ref as ar
import gradient_ref as gr
import oracle
from test_ancestral_gpu import _rooted_at_tip0
from test_engine_gpu import _branch_model_problem


@pytest.mark.parametrize("name", [s[0] for s in gr.REVERSIBLE_SHAPES])
def test_restatement_equals_the_oracles_branch_derivative_on_reversible_models(name):
    pb = gr.reversible_problem(name)
    t = pb.tree
    got = gr.gradient_of(pb, ar.matrices_from_oracle(pb))
    ref = oracle.evaluate(pb)
    assert np.max(np.abs(got["lnf"] - ref["lnf"])) <= 1e-9
    assert abs(got["lnL"] - ref["lnL"]) <= 1e-10 * abs(ref["lnL"])
    assert got["grad"][t.root] == 0 and not got["scores"][t.root].any()
    for b in range(t.n_nodes):
        if b == t.root:
            continue
        _, dl, _ = oracle.eval_branch(pb, b, np.array([t.branch[b]]))
        assert np.allclose(got["grad"][b], dl[0], rtol=1e-9, atol=1e-9), (b, got["grad"][b], dl[0])


def _central_differences(pb, step=1e-5):
    t = pb.tree
    assert t.branch[[v for v in range(t.n_nodes) if v != t.root]].min() >= 0.01      # (never difference a branch shorter than 10 steps)
    g = np.zeros(t.n_nodes)
    for b in range(t.n_nodes):
        if b == t.root:
            continue
        val = []
        for sgn in (1, -1):
            q = copy.copy(pb)
            q.tree = copy.copy(t)
            q.tree.branch = t.branch.copy()
            q.tree.branch[b] += sgn * step
            val.append(oracle.evaluate(q)["lnL"])
        g[b] = (val[0] - val[1]) / (2 * step)
    return g


def _irreversible_cases():
    return [("labels-4-K2", lambda: _branch_model_problem(4, 2, 306)),
            ("labels-61-K2-2genes", lambda: _branch_model_problem(61, 2, 363, n_genes=2)),
            ("tiproot-4-K2", lambda: _rooted_at_tip0(helpers.random_problem(4, 9, 140, K=2, seed=55))),
            ("tiproot-61-K2", lambda: _rooted_at_tip0(helpers.random_problem(61, 9, 140, K=2, seed=56)))]


@pytest.mark.parametrize("name", [c[0] for c in _irreversible_cases()])
def test_restatement_equals_central_differences_of_the_oracle(name):
    """Step 1e-5, every branch >= 0.01; the deviation relative to max(1, |g|).  Measured with the oracle's matrices: 7.6e-9
    (labels, 4 states), 1.1e-8 (labels, 61 states, two genes), 1.8e-7 and 7.7e-9 (the tip-rooted trees at 4 and 61 states).  Allowance 1e-5: about 50 x the largest of them; the error of the re-rooted form that this guards against is >= 0.2."""
    pb = dict(_irreversible_cases())[name]()
    got = gr.gradient_of(pb, ar.matrices_from_oracle(pb))
    fd = _central_differences(pb)
    dev = float(np.max(np.abs(got["grad"] - fd) / np.maximum(1.0, np.abs(fd))))
    print("%s: largest deviation from central differences %.3e" % (name, dev))
    assert dev <= 1e-5
    assert np.max(np.abs(got["lnf"] - oracle.evaluate(pb)["lnf"])) <= 1e-9


def test_one_mebibyte_cannot_hold_the_batching_case():
    """The GPU batching test relies on it: 61 states x 9 tips x 3000 patterns, one class.  The bytes a pattern takes in the workspace, as
    DESIGN 4 U documents them: 2 K n_int (n_s + 1) doubles for the down partials and the outer messages (n_s = 64 on the matrix cores),
    3 K n_nodes doubles for the two sums and their log factor per class, n_nodes + 1 for the scores and lnf."""
    K, n_int, n_nodes, n_patt = 1, 9 - 2, 2 * 9 - 2, 3000      # (an unrooted binary tree of 9 tips has 7 internal nodes)
    per_patt = 2 * K * n_int * (64 + 1) * 8 + 3 * K * n_nodes * 8 + (n_nodes + 1) * 8
    assert per_patt >= 2 * 7 * 65 * 8 and n_patt * per_patt > 1 << 20
