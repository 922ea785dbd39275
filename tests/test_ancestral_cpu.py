"""The yardstick of the ancestral-reconstruction tests (tests/ancestral_ref.py) pinned on the CPU, before any GPU run: on 5 tips x 4 states
x 12 patterns its joint recursion equals exhaustive enumeration of all 4^3 assignments, and its marginal equals the oracle's
node_posterior to the tolerances test_node_posterior_matches_oracle uses (rtol 1e-9, atol 1e-13)."""
import numpy as np
import pytest

import helpers
import ancestral_ref as ar

import oracle


@pytest.mark.parametrize("amb", [False, True])
def test_joint_restatement_equals_exhaustive_enumeration(amb):
    pb = helpers.random_problem(4, 5, 12, seed=7, ambiguity=amb)
    P, tips = ar.matrices_from_oracle(pb), ar.tips_of(pb)
    assert pb.tree.n_nodes - pb.tree.n_tips == 3
    states, ln_best = ar.joint(P, pb.pi, tips, pb.tree)
    brute = ar.enumerate_joint(P, pb.pi, tips, pb.tree)
    assert np.max(np.abs(ln_best - brute)) <= 1e-12
    assert np.max(np.abs(ar.joint_score(P, pb.pi, tips, pb.tree, states) - brute)) <= 1e-12
    gap = ar.second_best_gap(P, pb.pi, tips, pb.tree)
    assert np.all(gap >= 0)


@pytest.mark.parametrize("K,amb,genes", [(1, False, 1), (2, True, 1), (2, False, 2)])
def test_marginal_restatement_equals_the_oracle(K, amb, genes):
    pb = helpers.random_problem(4, 5, 12, K=K, seed=11 + K, ambiguity=amb, n_genes=genes)
    P, tips = ar.matrices_from_oracle(pb), ar.tips_of(pb)
    post = ar.marginal(P, pb.pi, pb.freqK, tips, pb.tree)
    for qi, node in enumerate(range(pb.tree.n_tips, pb.tree.n_nodes)):
        ref = oracle.node_posterior(pb, node)
        assert np.allclose(post[qi], ref, rtol=1e-9, atol=1e-13), (node, float(np.max(np.abs(post[qi] - ref))))


def test_one_mebibyte_cannot_hold_the_batching_case():
    """The GPU batching tests rely on it: 61 states x 9 tips x 3000 patterns, one class, every internal node queried.  The bytes a
    pattern takes in the workspace, as DESIGN 4 T documents them: marginal 2 K n_int (n_s + 1) doubles (n_s = 64 on the matrix cores)
    plus per queried node n doubles, one double and one byte; joint n_int n (8 + 1) bytes."""
    n, K, n_int, n_patt = 61, 1, 9 - 2, 3000      # (an unrooted binary tree of 9 tips has 7 internal nodes)
    marginal = 2 * K * n_int * (64 + 1) * 8 + n_int * (n * 8 + 8 + 1)
    joint = n_int * n * (8 + 1)
    assert n_patt * marginal > 1 << 20 and n_patt * joint > 1 << 20
