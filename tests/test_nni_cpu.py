"""The yardstick of the NNI tests (tests/nni_ref.py) and the host-only parts pinned on the CPU, before any GPU run: the restatement's lnf
of every canonical swap against oracle.evaluate of the rearranged problem at 1e-9 (the gradient tests' bound for lnf; measured: see the
tests' output, about 1e-14), the canonical list in Python against paml_amd_nni_list, its length on unrooted binary trees, Tree.nni's
trees, and the arithmetic the GPU batching test relies on."""
import os

import numpy as np
import pytest

import helpers
import ancestral_ref as ar
import gradient_ref as gr
import nni_ref as nr
import oracle
from paml_amd import engine
from paml_amd.problem import balanced_tree
from test_gradient_cpu import _irreversible_cases

CTL = os.path.join(helpers.GOLDEN, "ctl")


def _restatement_against_the_oracle(pb, scale_every=None):
    got = nr.nni_scores_of(pb, ar.matrices_from_oracle(pb))
    ref0 = oracle.evaluate(pb)
    assert np.max(np.abs(got["lnf0"] - ref0["lnf"])) <= 1e-9
    assert len(got["swaps"]) >= 1
    worst = 0.0
    for i, (v, s, x) in enumerate(got["swaps"]):
        ref = oracle.evaluate(nr.swapped_problem(pb, v, s, x, scale_every))
        worst = max(worst, float(np.max(np.abs(got["lnf"][i] - ref["lnf"]))))
    print("%d swaps: largest |lnf - oracle| %.3e" % (len(got["swaps"]), worst))
    assert worst <= 1e-9


@pytest.mark.parametrize("name", [s[0] for s in gr.REVERSIBLE_SHAPES])
def test_restatement_equals_the_oracle_on_the_rearranged_tree(name):
    _restatement_against_the_oracle(gr.reversible_problem(name), nr.scale_every_of(name))


@pytest.mark.parametrize("name", [c[0] for c in _irreversible_cases()])
def test_restatement_equals_the_oracle_on_irreversible_models(name):
    _restatement_against_the_oracle(dict(_irreversible_cases())[name]())


def _trees():
    out = [gr.reversible_problem(s[0]).tree for s in gr.REVERSIBLE_SHAPES]
    out += [c[1]().tree for c in _irreversible_cases()]
    out += [balanced_tree(k) for k in (4, 5, 8, 13)]
    out.append(helpers.random_problem(4, 30, 4, seed=9).tree)
    return out


def test_python_list_equals_the_librarys():
    for t in _trees():
        ptr, flat = t.csr()
        lib_list = engine.nni_list(t.n_tips, t.n_nodes, t.root, ptr, flat)
        mine = t.nni_swaps()
        assert mine.dtype == np.int32 and mine.shape == lib_list.shape and np.array_equal(mine, lib_list)
        # every entry is a swap as the engine defines one
        f = t.father()
        for v, s, x in mine:
            assert v != t.root and t.sons[v] and s in t.sons[v] and x != v and x in t.sons[f[v]]


def test_an_unrooted_binary_tree_has_two_swaps_per_internal_branch():
    seen = 0
    for t in _trees():
        binary = len(t.sons[t.root]) == 3 and all(len(t.sons[v]) in (0, 2) for v in range(t.n_nodes) if v != t.root)
        if binary:
            seen += 1
            assert len(t.nni_swaps()) == 2 * (t.n_tips - 3), t.n_tips
    assert seen >= 4


def test_the_polytomy_shape_has_the_count_of_the_issue():
    """61 states, 14 tips, a polytomy: 32 swaps."""
    assert len(gr.reversible_problem("61-14tips-polytomy").tree.nni_swaps()) == 32


def test_nni_leaves_every_node_with_one_father():
    for t in _trees():
        for v, s, x in t.nni_swaps():
            q = t.nni(v, s, x)
            count = np.zeros(t.n_nodes, dtype=int)
            for u in range(t.n_nodes):
                for c in q.sons[u]:
                    count[c] += 1
            assert count[q.root] == 0 and (np.delete(count, q.root) == 1).all()
            assert q.father()[s] == t.father()[v] and q.father()[x] == v
            assert [len(c) for c in q.sons] == [len(c) for c in t.sons]
            assert q.branch is t.branch and q.label is t.label and q.sons is not t.sons
            # every node is still reached from the root
            seen, stack = 0, [q.root]
            while stack:
                u = stack.pop()
                seen += 1
                stack.extend(q.sons[u])
            assert seen == t.n_nodes
    with pytest.raises(ValueError):
        t.nni(t.root, t.sons[t.root][0], 0)


def test_one_mebibyte_cannot_hold_the_batching_case():
    """The GPU batching test relies on it: 61 states x 9 tips x 3000 patterns, one class, all 12 swaps.  The bytes a pattern takes in
    the workspace, as DESIGN 4 V documents them: 2 K n_int (n_s + 1) doubles for the down partials and the outer messages (n_s = 64 on
    the matrix cores), then 2 K + 1 doubles (f_hk and its log factor per class, lnf) per swap and for the present tree."""
    K, n_int, n_swaps, n_patt = 1, 9 - 2, 2 * (9 - 3), 3000      # (an unrooted binary tree of 9 tips has 7 internal nodes)
    per_patt = 2 * K * n_int * (64 + 1) * 8 + (n_swaps + 1) * (2 * K + 1) * 8
    assert per_patt >= 2 * 7 * 65 * 8 and n_patt * per_patt > 1 << 20
    assert 64 * per_patt <= 1 << 20      # (and one tile with all swaps fits: the patterns are walked in batches, not the swaps in groups)


@pytest.mark.parametrize("ctl,word", [("brown_hky85_clock.ctl", "clock"), ("brown_hky85_adg.ctl", "rho")])
def test_host_refuses_clocks_and_rho_models_by_name(ctl, word):
    """Before anything reaches the engine: pamlh_nni_scores, pamlh_apply_nni and pamlh_nni_search alike."""
    from paml_amd import hostlib
    a = hostlib.Analysis(os.path.join(CTL, ctl), "baseml")
    x = np.array(a.default_x())
    for call in (lambda: a.nni_scores(x), lambda: a.apply_nni(a.n_tips + 1, 0, 1), lambda: a.nni_search(x)):
        with pytest.raises(RuntimeError, match=word):
            call()
