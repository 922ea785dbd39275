"""The yardstick of the SPR tests (tests/spr_ref.py) and the host-only parts pinned on the CPU, before any GPU run: the restatement's lnf
of every move of the canonical list against oracle.evaluate of the rearranged problem at 1e-11 (measured: see the tests' output, about
4e-15), the canonical list in Python against paml_amd_spr_list at three radii, the radius-1 list against the NNI neighbours as sets of
splits with the counts of moves and of topologies pinned per tree, Tree.spr's trees and refusals, and the host's refusals."""
import numpy as np
import pytest

import helpers
import gradient_ref as gr
import nni_ref as nr
import spr_ref as sr
import oracle
from paml_amd import engine
from paml_amd.problem import balanced_tree
from test_ancestral_gpu import _rooted_at_tip0
from test_engine_gpu import _branch_model_problem


def _restatement_against_the_oracle(pb, scale_every=None, phi=0.5):
    got = sr.spr_scores_of(pb, phi)
    assert np.max(np.abs(got["lnf0"] - oracle.evaluate(pb)["lnf"])) <= 1e-11
    assert len(got["moves"]) >= 20
    worst = 0.0
    for i, (s, x) in enumerate(got["moves"]):
        ref = oracle.evaluate(sr.moved_problem(pb, s, x, phi, scale_every))
        worst = max(worst, float(np.max(np.abs(got["lnf"][i] - ref["lnf"]))))
    print("%d moves, phi %.1f: largest |lnf - oracle| %.3e" % (len(got["moves"]), phi, worst))
    assert worst <= 1e-11


@pytest.mark.parametrize("phi", [0.5, 0.3])
def test_restatement_equals_the_oracle_on_the_rearranged_tree(phi):
    name = "4-K3-amb-scale3-2genes"
    _restatement_against_the_oracle(gr.reversible_problem(name), nr.scale_every_of(name), phi)


def test_restatement_equals_the_oracle_with_eigen_systems_per_label():
    """label[f] = label[x] picks another eigen system for the branch above f: the move is not a permutation of the present matrices."""
    _restatement_against_the_oracle(_branch_model_problem(4, 2, 306))


def _trees():
    out = [gr.reversible_problem(s[0]).tree for s in gr.REVERSIBLE_SHAPES]
    out.append(_rooted_at_tip0(helpers.random_problem(4, 9, 4, seed=55)).tree)
    out += [balanced_tree(k) for k in (5, 8)]
    return out


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_python_list_equals_the_librarys(radius):
    for t in _trees():
        ptr, flat = t.csr()
        lib_list = engine.spr_list(t.n_tips, t.n_nodes, t.root, ptr, flat, radius)
        mine = t.spr_moves(radius)
        assert mine.dtype == np.int32 and mine.shape == lib_list.shape and np.array_equal(mine, lib_list)
        assert len(mine) >= 1
        f = t.father()
        for s, x in mine:      # every entry is a move as the engine defines one
            assert s != t.root and f[s] != t.root and len(t.sons[f[s]]) == 2 and x != t.root and x != f[s] and x not in t.sons[f[s]]
    t = _trees()[0]
    full, near, two = t.spr_moves(0), t.spr_moves(1), t.spr_moves(2)
    as_set = lambda m: set(map(tuple, m))
    assert as_set(near) < as_set(two) < as_set(full)
    # s in node order, x in node order within s
    assert [tuple(r) for r in full] == sorted(tuple(r) for r in full)


# (tips, seed of helpers.random_problem) -> moves at radius 1, their topologies, moves without limit, the SPR neighbours they reach.
# How many moves there are, and how many neighbours they miss, depends on where the root sits in the shape, so the counts are pinned
# per tree: the first three are the counts the feature was specified with, the last three the trees README and DESIGN 4 X quote.
COUNTS = {(5, 3): (8, 4, 16, 12), (9, 3): (32, 12, 126, 106), (12, 5): (48, 18, 308, 278),
          (5, 5): (10, 4, 14, 8), (9, 9): (30, 12, 132, 114), (12, 12): (50, 18, 296, 264)}


@pytest.mark.parametrize("n_tips,seed", sorted(COUNTS))
def test_radius_one_is_the_nni_neighbourhood(n_tips, seed):
    """As sets of splits of the unrooted trees; an unrooted binary tree of n tips has 2 (n - 3) NNI and 2 (n - 3)(2 n - 7) SPR neighbours.
    The unlimited list reaches a part of the latter only: the prunes of the side of a branch that holds the root are out of scope."""
    t = helpers.random_problem(4, n_tips, 4, seed=seed).tree
    assert len(t.sons[t.root]) == 3 and all(len(t.sons[v]) in (0, 2) for v in range(t.n_nodes) if v != t.root)
    base = sr.splits_of(t)
    near = {sr.splits_of(t.spr(s, x)) for s, x in t.spr_moves(1)}
    nni = {sr.splits_of(t.nni(v, s, x)) for v, s, x in t.nni_swaps()}
    assert near == nni and len(nni) == 2 * (n_tips - 3) and base not in near
    every = {sr.splits_of(t.spr(s, x)) for s, x in t.spr_moves()}
    assert near <= every and base not in every
    total = 2 * (n_tips - 3) * (2 * n_tips - 7)
    assert total == {5: 12, 9: 132, 12: 306}[n_tips]
    print("%d tips: %d moves at radius 1 give %d topologies; %d moves without limit reach %d of the %d SPR neighbours"
          % (n_tips, len(t.spr_moves(1)), len(near), len(t.spr_moves()), len(every), total))
    assert (len(t.spr_moves(1)), len(near), len(t.spr_moves()), len(every)) == COUNTS[n_tips, seed]
    assert len(near) < len(every) <= total
    for topo in every:      # one prune and regraft away: the two trees share all but the splits along one path
        assert len(topo) == len(base)


def test_spr_leaves_every_node_with_one_father_and_keeps_the_length():
    for t in _trees():
        t.label = np.arange(t.n_nodes, dtype=np.int32)      # (every branch its own label: where the labels go is visible)
        fa = t.father()
        before = ([[int(u) for u in l] for l in t.sons], t.branch.copy())
        for phi in (0.5, 0.0, 1.0, 0.3):
            for s, x in t.spr_moves():
                q = t.spr(s, x, phi)
                f, c = int(fa[s]), next(int(u) for u in t.sons[fa[s]] if u != s)
                count = np.zeros(t.n_nodes, dtype=int)
                for u in range(t.n_nodes):
                    for v in q.sons[u]:
                        count[v] += 1
                assert count[q.root] == 0 and (np.delete(count, q.root) == 1).all()
                live = np.arange(t.n_nodes) != t.root
                assert abs(q.branch[live].sum() - t.branch[live].sum()) <= 1e-12
                assert q.sons[f] == [x, s] and q.father()[c] == fa[f] and q.father()[f] == fa[x]
                assert q.branch[c] == t.branch[c] + t.branch[f] and q.branch[s] == t.branch[s]
                assert q.branch[f] == (1 - phi) * t.branch[x] and q.branch[x] == phi * t.branch[x]
                assert q.label[f] == t.label[x] and (np.delete(q.label, f) == np.delete(t.label, f)).all()
                assert (q.root, q.n_nodes, q.n_tips) == (t.root, t.n_nodes, t.n_tips)
                assert q.branch is not t.branch and q.label is not t.label and q.sons is not t.sons
                seen, stack = 0, [q.root]      # every node is still reached from the root
                while stack:
                    u = stack.pop()
                    seen += 1
                    stack.extend(q.sons[u])
                assert seen == t.n_nodes
        assert [[int(u) for u in l] for l in t.sons] == before[0] and np.array_equal(t.branch, before[1])      # the tree itself is untouched


def test_spr_refuses_every_invalid_kind_of_move():
    t = gr.reversible_problem("61-14tips-polytomy").tree
    fa = t.father()
    s, x = (int(u) for u in t.spr_moves()[0])
    f = int(fa[s])
    c = next(int(u) for u in t.sons[f] if u != s)
    under_root = int(t.sons[t.root][0])
    from paml_amd.problem import parse_newick
    tp = parse_newick("((1: 0.1, 2: 0.1, 3: 0.1): 0.1, (4: 0.1, (5: 0.1, 6: 0.1): 0.1): 0.1, 7: 0.1);")      # a polytomy below the root
    poly = next(v for v in range(tp.n_nodes) if v != tp.root and len(tp.sons[v]) > 2)
    with pytest.raises(ValueError, match="exactly two sons"):
        tp.spr(int(tp.sons[poly][0]), 3)
    assert len(tp.spr_moves()) >= 1 and all(tp.father()[s] != poly for s, _ in tp.spr_moves())
    inner = next(v for v in range(t.n_tips, t.n_nodes) if v != t.root and fa[v] != t.root and len(t.sons[fa[v]]) == 2)
    for move, text in [((t.root, x), "is the root"), ((under_root, x), "father of %d is the root" % under_root),
                       ((s, t.root), "is the root"), ((s, f), "is the father"),
                       ((s, c), "sibling"), ((inner, int(t.sons[inner][0])), "lies in the subtree"), ((inner, inner), "lies in the subtree"),
                       ((t.n_nodes, x), "out of range"), ((s, -1), "out of range")]:
        with pytest.raises(ValueError, match=text):
            t.spr(*move)
    for phi in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="phi"):
            t.spr(s, x, phi)
    assert t.spr(s, x).sons[f] == [x, s]


@pytest.mark.parametrize("ctl,program,word", [("brown_hky85_clock.ctl", "baseml", "clock"), ("brown_hky85_adg.ctl", "baseml", "rho"),
                                              ("pairwise_hiv_f3x4.ctl", "codeml", "runmode = -2")])
def test_host_refuses_clocks_rho_models_and_pairwise_runs_by_name(ctl, program, word):
    """Before anything reaches the engine: pamlh_spr_scores, pamlh_apply_spr and pamlh_spr_search alike."""
    import os
    from paml_amd import hostlib
    a = hostlib.Analysis(os.path.join(helpers.GOLDEN, "ctl", ctl), program)
    x = np.zeros(max(a.np, 1)) if a.is_pairwise() else np.array(a.default_x())
    for call in (lambda: a.spr_scores(x[:a.np]), lambda: a.apply_spr(0, 1, 0.5, x[:a.np]), lambda: a.spr_search(x[:a.np])):
        with pytest.raises(RuntimeError, match=word):
            call()
