"""numpy restatement of the attachment scores (paml_amd_attach_scores), from the definition at the top of paml_amd/csrc/kernels_attach.h.
The tree's per-branch matrices are the CPU oracle's (ancestral_ref.matrices_from_oracle); a row's three matrices P_v(t_up), P_v(t_dn)
and P_{pendant_label}(t_pend) come from oracle.pmat_branch, the derivative matrices of the role's branch from edge_ref.pmat3.  For the row
(q, v, role) with lengths (t_up, t_dn, t_pend), f = the father of v, M_c = P_c L_c:

  H_v  = A_f prod_{c son of f, c != v} M_c                (A_root = pi, a root that is a tip: pi o its indicator)
  U    = P_v(t_up)^T H_v;   D = P_v(t_dn) L_v;   T = T_{t_pend}[code_q],  T_t[c][y] = sum_{x in set(c)} P_pend(t)[y][x]
  f_hk = sum_y U(y) D(y) T(y);    f'_hk, f''_hk: the one factor of `role` formed from dP/dt, d2P/dt2
  lnf = log sum_k freqK_k f_hk;  g1 = sum_k freqK_k f'_hk / sum_k freqK_k f_hk;  g2 = sum_k freqK_k f''_hk / sum_k freqK_k f_hk - g1^2
  lnL, d1, d2 = the sums of w lnf, w g1, w g2 over the patterns of weight > 0

Nothing is re-rooted and no reversibility is assumed.  Linear domain, no scaling: for the sizes of the tests."""
from __future__ import annotations

import dataclasses

import numpy as np

import edge_ref
from ancestral_ref import _father, _indicator, matrices_from_oracle, tips_of
from placement_ref import _with_branch, inserted_problem


def _pend_problem(pb, pendant_label):
    """(problem, node): pb with a non-root tip relabelled pendant_label: the slot the pendant's matrices are made in."""
    slot = 0 if pb.tree.root != 0 else 1
    lab = np.array(pb.tree.label, dtype=np.int32)
    lab[slot] = pendant_label
    return _with_branch(pb, pb.tree.branch, lab), slot


def row_matrices(pb, g, k, v, role, t3, pendant_label=0):
    """[3][3][n][n]: for the up, dn and pendant branch of the row, P from oracle.pmat_branch and, for the branch of the role, dP and d2P
    from edge_ref.pmat3 (zeros elsewhere)."""
    import oracle
    out = np.zeros((3, 3, pb.n, pb.n))
    qp, slot = _pend_problem(pb, pendant_label)
    for j, (prob, node) in enumerate(((pb, v), (pb, v), (qp, slot))):
        br = np.array(prob.tree.branch, dtype=np.float64)
        br[node] = t3[j]
        out[j, 0] = oracle.pmat_branch(_with_branch(prob, br), g, k, node)
        if j == role:
            out[j, 1:] = edge_ref.pmat3(prob, g, k, node, t3[j])[1:]
    return out


def attach_scores(pb, queries, rows, t3, pendant_label=0, P=None, passes=None):
    """dict(lnf, g1, g2 [n_rows][n_patt]; lnL, d1, d2 [n_rows]; lnf0 [n_patt], lnL0) of the definition above."""
    tree = pb.tree
    P = matrices_from_oracle(pb) if P is None else P
    per_class, lnf0 = edge_ref.tree_passes(pb, P) if passes is None else passes
    z, sets, _ = tips_of(pb)
    n, nt = pb.n, tree.n_tips
    father = _father(tree)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    t3 = np.asarray(t3, dtype=np.float64).reshape(-1, 3)
    queries = np.atleast_2d(np.asarray(queries, dtype=np.uint8))
    weights = np.asarray(pb.weights, dtype=np.float64)
    F = np.zeros((3, len(rows), len(weights)))
    for g, k, lo, hi, pi_g, L, M, A in per_class:
        for i, (q, v, role) in enumerate(rows):
            q, v, role = int(q), int(v), int(role)
            H = A[father[v]].copy()
            for c in tree.sons[father[v]]:
                if c != v:
                    H = H * M[c]
            Lv = L[v] if v >= nt else _indicator(z[v, lo:hi], sets, n)
            mats = row_matrices(pb, g, k, v, role, t3[i], pendant_label)
            codes = queries[q, lo:hi]
            for d in range(3 if role >= 0 else 1):
                pick = [d if role == j else 0 for j in range(3)]
                U = H @ mats[0, pick[0]]
                D = Lv @ mats[1, pick[1]].T
                table = np.stack([mats[2, pick[2]][:, s].sum(axis=1) for s in sets])
                F[d, i, lo:hi] += pb.freqK[k] * (U * D * table[codes]).sum(axis=1)
    lnf = np.log(F[0])
    g1 = F[1] / F[0]
    g2 = F[2] / F[0] - g1 * g1
    live = weights > 0
    return dict(lnf=lnf, g1=g1, g2=g2, lnL=lnf[:, live] @ weights[live], d1=g1[:, live] @ weights[live], d2=g2[:, live] @ weights[live],
                lnf0=lnf0, lnL0=float(np.dot(weights[live], lnf0[live])))


def attached_problem(pb, v, t3, qrow, pendant_label=0, scale_every=None):
    """(problem, nodes): pb on the tree with the query hung on the branch above v and the three lengths written in; nodes = the enlarged
    tree's nodes below the up, the dn and the pendant branch: the last node, new(v), node n_tips."""
    q = inserted_problem(pb, v, 0.5, float(t3[2]), qrow, pendant_label, scale_every)
    nt = pb.tree.n_tips
    nodes = (q.tree.n_nodes - 1, int(v) if v < nt else int(v) + 1, nt)
    branch = np.array(q.tree.branch, dtype=np.float64)
    for node, t in zip(nodes, t3):
        branch[node] = t
    q.tree = dataclasses.replace(q.tree, branch=branch)
    return q, nodes


def all_rows(pb, n_q, seed=2, pend=0.1):
    """Every non-root v with all four roles, the queries taken in turn, at lengths drawn in [0.5, 2] x (t_v / 2, t_v / 2, pend) (one draw
    per v, shared by its four rows): (rows [n][3], t3 [n][3])."""
    rng = np.random.default_rng(seed)
    rows, tt = [], []
    for v in range(pb.tree.n_nodes):
        if v == pb.tree.root:
            continue
        t = np.array([pb.tree.branch[v] / 2, pb.tree.branch[v] / 2, pend]) * rng.uniform(0.5, 2.0, 3)
        for role in (-1, 0, 1, 2):
            rows.append([(v + role + 1) % n_q, v, role])
            tt.append(t)
    return np.asarray(rows, dtype=np.int32).reshape(-1, 3), np.asarray(tt, dtype=np.float64).reshape(-1, 3)
