"""numpy restatement of the ancestral reconstructions (paml_amd_ancestral_marginal / paml_amd_ancestral_joint), from the definitions at the
top of paml_amd/csrc/kernels_ancestral.h.  Inputs are the per-branch matrices themselves — P[gene][class][node] = P(t) of the branch above
`node`, row = the father's state — so nothing here knows how P(t) is formed.

  tips   = (z [n_tips][n_patt] codes, sets: per code the list of its states, gene_off [n_genes + 1])      (tips_of(pb))
  tree   = anything with n_tips, n_nodes, root and sons (a list of son lists): paml_amd.problem.Tree

marginal(): belief propagation on the tree as an undirected graph (every node gets the product of the messages of ALL its neighbours: no
re-rooting, no reversibility assumed), sum-product in the linear domain.  joint(): the max-sum recursion as kernels_ancestral.h writes it.
max_marginals(): the same propagation in the (max, +) semiring, for the gap between the best and the second-best assignment.
joint_score(): the log probability of a given assignment."""
from __future__ import annotations

import numpy as np

TINY = 1e-300


def tips_of(pb):
    sets = [[int(s) for s in pb.chara_map[c, :pb.n_chara[c]]] for c in range(pb.n_codes)]
    return pb.z, sets, np.asarray(pb.gene_off)


def matrices_from_oracle(pb):
    """P[gene][class][node] from the CPU oracle (tests without a GPU)."""
    import oracle
    n, t = pb.n, pb.tree
    P = np.zeros((pb.n_genes, pb.K, t.n_nodes, n, n))
    for g in range(pb.n_genes):
        for k in range(pb.K):
            for v in range(t.n_nodes):
                if v != t.root:
                    P[g, k, v] = oracle.pmat_branch(pb, g, k, v)
    return P


def matrices_from_engine(eng, pb):
    """P[gene][class][node] as the engine's last evaluation built them (paml_amd_get_pmat)."""
    n, t = pb.n, pb.tree
    P = np.zeros((pb.n_genes, pb.K, t.n_nodes, n, n))
    for g in range(pb.n_genes):
        for k in range(pb.K):
            for v in range(t.n_nodes):
                if v != t.root:
                    P[g, k, v] = eng.get_pmat(g, k, v)
    return P


def _father(tree):
    f = [-1] * tree.n_nodes
    for v in range(tree.n_nodes):
        for s in tree.sons[v]:
            f[s] = v
    return f


def _indicator(z_row, sets, n):
    tab = np.zeros((len(sets), n))
    for c, s in enumerate(sets):
        tab[c, s] = 1
    return tab[z_row]


def _propagate(edge, local, tree, maxsum):
    """Beliefs [n_nodes][n_patt][n] of every node: local(v) combined with the messages of all neighbours.  edge[s] = the matrix of the
    branch above s, [father state][son state] (probabilities, or their logarithms with maxsum)."""
    father = _father(tree)
    nbr = [list(tree.sons[v]) + ([father[v]] if father[v] >= 0 else []) for v in range(tree.n_nodes)]
    memo = {}
    mul = (lambda a, b: a + b) if maxsum else (lambda a, b: a * b)

    def msg(u, v):      # from u to its neighbour v: a function of v's state
        if (u, v) in memo:
            return memo[(u, v)]
        h = local(u)
        for w in nbr[u]:
            if w != v:
                h = mul(h, msg(w, u))
        if father[u] == v:
            A = edge[u].T      # [u's state][v's state]
        else:
            A = edge[v]        # u is v's father: [u's state][v's state]
        out = (h[:, :, None] + A[None]).max(axis=1) if maxsum else h @ A
        memo[(u, v)] = out
        return out

    bel = []
    for v in range(tree.n_nodes):
        b = local(v)
        for w in nbr[v]:
            b = mul(b, msg(w, v))
        bel.append(b)
    return bel


def _locals(pi_g, z, sets, tree, n, maxsum):
    def local(v):
        if v < tree.n_tips:
            h = _indicator(z[v], sets, n)
        else:
            h = np.ones((z.shape[1], n))
        if v == tree.root:
            h = h * pi_g[None, :]
        return np.log(np.maximum(h, TINY)) if maxsum else h
    return local


def marginal(P, pi, freqK, tips, tree, nodes=None):
    """post[n_query][n_patt][n]: sum_k freqK_k Pr(data, state at node | class k), normalised over the states."""
    z, sets, gene_off = tips
    n = P.shape[-1]
    nodes = list(range(tree.n_tips, tree.n_nodes)) if nodes is None else list(nodes)
    post = np.zeros((len(nodes), z.shape[1], n))
    for g in range(len(gene_off) - 1):
        lo, hi = int(gene_off[g]), int(gene_off[g + 1])
        if hi <= lo:
            continue
        pi_g = pi[g if pi.shape[0] > 1 else 0]
        acc = np.zeros((len(nodes), hi - lo, n))
        for k in range(len(freqK)):
            bel = _propagate(P[g, k], _locals(pi_g, z[:, lo:hi], sets, tree, n, False), tree, False)
            for qi, v in enumerate(nodes):
                acc[qi] += freqK[k] * bel[v]
        post[:, lo:hi] = acc / acc.sum(axis=2, keepdims=True)
    return post


def _ln(P):
    return np.log(np.maximum(P, TINY))


def _postorder(tree):
    order, stack = [], [tree.root]
    while stack:
        v = stack.pop()
        order.append(v)
        stack.extend(tree.sons[v])
    return order[::-1]      # the reverse of a pre-order: every node after its whole subtree


def joint(P, pi, tips, tree):
    """(states [n_nodes - n_tips][n_patt] uint8, ln_best [n_patt]) by the max-sum recursion; one class (P[gene][0])."""
    z, sets, gene_off = tips
    n, nt, nn = P.shape[-1], tree.n_tips, tree.n_nodes
    father = _father(tree)
    states = np.zeros((nn - nt, z.shape[1]), dtype=np.uint8)
    ln_best = np.zeros(z.shape[1])
    order = _postorder(tree)
    for g in range(len(gene_off) - 1):
        lo, hi = int(gene_off[g]), int(gene_off[g + 1])
        if hi <= lo:
            continue
        lnP, lnpi = _ln(P[g, 0]), _ln(pi[g if pi.shape[0] > 1 else 0])
        m = hi - lo
        L, C, st = {}, {}, {}
        for v in order:
            if v < nt and v != tree.root:
                continue
            S = np.zeros((m, n))
            for s in tree.sons[v]:      # CSR order
                if s < nt:
                    tab = np.stack([lnP[s][:, sets[c]].max(axis=1) if sets[c] else np.full(n, -np.inf) for c in range(len(sets))])
                    S = S + tab[z[s, lo:hi]]
                else:
                    S = S + L[s]
            if v == tree.root:
                cand = lnpi[None, :] + S
                if v < nt:
                    cand = np.where(_indicator(z[v, lo:hi], sets, n) > 0, cand, -np.inf)
                st[v] = cand.argmax(axis=1)
                ln_best[lo:hi] = cand.max(axis=1)
            else:
                cand = lnP[v][None, :, :] + S[:, None, :]      # [pattern][x][y]
                L[v] = cand.max(axis=2)
                C[v] = cand.argmax(axis=2)      # (the first of equal maxima)
        for v in order[::-1]:
            if v >= nt and v != tree.root:
                st[v] = C[v][np.arange(m), st[father[v]]]
        for v in range(nt, nn):
            states[v - nt, lo:hi] = st[v]
    return states, ln_best


def joint_score(P, pi, tips, tree, states):
    """ln Pr(data, the assignment states[n_nodes - n_tips][n_patt]) [n_patt]; a tip contributes the largest entry over its set."""
    z, sets, gene_off = tips
    n, nt, nn = P.shape[-1], tree.n_tips, tree.n_nodes
    father = _father(tree)
    out = np.zeros(z.shape[1])
    for g in range(len(gene_off) - 1):
        lo, hi = int(gene_off[g]), int(gene_off[g + 1])
        if hi <= lo:
            continue
        lnP, lnpi = _ln(P[g, 0]), _ln(pi[g if pi.shape[0] > 1 else 0])
        m = hi - lo
        h = np.arange(m)
        st = {v: states[v - nt, lo:hi].astype(int) for v in range(nt, nn)}
        if tree.root < nt:      # the root is a tip: the state of its set that scores best
            best = np.full(m, -np.inf)
            for y in range(n):
                ok = _indicator(z[tree.root, lo:hi], sets, n)[:, y] > 0
                sc = lnpi[y] + sum(_branch_score(lnP, s, np.full(m, y), st, z[:, lo:hi], sets, nt, n) for s in tree.sons[tree.root])
                best = np.where(ok, np.maximum(best, sc), best)
            tot = best
            skip = set(tree.sons[tree.root])
        else:
            tot = lnpi[st[tree.root]].copy()
            skip = set()
        for v in range(nn):
            if v == tree.root or v in skip:
                continue
            tot = tot + _branch_score(lnP, v, st[father[v]], st, z[:, lo:hi], sets, nt, n)
        out[lo:hi] = tot
    return out


def _branch_score(lnP, v, xf, st, z, sets, nt, n):
    if v >= nt:
        return lnP[v][xf, st[v]]
    tab = np.stack([lnP[v][:, sets[c]].max(axis=1) if sets[c] else np.full(n, -np.inf) for c in range(len(sets))])      # [code][father state]
    return tab[z[v], xf]


def second_best_gap(P, pi, tips, tree):
    """ln(best) - ln(second best) of the joint assignment over the internal nodes (and a tip's choice within its set counted as one),
    [n_patt]: the second best differs from the best at some internal node v, so it is the largest max-marginal over (v, x != best_v)."""
    z, sets, gene_off = tips
    n, nt, nn = P.shape[-1], tree.n_tips, tree.n_nodes
    gap = np.zeros(z.shape[1])
    for g in range(len(gene_off) - 1):
        lo, hi = int(gene_off[g]), int(gene_off[g + 1])
        if hi <= lo:
            continue
        pi_g = pi[g if pi.shape[0] > 1 else 0]
        bel = _propagate(_ln(P[g, 0]), _locals(pi_g, z[:, lo:hi], sets, tree, n, True), tree, True)
        second = np.full(hi - lo, -np.inf)
        best = bel[nt].max(axis=1) if nn > nt else None
        for v in range(nt, nn):
            b = np.sort(bel[v], axis=1)
            second = np.maximum(second, b[:, -2])
        gap[lo:hi] = best - second
    return gap


def enumerate_joint(P, pi, tips, tree):
    """Exhaustive: the best assignment's score over all n^(internal nodes) assignments, [n_patt] (tiny cases only)."""
    import itertools
    z = tips[0]
    n, ni = P.shape[-1], tree.n_nodes - tree.n_tips
    best = np.full(z.shape[1], -np.inf)
    for combo in itertools.product(range(n), repeat=ni):
        st = np.repeat(np.array(combo, dtype=np.uint8)[:, None], z.shape[1], axis=1)
        best = np.maximum(best, joint_score(P, pi, tips, tree, st))
    return best
