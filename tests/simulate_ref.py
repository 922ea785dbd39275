"""numpy restatement of the simulation draw (paml_amd_simulate), from the description at the top of paml_amd/csrc/kernels_simulate.h and
nothing else.

    mix(z)             = the SplitMix64 finaliser, arithmetic modulo 2^64
    stream(seed, r, 0) = mix(seed + GAMMA * ((r << 32 | 0) + 1))
    u64(j, d)          = mix(stream + GAMMA * (j * (n_nodes + 2) + d + 1))          j = global site index
    u                  = (u64 >> 11) * 2^-53
    d = 0 the class, d = 1 the root state, d = 2 + node the state below the branch above `node`
    c_k = max(p_0, 0) + ... + max(p_k, 0), added one after the other in double; drawn = the first k with u < c_k, else the last k
    with p_k > 0
    pre-order walk from the root; a child's row is P[class][child][parent's state][.]
"""
import numpy as np

GAMMA = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)


def mix(z):
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64)).copy()
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
    return z ^ (z >> np.uint64(31))


def stream(seed, r, g=0):
    with np.errstate(over="ignore"):
        packed = np.atleast_1d(np.uint64((int(r) << 32) | int(g))) + np.uint64(1)
        return mix(np.atleast_1d(np.uint64(int(seed) & (2 ** 64 - 1))) + GAMMA * packed)[0]


def uniforms(seed, r, sites, n_nodes, d):
    """u of draw d for the global site indices `sites`."""
    with np.errstate(over="ignore"):
        ctr = np.asarray(sites, dtype=np.uint64) * np.uint64(n_nodes + 2) + np.uint64(d + 1)
        x = mix(np.atleast_1d(stream(seed, r, 0)) + GAMMA * ctr)
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def cumulative(p):
    """Rows of p -> (c, last): c[:, k] the sequential sum of max(p, 0) up to k, last = the last index with a positive entry (the
    last index of all where there is none)."""
    p = np.atleast_2d(np.asarray(p, dtype=np.float64))
    c = np.empty_like(p)
    run = np.zeros(p.shape[0])
    for k in range(p.shape[1]):
        run = run + np.where(p[:, k] > 0, p[:, k], 0.0)
        c[:, k] = run
    pos = p > 0
    last = np.where(pos.any(axis=1), p.shape[1] - 1 - np.argmax(pos[:, ::-1], axis=1), p.shape[1] - 1)
    return c, last


def draw(c_rows, last_rows, u):
    """One draw per row: the first k with u < c[k], else last."""
    lt = u[:, None] < c_rows
    return np.where(lt.any(axis=1), np.argmax(lt, axis=1), last_rows).astype(np.int64)


def preorder(sons, root):
    """(node, parent) pairs, a node after its parent, sons in their order."""
    out, stack, father = [], [root], {}
    while stack:
        v = stack.pop()
        if v != root:
            out.append((v, father[v]))
        for s in reversed(list(sons[v])):
            father[int(s)] = v
            stack.append(int(s))
    return out


def simulate(pi, freqK, P, sons, root, n_tips, n_sites, seed=1, replicate=0, first_site=0):
    """P[K][n_nodes][n][n] (the root's slot is not read).  Returns dict(z [n_tips][n_sites], cls [n_sites], anc [n_nodes - n_tips]
    [n_sites], states [n_nodes][n_sites]), uint8."""
    P = np.asarray(P, dtype=np.float64)
    K, n_nodes, n, _ = P.shape
    sites = np.arange(first_site, first_site + n_sites, dtype=np.uint64)
    cf, lf = cumulative(np.asarray(freqK, dtype=np.float64)[None, :])
    cls = draw(np.broadcast_to(cf, (n_sites, K)), np.broadcast_to(lf, (n_sites,)), uniforms(seed, replicate, sites, n_nodes, 0))
    cp, lp = cumulative(np.asarray(pi, dtype=np.float64).reshape(1, n))
    states = np.zeros((n_nodes, n_sites), dtype=np.int64)
    states[root] = draw(np.broadcast_to(cp, (n_sites, n)), np.broadcast_to(lp, (n_sites,)), uniforms(seed, replicate, sites, n_nodes, 1))
    for node, parent in preorder(sons, root):
        c, last = cumulative(P[:, node].reshape(K * n, n))
        row = cls * n + states[parent]
        states[node] = draw(c[row], last[row], uniforms(seed, replicate, sites, n_nodes, 2 + node))
    states = states.astype(np.uint8)
    return dict(z=states[:n_tips], cls=cls.astype(np.uint8), anc=states[n_tips:], states=states)


# ---- the closed-loop configuration the CPU and GPU tests share ----
def star_case():
    """3-taxon star, 4 states, GTR with pi = (0.1, 0.2, 0.3, 0.4), two classes (0.3, 0.7) with rates (0.2, 0.94 / 0.7) (mean 1), branch
    lengths 0.3 / 0.45 / 0.6, over the alignment that lists each of the 64 patterns once.  Returns (Problem, P[K][n_nodes][4][4])."""
    from paml_amd import models
    from paml_amd.problem import EIGEN_UVROOT, MODE_LFUNDG, Problem, Tree
    pi = np.array([0.1, 0.2, 0.3, 0.4])
    freqK, rate = np.array([0.3, 0.7]), np.array([0.2, (1 - 0.3 * 0.2) / 0.7])
    U, V, root = models.eigen_rev(models.gtr_q((1.3, 0.7, 0.9, 1.6, 0.5), pi), pi)
    branch = np.array([0.3, 0.45, 0.6, 0.0])
    tree = Tree(3, 4, 3, [[], [], [], [0, 1, 2]], branch, np.zeros(4, dtype=np.int32))
    pat = np.arange(64)
    z = np.stack([pat // 16, (pat // 4) % 4, pat % 4]).astype(np.uint8)
    pb = Problem(n=4, tree=tree, z=z, weights=np.ones(64), pi=pi[None, :], eigen=[dict(kind=EIGEN_UVROOT, U=U, V=V, Root=root)],
                 mode=MODE_LFUNDG, freqK=freqK, rate=rate, eigen_of=np.zeros((1, 2, 1), dtype=np.int32))
    P = np.zeros((2, 4, 4, 4))
    for k in range(2):
        for v in range(3):
            P[k, v] = models.expm_rev(U, V, root, branch[v] * rate[k])
    return pb, P


def chi2_bound(df=63, z=6.0):
    """Wilson-Hilferty value of chi-square with df degrees of freedom at z standard deviations."""
    return df * (1 - 2 / (9 * df) + z * np.sqrt(2 / (9 * df))) ** 3


def pattern_counts(z):
    """Counts of the 64 patterns of a 3-sequence, 4-state alignment, in star_case's order."""
    z = np.asarray(z, dtype=np.int64)
    return np.bincount(z[0] * 16 + z[1] * 4 + z[2], minlength=64)
