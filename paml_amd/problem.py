"""Plain-array description of one likelihood problem (tree + tips + model inputs), the Python mirror
of what the C host hands to the engine ABI (include/paml_amd.h).  Field names follow the reference's
globals: com.z, com.fpatt, com.posG, com.rgene, com.pi, com.freqK, com.rK, nodes[].sons/branch/label,
com.nodeScale (codeml.c:109-147, treesub.c:7177).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

EIGEN_UVROOT, EIGEN_CIJK, EIGEN_K80, EIGEN_JC69LIKE, EIGEN_QMAT = 0, 1, 2, 3, 4
MODE_LFUN, MODE_LFUNDG = 0, 1


@dataclass
class Tree:
    n_tips: int
    n_nodes: int
    root: int
    sons: list            # list of lists, nodes[i].sons order
    branch: np.ndarray    # [n_nodes] branch length above each node
    label: np.ndarray     # [n_nodes] int branch label
    names: list | None = None

    def csr(self):
        ptr = np.zeros(self.n_nodes + 1, dtype=np.int32)
        flat = []
        for i, s in enumerate(self.sons):
            ptr[i + 1] = ptr[i] + len(s)
            flat += list(s)
        return ptr, np.asarray(flat, dtype=np.int32)

    def father(self):
        f = np.full(self.n_nodes, -1, dtype=np.int32)
        for i, s in enumerate(self.sons):
            for c in s:
                f[c] = i
        return f

    def nni_swaps(self):
        """The canonical list of nearest-neighbour-interchange swaps (v, s, x), int32 [n_swaps][3], as paml_amd_nni_list writes it: every
        internal v that is not the root in node order, s over its sons, x over its father's other sons; a v with two sons under a root
        with exactly three sons lists its first son only (the other's swaps are the same unrooted trees), so an unrooted binary tree
        of ns tips has 2 (ns - 3)."""
        f = self.father()
        out = []
        for v in range(self.n_nodes):
            if v == self.root or f[v] < 0 or not self.sons[v]:
                continue
            fa = int(f[v])
            half = fa == self.root and len(self.sons[fa]) == 3 and len(self.sons[v]) == 2
            for s in (self.sons[v][:1] if half else self.sons[v]):
                out += [(v, int(s), int(x)) for x in self.sons[fa] if x != v]
        return np.asarray(out, dtype=np.int32).reshape(-1, 3)

    def edge_configs(self):
        """The edges that have three configurations, as paml_amd_edge_list writes them: (edges int32 [n_edges][3][3], five int32
        [n_edges][5]).  Every internal v that is not the root, has exactly two sons (s1, s2) and whose father f is a non-root node with
        two sons (v, c) or a root with exactly three sons (v, c1, c2), in node order: the present configuration (v, -1, -1) and the two
        swaps nni_swaps gives for that v, and the five branches s1, s2, v, then c and f, or c1 and c2."""
        f = self.father()
        edges, five = [], []
        for v in range(self.n_nodes):
            if v == self.root or f[v] < 0 or len(self.sons[v]) != 2:
                continue
            fa = int(f[v])
            nf = len(self.sons[fa])
            if not ((fa != self.root and nf == 2) or (fa == self.root and nf == 3)):
                continue
            c = [int(u) for u in self.sons[fa] if u != v]
            s1, s2 = (int(u) for u in self.sons[v])
            if nf == 2:
                edges.append([(v, -1, -1), (v, s1, c[0]), (v, s2, c[0])])
                five.append([s1, s2, v, c[0], fa])
            else:
                edges.append([(v, -1, -1), (v, s1, c[0]), (v, s1, c[1])])
                five.append([s1, s2, v, c[0], c[1]])
        return np.asarray(edges, dtype=np.int32).reshape(-1, 3, 3), np.asarray(five, dtype=np.int32).reshape(-1, 5)

    def nni(self, v, s, x):
        """A new Tree with son s of v and son x of the father of v exchanged in place in the two son lists: the subtrees change places,
        each keeps the branch above it.  Node ids, branch and label are untouched (shared with this tree)."""
        fa = int(self.father()[v])
        if v == self.root or fa < 0 or s not in self.sons[v] or x == v or x not in self.sons[fa]:
            raise ValueError("nni(%d, %d, %d): not a swap of this tree" % (v, s, x))
        sons = [list(c) for c in self.sons]
        sons[v][sons[v].index(s)] = int(x)
        sons[fa][sons[fa].index(x)] = int(s)
        return Tree(self.n_tips, self.n_nodes, self.root, sons, self.branch, self.label, self.names)

    def relabelled(self, v, label):
        """A new Tree with the label of the branch above v set to `label` (what paml_amd_relabel_scores scores).  Everything else is
        shared with this tree; label is a new array."""
        if not 0 <= v < self.n_nodes or v == self.root or self.father()[v] < 0:
            raise ValueError("relabelled(%s): the root or no node of this tree" % (v,))
        lab = np.array(self.label, dtype=np.int32)
        lab[v] = int(label)
        return Tree(self.n_tips, self.n_nodes, self.root, self.sons, self.branch, lab, self.names)

    def _spr_parts(self, s, x=None):
        """(f, g, c, below) of pruning s: f the father of s, g the father of f, c the other son of f, below[u]: u lies in the subtree
        below s, s included.  ValueError naming what makes the prune, or the move (s, x) when x is given, invalid (the definition at the
        top of paml_amd/csrc/kernels_spr.h)."""
        fa, nn = self.father(), self.n_nodes
        who = "spr(%s, %s): " % (s, x)
        if not 0 <= s < nn or (x is not None and not 0 <= x < nn):
            raise ValueError(who + "a node is out of range")
        if s == self.root or fa[s] < 0:
            raise ValueError(who + "%d is the root" % s)
        f = int(fa[s])
        if f == self.root or fa[f] < 0:
            raise ValueError(who + "the father of %d is the root" % s)
        if len(self.sons[f]) != 2:
            raise ValueError(who + "the father of %d does not have exactly two sons" % s)
        c = int(self.sons[f][0] if self.sons[f][1] == s else self.sons[f][1])
        below = np.zeros(nn, dtype=bool)
        stack = [int(s)]
        while stack:
            u = stack.pop()
            below[u] = True
            stack += [int(v) for v in self.sons[u]]
        if x is not None:
            if x == self.root:
                raise ValueError(who + "%d is the root" % x)
            if x == f:
                raise ValueError(who + "%d is the father of %d" % (x, s))
            if x == c:
                raise ValueError(who + "%d is the sibling of %d: the same topology" % (x, s))
            if below[x]:
                raise ValueError(who + "%d lies in the subtree below %d" % (x, s))
        return f, int(fa[f]), c, below

    def spr(self, s, x, phi=0.5):
        """A new Tree with the subtree below s pruned and regrafted on the branch above x (what paml_amd_spr_scores scores).  f = the
        father of s travels with it: c, the other son of f, takes f's place in the son list of g = the father of f on a branch of length
        t_c + t_f with c's label; f takes x's place in the son list of x's father with sons (x, s), the branch above f has length
        (1 - phi) t_x and x's label, the branch above x phi t_x.  Node ids, n_nodes and the root stay; branch and label are new arrays."""
        s, x = int(s), int(x)
        f, g, c, _ = self._spr_parts(s, x)
        if not 0 <= phi <= 1:
            raise ValueError("spr: phi = %r is outside [0, 1]" % (phi,))
        sons = [[int(u) for u in l] for l in self.sons]
        branch, label = np.array(self.branch, dtype=np.float64), np.array(self.label, dtype=np.int32)
        sons[g][sons[g].index(f)] = c
        branch[c] = self.branch[c] + self.branch[f]
        fx = next(i for i, l in enumerate(sons) if x in l and i != f)      # (x's father in the tree without s and f)
        sons[fx][sons[fx].index(x)] = f
        sons[f] = [x, s]
        tx = branch[x]
        branch[f], branch[x] = (1 - phi) * tx, phi * tx
        label[f] = label[x]
        return Tree(self.n_tips, self.n_nodes, self.root, sons, branch, label, self.names)

    def spr_moves(self, radius=0):
        """The canonical list of subtree-prune-and-regraft moves (s, x), int32 [n_moves][2], as paml_amd_spr_list writes it: every valid
        move with s in node order and x in node order within s, whose target branch lies within `radius` branches of the merged branch
        above c in the tree without s and f (radius <= 0: no limit; adjacent branches have distance 1)."""
        fa, nn = self.father(), self.n_nodes
        out = []
        for s in range(nn):
            try:
                f, g, c, below = self._spr_parts(s)
            except ValueError:
                continue
            # the nodes' distances from the merged branch (its ends g and c: 0) in the tree without s and f
            nb = [[] for _ in range(nn)]
            for u in range(nn):
                if u != self.root and u != f and not below[u]:
                    pu = g if u == c else int(fa[u])
                    nb[u].append(pu)
                    nb[pu].append(u)
            dist = np.full(nn, nn + 1)
            dist[g] = dist[c] = 0
            queue = [g, c]
            while queue:
                u = queue.pop(0)
                for v in nb[u]:
                    if dist[v] > dist[u] + 1:
                        dist[v] = dist[u] + 1
                        queue.append(v)
            for x in range(nn):
                if x == self.root or x == f or x == c or below[x]:
                    continue
                if radius <= 0 or min(dist[int(fa[x])], dist[x]) + 1 <= radius:
                    out.append((s, x))
        return np.asarray(out, dtype=np.int32).reshape(-1, 2)

    def insert_tip(self, v, phi, pendant, label=0):
        """A new Tree with one more tip hung on the branch above v (what paml_amd_placement_scores scores; the reference's AddSpecies,
        treesub.c:4592).  The new tip is node n_tips, the old internal nodes move up by one, the new internal node u is the last node.
        u takes v's place in the son list of v's father and its sons are (v, the new tip); the branch above u has length
        (1 - phi) t_v, the branch above v phi t_v, both with v's label; the new tip's branch has length `pendant` and label `label`."""
        fa = int(self.father()[v]) if 0 <= v < self.n_nodes else -1
        if v == self.root or fa < 0:
            raise ValueError("insert_tip(%d): the root has no branch above it" % v)
        if not 0 <= phi <= 1:
            raise ValueError("insert_tip: phi = %r is outside [0, 1]" % (phi,))
        nt, nn = self.n_tips, self.n_nodes
        new = lambda i: i if i < nt else i + 1
        u = nn + 1
        sons = [[] for _ in range(nn + 2)]
        branch, lab = np.zeros(nn + 2), np.zeros(nn + 2, dtype=np.int32)
        for i in range(nn):
            sons[new(i)] = [new(int(c)) for c in self.sons[i]]
            branch[new(i)], lab[new(i)] = self.branch[i], self.label[i]
        sons[new(fa)][sons[new(fa)].index(new(v))] = u
        sons[u] = [new(v), nt]
        branch[u], lab[u] = (1 - phi) * self.branch[v], self.label[v]
        branch[new(v)] = phi * self.branch[v]
        branch[nt], lab[nt] = pendant, label
        names = None if self.names is None else list(self.names[:nt]) + ["query"] + list(self.names[nt + 1:])
        return Tree(nt + 1, nn + 2, new(self.root), sons, branch, lab, names)

    def newick(self, names=None, lengths=True):
        names = names or self.names or [str(i + 1) for i in range(self.n_tips)]

        def rec(i):
            s = names[i] if i < self.n_tips and not self.sons[i] else "(" + ", ".join(rec(c) for c in self.sons[i]) + ")"
            if i != self.root and lengths:
                s += ": %.6f" % self.branch[i]
            return s
        return rec(self.root) + ";"


def parse_newick(text: str, names: list | None = None) -> Tree:
    """Newick -> Tree with the reference's numbering (ReadTreeN treesub.c:3048-3216): tips keep their
    sequence order (names looked up in `names`, or 1-based integers), internal nodes are numbered from
    n_tips upward in order of '(' appearance; '#k' after a node sets its label."""
    s = text.strip()
    s = s[: s.index(";")] if ";" in s else s
    # first pass: count tips
    toks = []
    i = 0
    while i < len(s):
        c = s[i]
        if c in "(),":
            toks.append(c)
            i += 1
        elif c.isspace():
            i += 1
        else:
            j = i
            while j < len(s) and s[j] not in "(),":
                j += 1
            toks.append(s[i:j].strip())
            i = j
    tipnames = []
    prev = None
    for t in toks:
        if t not in "(),":
            if prev in ("(", ",", None):
                tipnames.append(t)
        prev = t
    n_tips = len(tipnames)
    n_nodes_max = 2 * n_tips
    sons = [[] for _ in range(n_nodes_max)]
    branch = np.zeros(n_nodes_max)
    label = np.zeros(n_nodes_max, dtype=np.int32)
    next_internal = [n_tips]
    stack = []
    root = None
    last = None    # node whose attributes may follow

    def attrs(node, txt):
        # "name: 0.1 #1" pieces
        if ":" in txt:
            txt, rest = txt.split(":", 1)
            rest = rest.strip()
            num = rest.split("#")[0].split("$")[0].strip()
            if num:
                branch[node] = float(num)
            if "#" in rest:
                label[node] = int(float(rest.split("#")[1].split()[0]))
        if "#" in txt:
            label[node] = int(float(txt.split("#")[1].split()[0]))
        return txt.split("#")[0].strip()

    def tip_index(nm):
        if names is not None and nm in names:
            return names.index(nm)
        return int(nm.lstrip("tT")) - 1      # synthetic data use names t1..tN

    prev = None
    for t in toks:
        if t == "(":
            node = next_internal[0]
            next_internal[0] += 1
            if stack:
                sons[stack[-1]].append(node)
            else:
                root = node
            stack.append(node)
        elif t == ")":
            last = stack.pop()
        elif t == ",":
            pass
        else:
            if prev == ")":
                attrs(last, t)
            else:
                nm = t.split(":")[0].split("#")[0].strip()
                node = tip_index(nm)
                attrs(node, t)
                sons[stack[-1]].append(node)
        prev = t
    n_nodes = next_internal[0]
    return Tree(n_tips, n_nodes, root, sons[:n_nodes], branch[:n_nodes].copy(), label[:n_nodes].copy(),
                names=list(names) if names is not None else None)


def balanced_tree(n_tips: int, tip_len=0.1, int_len=0.05) -> Tree:
    """Unrooted 'balanced-ish' tree with a trifurcating root (SURVEY §8d recipe): the tips are split
    ~1/2, 1/4, 1/4 under the root and each part is a balanced binary tree."""
    a = n_tips // 2
    b = (n_tips - a) // 2
    parts = [a, b, n_tips - a - b]
    sons = [[] for _ in range(2 * n_tips)]
    nxt = [n_tips]
    tip = [0]

    def build(k):
        if k == 1:
            t = tip[0]
            tip[0] += 1
            return t
        node = nxt[0]
        nxt[0] += 1
        l = build((k + 1) // 2)
        r = build(k // 2)
        sons[node] = [l, r]
        return node

    root = nxt[0]
    nxt[0] += 1
    sons[root] = [build(p) for p in parts if p > 0]
    n_nodes = nxt[0]
    branch = np.full(n_nodes, int_len)
    branch[:n_tips] = tip_len
    branch[root] = 0
    return Tree(n_tips, n_nodes, root, sons[:n_nodes], branch, np.zeros(n_nodes, dtype=np.int32))


def set_node_scale(tree: Tree, every: int) -> np.ndarray:
    """com.nodeScale as SetNodeScale marks it (treesub.c:7177-7197): post-order tip count, mark a
    non-root node when the running count exceeds `every` (100 nuc / 15 codon / 50 aa)."""
    flags = np.zeros(tree.n_nodes, dtype=np.uint8)

    def rec(i):
        d = 0
        for c in tree.sons[i]:
            d += rec(c) if tree.sons[c] else 1
        if i != tree.root and d > every:
            flags[i] = 1
            d = 1
        return d
    rec(tree.root)
    return flags


@dataclass
class Problem:
    n: int
    tree: Tree
    z: np.ndarray                 # uint8 [n_tips, n_patt]
    weights: np.ndarray           # float64 [n_patt]
    pi: np.ndarray                # [n_pi, n]
    eigen: list                   # list of dicts: {"kind":..., "U","V","Root"} | {"kind":CIJK,"Cijk","Root","nR"} | {"kind":K80,"kappa"}
    mode: int = MODE_LFUN
    freqK: np.ndarray = field(default_factory=lambda: np.ones(1))
    rate: np.ndarray = field(default_factory=lambda: np.ones(1))
    eigen_of: np.ndarray | None = None   # int32 [n_genes, K, n_labels]
    qfactor: np.ndarray | None = None    # [K, n_labels]
    cleandata: int = 1
    n_chara: np.ndarray | None = None    # int32 [n_codes]
    chara_map: np.ndarray | None = None  # uint8 [n_codes, n]
    gene_off: np.ndarray | None = None   # int32 [n_genes+1]
    gene_rate: np.ndarray | None = None  # [n_genes]
    scale_node: np.ndarray | None = None # uint8 [n_nodes]
    rate_per_gene: bool = False          # Malpha: rate is [n_genes, K] (a gamma shape per gene)

    def __post_init__(self):
        self.z = np.ascontiguousarray(self.z, dtype=np.uint8)
        self.weights = np.ascontiguousarray(self.weights, dtype=np.float64)
        self.pi = np.ascontiguousarray(np.atleast_2d(self.pi), dtype=np.float64)
        self.freqK = np.ascontiguousarray(self.freqK, dtype=np.float64)
        self.rate = np.ascontiguousarray(self.rate, dtype=np.float64)
        K = self.K
        if self.gene_off is None:
            self.gene_off = np.array([0, self.n_patt], dtype=np.int32)
        self.gene_off = np.ascontiguousarray(self.gene_off, dtype=np.int32)
        G = self.n_genes
        if self.gene_rate is None:
            self.gene_rate = np.ones(G)
        self.gene_rate = np.ascontiguousarray(self.gene_rate, dtype=np.float64)
        n_labels = int(self.tree.label.max()) + 1
        if self.eigen_of is None:
            self.eigen_of = np.zeros((G, K, n_labels), dtype=np.int32)
        self.eigen_of = np.ascontiguousarray(self.eigen_of, dtype=np.int32).reshape(G, K, -1)
        if self.qfactor is None:
            self.qfactor = np.ones((K, self.eigen_of.shape[2]))
        self.qfactor = np.ascontiguousarray(self.qfactor, dtype=np.float64).reshape(K, -1)
        if self.n_chara is None:
            self.n_chara = np.ones(self.n, dtype=np.int32)
            self.chara_map = np.zeros((self.n, self.n), dtype=np.uint8)
            self.chara_map[:, 0] = np.arange(self.n)
        self.n_chara = np.ascontiguousarray(self.n_chara, dtype=np.int32)
        self.chara_map = np.ascontiguousarray(self.chara_map, dtype=np.uint8)
        if self.scale_node is not None:
            self.scale_node = np.ascontiguousarray(self.scale_node, dtype=np.uint8)

    @property
    def n_patt(self):
        return self.z.shape[1]

    @property
    def K(self):
        return len(self.freqK)

    @property
    def n_genes(self):
        return len(self.gene_off) - 1

    @property
    def n_labels(self):
        return self.eigen_of.shape[2]

    @property
    def n_codes(self):
        return len(self.n_chara)

    def slice_patterns(self, lo: int, hi: int) -> "Problem":
        """Contiguous pattern shard [lo, hi) (multi-GPU sharding).  Gene boundaries stay where they are in the global
        range: the shard holds the part of every gene inside it (possibly none of it)."""
        import copy
        p = copy.copy(self)
        p.z = np.ascontiguousarray(self.z[:, lo:hi])
        p.weights = np.ascontiguousarray(self.weights[lo:hi])
        p.gene_off = np.clip(np.asarray(self.gene_off, dtype=np.int64) - lo, 0, hi - lo).astype(np.int32)
        return p
