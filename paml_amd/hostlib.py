"""ctypes binding of libpamlh.so (include/pamlh.h): the C host that reads .ctl / sequence / tree files and turns a
parameter vector into engine inputs.  `load(ctl, program).problem(x)` returns the same plain-array Problem the tests
and the engine binding use, so the C host can be checked against the golden vectors on CPU (through the oracle, in the
tests) and on the GPU (through the engine)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from .problem import EIGEN_CIJK, EIGEN_JC69LIKE, EIGEN_K80, EIGEN_QMAT, EIGEN_UVROOT, Problem, Tree

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpamlh.so")
DRIVER_PATH = os.path.join(_HERE, "lib", "pamlh_lnl")


def build(force=False):
    from . import engine
    engine.build()
    srcs = [os.path.join(_HERE, "host", f) for f in ("pamlh_num.c", "pamlh_io.c", "pamlh_model.c", "pamlh_opt.c", "pamlh_pairwise.c", "pamlh_simulate.c", "pamlh_nni.c", "pamlh_place.c", "pamlh_spr.c", "pamlh_support.c", "pamlh_newton.c", "pamlh_hessian.c", "pamlh_counts.c", "pamlh_scan.c", "pamlh_lnl.c", "pamlh_internal.h", "Makefile")]
    srcs.append(os.path.join(os.path.dirname(_HERE), "include", "pamlh.h"))
    if force or not (os.path.exists(LIB_PATH) and os.path.exists(DRIVER_PATH)) or \
            any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs):
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "host"), "-B"], stdout=subprocess.DEVNULL)
    return LIB_PATH


_L = None


def lib():
    global _L
    if _L is None:
        C.CDLL(os.path.join(_HERE, "lib", "libpaml_amd.so"), mode=C.RTLD_GLOBAL)
        L = C.CDLL(build())
        for name, rt in [("pamlh_tips", C.c_void_p), ("pamlh_weights", C.c_void_p), ("pamlh_n_chara", C.c_void_p),
                         ("pamlh_chara_map", C.c_void_p), ("pamlh_sons_ptr", C.c_void_p), ("pamlh_sons", C.c_void_p),
                         ("pamlh_labels", C.c_void_p), ("pamlh_scale_nodes", C.c_void_p), ("pamlh_branch_order", C.c_void_p),
                         ("pamlh_branch", C.c_void_p), ("pamlh_pi", C.c_void_p), ("pamlh_freqK", C.c_void_p),
                         ("pamlh_rate", C.c_void_p), ("pamlh_eigen_of", C.c_void_p), ("pamlh_error", C.c_char_p)]:
            getattr(L, name).restype = rt
            getattr(L, name).argtypes = [C.c_void_p]
        L.pamlh_load.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
        L.pamlh_load_tree.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
        L.pamlh_n_trees.argtypes = [C.c_void_p]
        L.pamlh_load_with.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
        L.pamlh_ctl_option.argtypes = [C.c_void_p, C.c_char_p]
        L.pamlh_ctl_option.restype = C.c_char_p
        L.pamlh_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.pamlh_dnds.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.pamlh_free.argtypes = [C.c_void_p]
        L.pamlh_is_pairwise.argtypes = [C.c_void_p]
        L.pamlh_pairwise_n.argtypes = [C.c_void_p]
        L.pamlh_dims.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 10
        L.pamlh_default_x.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.pamlh_read_inx.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.pamlh_set_x.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.pamlh_model.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 4
        L.pamlh_eigen.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)] + [C.POINTER(C.c_void_p)] * 4
        L.pamlh_eval_gpu.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_void_p]
        L.pamlh_eval_batch_gpu.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.pamlh_bounds.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.pamlh_standard_errors.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.pamlh_optimize.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int)]
        _L = L
    return _L


def _arr(ptr, dtype, n):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(n,)).copy()


DEFAULT_OMEGA2_GRID = (1, 1.5, 2, 3, 5, 8, 12, 20, 50)


def mixture_max(w, lnf4, s0=0.5, r0=0.5):
    """pamlh_mixture_max, host only: the proportions of branch-site model A's four site classes at fixed class likelihoods.  w pattern
    counts, lnf4 [4][n_patt] the logs of f0, f1, f2a, f2b (-inf allowed); start (s0, r0) = (p0 + p1, p0 / (p0 + p1)) -> dict(p0, p1, lnL)."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    f = np.ascontiguousarray(lnf4, dtype=np.float64)
    if f.shape != (4, len(w)):
        raise ValueError("mixture_max: lnf4 must be [4][%d]" % len(w))
    L = lib()
    L.pamlh_mixture_max.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_double] + [C.POINTER(C.c_double)] * 3
    p0, p1, lnl = C.c_double(), C.c_double(), C.c_double()
    if L.pamlh_mixture_max(len(w), w.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), float(s0), float(r0), C.byref(p0), C.byref(p1), C.byref(lnl)) != 0:
        raise RuntimeError("pamlh_mixture_max: bad arguments, or a pattern of weight > 0 without a likelihood under any class")
    return dict(p0=p0.value, p1=p1.value, lnL=lnl.value)


def tree_comparison(lnf, w, gene_off=None, n_rep=0, seed=1, device=False):
    """pamlh_tree_comparison: lnf [n_trees][n_patt], w pattern counts -> dict of li, dli, se, pKH, pSH, pRELL (arrays) and best.
    device=True: pamlh_tree_comparison_gpu — the replicates are drawn on the GPU, n_rep = 0 means 10 000 at every alignment length."""
    L = lib()
    lnf = np.ascontiguousarray(lnf, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    nt, npatt = lnf.shape
    go = np.ascontiguousarray(gene_off, dtype=np.int32) if gene_off is not None else None
    out = [np.zeros(nt) for _ in range(6)]
    best = C.c_int()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    fn = L.pamlh_tree_comparison_gpu if device else L.pamlh_tree_comparison
    fn.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_void_p, C.c_int, C.c_ulonglong] + [C.POINTER(C.c_double)] * 6 + [C.POINTER(C.c_int)]
    rc = fn(nt, npatt, dp(w), dp(lnf), (len(go) - 1) if go is not None else 1, go.ctypes.data if go is not None else None, n_rep, seed,
            *[dp(a) for a in out], C.byref(best))
    if rc != 0 and device:
        from . import engine
        E = engine.lib()
        raise RuntimeError("pamlh_tree_comparison_gpu: %s (code %d)" % (E.paml_amd_last_error(None).decode(), rc))
    if rc != 0:
        raise RuntimeError("pamlh_tree_comparison: bad arguments")
    return dict(zip(("li", "dli", "se", "pKH", "pSH", "pRELL"), out), best=best.value)


def branch_supports_from_replicates(rep, l3):
    """delta = 2 (l0 - max(l1, l2)) and the SH-like support of every edge from the replicate sums of its three configurations
    (pamlh_branch_supports_from_replicates, host only): rep [n_rep][3 n_edges], l3 [n_edges][3] -> (delta, support)."""
    L = lib()
    rep = np.ascontiguousarray(rep, dtype=np.float64)
    l3 = np.ascontiguousarray(l3, dtype=np.float64).reshape(-1, 3)
    n = len(l3)
    if rep.ndim != 2 or rep.shape[1] != 3 * n:
        raise ValueError("branch_supports_from_replicates: rep must be [n_rep][3 n_edges]")
    delta, sup = np.zeros(n), np.zeros(n)
    L.pamlh_branch_supports_from_replicates.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if L.pamlh_branch_supports_from_replicates(n, rep.shape[0], rep.ctypes.data_as(C.c_void_p), l3.ctypes.data_as(C.c_void_p), delta.ctypes.data_as(C.c_void_p),
                                               sup.ctypes.data_as(C.c_void_p)) != 0:
        raise ValueError("branch_supports_from_replicates: bad arguments")
    return delta, sup


def tree_comparison_from_replicates(lnf, w, rep):
    """pamlh_tree_comparison_from_replicates: the table's columns from a given replicate matrix rep[n_rep][n_trees]."""
    L = lib()
    lnf = np.ascontiguousarray(lnf, dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    rep = np.ascontiguousarray(rep, dtype=np.float64)
    nt, npatt = lnf.shape
    assert rep.ndim == 2 and rep.shape[1] == nt
    out = [np.zeros(nt) for _ in range(6)]
    best = C.c_int()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    L.pamlh_tree_comparison_from_replicates.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)] + [C.POINTER(C.c_double)] * 6 + [C.POINTER(C.c_int)]
    if L.pamlh_tree_comparison_from_replicates(nt, npatt, dp(w), dp(lnf), rep.shape[0], dp(rep), *[dp(a) for a in out], C.byref(best)) != 0:
        raise RuntimeError("pamlh_tree_comparison_from_replicates: bad arguments")
    return dict(zip(("li", "dli", "se", "pKH", "pSH", "pRELL"), out), best=best.value)


class Analysis:
    def __init__(self, ctl_path, program="codeml", tree_index=0, overrides=None, placement=False):
        """placement=True: pamlh_load_placement — the tree may name only some of the sequences, the others are the queries."""
        L = lib()
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        L.pamlh_load_placement.argtypes = L.pamlh_load_with.argtypes
        if (L.pamlh_load_placement if placement else L.pamlh_load_with)(C.byref(h), os.fsencode(ctl_path), program.encode(), tree_index, overrides.encode() if overrides else None, err, 512) != 0:
            raise RuntimeError("pamlh_load: " + err.value.decode())
        self._h, self._L = h, L
        d = [C.c_int() for _ in range(10)]
        L.pamlh_dims(h, *[C.byref(v) for v in d])
        (self.n, self.n_tips, self.n_patt, self.n_nodes, self.root, self.n_codes, self.cleandata, self.ls, self.np,
         self.ntime) = [v.value for v in d]
        L.pamlh_n_queries.argtypes = [C.c_void_p]
        self.n_queries = int(L.pamlh_n_queries(h))

    def is_pairwise(self):
        return bool(self._L.pamlh_is_pairwise(self._h))

    def n_pairs(self):
        return int(self._L.pamlh_pairwise_n(self._h))

    def seq_names(self):
        self._L.pamlh_seq_name.restype = C.c_char_p
        self._L.pamlh_seq_name.argtypes = [C.c_void_p, C.c_int]
        return [self._L.pamlh_seq_name(self._h, i).decode() for i in range(self.n_tips)]

    def pairwise(self):
        """runmode = -2 on the GPU (pamlh_pairwise): dict of arrays over the pairs in the reference's order (2,1), (3,1), (3,2), ... —
        pairs[k] = (i, j) 0-based with j < i, t, kappa, omega, lnL, S, N, dN, dS, n_eval — plus the counters of the run."""
        npair = self.n_pairs()
        out, cnt = np.zeros((npair, 9)), (C.c_long * 4)()
        self._L.pamlh_pairwise.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        if self._L.pamlh_pairwise(self._h, out.ctypes.data_as(C.c_void_p), cnt, 0) != 0:
            raise RuntimeError("pamlh_pairwise: " + self._L.pamlh_error(self._h).decode())
        res = {k: out[:, i].copy() for i, k in enumerate(("t", "kappa", "omega", "lnL", "S", "N", "dN", "dS", "n_eval"))}
        res["pairs"] = np.array([(i, j) for i in range(1, self.n_tips) for j in range(i)], dtype=np.int32)
        res["counters"] = dict(n_elem=cnt[0], n_decomp=cnt[1], n_calls=cnt[2], n_host_redone=cnt[3])
        res["table"] = out
        return res

    def pairwise_freqs(self, fp, ls):
        """Codon frequencies of a pair from its count table fp[n][n] (row = the larger state) by GetCodonFreqs2 (host only)."""
        fp = np.ascontiguousarray(fp, dtype=np.float64)
        pi = np.zeros(self.n)
        self._L.pamlh_pairwise_freqs.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
        if self._L.pamlh_pairwise_freqs(self._h, fp.ctypes.data_as(C.c_void_p), float(ls), pi.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_pairwise_freqs failed")
        return pi

    def pairwise_write(self, table, directory):
        """2ML.t, 2ML.dN, 2ML.dS and rst in the reference's layout from table[n_pairs][9] (host only)."""
        tb = np.ascontiguousarray(table, dtype=np.float64)
        assert tb.shape == (self.n_pairs(), 9)
        self._L.pamlh_pairwise_write.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p]
        if self._L.pamlh_pairwise_write(self._h, tb.ctypes.data_as(C.c_void_p), os.fsencode(directory)) != 0:
            raise RuntimeError("pamlh_pairwise_write: " + self._L.pamlh_error(self._h).decode())

    def dnds(self, x):
        """[n_branches][6] = t, N, S, omega, dN, dS (the reference's "dN & dS for each branch" table)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros((self.n_nodes - 1, 6))
        if self._L.pamlh_dnds(self._h, x.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double))) != 0:
            raise RuntimeError("pamlh_dnds: " + self._L.pamlh_error(self._h).decode())
        return out

    def set_shard(self, rank, world, comm_id=None):
        """Keep this rank's block of site patterns (pamlh_set_shard; before the first evaluation).  comm_id: the 128-byte RCCL id, or
        None for the sharding alone (CPU tests; one-GPU emulation of the ranks)."""
        buf = (C.c_ubyte * 128).from_buffer_copy(comm_id) if comm_id is not None else None
        if self._L.pamlh_set_shard(self._h, rank, world, buf) != 0:
            raise RuntimeError("pamlh_set_shard: " + self._L.pamlh_error(self._h).decode())
        d = [C.c_int() for _ in range(10)]
        self._L.pamlh_dims(self._h, *[C.byref(v) for v in d])
        self.n_patt = d[2].value

    def ctl_option(self, key):
        v = self._L.pamlh_ctl_option(self._h, key.encode())
        return v.decode() if v is not None else None

    def n_trees(self):
        return self._L.pamlh_n_trees(self._h)

    def gene_subset(self, g):
        """Mgene = 1: gene g as an analysis of its own (pamlh_gene_subset)."""
        h = C.c_void_p()
        self._L.pamlh_gene_subset.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        if self._L.pamlh_gene_subset(self._h, int(g), C.byref(h)) != 0:
            raise RuntimeError("pamlh_gene_subset failed")
        a = Analysis.__new__(Analysis)
        a._h, a._L = h, self._L
        d = [C.c_int() for _ in range(10)]
        self._L.pamlh_dims(h, *[C.byref(v) for v in d])
        (a.n, a.n_tips, a.n_patt, a.n_nodes, a.root, a.n_codes, a.cleandata, a.ls, a.np, a.ntime) = [v.value for v in d]
        return a

    def n_genes(self):
        self._L.pamlh_genes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        return self._L.pamlh_genes(self._h, None, None, None, None)

    def close(self):
        if getattr(self, "_h", None):
            self._L.pamlh_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def simulate(self, x=None, n_sites=None, seed=1, replicate=0):
        """Draw an alignment under the model at x (None: the model state as it stands) on the GPU (pamlh_simulate): dict(z=[n_tips]
        [n_sites] uint8 states, cls=[n_sites] site classes).  n_sites None: the alignment's own length."""
        if n_sites is None:
            n_sites = len(self.pose())
        n_sites = int(n_sites)
        xa = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
        if xa is not None and len(xa) != self.np:
            raise ValueError("simulate: %d values for %d parameters" % (len(xa), self.np))
        z = np.zeros((self.n_tips, max(n_sites, 0)), dtype=np.uint8)
        cls = np.zeros(max(n_sites, 0), dtype=np.uint8)
        self._L.pamlh_simulate.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_ulonglong, C.c_uint, C.c_void_p, C.c_void_p]
        if self._L.pamlh_simulate(self._h, None if xa is None else xa.ctypes.data_as(C.c_void_p), n_sites, int(seed) & (2**64 - 1), int(replicate),
                                  z.ctypes.data_as(C.c_void_p), cls.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_simulate: " + self._L.pamlh_error(self._h).decode())
        return dict(z=z, cls=cls)

    def write_alignment(self, z, path):
        """States z[n_tips][n_sites] as a sequential PHYLIP file (pamlh_write_alignment; host only)."""
        z = np.ascontiguousarray(z, dtype=np.uint8)
        assert z.ndim == 2 and z.shape[0] == self.n_tips
        self._L.pamlh_write_alignment.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_char_p]
        if self._L.pamlh_write_alignment(self._h, z.ctypes.data_as(C.c_void_p), z.shape[1], os.fsencode(path)) != 0:
            raise RuntimeError("pamlh_write_alignment: " + self._L.pamlh_error(self._h).decode())

    def default_x(self):
        x = np.zeros(max(1, self.np))
        k = self._L.pamlh_default_x(self._h, x.ctypes.data_as(C.c_void_p), len(x))
        return x[:k]

    def read_inx(self):
        x = np.zeros(4096)
        k = self._L.pamlh_read_inx(self._h, x.ctypes.data_as(C.c_void_p), len(x))
        return x[:k]

    def set_x(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if self._L.pamlh_set_x(self._h, x.ctypes.data_as(C.c_void_p), len(x)) != 0:
            raise RuntimeError("pamlh_set_x: " + self._L.pamlh_error(self._h).decode())

    def problem(self, x) -> Problem:
        """SetParameters(x) in the C host, then everything as plain arrays."""
        self.set_x(x)
        L, h = self._L, self._h
        n, nn = self.n, self.n_nodes
        m = [C.c_int() for _ in range(4)]
        L.pamlh_model(h, *[C.byref(v) for v in m])
        mode, K, n_eigen, n_labels = [v.value for v in m]
        ptr = _arr(L.pamlh_sons_ptr(h), np.int32, nn + 1)
        sons_flat = _arr(L.pamlh_sons(h), np.int32, int(ptr[-1]))
        sons = [list(sons_flat[ptr[i]:ptr[i + 1]]) for i in range(nn)]
        tree = Tree(self.n_tips, nn, self.root, sons, _arr(L.pamlh_branch(h), np.float64, nn), _arr(L.pamlh_labels(h), np.int32, nn))
        eig = []
        for i in range(n_eigen):
            kind, nR, kappa = C.c_int(), C.c_int(), C.c_double()
            ps = [C.c_void_p() for _ in range(4)]
            L.pamlh_eigen(h, i, C.byref(kind), C.byref(nR), C.byref(kappa), *[C.byref(v) for v in ps])
            e = dict(kind=kind.value)
            if kind.value == EIGEN_UVROOT:
                e.update(U=_arr(ps[0].value, np.float64, n * n).reshape(n, n), V=_arr(ps[1].value, np.float64, n * n).reshape(n, n),
                         Root=_arr(ps[2].value, np.float64, n))
            elif kind.value == EIGEN_CIJK:
                e.update(nR=nR.value, Cijk=_arr(ps[3].value, np.float64, n * n * nR.value), Root=_arr(ps[2].value, np.float64, nR.value))
            elif kind.value == EIGEN_K80:
                e.update(kappa=kappa.value)
            elif kind.value == EIGEN_QMAT:
                e.update(Q=_arr(ps[0].value, np.float64, n * n).reshape(n, n))
            eig.append(e)
        scale = _arr(L.pamlh_scale_nodes(h), np.uint8, nn)
        L.pamlh_qfactor.restype = C.c_void_p
        L.pamlh_qfactor.argtypes = [C.c_void_p]
        qf = L.pamlh_qfactor(h)
        # several genes (option G): pattern offsets, rates, one frequency vector / eigen system per gene where the model has them
        go, gr, geo, npi = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int()
        L.pamlh_genes.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_void_p)]
        G = L.pamlh_genes(h, C.byref(go), C.byref(gr), C.byref(npi), C.byref(geo))
        malpha = bool(L.pamlh_malpha(h)) and G > 1
        genes = {}
        if G > 1:
            genes = dict(gene_off=_arr(go.value, np.int32, G + 1), gene_rate=_arr(gr.value, np.float64, G))
        return Problem(qfactor=None if not qf else _arr(qf, np.float64, K * n_labels).reshape(K, n_labels), **genes,
                       n=n, tree=tree, z=_arr(L.pamlh_tips(h), np.uint8, self.n_tips * self.n_patt).reshape(self.n_tips, self.n_patt),
                       weights=_arr(L.pamlh_weights(h), np.float64, self.n_patt), pi=_arr(L.pamlh_pi(h), np.float64, n * npi.value).reshape(npi.value, n), eigen=eig,
                       mode=mode, freqK=_arr(L.pamlh_freqK(h), np.float64, K), rate=_arr(L.pamlh_rate(h), np.float64, K * (G if malpha else 1)), rate_per_gene=malpha,
                       eigen_of=(_arr(geo.value, np.int32, G * K).reshape(G, K, 1) if G > 1 else
                                 _arr(L.pamlh_eigen_of(h), np.int32, K * n_labels).reshape(1, K, n_labels)), cleandata=self.cleandata,
                       n_chara=_arr(L.pamlh_n_chara(h), np.int32, self.n_codes),
                       chara_map=_arr(L.pamlh_chara_map(h), np.uint8, self.n_codes * n).reshape(self.n_codes, n),
                       scale_node=scale if scale.any() else None)

    def eval_gpu(self, x, want_lnf=True):
        self.set_x(x)
        lnl = C.c_double()
        lnf = np.zeros(self.n_patt) if want_lnf else None
        if self._L.pamlh_eval_gpu(self._h, C.byref(lnl), None if lnf is None else lnf.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_eval_gpu: " + self._L.pamlh_error(self._h).decode())
        return lnl.value, lnf

    def eval_batch_gpu(self, xs):
        """lnL at every row of xs[n_batch][np] in one launch (pamlh_eval_batch_gpu)."""
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        assert xs.ndim == 2 and xs.shape[1] == self.np
        out = np.zeros(xs.shape[0])
        if self._L.pamlh_eval_batch_gpu(self._h, xs.shape[0], xs.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_eval_batch_gpu: " + self._L.pamlh_error(self._h).decode())
        return out

    def bounds(self):
        lo, hi = np.zeros(self.np), np.zeros(self.np)
        if self._L.pamlh_bounds(self._h, lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_bounds failed")
        return lo, hi

    def optimize(self, x0, max_iter=500, tol=1e-10, verbose=False, analytic_gradient=False):
        """Maximum-likelihood estimation from x0 (pamlh_optimize).  Returns dict(x, lnL, converged, n_eval).  analytic_gradient: True or 1:
        the branch lengths' derivatives from one engine call per gradient (pamlh_use_analytic_gradient; counted as one evaluation); 2:
        every parameter's from one engine call per gradient (pamlh_gradient_full)."""
        x = np.ascontiguousarray(x0, dtype=np.float64).copy()
        lnl, nev = C.c_double(), C.c_int()
        self._L.pamlh_use_analytic_gradient.argtypes = [C.c_void_p, C.c_int]
        self._L.pamlh_use_analytic_gradient(self._h, 2 if analytic_gradient == 2 else int(bool(analytic_gradient)))
        try:
            rc = self._L.pamlh_optimize(self._h, x.ctypes.data_as(C.c_void_p), C.byref(lnl), max_iter, tol, int(verbose), C.byref(nev))
        finally:
            self._L.pamlh_use_analytic_gradient(self._h, 0)
        if rc < 0:
            raise RuntimeError("pamlh_optimize: " + self._L.pamlh_error(self._h).decode())
        return dict(x=x, lnL=lnl.value, converged=rc == 0, n_eval=nev.value)

    def nni_scores(self, x):
        """The lnL of every nearest-neighbour-interchange neighbour of the tree as it stands at x, from one engine call
        (pamlh_nni_scores): dict(lnL0, swaps=[n_swaps][3] (v, s, x; 0-based nodes), lnL=[n_swaps])."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        n, l0 = C.c_int(), C.c_double()
        f = self._L.pamlh_nni_scores
        f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_double), C.c_void_p]
        if len(x) != self.np or f(self._h, None, C.byref(n), None, None, None) != 0:
            raise RuntimeError("pamlh_nni_scores: " + self._L.pamlh_error(self._h).decode())
        swaps, lnl = np.zeros((max(1, n.value), 3), dtype=np.int32), np.zeros(max(1, n.value))
        if f(self._h, x.ctypes.data_as(C.c_void_p), C.byref(n), swaps.ctypes.data_as(C.c_void_p), C.byref(l0), lnl.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_nni_scores: " + self._L.pamlh_error(self._h).decode())
        return dict(lnL0=l0.value, swaps=swaps[:n.value], lnL=lnl[:n.value])

    def edge_list(self):
        """The edges of the tree as it stands that have three configurations (pamlh_edge_list -> paml_amd_edge_list): (edges int32
        [n_edges][3][3] = per edge the present configuration (v, -1, -1) and its two swaps, five int32 [n_edges][5])."""
        n = C.c_int()
        f = self._L.pamlh_edge_list
        f.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
        if f(self._h, C.byref(n), None, None) != 0:
            raise RuntimeError("pamlh_edge_list: " + self._L.pamlh_error(self._h).decode())
        edges, five = np.zeros((max(1, n.value), 3, 3), dtype=np.int32), np.zeros((max(1, n.value), 5), dtype=np.int32)
        if f(self._h, C.byref(n), edges.ctypes.data_as(C.c_void_p), five.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_edge_list: " + self._L.pamlh_error(self._h).decode())
        return edges[:n.value], five[:n.value]

    def edge_optimize(self, x, edges=None, five=None):
        """Every configuration of every edge maximised over the five branches around it at the parameters of x, in lock step, one
        engine call per Newton step (pamlh_edge_optimize): dict(edges, five, t5=[n_edges][3][5] the maximising lengths in the order of
        five, lnL=[n_edges][3], sweeps, calls, rows_at_bound).  edges, five None: edge_list()."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if edges is None or five is None:
            edges, five = self.edge_list()
        edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 3, 3)
        five = np.ascontiguousarray(five, dtype=np.int32).reshape(-1, 5)
        n = len(edges)
        t5, l3, stats = np.zeros((n, 3, 5)), np.zeros((n, 3)), (C.c_int * 3)()
        f = self._L.pamlh_edge_optimize
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if len(x) != self.np or len(five) != n or f(self._h, x.ctypes.data_as(C.c_void_p), n, edges.ctypes.data_as(C.c_void_p), five.ctypes.data_as(C.c_void_p),
                                                   t5.ctypes.data_as(C.c_void_p), l3.ctypes.data_as(C.c_void_p), stats) != 0:
            raise RuntimeError("pamlh_edge_optimize: " + self._L.pamlh_error(self._h).decode())
        return dict(edges=edges, five=five, t5=t5, lnL=l3, sweeps=stats[0], calls=stats[1], rows_at_bound=stats[2])

    def edge_lnf(self, x, edges, five, t5):
        """lnL [n_edges][3] and lnf [n_edges][3][n_patt] of every configuration at the lengths t5 [n_edges][3][5] and the parameters of
        x, from one engine call (pamlh_edge_lnf)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 3, 3)
        five = np.ascontiguousarray(five, dtype=np.int32).reshape(-1, 5)
        t5 = np.ascontiguousarray(t5, dtype=np.float64).reshape(-1, 3, 5)
        n = len(edges)
        l3, lnf = np.zeros((n, 3)), np.zeros((n, 3, self.n_patt))
        f = self._L.pamlh_edge_lnf
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if len(x) != self.np or len(five) != n or len(t5) != n or f(self._h, x.ctypes.data_as(C.c_void_p), n, edges.ctypes.data_as(C.c_void_p), five.ctypes.data_as(C.c_void_p),
                                                                  t5.ctypes.data_as(C.c_void_p), l3.ctypes.data_as(C.c_void_p), lnf.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_edge_lnf: " + self._L.pamlh_error(self._h).decode())
        return l3, lnf

    def lnL(self, x):
        """lnL at x: one evaluation on the GPU (eval_gpu without the per-pattern values)."""
        return self.eval_gpu(x, want_lnf=False)[0]

    def branch_supports(self, x, n_rep=1000, seed=1):
        """SH-like aLRT supports of the internal branches of the tree as it stands at the parameters of x (pamlh_branch_supports):
        dict(edge_node=[n_edges] (the branch above that node), delta, support=[n_edges], lnL=[n_edges][3], newick (the supports as
        internal-node labels))."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        n = C.c_int()
        f = self._L.pamlh_branch_supports
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_ulonglong, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if len(x) != self.np or f(self._h, None, int(n_rep), int(seed), C.byref(n), None, None, None, None) != 0:
            raise RuntimeError("pamlh_branch_supports: " + self._L.pamlh_error(self._h).decode())
        m = max(1, n.value)
        node, delta, sup, l3 = np.zeros(m, dtype=np.int32), np.zeros(m), np.zeros(m), np.zeros((m, 3))
        if f(self._h, x.ctypes.data_as(C.c_void_p), int(n_rep), int(seed), C.byref(n), node.ctypes.data_as(C.c_void_p), delta.ctypes.data_as(C.c_void_p),
             sup.ctypes.data_as(C.c_void_p), l3.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_branch_supports: " + self._L.pamlh_error(self._h).decode())
        m = n.value
        buf = C.create_string_buffer(160 * self.n_nodes + 256)
        self._L.pamlh_newick_supports.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
        self._L.pamlh_newick_supports(self._h, m, node.ctypes.data_as(C.c_void_p), sup.ctypes.data_as(C.c_void_p), buf, len(buf))
        return dict(edge_node=node[:m], delta=delta[:m], support=sup[:m], lnL=l3[:m], newick=buf.value.decode())

    @staticmethod
    def branch_supports_from_replicates(rep, l3):
        """The table arithmetic of branch_supports, host only (pamlh_branch_supports_from_replicates): rep [n_rep][3 n_edges] replicate
        sums, l3 [n_edges][3] -> (delta [n_edges], support [n_edges])."""
        return branch_supports_from_replicates(rep, l3)

    def apply_nni(self, v, s, x):
        """Exchange son s of v with son x of the father of v on the analysis's tree (pamlh_apply_nni); apply_nni(v, x, s) undoes it."""
        self._L.pamlh_apply_nni.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        if self._L.pamlh_apply_nni(self._h, int(v), int(s), int(x)) != 0:
            raise RuntimeError("pamlh_apply_nni: " + self._L.pamlh_error(self._h).decode())

    def foreground_scan(self, x, omega2=None):
        """Every non-root branch as the only foreground branch of branch-site model A, at every omega2 of an ascending grid that starts
        at 1 (pamlh_foreground_scan; one engine call): dict(node=[n_br], omega2=[n_grid], lnL_base, lnL, p0, p1 = [n_br][n_grid],
        delta=[n_br] = 2 (max over omega2 > 1 - the value at omega2 = 1), best=[n_br] the grid index of that maximum)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        grid = np.ascontiguousarray(DEFAULT_OMEGA2_GRID if omega2 is None else omega2, dtype=np.float64)
        f = self._L.pamlh_foreground_scan
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_double)] + [C.c_void_p] * 5
        n, base = C.c_int(), C.c_double()
        if len(x) != self.np or f(self._h, None, 0, None, C.byref(n), None, None, None, None, None, None, None) != 0:
            raise RuntimeError("pamlh_foreground_scan: " + self._L.pamlh_error(self._h).decode())
        nb, ng = n.value, len(grid)
        node, best = np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32)
        lnl, p0, p1, delta = np.zeros((nb, ng)), np.zeros((nb, ng)), np.zeros((nb, ng)), np.zeros(nb)
        q = lambda a: a.ctypes.data_as(C.c_void_p)
        if f(self._h, q(x), ng, q(grid), C.byref(n), q(node), C.byref(base), q(lnl), q(p0), q(p1), q(delta), q(best)) != 0:
            raise RuntimeError("pamlh_foreground_scan: " + self._L.pamlh_error(self._h).decode())
        return dict(node=node, omega2=grid, lnL_base=base.value, lnL=lnl, p0=p0, p1=p1, delta=delta, best=best)

    def foreground_point(self, x, node, omega2, p0, p1):
        """The model-A parameter vector of a row of foreground_scan, in x's layout, for the tree with `node` as the only foreground
        branch (pamlh_foreground_point); not clamped into bounds()."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        xa = np.zeros(self.np)
        f = self._L.pamlh_foreground_point
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p]
        if len(x) != self.np or f(self._h, x.ctypes.data_as(C.c_void_p), int(node), float(omega2), float(p0), float(p1), xa.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_foreground_point: " + self._L.pamlh_error(self._h).decode())
        return xa

    def set_foreground(self, node):
        """Label 1 on the branch above `node` and 0 elsewhere, on the analysis's tree in place (pamlh_set_foreground)."""
        self._L.pamlh_set_foreground.argtypes = [C.c_void_p, C.c_int]
        if self._L.pamlh_set_foreground(self._h, int(node)) != 0:
            raise RuntimeError("pamlh_set_foreground: " + self._L.pamlh_error(self._h).decode())

    def newick(self):
        """The tree with the branch lengths of the last set_x and its '#' labels (pamlh_newick)."""
        buf = C.create_string_buffer(160 * self.n_nodes + 256)
        self._L.pamlh_newick.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        if self._L.pamlh_newick(self._h, buf, len(buf)) != 0:
            raise RuntimeError("pamlh_newick failed")
        return buf.value.decode()

    def nni_search(self, x0, max_moves=0, verbose=False):
        """NNI hill climb from the tree as it stands (pamlh_nni_search): dict(x, lnL, moves, screening_calls, optimisations, newick)."""
        x = np.ascontiguousarray(x0, dtype=np.float64).copy()
        lnl, stats = C.c_double(), (C.c_int * 3)()
        self._L.pamlh_nni_search.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_void_p]
        if len(x) != self.np or self._L.pamlh_nni_search(self._h, x.ctypes.data_as(C.c_void_p), C.byref(lnl), int(max_moves), int(bool(verbose)), stats) != 0:
            raise RuntimeError("pamlh_nni_search: " + self._L.pamlh_error(self._h).decode())
        buf = C.create_string_buffer(160 * self.n_nodes + 256)
        self._L.pamlh_newick.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        newick = buf.value.decode() if self._L.pamlh_newick(self._h, buf, len(buf)) == 0 else None
        return dict(x=x, lnL=lnl.value, moves=stats[0], screening_calls=stats[1], optimisations=stats[2], newick=newick)

    def spr_scores(self, x, radius=0, phi=0.5):
        """The lnL of every subtree-prune-and-regraft neighbour of the tree as it stands within `radius` branches (<= 0: no limit) at x,
        from one engine call (pamlh_spr_scores): dict(lnL0, moves=[n_moves][2] (s, x; 0-based nodes), lnL=[n_moves])."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        n, l0 = C.c_int(), C.c_double()
        f = self._L.pamlh_spr_scores
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_double), C.c_void_p]
        if len(x) != self.np or f(self._h, None, int(radius), float(phi), C.byref(n), None, None, None) != 0:
            raise RuntimeError("pamlh_spr_scores: " + self._L.pamlh_error(self._h).decode())
        moves, lnl = np.zeros((max(1, n.value), 2), dtype=np.int32), np.zeros(max(1, n.value))
        if f(self._h, x.ctypes.data_as(C.c_void_p), int(radius), float(phi), C.byref(n), moves.ctypes.data_as(C.c_void_p), C.byref(l0), lnl.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_spr_scores: " + self._L.pamlh_error(self._h).decode())
        return dict(lnL0=l0.value, moves=moves[:n.value], lnL=lnl[:n.value])

    def apply_spr(self, s, x, phi, xvec):
        """Prune the subtree below s and regraft it on the branch above x on the analysis's tree (pamlh_apply_spr); returns the parameter
        vector with the three branch lengths the move changes rewritten."""
        xv = np.ascontiguousarray(xvec, dtype=np.float64).copy()
        self._L.pamlh_apply_spr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]
        if len(xv) != self.np or self._L.pamlh_apply_spr(self._h, int(s), int(x), float(phi), xv.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_apply_spr: " + self._L.pamlh_error(self._h).decode())
        return xv

    def spr_search(self, x0, radius=0, top=0, max_moves=0, verbose=False):
        """SPR hill climb from the tree as it stands (pamlh_spr_search): dict(x, lnL, moves, screening_calls, optimisations, newick)."""
        x = np.ascontiguousarray(x0, dtype=np.float64).copy()
        lnl, stats = C.c_double(), (C.c_int * 3)()
        self._L.pamlh_spr_search.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        if len(x) != self.np or self._L.pamlh_spr_search(self._h, x.ctypes.data_as(C.c_void_p), C.byref(lnl), int(radius), int(top), int(max_moves), int(bool(verbose)), stats) != 0:
            raise RuntimeError("pamlh_spr_search: " + self._L.pamlh_error(self._h).decode())
        buf = C.create_string_buffer(160 * self.n_nodes + 256)
        self._L.pamlh_newick.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        newick = buf.value.decode() if self._L.pamlh_newick(self._h, buf, len(buf)) == 0 else None
        return dict(x=x, lnL=lnl.value, moves=stats[0], screening_calls=stats[1], optimisations=stats[2], newick=newick)

    def query_names(self):
        """The names of the sequences the tree leaves out (pamlh_load_placement), in file order."""
        self._L.pamlh_query_name.restype = C.c_char_p
        self._L.pamlh_query_name.argtypes = [C.c_void_p, C.c_int]
        return [self._L.pamlh_query_name(self._h, i).decode() for i in range(self.n_queries)]

    def query_codes(self):
        """The queries' character codes per site pattern, uint8 [n_queries][n_patt] (pamlh_query_codes)."""
        self._L.pamlh_query_codes.restype = C.c_void_p
        self._L.pamlh_query_codes.argtypes = [C.c_void_p]
        if not self.n_queries:
            return np.zeros((0, self.n_patt), dtype=np.uint8)
        return _arr(self._L.pamlh_query_codes(self._h), np.uint8, self.n_queries * self.n_patt).reshape(self.n_queries, self.n_patt)

    def placement_scores(self, x, pendant=(0.1,), phi=0.5):
        """The lnL of the tree at x with a query hung on a branch, for every query, every branch of x's branch-length block
        (branch_order()) and every pendant length, from one engine call (pamlh_placement_scores): dict(lnL0, edges=[n_branches] (the node
        below the branch), lnL=[n_queries][n_branches][n_pend])."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        pe = np.ascontiguousarray(np.atleast_1d(pendant), dtype=np.float64)
        l0, lnl = C.c_double(), np.zeros((max(1, self.n_queries), self.n_nodes - 1, len(pe)))
        f = self._L.pamlh_placement_scores
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.POINTER(C.c_double), C.c_void_p]
        if len(x) != self.np or f(self._h, x.ctypes.data_as(C.c_void_p), len(pe), pe.ctypes.data_as(C.c_void_p), float(phi), C.byref(l0), lnl.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_placement_scores: " + self._L.pamlh_error(self._h).decode())
        return dict(lnL0=l0.value, edges=self.branch_order(), lnL=lnl[:self.n_queries])

    def place(self, x, pendant=(0.1,), phi=0.5):
        """Per query the best (branch, pendant length) of the grid and the likelihood weight ratios of the branches (pamlh_place):
        dict(best_edge=[n_queries] (index into branch_order()), best_pendant, best_lnL, lwr=[n_queries][n_branches])."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        pe = np.ascontiguousarray(np.atleast_1d(pendant), dtype=np.float64)
        nq = max(1, self.n_queries)
        be, bp, bl, lwr = np.zeros(nq, dtype=np.int32), np.zeros(nq), np.zeros(nq), np.zeros((nq, self.n_nodes - 1))
        f = self._L.pamlh_place
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        if len(x) != self.np or f(self._h, x.ctypes.data_as(C.c_void_p), len(pe), pe.ctypes.data_as(C.c_void_p), float(phi), be.ctypes.data_as(C.c_void_p),
                                  bp.ctypes.data_as(C.c_void_p), bl.ctypes.data_as(C.c_void_p), lwr.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_place: " + self._L.pamlh_error(self._h).decode())
        nq = self.n_queries
        return dict(best_edge=be[:nq], best_pendant=bp[:nq], best_lnL=bl[:nq], lwr=lwr[:nq])

    def placement_newick(self, q, edge, phi=0.5, pendant=0.1):
        """The tree with query q hung on branch `edge` (index into branch_order()), with the lengths of the last x (pamlh_placement_newick)."""
        buf = C.create_string_buffer(160 * (self.n_nodes + 2) + 256)
        self._L.pamlh_placement_newick.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_char_p, C.c_int]
        if self._L.pamlh_placement_newick(self._h, int(q), int(edge), float(phi), float(pendant), buf, len(buf)) != 0:
            raise RuntimeError("pamlh_placement_newick: " + self._L.pamlh_error(self._h).decode())
        return buf.value.decode()

    def attach_scores(self, x, q, edge, role, t3):
        """lnL, d1 and d2 of query q[i] hung on branch edge[i] (index into branch_order()) at the lengths t3[i] = (t_up, t_dn, t_pend),
        the derivatives along the branch role[i] names (-1: none, 0: up, 1: dn, 2: pendant), from one engine call (pamlh_attach_scores):
        dict(lnL0, lnL, d1, d2)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        qi, ed, ro = (np.ascontiguousarray(np.atleast_1d(a), dtype=np.int32) for a in (q, edge, role))
        tt = np.ascontiguousarray(t3, dtype=np.float64).reshape(-1, 3)
        n = len(qi)
        l0, lnl, d1, d2 = C.c_double(), np.zeros(max(1, n)), np.zeros(max(1, n)), np.zeros(max(1, n))
        f = self._L.pamlh_attach_scores
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.POINTER(C.c_double)] + [C.c_void_p] * 3
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        if len(x) != self.np or not (len(ed) == len(ro) == len(tt) == n) or f(self._h, p(x), n, p(qi), p(ed), p(ro), p(tt), C.byref(l0), p(lnl), p(d1), p(d2)) != 0:
            raise RuntimeError("pamlh_attach_scores: " + self._L.pamlh_error(self._h).decode())
        return dict(lnL0=l0.value, lnL=lnl[:n], d1=d1[:n], d2=d2[:n])

    def place_optimize(self, x, q, edge, t3):
        """Every row (q[i], edge[i]) maximised over its three attachment lengths from the start t3[i], all rows in lock step with one
        engine call per Newton step (pamlh_place_optimize): dict(t3=[n_rows][3] the maximising lengths, lnL=[n_rows], sweeps, calls,
        at_bound)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        qi, ed = (np.ascontiguousarray(np.atleast_1d(a), dtype=np.int32) for a in (q, edge))
        tt = np.ascontiguousarray(t3, dtype=np.float64).reshape(-1, 3).copy()
        n = len(qi)
        lnl, stats = np.zeros(max(1, n)), (C.c_int * 3)()
        f = self._L.pamlh_place_optimize
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        if len(x) != self.np or not (len(ed) == len(tt) == n) or f(self._h, p(x), n, p(qi), p(ed), p(tt), p(lnl), stats) != 0:
            raise RuntimeError("pamlh_place_optimize: " + self._L.pamlh_error(self._h).decode())
        return dict(t3=tt, lnL=lnl[:n], sweeps=stats[0], calls=stats[1], at_bound=stats[2])

    def place_ml(self, x, keep=0, pendant=(0.05, 0.1, 0.2, 0.4), phi=0.5):
        """Maximum-likelihood placement (pamlh_place_ml): the grid call, then per query its `keep` best branches (keep <= 0: all) maximised
        over the three lengths at the new node: dict(q, edge (index into branch_order()), t3=[n_rows][3], lnL, lwr = [n_rows] — the
        likelihood weight ratios over each query's kept rows)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        pe = np.ascontiguousarray(np.atleast_1d(pendant), dtype=np.float64)
        cap = max(1, self.n_queries) * (self.n_nodes - 1)
        rq, re, tt, lnl, lwr, n = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros((cap, 3)), np.zeros(cap), np.zeros(cap), C.c_int()
        f = self._L.pamlh_place_ml
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double] + [C.c_void_p] * 5 + [C.POINTER(C.c_int)]
        p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        if len(x) != self.np or f(self._h, p(x), int(keep), len(pe), p(pe), float(phi), p(rq), p(re), p(tt), p(lnl), p(lwr), C.byref(n)) != 0:
            raise RuntimeError("pamlh_place_ml: " + self._L.pamlh_error(self._h).decode())
        k = n.value
        return dict(q=rq[:k], edge=re[:k], t3=tt[:k], lnL=lnl[:k], lwr=lwr[:k])

    def placement_newick3(self, q, edge, t_up, t_dn, t_pend):
        """The tree with query q hung on branch `edge` (index into branch_order()) with the three attachment lengths written in, the
        other lengths those of the last x (pamlh_placement_newick3)."""
        buf = C.create_string_buffer(160 * (self.n_nodes + 2) + 256)
        self._L.pamlh_placement_newick3.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_char_p, C.c_int]
        if self._L.pamlh_placement_newick3(self._h, int(q), int(edge), float(t_up), float(t_dn), float(t_pend), buf, len(buf)) != 0:
            raise RuntimeError("pamlh_placement_newick3: " + self._L.pamlh_error(self._h).decode())
        return buf.value.decode()

    def write_bv(self, x, path):
        """The gradient and Hessian of the branch lengths at x in the layout of the reference's rst2 block (pamlh_write_bv)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        self._L.pamlh_write_bv.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p]
        if len(x) != self.np or self._L.pamlh_write_bv(self._h, x.ctypes.data_as(C.c_void_p), os.fsencode(str(path))) != 0:
            raise RuntimeError("pamlh_write_bv: " + self._L.pamlh_error(self._h).decode())

    def branch_order(self):
        """The node below the i-th branch of x's branch-length block, [n_nodes - 1] (pamlh_branch_order: tree.branches order)."""
        return _arr(self._L.pamlh_branch_order(self._h), np.int32, self.n_nodes - 1)

    def gradient(self, x):
        """d lnL / d x at x (pamlh_gradient): dict(lnL, grad=[np]) — the plain branch lengths from one engine call (paml_amd_gradient),
        the other parameters by central differences in one batch."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        lnl, g = C.c_double(), np.zeros(max(1, self.np))
        self._L.pamlh_gradient.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_void_p]
        if len(x) != self.np or self._L.pamlh_gradient(self._h, x.ctypes.data_as(C.c_void_p), C.byref(lnl), g.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_gradient: " + self._L.pamlh_error(self._h).decode())
        return dict(lnL=lnl.value, grad=g[:self.np])

    def gradient_full(self, x):
        """d lnL / d x at x from ONE engine call and a chain rule on the host (pamlh_gradient_full): dict(lnL, grad=[np]), or None where
        the call does not serve (a clock, fix_blength = 3, rho != 0, UNREST)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        lnl, g = C.c_double(), np.zeros(max(1, self.np))
        self._L.pamlh_gradient_full.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_void_p]
        rc = -1 if len(x) != self.np else self._L.pamlh_gradient_full(self._h, x.ctypes.data_as(C.c_void_p), C.byref(lnl), g.ctypes.data_as(C.c_void_p))
        if rc < 0:
            raise RuntimeError("pamlh_gradient_full: " + self._L.pamlh_error(self._h).decode())
        return None if rc else dict(lnL=lnl.value, grad=g[:self.np])

    def rate_matrix(self, set_id):
        """A[n][n]: the matrix the engine exponentiates for eigen set set_id of the present model state (pamlh_rate_matrix)."""
        A = np.zeros((self.n, self.n))
        self._L.pamlh_rate_matrix.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        if self._L.pamlh_rate_matrix(self._h, int(set_id), A.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_rate_matrix: " + self._L.pamlh_error(self._h).decode())
        return A

    def branch_hessian(self, x):
        """dict(grad=[ntime], H=[ntime][ntime]) over the branch lengths at x, H_ij = -sum_h w_h s_i(h) s_j(h) from the analytic
        per-pattern scores (pamlh_branch_hessian)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        nt = self.ntime
        g, H = np.zeros(max(1, nt)), np.zeros((max(1, nt), max(1, nt)))
        self._L.pamlh_branch_hessian.argtypes = [C.c_void_p] * 4
        if len(x) != self.np or self._L.pamlh_branch_hessian(self._h, x.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_branch_hessian: " + self._L.pamlh_error(self._h).decode())
        return dict(grad=g[:nt], H=H[:nt, :nt])

    def optimize_minb(self, x0, e0=1e-6, verbose=0):
        """method = 1 (pamlh_optimize_minb): branch lengths one at a time by Newton steps on the branch-local derivatives, the
        other parameters by BFGS in between.  Returns dict(x, lnL, converged, n_eval, branch_calls, nodes_recomputed)."""
        from . import engine
        x = np.ascontiguousarray(x0, dtype=np.float64).copy()
        lnl, nev = C.c_double(), C.c_int()
        self._L.pamlh_optimize_minb.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_double, C.c_int, C.POINTER(C.c_int)]
        rc = self._L.pamlh_optimize_minb(self._h, x.ctypes.data_as(C.c_void_p), C.byref(lnl), float(e0), int(verbose), C.byref(nev))
        if rc < 0:
            raise RuntimeError("pamlh_optimize_minb: " + self._L.pamlh_error(self._h).decode())
        a, b = C.c_long(), C.c_long()
        self._L.pamlh_engine_handle.restype = C.c_void_p
        self._L.pamlh_engine_handle.argtypes = [C.c_void_p]
        L = engine.lib()
        L.paml_amd_branch_counters.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]
        L.paml_amd_branch_counters(C.c_void_p(self._L.pamlh_engine_handle(self._h)), C.byref(a), C.byref(b))
        return dict(x=x, lnL=lnl.value, converged=rc == 0, n_eval=nev.value, branch_calls=a.value, nodes_recomputed=b.value)

    def curvature(self, x):
        """lnL at x and, over x's branch-length block (branch_order), the gradient and the curvature d2 lnL / d t2 along every branch
        from one engine call (pamlh_curvature -> paml_amd_curvature): dict(lnL, grad=[ntime], curv=[ntime])."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        nt = self.ntime
        lnl, g, h = C.c_double(), np.zeros(max(1, nt)), np.zeros(max(1, nt))
        self._L.pamlh_curvature.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
        if len(x) != self.np or self._L.pamlh_curvature(self._h, x.ctypes.data_as(C.c_void_p), C.byref(lnl), g.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_curvature: " + self._L.pamlh_error(self._h).decode())
        return dict(lnL=lnl.value, grad=g[:nt], curv=h[:nt])

    def count_labels(self, kind=None):
        """The substitution labels that go with the analysis's data type (pamlh_count_labels): (names, M[n_lab][n][n]).  kind None or
        "standard": synonymous / nonsynonymous (codons, by the genetic code), transitions / transversions (nucleotides), changes (amino
        acids); "total": every jump; "dwell": the identity, whose count is the branch length."""
        nl = C.c_int()
        M = np.zeros((2, self.n, self.n))
        names = ((C.c_char * 32) * 2)()
        self._L.pamlh_count_labels.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
        if self._L.pamlh_count_labels(self._h, None if kind is None else kind.encode(), C.byref(nl), M.ctypes.data_as(C.c_void_p), names) != 0:
            raise RuntimeError("pamlh_count_labels: " + self._L.pamlh_error(self._h).decode())
        return [names[i].value.decode() for i in range(nl.value)], M[:nl.value].copy()

    def subst_counts(self, x, labels=None, per_site=False):
        """Posterior expected labelled substitution counts at x over x's branch-length block (branch_order) from one engine call
        (pamlh_subst_counts -> paml_amd_subst_counts): dict(names, counts=[n_lab][ntime] summed over the alignment's sites,
        site_counts=[n_lab][ntime][sites] with per_site, else None).  labels None: the standard set of count_labels()."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        names = None
        if labels is None:
            names, labels = self.count_labels()
        M = np.ascontiguousarray(labels, dtype=np.float64).reshape(-1, self.n, self.n)
        nt = self.ntime
        counts = np.zeros((len(M), max(1, nt)))
        sites = np.zeros((len(M), max(1, nt), len(self.pose()))) if per_site else None
        self._L.pamlh_subst_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        if len(x) != self.np or self._L.pamlh_subst_counts(self._h, x.ctypes.data_as(C.c_void_p), len(M), M.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                                           None if sites is None else sites.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_subst_counts: " + self._L.pamlh_error(self._h).decode())
        return dict(names=names, counts=counts[:, :nt], site_counts=None if sites is None else sites[:, :nt])

    def newton_branches(self, x, e=1e-8, max_sweeps=50, verbose=0):
        """Maximises lnL over x's branch-length block by Newton steps on every branch at once, one engine call per sweep, the rest of x
        held (pamlh_newton_branches).  Returns dict(x, lnL, sweeps, calls, rejected)."""
        x = np.ascontiguousarray(x, dtype=np.float64).copy()
        lnl, st = C.c_double(), (C.c_int * 3)()
        self._L.pamlh_newton_branches.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_void_p]
        if len(x) != self.np or self._L.pamlh_newton_branches(self._h, x.ctypes.data_as(C.c_void_p), float(e), int(max_sweeps), C.byref(lnl), int(verbose), st) != 0:
            raise RuntimeError("pamlh_newton_branches: " + self._L.pamlh_error(self._h).decode())
        return dict(x=x, lnL=lnl.value, sweeps=st[0], calls=st[1], rejected=st[2])

    def minbranches(self, x, e=1e-8, verbose=0):
        """One run of the branch-at-a-time Newton cycles over x's branch-length block, the rest of x held (pamlh_minbranches, method = 1's
        inner step).  Returns dict(x, lnL, branch_calls = the paml_amd_eval_branch calls it made)."""
        from . import engine
        x = np.ascontiguousarray(x, dtype=np.float64).copy()
        lnl, a0, a1, b = C.c_double(), C.c_long(), C.c_long(), C.c_long()
        self._L.pamlh_engine_handle.restype = C.c_void_p
        self._L.pamlh_engine_handle.argtypes = [C.c_void_p]
        L = engine.lib()
        L.paml_amd_branch_counters.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]
        self.eval_gpu(x, want_lnf=False)      # (the engine exists from here on)
        L.paml_amd_branch_counters(C.c_void_p(self._L.pamlh_engine_handle(self._h)), C.byref(a0), C.byref(b))
        self._L.pamlh_minbranches.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_double), C.c_int]
        if len(x) != self.np or self._L.pamlh_minbranches(self._h, x.ctypes.data_as(C.c_void_p), float(e), C.byref(lnl), int(verbose)) != 0:
            raise RuntimeError("pamlh_minbranches: " + self._L.pamlh_error(self._h).decode())
        L.paml_amd_branch_counters(C.c_void_p(self._L.pamlh_engine_handle(self._h)), C.byref(a1), C.byref(b))
        return dict(x=x, lnL=lnl.value, branch_calls=a1.value - a0.value)

    def optimize_newton(self, x0, e0=1e-6, verbose=0):
        """pamlh_optimize_newton: the alternation of optimize_minb with newton_branches in the place of the branch-at-a-time steps.
        Returns dict(x, lnL, converged, n_eval)."""
        x = np.ascontiguousarray(x0, dtype=np.float64).copy()
        lnl, nev = C.c_double(), C.c_int()
        self._L.pamlh_optimize_newton.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_double, C.c_int, C.POINTER(C.c_int)]
        rc = -1 if len(x) != self.np else self._L.pamlh_optimize_newton(self._h, x.ctypes.data_as(C.c_void_p), C.byref(lnl), float(e0), int(verbose), C.byref(nev))
        if rc < 0:
            raise RuntimeError("pamlh_optimize_newton: " + self._L.pamlh_error(self._h).decode())
        return dict(x=x, lnL=lnl.value, converged=rc == 0, n_eval=nev.value)

    def branch_hessian_exact(self, x):
        """lnL at x, the gradient and the Hessian d2 lnL / d t_i d t_j over x's branch-length block (branch_order) from one engine call
        (pamlh_branch_hessian_exact -> paml_amd_hessian): dict(lnL, grad=[ntime], H=[ntime][ntime])."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        nt = self.ntime
        lnl, g, H = C.c_double(), np.zeros(max(1, nt)), np.zeros((max(1, nt), max(1, nt)))
        self._L.pamlh_branch_hessian_exact.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
        if len(x) != self.np or self._L.pamlh_branch_hessian_exact(self._h, x.ctypes.data_as(C.c_void_p), C.byref(lnl), g.ctypes.data_as(C.c_void_p),
                                                                   H.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_branch_hessian_exact: " + self._L.pamlh_error(self._h).decode())
        return dict(lnL=lnl.value, grad=g[:nt], H=H.reshape(-1)[:nt * nt].reshape(nt, nt))

    def write_bv_exact(self, x, path):
        """write_bv's block with the exact Hessian of branch_hessian_exact (pamlh_write_bv_exact)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        self._L.pamlh_write_bv_exact.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p]
        if len(x) != self.np or self._L.pamlh_write_bv_exact(self._h, x.ctypes.data_as(C.c_void_p), os.fsencode(str(path))) != 0:
            raise RuntimeError("pamlh_write_bv_exact: " + self._L.pamlh_error(self._h).decode())

    def standard_errors_exact(self, x):
        """Standard errors from the observed information over all free parameters (pamlh_standard_errors_exact): branch x branch from one
        engine call, branch x model parameter from differences of the branch gradient, model x model from method 1's stencil.
        Returns dict(se=[np] (-1: left out at a bound), hess=[np][np] the information matrix)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        n = self.np
        se, H = np.zeros(max(1, n)), np.zeros((max(1, n), max(1, n)))
        self._L.pamlh_standard_errors_exact.argtypes = [C.c_void_p] * 4
        if len(x) != n or self._L.pamlh_standard_errors_exact(self._h, x.ctypes.data_as(C.c_void_p), se.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_standard_errors_exact: " + self._L.pamlh_error(self._h).decode())
        return dict(se=se[:n], hess=H.reshape(-1)[:n * n].reshape(n, n))

    def newton_full(self, x, e=1e-8, max_sweeps=50, verbose=0):
        """newton_branches with the step from the whole Hessian block, one engine call per sweep (pamlh_newton_full).  Returns dict(x, lnL,
        sweeps, calls, rejected)."""
        x = np.ascontiguousarray(x, dtype=np.float64).copy()
        lnl, st = C.c_double(), (C.c_int * 3)()
        self._L.pamlh_newton_full.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_void_p]
        if len(x) != self.np or self._L.pamlh_newton_full(self._h, x.ctypes.data_as(C.c_void_p), float(e), int(max_sweeps), C.byref(lnl), int(verbose), st) != 0:
            raise RuntimeError("pamlh_newton_full: " + self._L.pamlh_error(self._h).decode())
        return dict(x=x, lnL=lnl.value, sweeps=st[0], calls=st[1], rejected=st[2])

    def lnpd_locus(self, age, rgene=1.0, rate=None, model_changed=True):
        """mcmctree's lnpD_locus on the GPU (pamlh_lnpd_locus): lnL for node ages age[n_nodes] and a locus rate / branch rates."""
        a = np.ascontiguousarray(age, dtype=np.float64)
        assert a.shape == (self.n_nodes,)
        r = None if rate is None else np.ascontiguousarray(rate, dtype=np.float64)
        lnl = C.c_double()
        self._L.pamlh_lnpd_locus.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        if self._L.pamlh_lnpd_locus(self._h, a.ctypes.data_as(C.c_void_p), float(rgene), None if r is None else r.ctypes.data_as(C.c_void_p),
                                    int(model_changed), C.byref(lnl)) != 0:
            raise RuntimeError("pamlh_lnpd_locus: " + self._L.pamlh_error(self._h).decode())
        return lnl.value

    def standard_errors(self, x, method=0):
        """Standard errors at the estimate x (pamlh_standard_errors): method 0 = the reference's HessianSKT2004 outer
        product of scores, method 1 = second differences of lnL; -1 marks a parameter without an estimate."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        se, H = np.zeros(self.np), np.zeros((self.np, self.np))
        if self._L.pamlh_standard_errors(self._h, x.ctypes.data_as(C.c_void_p), int(method), se.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_standard_errors: " + self._L.pamlh_error(self._h).decode())
        return se, H

    def neb(self, x):
        """NEB site-class posteriors at x: (post[K][n_sites], mean_omega[n_sites]) in the order of the (cleaned) sites."""
        self.set_x(x)
        mode, K, ne, nl = (C.c_int(), C.c_int(), C.c_int(), C.c_int())
        self._L.pamlh_model(self._h, C.byref(mode), C.byref(K), C.byref(ne), C.byref(nl))
        post, mw = np.zeros((K.value, self.n_patt)), np.zeros(self.n_patt)
        self._L.pamlh_neb.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        if self._L.pamlh_neb(self._h, post.ctypes.data_as(C.c_void_p), mw.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_neb: " + self._L.pamlh_error(self._h).decode())
        ns = C.c_int()
        self._L.pamlh_pose.restype = C.c_void_p
        self._L.pamlh_pose.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        ptr = self._L.pamlh_pose(self._h, C.byref(ns))
        pose = _arr(ptr, np.int32, ns.value)
        return post[:, pose], mw[pose]

    def _is_branchsite(self):
        return self._L.pamlh_positive_classes(self._h) == 2

    def pose(self):
        """com.pose: pattern of every (cleaned) site, in site order."""
        ns = C.c_int()
        self._L.pamlh_pose.restype = C.c_void_p
        self._L.pamlh_pose.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        return _arr(self._L.pamlh_pose(self._h, C.byref(ns)), np.int32, ns.value)

    def adg_matrix(self, x):
        """Auto-discrete-gamma transition matrix MK[K][K] of the model at x (None when the model has no rho)."""
        self.set_x(x)
        m = [C.c_int() for _ in range(4)]
        self._L.pamlh_model(self._h, *[C.byref(v) for v in m])
        K = m[1].value
        self._L.pamlh_adg_matrix.restype = C.c_void_p
        self._L.pamlh_adg_matrix.argtypes = [C.c_void_p]
        ptr = self._L.pamlh_adg_matrix(self._h)
        return _arr(ptr, np.float64, K * K).reshape(K, K) if ptr else None

    def plfun(self, x):
        """-lnL at x with com.plfun's convention (pamlh_plfun)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        self._L.pamlh_plfun.restype = C.c_double
        self._L.pamlh_plfun.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        return self._L.pamlh_plfun(self._h, x.ctypes.data_as(C.c_void_p), len(x))

    def node_posterior(self, x, node):
        """Marginal reconstruction at internal node `node` (0-based) at x: post[n_patt][n] (pamlh_node_posterior)."""
        self.set_x(x)
        post = np.zeros((self.n_patt, self.n))
        self._L.pamlh_node_posterior.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        if self._L.pamlh_node_posterior(self._h, int(node), post.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_node_posterior: " + self._L.pamlh_error(self._h).decode())
        return post

    def joint_reconstruction(self, x):
        """Best joint assignment of states to the internal nodes per pattern and its probability (pamlh_joint_reconstruction)."""
        self.set_x(x)
        ni = self.n_nodes - self.n_tips
        st, pr = np.zeros((self.n_patt, ni), dtype=np.int32), np.zeros(self.n_patt)
        self._L.pamlh_joint_reconstruction.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        if self._L.pamlh_joint_reconstruction(self._h, st.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_joint_reconstruction: " + self._L.pamlh_error(self._h).decode())
        return st, pr

    def ancestral_marginal(self, x, want_post=True):
        """Marginal reconstruction at every internal node at x in one engine call (pamlh_ancestral_marginal): dict(best=[ni][n_patt]
        uint8, prob=[ni][n_patt], post=[ni][n_patt][n] or None)."""
        self.set_x(x)
        ni = self.n_nodes - self.n_tips
        best, prob = np.zeros((ni, self.n_patt), dtype=np.uint8), np.zeros((ni, self.n_patt))
        post = np.zeros((ni, self.n_patt, self.n)) if want_post else None
        self._L.pamlh_ancestral_marginal.argtypes = [C.c_void_p] * 4
        if self._L.pamlh_ancestral_marginal(self._h, best.ctypes.data_as(C.c_void_p), prob.ctypes.data_as(C.c_void_p),
                                            None if post is None else post.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_ancestral_marginal: " + self._L.pamlh_error(self._h).decode())
        return dict(best=best, prob=prob, post=post)

    def ancestral_joint(self, x):
        """Joint reconstruction at x on the device (pamlh_ancestral_joint): dict(states=[ni][n_patt] uint8, ln_best=[n_patt])."""
        self.set_x(x)
        ni = self.n_nodes - self.n_tips
        st, lb = np.zeros((ni, self.n_patt), dtype=np.uint8), np.zeros(self.n_patt)
        self._L.pamlh_ancestral_joint.argtypes = [C.c_void_p] * 3
        if self._L.pamlh_ancestral_joint(self._h, st.ctypes.data_as(C.c_void_p), lb.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_ancestral_joint: " + self._L.pamlh_error(self._h).decode())
        return dict(states=st, ln_best=lb)

    def beb_acd(self, x):
        """BEB under branch-site model A (4 site classes: 0, 1, 2a, 2b) or clade model C / D (3) at x: class posteriors per site,
        [nc][n_sites] (pamlh_beb_acd)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        self.set_x(x)
        post = np.zeros((4 if self._is_branchsite() else 3, self.n_patt))
        self._L.pamlh_beb_acd.argtypes = [C.c_void_p] * 3
        if self._L.pamlh_beb_acd(self._h, x.ctypes.data_as(C.c_void_p), post.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("pamlh_beb_acd: " + self._L.pamlh_error(self._h).decode())
        ns = C.c_int()
        self._L.pamlh_pose.restype = C.c_void_p
        self._L.pamlh_pose.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        pose = _arr(self._L.pamlh_pose(self._h, C.byref(ns)), np.int32, ns.value)
        return post[:, pose]

    def beb(self, x):
        """BEB under M2a / M8 at x: (Pr(w>1), mean omega, sd omega) per site (pamlh_beb)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        pr, mw, se = np.zeros(self.n_patt), np.zeros(self.n_patt), np.zeros(self.n_patt)
        self._L.pamlh_beb.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        if self._L.pamlh_beb(self._h, *[a.ctypes.data_as(C.c_void_p) for a in (x, pr, mw, se)]) != 0:
            raise RuntimeError("pamlh_beb: " + self._L.pamlh_error(self._h).decode())
        ns = C.c_int()
        self._L.pamlh_pose.restype = C.c_void_p
        self._L.pamlh_pose.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        pose = _arr(self._L.pamlh_pose(self._h, C.byref(ns)), np.int32, ns.value)
        return pr[pose], mw[pose], se[pose]
