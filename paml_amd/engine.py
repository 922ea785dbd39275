"""ctypes binding of libpaml_amd.so (include/paml_amd.h) — thin, no torch types in the ABI.

`Engine` mirrors the call sequence a PAML driver performs around com.plfun: create once per data
set, upload tips/tree, then per evaluation set eigen systems / classes / branch lengths and evaluate.
There is no CPU fallback: constructing an Engine without the built HIP library or without a GPU
raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from .problem import EIGEN_CIJK, EIGEN_JC69LIKE, EIGEN_K80, EIGEN_QMAT, EIGEN_UVROOT, Problem

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PAML_AMD_LIB") or os.path.join(_HERE, "lib", "libpaml_amd.so")   # override: kernel experiments
CSRC = os.path.join(_HERE, "csrc")
KEEP_PARTIALS = 1
JIT = 2
SHARD = 4      # the engine holds one rank's shard of a larger alignment (include/paml_amd.h)

EXPORTS = [
    "paml_amd_set_gene_class_rates", "paml_amd_get_branch_partials", "paml_amd_create", "paml_amd_destroy", "paml_amd_last_error", "paml_amd_set_stream", "paml_amd_set_tips",
    "paml_amd_set_tree", "paml_amd_set_pi", "paml_amd_set_eigen_uvroot", "paml_amd_set_eigen_cijk",
    "paml_amd_set_eigen_qrev_batch", "paml_amd_set_eigen_qrev_batch_sparse", "paml_amd_set_eigen_warm_start", "paml_amd_get_eigen", "paml_amd_eigen_counters", "paml_amd_set_eigen_k80", "paml_amd_set_eigen_jc69like", "paml_amd_set_eigen_qmat", "paml_amd_set_classes", "paml_amd_eval",
    "paml_amd_eval_batch", "paml_amd_eval_adg", "paml_amd_beb_grid", "paml_amd_beb_grid_classes", "paml_amd_compress_patterns", "paml_amd_eval_device", "paml_amd_eval_dirty", "paml_amd_eval_branch", "paml_amd_node_posterior", "paml_amd_get_pmat", "paml_amd_get_partials", "paml_amd_get_scale",
    "paml_amd_device_count", "paml_amd_set_device", "paml_amd_shard_bounds", "paml_amd_max_ranks", "paml_amd_flush", "paml_amd_eigen_status", "paml_amd_comm_unique_id", "paml_amd_comm_init", "paml_amd_comm_destroy", "paml_amd_comm_info", "paml_amd_comm_library", "paml_amd_comm_stats", "paml_amd_get_partial_sums", "paml_amd_branch_counters", "paml_amd_branch_coef_hits", "paml_amd_branch_refill_kernels", "paml_amd_branch_kernel_ms",
    "paml_amd_jit_prebuild", "paml_amd_profile", "paml_amd_profile_read", "paml_amd_counters", "paml_amd_kernel_name", "paml_amd_debug_program", "paml_amd_debug_jit",
    "paml_amd_cherry_tables", "paml_amd_debug_jit_tables",
    "paml_amd_subtree_tables", "paml_amd_subtree_order", "paml_amd_debug_subtree_order", "paml_amd_debug_subtree_classes", "paml_amd_debug_jit_subtree", "paml_amd_debug_subtree_select",
    "paml_amd_gather_walk", "paml_amd_debug_gather_tiles",
    "paml_amd_debug_code_order", "paml_amd_debug_branch_plan", "paml_amd_debug_device_bytes",
    "paml_amd_pairset_create", "paml_amd_pairset_destroy", "paml_amd_pairset_get_counts", "paml_amd_pairset_set_pi", "paml_amd_pairset_set_pattern",
    "paml_amd_pairset_eval", "paml_amd_pairset_failed", "paml_amd_pairset_counters",
    "paml_amd_rell_replicates", "paml_amd_rell_info",
    "paml_amd_simulate", "paml_amd_simulate_info",
    "paml_amd_ancestral_marginal", "paml_amd_ancestral_joint", "paml_amd_ancestral_info",
    "paml_amd_gradient", "paml_amd_gradient_info",
    "paml_amd_curvature", "paml_amd_curvature_info",
    "paml_amd_hessian", "paml_amd_hessian_info",
    "paml_amd_model_gradient", "paml_amd_model_gradient_info", "paml_amd_model_gradient_segment", "paml_amd_model_gradient_sizes",
    "paml_amd_subst_counts", "paml_amd_subst_counts_info",
    "paml_amd_nni_scores", "paml_amd_nni_info", "paml_amd_nni_list",
    "paml_amd_edge_scores", "paml_amd_edge_info", "paml_amd_edge_list",
    "paml_amd_relabel_scores", "paml_amd_relabel_info",
    "paml_amd_placement_scores", "paml_amd_placement_info",
    "paml_amd_attach_scores", "paml_amd_attach_info",
    "paml_amd_spr_scores", "paml_amd_spr_info", "paml_amd_spr_list",
]


class EngineError(RuntimeError):
    pass


# per-unit compiler flags (none at present; -mllvm -disable-machine-licm on engine_branch lowers its kernels' register counts from
# 220 - 256 to 186 - 224 — the logarithm's constants are no longer hoisted out of the main loops — and changes no timing: measured
# A / B on one box, profiles/r04_branch.txt)
UNIT_FLAGS = {}
# kernel experiments: a variant library beside the default one — PAML_AMD_LIB=<dir>/libpaml_amd.so PAML_AMD_EXTRA_FLAGS="-DX=1" python -c
# "from paml_amd import engine; engine.build()" compiles every unit with the extra flags into <dir> (objects in <dir>/obj)
EXTRA_FLAGS = os.environ.get("PAML_AMD_EXTRA_FLAGS", "").split()
UNITS = ("engine_core", "engine_comm", "engine_eval", "engine_branch", "engine_beb", "engine_jitdbg", "engine_compress", "engine_pairwise", "engine_rell", "engine_simulate", "engine_ancestral", "engine_gradient", "engine_curvature", "engine_hessian", "engine_modelgrad", "engine_counts", "engine_nni", "engine_place", "engine_attach", "engine_spr", "engine_edge", "engine_relabel")


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP engine for gfx950 in-tree (hipcc cross-compiles without a GPU): one object per translation unit, in
    parallel, then the shared library."""
    import glob
    from concurrent.futures import ThreadPoolExecutor
    hdrs = glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(os.path.dirname(_HERE), "include", "paml_amd.h")]
    newest_hdr = max(os.path.getmtime(h) for h in hdrs)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(os.path.dirname(LIB_PATH), "obj")
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    for u in UNITS:
        src, obj = os.path.join(CSRC, u + ".hip"), os.path.join(objdir, u + ".o")
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(newest_hdr, os.path.getmtime(src)):
            jobs.append([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + UNIT_FLAGS.get(u, []) + EXTRA_FLAGS + ["-c", src, "-o", obj])
    objs = [os.path.join(objdir, u + ".o") for u in UNITS]
    if not jobs and os.path.exists(LIB_PATH) and all(os.path.getmtime(o) <= os.path.getmtime(LIB_PATH) for o in objs):
        return LIB_PATH

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), os.cpu_count() or 1))) as ex:
        list(ex.map(run, jobs))
    run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs + ["-lhiprtc", "-ldl"])
    return LIB_PATH


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError("libpaml_amd.so is not built (run python -c 'import __graft_entry__ as g; g.build()')")
        L = C.CDLL(LIB_PATH)
        L.paml_amd_last_error.restype = C.c_char_p
        L.paml_amd_kernel_name.restype = C.c_char_p
        L.paml_amd_destroy.restype = None
        L.paml_amd_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint]
        L.paml_amd_destroy.argtypes = [C.c_void_p]
        L.paml_amd_last_error.argtypes = [C.c_void_p]
        L.paml_amd_kernel_name.argtypes = [C.c_void_p]
        L.paml_amd_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.paml_amd_set_tips.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.paml_amd_set_tree.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.paml_amd_set_pi.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.paml_amd_set_eigen_uvroot.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.paml_amd_set_eigen_cijk.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.paml_amd_set_eigen_qrev_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.paml_amd_set_eigen_qrev_batch_sparse.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.paml_amd_get_eigen.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.paml_amd_eigen_counters.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.c_void_p, C.c_int]
        L.paml_amd_set_eigen_k80.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.paml_amd_set_eigen_jc69like.argtypes = [C.c_void_p, C.c_int]
        L.paml_amd_set_classes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.paml_amd_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
        L.paml_amd_eval_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.paml_amd_eval_dirty.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        L.paml_amd_eval_branch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.paml_amd_get_pmat.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.paml_amd_get_partials.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.paml_amd_get_scale.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.paml_amd_profile.argtypes = [C.c_void_p, C.c_int]
        L.paml_amd_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_long)]
        L.paml_amd_counters.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]
        L.paml_amd_shard_bounds.argtypes = [C.c_long, C.c_int, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_long)]
        L.paml_amd_max_ranks.argtypes = [C.c_long]
        L.paml_amd_flush.argtypes = [C.c_void_p]
        L.paml_amd_comm_unique_id.argtypes = [C.c_void_p]
        L.paml_amd_comm_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_long]
        L.paml_amd_comm_destroy.argtypes = [C.c_void_p]
        L.paml_amd_comm_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_int)]
        _LIB = L
    return _LIB


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Engine:
    def __init__(self, n_states, n_tips, n_patt, max_classes=1, n_genes=1, flags=0):
        self._L = lib()
        h = C.c_void_p()
        rc = self._L.paml_amd_create(C.byref(h), n_states, n_tips, n_patt, max_classes, n_genes, flags)
        if rc != 0:
            raise EngineError("paml_amd_create failed (%d): no MI355X/HIP device visible or bad sizes" % rc)
        self._h = h
        self.n, self.n_tips, self.n_patt, self.n_genes = n_states, n_tips, n_patt, n_genes
        self.K = 1
        self.n_nodes = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.paml_amd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise EngineError("%s (code %d)" % (self._L.paml_amd_last_error(self._h).decode(), rc))

    @property
    def kernel_name(self):
        return self._L.paml_amd_kernel_name(self._h).decode()

    # ---- pattern shards over several GPUs (paml_amd_comm_*) ----
    def comm_init(self, rank, world, unique_id, n_patt_global, first_pattern):
        """Collective: join the RCCL communicator of the ranks' engines.  `unique_id` = the 128 bytes rank 0 got from
        comm_unique_id() (None with world = 1: global chunking only, no communicator)."""
        buf = None if unique_id is None else C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        self._chk(self._L.paml_amd_comm_init(self._h, int(rank), int(world), buf, int(n_patt_global), int(first_pattern)))

    def comm_destroy(self):
        self._chk(self._L.paml_amd_comm_destroy(self._h))

    def comm_info(self):
        r, w, ch = C.c_int(), C.c_int(), C.c_int()
        ng, fp = C.c_long(), C.c_long()
        self._L.paml_amd_comm_info(self._h, C.byref(r), C.byref(w), C.byref(ng), C.byref(fp), C.byref(ch))
        return dict(rank=r.value, world=w.value, n_patt_global=ng.value, first_pattern=fp.value, chunk=ch.value)

    def comm_stats(self, enable=True, read=False):
        """Timed events around the exchange step (paml_amd_comm_stats).  read=True returns the figures of the last <= 64
        evaluations (flush and synchronise first): dict(n, exchange_us, exchange_us_max, lane_wait_us, lane_wait_us_max)."""
        self._L.paml_amd_comm_stats.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)] + [C.POINTER(C.c_double)] * 4
        if not read:
            self._chk(self._L.paml_amd_comm_stats(self._h, int(bool(enable)), None, None, None, None, None))
            return None
        n = C.c_int()
        v = [C.c_double() for _ in range(4)]
        self._chk(self._L.paml_amd_comm_stats(self._h, int(bool(enable)), C.byref(n), *[C.byref(x) for x in v]))
        return dict(n=n.value, exchange_us=v[0].value, exchange_us_max=v[1].value, lane_wait_us=v[2].value, lane_wait_us_max=v[3].value)

    def partial_sums(self):
        """Per-chunk partial sums of the last evaluation at their global positions (paml_amd_get_partial_sums)."""
        cap = 1 << 14
        out = np.zeros(cap)
        self._L.paml_amd_get_partial_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        n = self._L.paml_amd_get_partial_sums(self._h, _p(out), cap)
        if n < 0:
            self._chk(n)
        return out[:n].copy()

    def set_stream(self, stream_ptr):
        self._chk(self._L.paml_amd_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_tips(self, z, weights, cleandata=1, n_chara=None, chara_map=None, gene_off=None):
        z = np.ascontiguousarray(z, dtype=np.uint8)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        assert z.shape == (self.n_tips, self.n_patt) and w.shape == (self.n_patt,)
        nch = None if n_chara is None else np.ascontiguousarray(n_chara, dtype=np.int32)
        cm = None if chara_map is None else np.ascontiguousarray(chara_map, dtype=np.uint8)
        go = None if gene_off is None else np.ascontiguousarray(gene_off, dtype=np.int32)
        self._chk(self._L.paml_amd_set_tips(self._h, _p(z), int(cleandata), 0 if nch is None else len(nch), _p(nch), _p(cm),
                                            _p(w), _p(go)))

    def set_tree(self, tree, scale_node=None):
        ptr, flat = tree.csr()
        lab = np.ascontiguousarray(tree.label, dtype=np.int32)
        sc = None if scale_node is None else np.ascontiguousarray(scale_node, dtype=np.uint8)
        self.n_nodes = tree.n_nodes
        self._chk(self._L.paml_amd_set_tree(self._h, tree.n_nodes, tree.root, _p(ptr), _p(flat), _p(lab), _p(sc)))
        self._tree_csr = (tree.root, ptr, flat)      # (for nni_scores' canonical list)

    def set_pi(self, pi):
        pi = np.ascontiguousarray(np.atleast_2d(pi), dtype=np.float64)
        self._chk(self._L.paml_amd_set_pi(self._h, pi.shape[0], _p(pi)))

    def set_eigen(self, set_id, e):
        k = e["kind"]
        if k == EIGEN_UVROOT:
            U, V, R = (np.ascontiguousarray(e[x], dtype=np.float64) for x in ("U", "V", "Root"))
            self._chk(self._L.paml_amd_set_eigen_uvroot(self._h, set_id, _p(U), _p(V), _p(R)))
        elif k == EIGEN_CIJK:
            Cj, R = (np.ascontiguousarray(e[x], dtype=np.float64) for x in ("Cijk", "Root"))
            self._chk(self._L.paml_amd_set_eigen_cijk(self._h, set_id, int(e["nR"]), _p(Cj), _p(R)))
        elif k == EIGEN_K80:
            self._chk(self._L.paml_amd_set_eigen_k80(self._h, set_id, float(e["kappa"])))
        elif k == EIGEN_JC69LIKE:
            self._chk(self._L.paml_amd_set_eigen_jc69like(self._h, set_id))
        elif k == EIGEN_QMAT:
            Q = np.ascontiguousarray(e["Q"], dtype=np.float64)
            self._L.paml_amd_set_eigen_qmat.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            self._chk(self._L.paml_amd_set_eigen_qmat(self._h, set_id, _p(Q)))
        else:
            raise ValueError(k)

    def set_classes(self, mode, freqK, rate, eigen_of, qfactor=None):
        f = np.ascontiguousarray(freqK, dtype=np.float64)
        r = np.ascontiguousarray(rate, dtype=np.float64)
        eo = np.ascontiguousarray(eigen_of, dtype=np.int32)
        K = len(f)
        n_labels = eo.size // (self.n_genes * K)
        q = None if qfactor is None else np.ascontiguousarray(qfactor, dtype=np.float64)
        self.K = K
        self._chk(self._L.paml_amd_set_classes(self._h, int(mode), K, _p(f), _p(r), n_labels, _p(eo), _p(q)))
        self.n_labels = n_labels

    def load(self, pb: Problem):
        """Upload everything a Problem holds (tips, tree, pi, eigen systems, classes)."""
        self.set_tips(pb.z, pb.weights, pb.cleandata, None if pb.cleandata else pb.n_chara,
                      None if pb.cleandata else pb.chara_map, pb.gene_off if pb.n_genes > 1 else None)
        self.set_tree(pb.tree, pb.scale_node)
        self.set_pi(pb.pi)
        for i, e in enumerate(pb.eigen):
            self.set_eigen(i, e)
        self.set_classes(pb.mode, pb.freqK, pb.rate[:pb.K] if getattr(pb, "rate_per_gene", False) else pb.rate, pb.eigen_of, pb.qfactor)
        if getattr(pb, "rate_per_gene", False):
            r = np.ascontiguousarray(pb.rate, dtype=np.float64).reshape(pb.n_genes * pb.K)
            self._L.paml_amd_set_gene_class_rates.argtypes = [C.c_void_p, C.c_void_p]
            self._chk(self._L.paml_amd_set_gene_class_rates(self._h, _p(r)))
        return self

    def eval(self, branch, gene_rate=None, want_lnf=False, want_fhk=False):
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        lnL = C.c_double()
        lnf = np.zeros(self.n_patt) if want_lnf else None
        fhk = np.zeros((self.K, self.n_patt)) if want_fhk else None
        self._chk(self._L.paml_amd_eval(self._h, _p(b), _p(g), C.byref(lnL), _p(lnf), _p(fhk)))
        return dict(lnL=lnL.value, lnf=lnf, fhK=fhk)

    def eval_batch(self, branch, gene_rate=None, eigen_of=None, qfactor=None, freqK=None, rate=None, want_lnf=False):
        """lnL of every row of branch[n_batch][n_nodes] in one launch (paml_amd_eval_batch); the optional tables carry
        one leading batch axis over the layouts of set_classes."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        assert b.ndim == 2
        nb = b.shape[0]

        def opt(a, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            assert a.shape[0] == nb
            return a
        g, eo = opt(gene_rate, np.float64), opt(eigen_of, np.int32)
        qf, fk, rt = opt(qfactor, np.float64), opt(freqK, np.float64), opt(rate, np.float64)
        out = np.zeros(nb)
        lnf = np.zeros((nb, self.n_patt)) if want_lnf else None
        self._L.paml_amd_eval_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
        self._chk(self._L.paml_amd_eval_batch(self._h, nb, _p(b), _p(g), _p(eo), _p(qf), _p(fk), _p(rt), _p(out), _p(lnf)))
        return (out, lnf) if want_lnf else out

    def eval_adg(self, branch, MK, pose, gene_rate=None):
        """lfunAdG: +lnL of the rate chain MK[K][K] over the sites pose[ls] (site -> pattern), fx_r on the device."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        MK = np.ascontiguousarray(MK, dtype=np.float64)
        pose = np.ascontiguousarray(pose, dtype=np.int32)
        lnL = C.c_double()
        self._L.paml_amd_eval_adg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        self._chk(self._L.paml_amd_eval_adg(self._h, _p(b), _p(g), _p(MK), _p(pose), len(pose), C.byref(lnL)))
        return lnL.value

    def beb_grid(self, pcl, iw, w_class):
        """BEB grid integral over the fhK of the last evaluation (paml_amd_beb_grid): pcl[n_grid][n_cls], iw[n_grid][n_cls],
        w_class[K] -> dict(ln_fx, pr_last[n_patt], mean_w[n_patt], sd_w[n_patt])."""
        pcl = np.ascontiguousarray(pcl, dtype=np.float64)
        iw = np.ascontiguousarray(iw, dtype=np.int32)
        wc = np.ascontiguousarray(w_class, dtype=np.float64)
        assert pcl.shape == iw.shape and pcl.ndim == 2
        lnfx = C.c_double()
        pr, mw, sd = np.zeros(self.n_patt), np.zeros(self.n_patt), np.zeros(self.n_patt)
        self._L.paml_amd_beb_grid.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                                              C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self._L.paml_amd_beb_grid(self._h, pcl.shape[0], pcl.shape[1], _p(pcl), _p(iw), _p(wc), C.byref(lnfx), _p(pr), _p(mw), _p(sd)))
        return dict(ln_fx=lnfx.value, pr_last=pr, mean_w=mw, sd_w=sd)

    def beb_grid_classes(self, pcl, iw):
        """Posterior of every mixture class over the grid (paml_amd_beb_grid_classes) -> dict(ln_fx, post[n_cls][n_patt])."""
        pcl = np.ascontiguousarray(pcl, dtype=np.float64)
        iw = np.ascontiguousarray(iw, dtype=np.int32)
        assert pcl.shape == iw.shape and pcl.ndim == 2
        lnfx = C.c_double()
        post = np.zeros((pcl.shape[1], self.n_patt))
        self._L.paml_amd_beb_grid_classes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_void_p]
        self._chk(self._L.paml_amd_beb_grid_classes(self._h, pcl.shape[0], pcl.shape[1], _p(pcl), _p(iw), C.byref(lnfx), _p(post)))
        return dict(ln_fx=lnfx.value, post=post)

    def eval_device(self, branch, d_lnL_ptr, gene_rate=None):
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        self._chk(self._L.paml_amd_eval_device(self._h, _p(b), _p(g), C.c_void_p(d_lnL_ptr)))

    def set_eigen_warm_start(self, on=-1):
        """paml_amd_set_eigen_warm_start: switch (1 / 0; -1 leaves it), returns the number of warm-started decompositions so far."""
        n = C.c_long()
        self._L.paml_amd_set_eigen_warm_start.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_long)]
        self._chk(self._L.paml_amd_set_eigen_warm_start(self._h, int(on), C.byref(n)))
        return n.value

    def set_eigen_qrev_batch(self, set_ids, Q, pi, scale=None):
        """Decompose the reversible rate matrices Q[k] (frequencies pi[k]) on the device into eigen sets set_ids[k]; Root is divided by scale[k]."""
        ids = np.ascontiguousarray(set_ids, dtype=np.int32)
        Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(len(ids), self.n, self.n)
        pi = np.ascontiguousarray(pi, dtype=np.float64).reshape(len(ids), self.n)
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(len(ids))
        self._chk(self._L.paml_amd_set_eigen_qrev_batch(self._h, len(ids), _p(ids), _p(Q), _p(pi), _p(sc)))

    def set_eigen_qrev_batch_sparse(self, set_ids, row, col, vals, pi, scale=None):
        """As set_eigen_qrev_batch, the matrices given by their elements at (row[k] >= col[k]), vals[set][k]; everything else zero."""
        ids = np.ascontiguousarray(set_ids, dtype=np.int32)
        row = np.ascontiguousarray(row, dtype=np.int32); col = np.ascontiguousarray(col, dtype=np.int32)
        vals = np.ascontiguousarray(vals, dtype=np.float64).reshape(len(ids), len(row))
        pi = np.ascontiguousarray(pi, dtype=np.float64).reshape(len(ids), self.n)
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64).reshape(len(ids))
        self._chk(self._L.paml_amd_set_eigen_qrev_batch_sparse(self._h, len(ids), _p(ids), len(row), _p(row), _p(col), _p(vals), _p(pi), _p(sc)))

    def get_eigen(self, set_id):
        U, V, R = np.empty((self.n, self.n)), np.empty((self.n, self.n)), np.empty(self.n)
        self._chk(self._L.paml_amd_get_eigen(self._h, int(set_id), _p(U), _p(V), _p(R)))
        return U, V, R

    def eigen_counters(self, cap=4096):
        n, sw = C.c_long(), np.zeros(cap, dtype=np.int32)
        m = self._L.paml_amd_eigen_counters(self._h, C.byref(n), _p(sw), cap)
        return {"n_decomposed": n.value, "sweeps": sw[:max(m, 0)].copy()}

    def flush(self):
        """After a run of eval_device calls: the engine's stream waits for the totals still on the collective stream."""
        self._chk(self._L.paml_amd_flush(self._h))

    def eigen_status(self):
        """paml_amd_eigen_status: waits for the engine's stream; raises (code -5) if a queued device eigen-decomposition did not converge."""
        self._L.paml_amd_eigen_status.argtypes = [C.c_void_p]
        self._chk(self._L.paml_amd_eigen_status(self._h))

    def eval_dirty(self, branch, clean, gene_rate=None):
        b = np.ascontiguousarray(branch, dtype=np.float64)
        c = np.ascontiguousarray(clean, dtype=np.uint8)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        lnL = C.c_double()
        self._chk(self._L.paml_amd_eval_dirty(self._h, _p(b), _p(g), _p(c), C.byref(lnL)))
        return lnL.value

    def eval_branch(self, node_b, t, branch, gene_rate=None):
        """lnL(t), dlnL/dt, d2lnL/dt2 of the branch above node_b at the trial lengths t (lfuntdd)."""
        tt = np.ascontiguousarray(np.atleast_1d(t), dtype=np.float64)
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        l, dl, ddl = np.zeros(len(tt)), np.zeros(len(tt)), np.zeros(len(tt))
        self._chk(self._L.paml_amd_eval_branch(self._h, int(node_b), len(tt), _p(tt), _p(b), _p(g), _p(l), _p(dl), _p(ddl)))
        return l, dl, ddl

    def branch_partials(self):
        """Per-block partial sums of the last eval_branch: array [rows, 3 n_t] (paml_amd_get_branch_partials)."""
        rows, cols = C.c_long(), C.c_int()
        self._L.paml_amd_get_branch_partials.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_int)]
        self._chk(self._L.paml_amd_get_branch_partials(self._h, None, 0, C.byref(rows), C.byref(cols)))
        out = np.zeros((rows.value, cols.value))
        self._chk(self._L.paml_amd_get_branch_partials(self._h, _p(out), out.size, C.byref(rows), C.byref(cols)))
        return out

    def branch_counters(self):
        a, b = C.c_long(), C.c_long()
        self._L.paml_amd_branch_counters.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]
        self._L.paml_amd_branch_counters(self._h, C.byref(a), C.byref(b))
        self._L.paml_amd_branch_coef_hits.restype = C.c_long
        self._L.paml_amd_branch_coef_hits.argtypes = [C.c_void_p]
        self._L.paml_amd_branch_refill_kernels.restype = C.c_long
        self._L.paml_amd_branch_refill_kernels.argtypes = [C.c_void_p]
        return dict(n_calls=a.value, n_nodes=b.value, coef_hits=self._L.paml_amd_branch_coef_hits(self._h),
                    refill_kernels=self._L.paml_amd_branch_refill_kernels(self._h))

    def branch_kernel_ms(self):
        """Duration of the last eval_branch's contraction kernels by HIP events (needs profile(True)); < 0: not timed."""
        self._L.paml_amd_branch_kernel_ms.restype = C.c_double
        self._L.paml_amd_branch_kernel_ms.argtypes = [C.c_void_p]
        return float(self._L.paml_amd_branch_kernel_ms(self._h))

    def node_posterior(self, node, branch, gene_rate=None):
        """Posterior probabilities of the states at an internal node, [n_patt][n] (paml_amd_node_posterior)."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        post = np.zeros((self.n_patt, self.n))
        self._L.paml_amd_node_posterior.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self._L.paml_amd_node_posterior(self._h, int(node), _p(b), _p(g), _p(post)))
        return post

    def simulate(self, branch, n_sites, seed=1, replicate=0, first_site=0, gene_rate=None, want_classes=False, want_ancestors=False):
        """Draw n_sites sites under the loaded model (paml_amd_simulate): dict(z=[n_tips][n_sites] uint8 states, cls=[n_sites] or
        None, anc=[n_nodes - n_tips][n_sites] or None).  Site first_site + j is a pure function of (seed, replicate, first_site + j)."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        n_sites = int(n_sites)
        m = max(n_sites, 0)
        z = np.zeros((self.n_tips, m), dtype=np.uint8)
        cls = np.zeros(m, dtype=np.uint8) if want_classes else None
        anc = np.zeros((max(self.n_nodes - self.n_tips, 0), m), dtype=np.uint8) if want_ancestors else None
        self._L.paml_amd_simulate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_ulonglong, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self._L.paml_amd_simulate(self._h, _p(b), _p(g), n_sites, int(first_site), int(seed) & (2**64 - 1), int(replicate), _p(z), _p(cls), _p(anc)))
        return dict(z=z, cls=cls, anc=anc)

    def ancestral_marginal(self, branch, gene_rate=None, nodes=None, want_post=True):
        """Marginal reconstruction at many internal nodes in one call (paml_amd_ancestral_marginal): dict(best=[n_query][n_patt] uint8,
        prob=[n_query][n_patt], post=[n_query][n_patt][n] or None).  nodes None: every internal node, in node order."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        nd = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.int32)
        nq = max(self.n_nodes - self.n_tips, 0) if nd is None else len(nd)
        best = np.zeros((nq, self.n_patt), dtype=np.uint8)
        prob = np.zeros((nq, self.n_patt))
        post = np.zeros((nq, self.n_patt, self.n)) if want_post else None
        self._L.paml_amd_ancestral_marginal.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self._L.paml_amd_ancestral_marginal(self._h, _p(b), _p(g), 0 if nd is None else len(nd), _p(nd), _p(best), _p(prob), _p(post)))
        return dict(best=best, prob=prob, post=post)

    def ancestral_joint(self, branch, gene_rate=None):
        """Joint reconstruction, best assignment only (paml_amd_ancestral_joint): dict(states=[n_nodes - n_tips][n_patt] uint8,
        ln_best=[n_patt] log probability of data and assignment).  One class."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        states = np.zeros((max(self.n_nodes - self.n_tips, 0), self.n_patt), dtype=np.uint8)
        ln_best = np.zeros(self.n_patt)
        self._L.paml_amd_ancestral_joint.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self._L.paml_amd_ancestral_joint(self._h, _p(b), _p(g), _p(states), _p(ln_best)))
        return dict(states=states, ln_best=ln_best)

    def gradient(self, branch, gene_rate=None, want_lnf=False, want_scores=False):
        """The derivative of lnL with respect to every branch length in one call (paml_amd_gradient): dict(lnL, grad=[n_nodes] (the
        root's entry 0), lnf=[n_patt] or None, scores=[n_nodes][n_patt] d log f_h / d branch[v] or None)."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        lnL = C.c_double()
        grad = np.zeros(self.n_nodes)
        lnf = np.zeros(self.n_patt) if want_lnf else None
        scores = np.zeros((self.n_nodes, self.n_patt)) if want_scores else None
        self._L.paml_amd_gradient.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self._L.paml_amd_gradient(self._h, _p(b), _p(g), C.byref(lnL), _p(grad), _p(lnf), _p(scores)))
        return dict(lnL=lnL.value, grad=grad, lnf=lnf, scores=scores)

    def curvature(self, branch, gene_rate=None, want_lnf=False):
        """lnL, its derivative and its second derivative along every branch length in one call (paml_amd_curvature): dict(lnL,
        grad=[n_nodes], curv=[n_nodes] d^2 lnL / d branch[v]^2 (the root's entries 0), lnf=[n_patt] or None).  lnL, grad and lnf have
        the bytes Engine.gradient returns."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        lnL = C.c_double()
        grad, curv = np.zeros(self.n_nodes), np.zeros(self.n_nodes)
        lnf = np.zeros(self.n_patt) if want_lnf else None
        self._L.paml_amd_curvature.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self._L.paml_amd_curvature(self._h, _p(b), _p(g), C.byref(lnL), _p(grad), _p(curv), _p(lnf)))
        return dict(lnL=lnL.value, grad=grad, curv=curv, lnf=lnf)

    def hessian(self, branch, gene_rate=None, nodes=None, want_lnf=False):
        """lnL, its gradient and its Hessian over all branch lengths in one call (paml_amd_hessian): dict(lnL, grad=[n_nodes],
        hess=[n_nodes][n_nodes] d^2 lnL / d branch[u] d branch[v] (the root's row and column 0) or, with a list of `nodes`,
        [len(nodes)][len(nodes)] in the list's order, lnf=[n_patt] or None).  lnL, grad and lnf have the bytes Engine.gradient returns,
        the diagonal those of Engine.curvature's curv; hess equals its transpose."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        nl = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.int32)
        dim = self.n_nodes if nl is None else len(nl)
        lnL = C.c_double()
        grad, hess = np.zeros(self.n_nodes), np.zeros((dim, dim))
        lnf = np.zeros(self.n_patt) if want_lnf else None
        self._L.paml_amd_hessian.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self._L.paml_amd_hessian(self._h, _p(b), _p(g), _p(nl), 0 if nl is None else len(nl), C.byref(lnL), _p(grad), _p(hess), _p(lnf)))
        return dict(lnL=lnL.value, grad=grad, hess=hess, lnf=lnf)

    def model_gradient(self, branch, gene_rate=None, want_pairs=False):
        """The derivative of lnL with respect to every input of the engine in one call (paml_amd_model_gradient): dict(lnL,
        g_eff=[n_genes][K][n_nodes] d lnL / d (effective length), g_freqK=[K], g_pi=[n_pi][n], g_A=[n_eigen][n][n] d lnL / d A_ab of every
        set's rate matrix (every element independent), W=[n_genes][K][n_nodes][n][n] d lnL / d P_v(y, x) with want_pairs, else None)."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        lnL = C.c_double()
        n, K = self.n, self.K
        g_eff = np.zeros((self.n_genes, K, self.n_nodes))
        g_freqK = np.zeros(K)
        n_pi, n_eigen = C.c_int(), C.c_int()
        self._L.paml_amd_model_gradient_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self._chk(self._L.paml_amd_model_gradient_sizes(self._h, C.byref(n_pi), C.byref(n_eigen)))
        g_pi = np.zeros((n_pi.value, n))
        g_A = np.zeros((n_eigen.value, n, n))
        W = np.zeros((self.n_genes, K, self.n_nodes, n, n)) if want_pairs else None
        self._L.paml_amd_model_gradient.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)] + [C.c_void_p] * 5
        self._chk(self._L.paml_amd_model_gradient(self._h, _p(b), _p(g), C.byref(lnL), _p(g_eff), _p(g_freqK), _p(g_pi), _p(g_A), _p(W)))
        return dict(lnL=lnL.value, g_eff=g_eff, g_freqK=g_freqK, g_pi=g_pi, g_A=g_A, W=W)

    def subst_counts(self, branch, gene_rate=None, labels=None, nodes=None, want_sites=False, want_lnf=False):
        """Posterior expected labelled substitution counts and dwell times on every branch in one call (paml_amd_subst_counts):
        dict(lnL, counts=[n_lab][n_nodes] (the root's entries 0) or, with a list of non-root `nodes`, [n_lab][len(nodes)] in the list's
        order, site_counts=the same with a last axis [n_patt] or None, lnf=[n_patt] or None).  labels: [n_lab][n][n] weights, off the
        diagonal of the jumps a -> b, on it of the time spent in a (in units of branch[v])."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        if labels is None:
            raise EngineError("subst_counts: no labels")
        M = np.ascontiguousarray(labels, dtype=np.float64)
        if M.ndim == 2:
            M = M[None]
        if M.ndim != 3 or M.shape[1:] != (self.n, self.n):
            raise EngineError("subst_counts: labels must be [n_lab][%d][%d]" % (self.n, self.n))
        nd = None if nodes is None else np.ascontiguousarray(nodes, dtype=np.int32)
        nq = self.n_nodes if nd is None else len(nd)
        lnL = C.c_double()
        counts = np.zeros((len(M), nq))
        sites = np.zeros((len(M), nq, self.n_patt)) if want_sites else None
        lnf = np.zeros(self.n_patt) if want_lnf else None
        self._L.paml_amd_subst_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_double),
                                                  C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self._L.paml_amd_subst_counts(self._h, _p(b), _p(g), len(M), _p(M), 0 if nd is None else len(nd), _p(nd), C.byref(lnL), _p(counts), _p(sites), _p(lnf)))
        return dict(lnL=lnL.value, counts=counts, site_counts=sites, lnf=lnf)

    def nni_scores(self, branch, gene_rate=None, swaps=None, want_lnf=False):
        """The lnL of nearest-neighbour-interchange neighbours of the tree at `branch` in one call (paml_amd_nni_scores): dict(lnL0 (the
        present tree's), swaps=[n_swaps][3] (v, s, x), lnL=[n_swaps], lnf=[n_swaps][n_patt] or None).  swaps None: the canonical list
        (paml_amd_nni_list) of the tree last set."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        if swaps is None:
            if getattr(self, "_tree_csr", None) is None:
                raise EngineError("nni_scores: no tree was set through this object")
            swaps = nni_list(self.n_tips, self.n_nodes, *self._tree_csr)
        sw = np.ascontiguousarray(swaps, dtype=np.int32).reshape(-1, 3)
        lnL0 = C.c_double()
        lnL = np.zeros(len(sw))
        lnf = np.zeros((len(sw), self.n_patt)) if want_lnf else None
        self._L.paml_amd_nni_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
        self._chk(self._L.paml_amd_nni_scores(self._h, _p(b), _p(g), len(sw), _p(sw), C.byref(lnL0), _p(lnL), _p(lnf)))
        return dict(lnL0=lnL0.value, swaps=sw, lnL=lnL, lnf=lnf)

    def edge_scores(self, branch, gene_rate=None, rows=None, ovr_node=None, ovr_t=None, want_lnf=False):
        """The lnL of configurations of internal edges at trial lengths of the five branches around them, with the first and second
        derivative along one of them, in one call (paml_amd_edge_scores): dict(lnL0 (the present tree's at `branch`), lnL, d1, d2 =
        [n_rows], lnf=[n_rows][n_patt] or None).  rows: int [n_rows][4] = v, s, x, u (s = x = -1: the present configuration; u = -1: no
        derivative); ovr_node: int [n_rows][5] (-1: unused) and ovr_t: [n_rows][5], the branches whose lengths replace `branch`'s."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        if rows is None or ovr_node is None or ovr_t is None:
            raise EngineError("edge_scores: rows, ovr_node and ovr_t are needed")
        rw = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 4)
        on = np.ascontiguousarray(ovr_node, dtype=np.int32).reshape(-1, 5)
        ot = np.ascontiguousarray(ovr_t, dtype=np.float64).reshape(-1, 5)
        if not (len(rw) == len(on) == len(ot)):
            raise EngineError("edge_scores: rows, ovr_node and ovr_t differ in length")
        lnL0 = C.c_double()
        lnL, d1, d2 = np.zeros(len(rw)), np.zeros(len(rw)), np.zeros(len(rw))
        lnf = np.zeros((len(rw), self.n_patt)) if want_lnf else None
        self._L.paml_amd_edge_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self._L.paml_amd_edge_scores(self._h, _p(b), _p(g), len(rw), _p(rw), _p(on), _p(ot), C.byref(lnL0), _p(lnL), _p(d1), _p(d2), _p(lnf)))
        return dict(lnL0=lnL0.value, lnL=lnL, d1=d1, d2=d2, lnf=lnf)

    def relabel_scores(self, branch, gene_rate=None, rows=None, base_label=None, want_lnf=False, want_classes=False):
        """The lnL of the tree at `branch` with the label of one branch changed, for every (node, label) row in one call
        (paml_amd_relabel_scores): dict(lnL0 (the present tree's), rows=[n_rows][2] (v, label), lnL=[n_rows], lnf=[n_rows][n_patt] or
        None, lnfk0=[K][n_patt] and lnfk=[n_rows][K][n_patt] with want_classes (the logs of the class-conditional likelihoods, without
        freqK), else None).  rows None: every non-root node of the tree last set with every label of the class table, in node order.
        base_label: int [n_nodes], the labels the rows start from instead of the tree's own."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        if rows is None:
            if getattr(self, "_tree_csr", None) is None or getattr(self, "n_labels", None) is None:
                raise EngineError("relabel_scores: no tree or no class table was set through this object")
            rows = [(v, l) for v in range(self.n_nodes) if v != self._tree_csr[0] for l in range(self.n_labels)]
        rw = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 2)
        bl = None if base_label is None else np.ascontiguousarray(base_label, dtype=np.int32)
        if bl is not None and bl.shape != (self.n_nodes,):
            raise EngineError("relabel_scores: base_label must be [n_nodes]")
        lnL0 = C.c_double()
        lnL = np.zeros(len(rw))
        lnf = np.zeros((len(rw), self.n_patt)) if want_lnf else None
        lnfk0 = np.zeros((self.K, self.n_patt)) if want_classes else None
        lnfk = np.zeros((len(rw), self.K, self.n_patt)) if want_classes else None
        self._L.paml_amd_relabel_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_double),
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self._L.paml_amd_relabel_scores(self._h, _p(b), _p(g), _p(bl), len(rw), _p(rw), C.byref(lnL0), _p(lnL), _p(lnf), _p(lnfk0), _p(lnfk)))
        return dict(lnL0=lnL0.value, rows=rw, lnL=lnL, lnf=lnf, lnfk0=lnfk0, lnfk=lnfk)

    def placement_scores(self, branch, gene_rate=None, queries=None, edges=None, pendant=(0.1,), phi=0.5, pendant_label=0, want_lnf=False):
        """The lnL of the tree at `branch` with a query tip hung on a branch, for every query, edge and pendant length in one call
        (paml_amd_placement_scores): dict(lnL0 (the present tree's), edges=[n_edges] (nodes v: the branch above v), lnL=[n_q][n_edges][n_pend],
        lnf=[n_q][n_edges][n_pend][n_patt] or None).  queries: uint8 [n_q][n_patt] character codes; edges None: every non-root node of the
        tree last set, in node order.  The new node splits the branch above v into phi t_v (above v) and (1 - phi) t_v."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        if queries is None:
            raise EngineError("placement_scores: no queries")
        qz = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.uint8)
        if qz.ndim != 2 or qz.shape[1] != self.n_patt:
            raise EngineError("placement_scores: queries must be [n_q][n_patt]")
        if edges is None:
            if getattr(self, "_tree_csr", None) is None:
                raise EngineError("placement_scores: no tree was set through this object")
            edges = [v for v in range(self.n_nodes) if v != self._tree_csr[0]]
        ed = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1)
        pe = np.ascontiguousarray(np.atleast_1d(pendant), dtype=np.float64).reshape(-1)
        lnL0 = C.c_double()
        lnL = np.zeros((len(qz), len(ed), len(pe)))
        lnf = np.zeros((len(qz), len(ed), len(pe), self.n_patt)) if want_lnf else None
        self._L.paml_amd_placement_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                      C.c_double, C.c_int, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
        self._chk(self._L.paml_amd_placement_scores(self._h, _p(b), _p(g), len(qz), _p(qz), len(ed), _p(ed), len(pe), _p(pe), float(phi),
                                                    int(pendant_label), C.byref(lnL0), _p(lnL), _p(lnf)))
        return dict(lnL0=lnL0.value, edges=ed, lnL=lnL, lnf=lnf)

    def attach_scores(self, branch, gene_rate=None, queries=None, rows=None, t3=None, pendant_label=0, want_lnf=False):
        """The lnL of the tree at `branch` with a query tip hung on a branch at the row's own three lengths, and its first and second
        derivative along one of them, for many rows in one call (paml_amd_attach_scores): dict(lnL0 (the present tree's), rows, lnL, d1,
        d2 = [n_rows], lnf=[n_rows][n_patt] or None).  queries: uint8 [n_q][n_patt] character codes; rows: [n_rows][3] = q, v (the branch
        above v), role (-1: no derivative, 0: the branch above the new node, 1: the branch above v, 2: the query's); t3: [n_rows][3] =
        t_up, t_dn, t_pend."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        if queries is None or rows is None or t3 is None:
            raise EngineError("attach_scores: queries, rows and t3 are all needed")
        qz = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.uint8)
        if qz.ndim != 2 or qz.shape[1] != self.n_patt:
            raise EngineError("attach_scores: queries must be [n_q][n_patt]")
        rw = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 3)
        tt = np.ascontiguousarray(t3, dtype=np.float64).reshape(-1, 3)
        if len(tt) != len(rw):
            raise EngineError("attach_scores: t3 must be [n_rows][3]")
        lnL0 = C.c_double()
        lnL, d1, d2 = np.zeros(len(rw)), np.zeros(len(rw)), np.zeros(len(rw))
        lnf = np.zeros((len(rw), self.n_patt)) if want_lnf else None
        self._L.paml_amd_attach_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                   C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self._L.paml_amd_attach_scores(self._h, _p(b), _p(g), len(qz), _p(qz), len(rw), _p(rw), _p(tt), int(pendant_label), C.byref(lnL0),
                                                 _p(lnL), _p(d1), _p(d2), _p(lnf)))
        return dict(lnL0=lnL0.value, rows=rw, lnL=lnL, d1=d1, d2=d2, lnf=lnf)

    def spr_scores(self, branch, gene_rate=None, moves=None, radius=0, phi=0.5, want_lnf=False):
        """The lnL of subtree-prune-and-regraft neighbours of the tree at `branch` in one call (paml_amd_spr_scores): dict(lnL0 (the
        present tree's), moves=[n_moves][2] (s, x), lnL=[n_moves], lnf=[n_moves][n_patt] or None).  The subtree below s is hung on the
        branch above x, which the new node splits into phi t_x (above x) and (1 - phi) t_x (Tree.spr).  moves None: the canonical list
        (paml_amd_spr_list) of the tree last set, within `radius` branches (radius <= 0: no limit)."""
        b = np.ascontiguousarray(branch, dtype=np.float64)
        g = None if gene_rate is None else np.ascontiguousarray(gene_rate, dtype=np.float64)
        if moves is None:
            if getattr(self, "_tree_csr", None) is None:
                raise EngineError("spr_scores: no tree was set through this object")
            moves = spr_list(self.n_tips, self.n_nodes, *self._tree_csr, radius=radius)
        mv = np.ascontiguousarray(moves, dtype=np.int32).reshape(-1, 2)
        lnL0 = C.c_double()
        lnL = np.zeros(len(mv))
        lnf = np.zeros((len(mv), self.n_patt)) if want_lnf else None
        self._L.paml_amd_spr_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
        self._chk(self._L.paml_amd_spr_scores(self._h, _p(b), _p(g), len(mv), _p(mv), float(phi), C.byref(lnL0), _p(lnL), _p(lnf)))
        return dict(lnL0=lnL0.value, moves=mv, lnL=lnL, lnf=lnf)

    def get_pmat(self, gene, iclass, node):
        P = np.zeros((self.n, self.n))
        self._chk(self._L.paml_amd_get_pmat(self._h, gene, iclass, node, _p(P)))
        return P

    def get_partials(self, node, iclass=0):
        a = np.zeros((self.n_patt, self.n))
        self._chk(self._L.paml_amd_get_partials(self._h, node, iclass, _p(a)))
        return a

    def get_scale(self, node, iclass=0):
        a = np.zeros(self.n_patt)
        self._chk(self._L.paml_amd_get_scale(self._h, node, iclass, _p(a)))
        return a

    def profile(self, on=True):
        self._chk(self._L.paml_amd_profile(self._h, int(on)))

    def profile_read(self):
        a, b, c, n = C.c_double(), C.c_double(), C.c_double(), C.c_long()
        self._chk(self._L.paml_amd_profile_read(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return dict(ms_pmat=a.value, ms_prune=b.value, ms_reduce=c.value, n_evals=n.value)

    def cherry_tables(self):
        """(cherries tabulated, table bytes) of the last evaluation; (0, 0) when it ran without cherry tables."""
        a, b = C.c_long(), C.c_long()
        self._L.paml_amd_cherry_tables.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]
        self._chk(self._L.paml_amd_cherry_tables(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def subtree_tables(self):
        """Subtree tables of the last evaluation: dict(nodes, u — the nodes tabulated above the cherries and their numbers of classes, sons
        before fathers —, bytes, blocks_left — operand blocks left per tile, -1 without subtree tables —, n_computed — class computations
        of this engine so far)."""
        cap = 256
        n, by, bl, nc = C.c_long(), C.c_long(), C.c_long(), C.c_long()
        nodes, u = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int64)
        self._L.paml_amd_subtree_tables.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.c_void_p, C.c_void_p, C.c_int] + [C.POINTER(C.c_long)] * 3
        self._chk(self._L.paml_amd_subtree_tables(self._h, C.byref(n), _p(nodes), _p(u), cap, C.byref(by), C.byref(bl), C.byref(nc)))
        k = min(n.value, cap)
        return dict(nodes=nodes[:k].tolist(), u=u[:k].tolist(), bytes=by.value, blocks_left=bl.value, n_computed=nc.value)

    def subtree_order(self):
        """The pattern order of the walk with subtree tables: dict(in_use — the last evaluation ran with it —, n_computed — order
        computations of this engine so far —, host_seconds of the last one)."""
        use, nc, sec = C.c_int(), C.c_long(), C.c_double()
        self._L.paml_amd_subtree_order.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_double)]
        self._chk(self._L.paml_amd_subtree_order(self._h, C.byref(use), C.byref(nc), C.byref(sec)))
        return dict(in_use=bool(use.value), n_computed=nc.value, host_seconds=sec.value)

    def gather_walk(self):
        """The gathering walk (csrc/kernels_prune.h: gather_walk_kernel): dict(in_use — the last evaluation ran on it —, tiles, rows — of
        its layout, the distinct rows per class of the model —, R — the most rows of a tile —, n_computed — layouts of this engine so
        far —, host_seconds of the last one)."""
        use, nt, nr, r, nc, sec = C.c_int(), C.c_long(), C.c_long(), C.c_int(), C.c_long(), C.c_double()
        self._L.paml_amd_gather_walk.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_int), C.POINTER(C.c_long),
                                                 C.POINTER(C.c_double)]
        self._chk(self._L.paml_amd_gather_walk(self._h, C.byref(use), C.byref(nt), C.byref(nr), C.byref(r), C.byref(nc), C.byref(sec)))
        return dict(in_use=bool(use.value), tiles=nt.value, rows=nr.value, R=r.value, n_computed=nc.value, host_seconds=sec.value)

    def counters(self):
        a, b = C.c_long(), C.c_long()
        self._L.paml_amd_counters(self._h, C.byref(a), C.byref(b))
        return dict(n_eval=a.value, n_pmat=b.value)


class PairSet:
    """Pairwise ML comparisons on an engine's clean tips (paml_amd_pairset_*): pairs[k] = (a, b), 0-based sequences."""

    def __init__(self, eng: Engine, pairs):
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        a, b = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        L = eng._L
        L.paml_amd_pairset_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p]
        L.paml_amd_pairset_destroy.argtypes = [C.c_void_p]
        L.paml_amd_pairset_destroy.restype = None
        L.paml_amd_pairset_get_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.paml_amd_pairset_set_pi.argtypes = [C.c_void_p, C.c_void_p]
        L.paml_amd_pairset_set_pattern.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.paml_amd_pairset_eval.argtypes = [C.c_void_p, C.c_long] + [C.c_void_p] * 5
        L.paml_amd_pairset_failed.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
        L.paml_amd_pairset_counters.argtypes = [C.c_void_p] + [C.POINTER(C.c_long)] * 4
        self._eng, self._L, self.n, self.n_pairs = eng, L, eng.n, len(pr)
        h = C.c_void_p()
        eng._chk(L.paml_amd_pairset_create(eng._h, C.byref(h), len(pr), _p(a), _p(b)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.paml_amd_pairset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def counts(self):
        """(fp[n_pairs][n][n] with row = the larger state, ls_pair[n_pairs])."""
        fp, ls = np.zeros((self.n_pairs, self.n, self.n)), np.zeros(self.n_pairs)
        self._eng._chk(self._L.paml_amd_pairset_get_counts(self._h, _p(fp), _p(ls)))
        return fp, ls

    def set_pi(self, pi):
        pi = np.ascontiguousarray(pi, dtype=np.float64)
        assert pi.shape == (self.n_pairs, self.n)
        self._eng._chk(self._L.paml_amd_pairset_set_pi(self._h, _p(pi)))

    def set_pattern(self, row, col, flags):
        row, col = np.ascontiguousarray(row, dtype=np.int32), np.ascontiguousarray(col, dtype=np.int32)
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        assert len(row) == len(col) == len(fl)
        self._eng._chk(self._L.paml_amd_pairset_set_pattern(self._h, len(row), _p(row), _p(col), _p(fl)))

    def eval(self, pair, t, kappa, omega):
        """lnL of the elements (pair[i], t[i], kappa[i], omega[i]); raises EngineError (code -5) if a decomposition did not converge —
        failed() then lists those elements."""
        pr = np.ascontiguousarray(pair, dtype=np.int32)
        t, k, w = (np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), pr.shape)) for x in (t, kappa, omega))
        out = np.zeros(len(pr))
        self._eng._chk(self._L.paml_amd_pairset_eval(self._h, len(pr), _p(pr), _p(t), _p(k), _p(w), _p(out)))
        return out

    def failed(self):
        n = self._L.paml_amd_pairset_failed(self._h, None, 0)
        idx = np.zeros(max(n, 1), dtype=np.int64)
        self._L.paml_amd_pairset_failed(self._h, _p(idx), n)
        return idx[:n]

    def counters(self):
        v = [C.c_long() for _ in range(4)]
        self._L.paml_amd_pairset_counters(self._h, *[C.byref(x) for x in v])
        return dict(n_elem=v[0].value, n_decomp=v[1].value, n_chunks=v[2].value, arena_slots=v[3].value)


COMM_ID_BYTES = 128


def shard_bounds(n_patt_global, world, rank):
    """(first, count) of rank's contiguous pattern shard — paml_amd_shard_bounds, host only (no GPU needed)."""
    first, count = C.c_long(), C.c_long()
    rc = lib().paml_amd_shard_bounds(int(n_patt_global), int(world), int(rank), C.byref(first), C.byref(count))
    if rc != 0:
        raise EngineError("paml_amd_shard_bounds(%d patterns, world %d) failed (%d): at most %d ranks for this many patterns"
                          % (n_patt_global, world, rc, lib().paml_amd_max_ranks(int(n_patt_global))))
    return first.value, count.value


def max_ranks(n_patt_global):
    """The largest number of ranks the patterns can be sharded over (= the number of reduction chunks)."""
    return lib().paml_amd_max_ranks(int(n_patt_global))


def comm_unique_id():
    """The 128-byte RCCL id rank 0 creates and passes to the other ranks (paml_amd_comm_unique_id)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = lib().paml_amd_comm_unique_id(buf)
    if rc != 0:
        raise EngineError("paml_amd_comm_unique_id failed (%d): librccl.so.1 not found?" % rc)
    return buf.raw


def comm_library():
    """Path of the collective library the exchange step is bound to (paml_amd_comm_library: dladdr of ncclAllReduce)."""
    buf = C.create_string_buffer(4096)
    L = lib()
    L.paml_amd_comm_library.argtypes = [C.c_char_p, C.c_int]
    rc = L.paml_amd_comm_library(buf, len(buf))
    if rc < 0:
        raise EngineError("paml_amd_comm_library failed (%d): librccl.so.1 not found?" % rc)
    return buf.value.decode()


def device_count():
    """GPUs visible to this process (paml_amd_device_count)."""
    return int(lib().paml_amd_device_count())


def debug_program(tree, scale_node=None, keep=False, clean=None):
    """Host-only: the flattened tree program (list of (code, a, b, c)) and its stack depth."""
    L = lib()
    ptr, flat = tree.csr()
    sc = None if scale_node is None else np.ascontiguousarray(scale_node, dtype=np.uint8)
    cl = None if clean is None else np.ascontiguousarray(clean, dtype=np.uint8)
    cap = 8 * tree.n_nodes + 8
    ops = np.zeros((cap, 4), dtype=np.int32)
    ms = C.c_int()
    L.paml_amd_debug_program.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    nops = L.paml_amd_debug_program(tree.n_tips, tree.n_nodes, tree.root, _p(ptr), _p(flat), _p(sc), int(keep), _p(cl),
                                    _p(ops), cap, C.byref(ms))
    if nops < 0:
        raise EngineError("debug_program failed (%d)" % nops)
    return [tuple(int(v) for v in r) for r in ops[:nops]], ms.value


def debug_branch_plan(tree, calls, scale_node=None):
    """Host-only: the bookkeeping of eval_branch (paml_amd_debug_branch_plan) played for `calls`, a list of (node_b, branch[n_nodes]),
    each call forming what it finds dirty.  Returns (ends [n_calls][2] = (A, B), up [n_calls][n_nodes], clean [n_calls][n_nodes], the ops
    of the last call's program of dirty subtrees as debug_program gives them)."""
    L = lib()
    ptr, flat = tree.csr()
    sc = None if scale_node is None else np.ascontiguousarray(scale_node, dtype=np.uint8)
    nb = np.ascontiguousarray([c[0] for c in calls], dtype=np.int32)
    br = np.ascontiguousarray([c[1] for c in calls], dtype=np.float64).reshape(len(calls), tree.n_nodes)
    ends = np.zeros((len(calls), 2), dtype=np.int32)
    up = np.zeros((len(calls), tree.n_nodes), dtype=np.int32)
    clean = np.zeros((len(calls), tree.n_nodes), dtype=np.uint8)
    cap = 8 * tree.n_nodes + 8
    ops = np.zeros((cap, 4), dtype=np.int32)
    L.paml_amd_debug_branch_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    nops = L.paml_amd_debug_branch_plan(tree.n_tips, tree.n_nodes, tree.root, _p(ptr), _p(flat), _p(sc), len(calls), _p(nb), _p(br),
                                        _p(ends), _p(up), _p(clean), _p(ops), cap)
    if nops < 0:
        raise EngineError("debug_branch_plan failed (%d)" % nops)
    return ends, up, clean, [tuple(int(v) for v in r) for r in ops[:nops]]


def debug_code_order(n_states, n_chara, chara_map, z):
    """Host-only: the order in which set_tips keeps the codes of a table of more than 64 codes at 21..64 states: order[new code] = the
    caller's code (paml_amd_debug_code_order)."""
    L = lib()
    nch = np.ascontiguousarray(n_chara, dtype=np.int32)
    cm = np.ascontiguousarray(chara_map, dtype=np.uint8)
    zz = np.ascontiguousarray(z, dtype=np.uint8).ravel()
    order = np.zeros(len(nch), dtype=np.int32)
    L.paml_amd_debug_code_order.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    rc = L.paml_amd_debug_code_order(int(n_states), len(nch), _p(nch), _p(cm), _p(zz), zz.size, _p(order))
    if rc < 0:
        raise EngineError("debug_code_order failed (%d)" % rc)
    return order


def debug_jit(tree, scale_node=None, compile=True, n_states=0, fused=None):
    """Host-only: source of the kernel specialised for `tree` (hiprtc-compiled for gfx950 when compile=True);
    n_states 4 / 5 / 20 selects the one-pattern-per-lane kernels, anything else the 61-state MFMA kernel."""
    L = lib()
    ptr, flat = tree.csr()
    sc = None if scale_node is None else np.ascontiguousarray(scale_node, dtype=np.uint8)
    cap = 1 << 20
    buf = C.create_string_buffer(cap)
    L.paml_amd_debug_jit.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    flags = int(bool(compile)) | (int(n_states) << 8)
    if fused:      # (K classes, n_codes[, reduction chunk]): the fused 4 / 5-state kernel
        flags |= 2 | (int(fused[0]) << 16) | (int(fused[1]) << 24) | ((int(fused[2]) // 256 if len(fused) > 2 else 1) << 2)
    rc = L.paml_amd_debug_jit(tree.n_tips, tree.n_nodes, tree.root, _p(ptr), _p(flat), _p(sc), buf, cap, flags)
    if rc < 0:
        raise EngineError("debug_jit failed (%d): %s" % (rc, buf.value.decode(errors="replace")[-3000:]))
    return buf.value.decode()


def debug_jit_tables(tree, scale_node=None, max_tabs=1 << 20):
    """Host-only: the cherry-table form of the 61-state kernel specialised for `tree`: (source, operand stream as (is_tip, node) pairs,
    tabulated cherries as (tip a, tip b, node) triples); at most max_tabs cherries are tabulated."""
    L = lib()
    ptr, flat = tree.csr()
    sc = None if scale_node is None else np.ascontiguousarray(scale_node, dtype=np.uint8)
    cap = 1 << 21
    buf = C.create_string_buffer(cap)
    stream = np.zeros(4 * tree.n_nodes + 8, dtype=np.int32)
    tabs = np.zeros(3 * tree.n_tips + 3, dtype=np.int32)
    ns = C.c_int()
    L.paml_amd_debug_jit_tables.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int,
                                            C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_int]
    rc = L.paml_amd_debug_jit_tables(tree.n_tips, tree.n_nodes, tree.root, _p(ptr), _p(flat), _p(sc), int(max_tabs), buf, cap,
                                     _p(stream), len(stream), C.byref(ns), _p(tabs), len(tabs))
    if rc < 0:
        raise EngineError("debug_jit_tables failed (%d)" % rc)
    return buf.value.decode(), [tuple(x) for x in stream[:2 * ns.value].reshape(-1, 2)], [tuple(x) for x in tabs[:3 * rc].reshape(-1, 3)]


def debug_subtree_classes(tree, z, n_codes, want_classes=False):
    """Host-only: the subtree classes (csrc/subtree_classes.h) of tip codes z[n_tips][n_patt] on `tree`: u[n_nodes], the number of classes
    of every internal node below the root (0 elsewhere); with want_classes also cls[n_nodes][n_patt]."""
    L = lib()
    ptr, flat = tree.csr()
    z = np.ascontiguousarray(z, dtype=np.uint8)
    n_patt = z.shape[1]
    u = np.zeros(tree.n_nodes, dtype=np.uint32)
    cls = np.zeros((tree.n_nodes, n_patt), dtype=np.uint32) if want_classes else None
    L.paml_amd_debug_subtree_classes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_void_p]
    rc = L.paml_amd_debug_subtree_classes(tree.n_tips, tree.n_nodes, tree.root, _p(ptr), _p(flat), _p(z), n_patt, int(n_codes), _p(u), _p(cls))
    if rc < 0:
        raise EngineError("debug_subtree_classes failed (%d)" % rc)
    return (u, cls) if want_classes else u


def debug_subtree_order(keys, bound, largest_first=False, as_given=False):
    """Host-only: the pattern order (csrc/subtree_classes.h: subtree_pattern_order) for class arrays keys[n_keys][n_patt] below bound[n_keys]:
    order[position] = pattern, sorted by the engine's sequence of the keys (or, as_given, by the keys in the order given)."""
    L = lib()
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    bound = np.ascontiguousarray(bound, dtype=np.uint32)
    out = np.zeros(keys.shape[1], dtype=np.uint32)
    L.paml_amd_debug_subtree_order.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p]
    rc = L.paml_amd_debug_subtree_order(keys.shape[0], _p(keys), _p(bound), keys.shape[1], int(largest_first), int(as_given), _p(out))
    if rc < 0:
        raise EngineError("debug_subtree_order failed (%d)" % rc)
    return out


def debug_gather_tiles(keys, bound, order=None, wflag=None, R=128):
    """Host-only: the tiles of the gathering walk (csrc/gather_tiles.h) for row arrays keys[n_keys][n_patt] below bound[n_keys] along
    order[position] = pattern (None: the identity): a list of dicts, one per tile — first, count, rows (one list per key), slot
    [n_keys][count] (into that key's list), flag[count], patt[count] — decoded from the blocks the kernel reads, and the number of
    distinct rows in all."""
    L = lib()
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    bound = np.ascontiguousarray(bound, dtype=np.uint32)
    nk, n_patt = keys.shape
    order = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    wflag = None if wflag is None else np.ascontiguousarray(wflag, dtype=np.uint8)
    L.paml_amd_debug_gather_tiles.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long,
                                              C.POINTER(C.c_long), C.POINTER(C.c_long)]
    nt, nr = C.c_long(), C.c_long()
    db = L.paml_amd_debug_gather_tiles(nk, _p(keys), _p(bound), _p(order), _p(wflag), n_patt, int(R), None, 0, C.byref(nt), C.byref(nr))
    if db < 0:
        raise EngineError("debug_gather_tiles failed (%d)" % db)
    blocks = np.zeros(nt.value * db, dtype=np.uint8)
    L.paml_amd_debug_gather_tiles(nk, _p(keys), _p(bound), _p(order), _p(wflag), n_patt, int(R), _p(blocks), blocks.size, C.byref(nt), C.byref(nr))
    off_slot = 32 + 4 * (R + 4)
    tiles = []
    for t in range(nt.value):
        d = blocks[t * db:(t + 1) * db]
        head = d[:32].view(np.int32)
        rows = d[32:off_slot].view(np.uint32)
        start = [0, int(head[2]), int(head[3]), int(head[4]), int(head[5])]
        count = int(head[1])
        slot = d[off_slot:off_slot + 512].reshape(4, 128)
        tiles.append(dict(first=int(head[0]), count=count, slots=int(head[5]), start=start[:nk],
                          rows=[rows[start[k]:start[k + 1]].tolist() for k in range(nk)],
                          slot=np.stack([slot[k, :count].astype(np.int64) - start[k] for k in range(nk)]), slot_tail=slot[:nk, count:].copy(),
                          flag=d[off_slot + 512:off_slot + 640][:count].copy(), flag_tail=d[off_slot + 512:off_slot + 640][count:].copy(),
                          patt=d[off_slot + 640:off_slot + 640 + 512].view(np.int32)[:count].copy()))
    return tiles, nr.value


def debug_subtree_select(tree, z, n_states, n_codes, K=1, scale_node=None):
    """Host-only: the nodes an engine of these sizes would tabulate above the cherries for tip codes z (the switches of the environment
    apply), sons before fathers."""
    L = lib()
    ptr, flat = tree.csr()
    z = np.ascontiguousarray(z, dtype=np.uint8)
    sc = None if scale_node is None else np.ascontiguousarray(scale_node, dtype=np.uint8)
    sel = np.zeros(tree.n_nodes, dtype=np.int32)
    L.paml_amd_debug_subtree_select.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long,
                                                C.c_void_p, C.c_int]
    n = L.paml_amd_debug_subtree_select(tree.n_tips, tree.n_nodes, tree.root, _p(ptr), _p(flat), _p(sc), int(n_states), int(n_codes), int(K), _p(z), z.shape[1],
                                        _p(sel), len(sel))
    if n < 0:
        raise EngineError("debug_subtree_select failed (%d)" % n)
    return sel[:n].tolist()


def debug_jit_subtree(tree, nodes, n_states=61, n_codes=61, K=1, compile=True, scale_node=None, directory=None):
    """Host-only: the per-tree kernel with subtree tables of `nodes` (sons before fathers) beside the cherry tables: (source, operand blocks
    left per tile); compiled for gfx950 when compile=True, into `directory` when given.  ("", None) when the table form does not apply."""
    L = lib()
    ptr, flat = tree.csr()
    sc = None if scale_node is None else np.ascontiguousarray(scale_node, dtype=np.uint8)
    sel = np.ascontiguousarray(nodes, dtype=np.int32)
    cap = 1 << 21
    buf = C.create_string_buffer(cap)
    left = C.c_int(-1)
    L.paml_amd_debug_jit_subtree.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                             C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    if directory:
        os.makedirs(directory, exist_ok=True)
    rc = L.paml_amd_debug_jit_subtree(tree.n_tips, tree.n_nodes, tree.root, _p(ptr), _p(flat), _p(sc), int(n_states), int(n_codes), int(K), _p(sel), len(sel),
                                      int(bool(compile)), os.fsencode(directory) if directory else None, buf, cap, C.byref(left))
    if rc < 0:
        raise EngineError("debug_jit_subtree failed (%d): %s" % (rc, buf.value.decode(errors="replace")[-3000:]))
    if rc == 0:
        return "", None
    return buf.value.decode(), left.value


JIT_SHIPPED_DIR = os.path.join(_HERE, "lib", "jit")


def jit_prebuild(tree, n_states, n_codes, K=1, n_patt_global=1_000_000, scale_node=None, directory=None):
    """Host-only: compile the per-tree kernel for (tree, sizes) into `directory` (default: the library's lib/jit)."""
    L = lib()
    ptr, flat = tree.csr()
    sc = None if scale_node is None else np.ascontiguousarray(scale_node, dtype=np.uint8)
    d = directory or JIT_SHIPPED_DIR
    os.makedirs(d, exist_ok=True)
    log = C.create_string_buffer(1 << 16)
    L.paml_amd_jit_prebuild.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_char_p, C.c_char_p, C.c_int]
    rc = L.paml_amd_jit_prebuild(int(n_states), tree.n_tips, int(n_codes), int(K), int(n_patt_global), tree.n_nodes, tree.root, _p(ptr), _p(flat),
                                 _p(sc), os.fsencode(d), log, len(log))
    if rc != 0:
        raise EngineError("jit_prebuild failed (%d): %s" % (rc, log.value.decode(errors="replace")[-2000:]))


def compress_patterns(chars, gene=None):
    """PatternWeight on the device (paml_amd_compress_patterns): chars uint8 [n_seq][n_sites * width] or [n_seq][n_sites][width].
    Returns dict(first_site[n_patt], weights[n_patt], pose[n_sites])."""
    chars = np.ascontiguousarray(chars, dtype=np.uint8)
    width = 1 if chars.ndim == 2 else chars.shape[2]
    n_seq, n_sites = chars.shape[0], chars.shape[1]
    g = None if gene is None else np.ascontiguousarray(gene, dtype=np.int32)
    npatt = C.c_int()
    first, w, pose = np.zeros(n_sites, dtype=np.int32), np.zeros(n_sites), np.zeros(n_sites, dtype=np.int32)
    L = lib()
    L.paml_amd_compress_patterns.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p]
    rc = L.paml_amd_compress_patterns(n_seq, n_sites, width, _p(chars), _p(g), C.byref(npatt), _p(first), _p(w), _p(pose))
    if rc != 0:
        raise EngineError("paml_amd_compress_patterns failed (%d)" % rc)
    return dict(first_site=first[:npatt.value].copy(), weights=w[:npatt.value].copy(), pose=pose)


def rell_info():
    """Constants of the replicate kernels and the batches of this thread's last rell_replicates (paml_amd_rell_info):
    dict(chunk, tree_block, last_batches, last_kernel_ms).  Host only."""
    v, ms = [C.c_int() for _ in range(3)], C.c_double()
    L = lib()
    L.paml_amd_rell_info.argtypes = [C.POINTER(C.c_int)] * 3 + [C.POINTER(C.c_double)]
    L.paml_amd_rell_info.restype = None
    L.paml_amd_rell_info(*[C.byref(x) for x in v], C.byref(ms))
    return dict(chunk=v[0].value, tree_block=v[1].value, last_batches=v[2].value, last_kernel_ms=ms.value)


def simulate_info():
    """Batches walked by this thread's last Engine.simulate and the time of its kernels by HIP events (paml_amd_simulate_info):
    dict(last_batches, last_kernel_ms)."""
    L = lib()
    nb, ms = C.c_int(), C.c_double()
    L.paml_amd_simulate_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.paml_amd_simulate_info.restype = None
    L.paml_amd_simulate_info(C.byref(nb), C.byref(ms))
    return dict(last_batches=nb.value, last_kernel_ms=ms.value)


def ancestral_info():
    """Batches walked by this thread's last Engine.ancestral_marginal / ancestral_joint and the time of its kernels by HIP events
    (paml_amd_ancestral_info): dict(last_batches, last_kernel_ms)."""
    L = lib()
    nb, ms = C.c_int(), C.c_double()
    L.paml_amd_ancestral_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.paml_amd_ancestral_info.restype = None
    L.paml_amd_ancestral_info(C.byref(nb), C.byref(ms))
    return dict(last_batches=nb.value, last_kernel_ms=ms.value)


def gradient_info():
    """Batches walked by this thread's last Engine.gradient and the time of its kernels by HIP events (paml_amd_gradient_info):
    dict(last_batches, last_kernel_ms)."""
    L = lib()
    nb, ms = C.c_int(), C.c_double()
    L.paml_amd_gradient_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.paml_amd_gradient_info.restype = None
    L.paml_amd_gradient_info(C.byref(nb), C.byref(ms))
    return dict(last_batches=nb.value, last_kernel_ms=ms.value)


def curvature_info():
    """Batches walked by this thread's last Engine.curvature and the time of its kernels by HIP events (paml_amd_curvature_info):
    dict(last_batches, last_kernel_ms)."""
    L = lib()
    nb, ms = C.c_int(), C.c_double()
    L.paml_amd_curvature_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.paml_amd_curvature_info.restype = None
    L.paml_amd_curvature_info(C.byref(nb), C.byref(ms))
    return dict(last_batches=nb.value, last_kernel_ms=ms.value)


def hessian_info():
    """Batches walked by this thread's last Engine.hessian and the time of its kernels by HIP events (paml_amd_hessian_info):
    dict(last_batches, last_kernel_ms)."""
    L = lib()
    nb, ms = C.c_int(), C.c_double()
    L.paml_amd_hessian_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.paml_amd_hessian_info.restype = None
    L.paml_amd_hessian_info(C.byref(nb), C.byref(ms))
    return dict(last_batches=nb.value, last_kernel_ms=ms.value)


def subst_counts_info():
    """Batches walked by this thread's last Engine.subst_counts and the time of its kernels by HIP events (paml_amd_subst_counts_info):
    dict(last_batches, last_kernel_ms)."""
    L = lib()
    nb, ms = C.c_int(), C.c_double()
    L.paml_amd_subst_counts_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.paml_amd_subst_counts_info.restype = None
    L.paml_amd_subst_counts_info(C.byref(nb), C.byref(ms))
    return dict(last_batches=nb.value, last_kernel_ms=ms.value)


def counts_bytes_per_pattern(K, n_int, n_nodes, ns, n_lab, n_query):
    """Bytes of batch workspace paml_amd_subst_counts takes per pattern (counts_bytes_per_pattern, csrc/kernels_counts.h); ns: the states
    of a stored partial, 64 on the matrix cores."""
    return 8.0 * (2.0 * K * n_int * (ns + 1) + K * n_nodes * ns + 2.0 * K * n_nodes + K * (ns + 2) + (2.0 + K) + n_lab * n_query)


def model_gradient_info():
    """Batches walked by this thread's last Engine.model_gradient and the time of its kernels by HIP events
    (paml_amd_model_gradient_info): dict(last_batches, last_kernel_ms, segment = the patterns of one summation segment of W)."""
    L = lib()
    nb, ms = C.c_int(), C.c_double()
    L.paml_amd_model_gradient_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.paml_amd_model_gradient_info.restype = None
    L.paml_amd_model_gradient_info(C.byref(nb), C.byref(ms))
    return dict(last_batches=nb.value, last_kernel_ms=ms.value, segment=int(L.paml_amd_model_gradient_segment()))


def nni_info():
    """Batches walked by this thread's last Engine.nni_scores and the time of its kernels by HIP events (paml_amd_nni_info):
    dict(last_batches, last_kernel_ms)."""
    L = lib()
    nb, ms = C.c_int(), C.c_double()
    L.paml_amd_nni_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.paml_amd_nni_info.restype = None
    L.paml_amd_nni_info(C.byref(nb), C.byref(ms))
    return dict(last_batches=nb.value, last_kernel_ms=ms.value)


def edge_info():
    """Batches walked by this thread's last Engine.edge_scores and the time of its kernels by HIP events (paml_amd_edge_info):
    dict(last_batches, last_kernel_ms)."""
    L = lib()
    nb, ms = C.c_int(), C.c_double()
    L.paml_amd_edge_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.paml_amd_edge_info.restype = None
    L.paml_amd_edge_info(C.byref(nb), C.byref(ms))
    return dict(last_batches=nb.value, last_kernel_ms=ms.value)


def relabel_info():
    """Batches walked by this thread's last Engine.relabel_scores and the time of its kernels by HIP events (paml_amd_relabel_info):
    dict(last_batches, last_kernel_ms)."""
    L = lib()
    nb, ms = C.c_int(), C.c_double()
    L.paml_amd_relabel_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.paml_amd_relabel_info.restype = None
    L.paml_amd_relabel_info(C.byref(nb), C.byref(ms))
    return dict(last_batches=nb.value, last_kernel_ms=ms.value)


def edge_list(tree):
    """The edges of `tree` (a problem.Tree) that have three configurations (paml_amd_edge_list, host only): (edges int32 [n_edges][3][3] =
    per edge the present configuration (v, -1, -1) and its two swaps (v, s, x); five int32 [n_edges][5] = the branches around it)."""
    L = lib()
    ptr = np.zeros(tree.n_nodes + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(s) for s in tree.sons])
    flat = np.ascontiguousarray([c for s in tree.sons for c in s], dtype=np.int32)
    L.paml_amd_edge_list.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    n = L.paml_amd_edge_list(int(tree.n_tips), int(tree.n_nodes), int(tree.root), _p(ptr), _p(flat), None, None, 0)
    if n < 0:
        raise EngineError("paml_amd_edge_list failed (%d): not a tree" % n)
    edges, five = np.zeros((n, 3, 3), dtype=np.int32), np.zeros((n, 5), dtype=np.int32)
    if n and L.paml_amd_edge_list(int(tree.n_tips), int(tree.n_nodes), int(tree.root), _p(ptr), _p(flat), _p(edges), _p(five), n) != n:
        raise EngineError("paml_amd_edge_list: the list changed its length")
    return edges, five


def placement_info():
    """Batches walked by this thread's last Engine.placement_scores and the time of its kernels by HIP events
    (paml_amd_placement_info): dict(last_batches, last_kernel_ms)."""
    L = lib()
    nb, ms = C.c_int(), C.c_double()
    L.paml_amd_placement_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.paml_amd_placement_info.restype = None
    L.paml_amd_placement_info(C.byref(nb), C.byref(ms))
    return dict(last_batches=nb.value, last_kernel_ms=ms.value)


def attach_info():
    """Batches walked by this thread's last Engine.attach_scores and the time of its kernels by HIP events
    (paml_amd_attach_info): dict(last_batches, last_kernel_ms)."""
    L = lib()
    nb, ms = C.c_int(), C.c_double()
    L.paml_amd_attach_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.paml_amd_attach_info.restype = None
    L.paml_amd_attach_info(C.byref(nb), C.byref(ms))
    return dict(last_batches=nb.value, last_kernel_ms=ms.value)


def spr_info():
    """Batches walked by this thread's last Engine.spr_scores and the time of its kernels by HIP events (paml_amd_spr_info):
    dict(last_batches, last_kernel_ms)."""
    L = lib()
    nb, ms = C.c_int(), C.c_double()
    L.paml_amd_spr_info.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.paml_amd_spr_info.restype = None
    L.paml_amd_spr_info(C.byref(nb), C.byref(ms))
    return dict(last_batches=nb.value, last_kernel_ms=ms.value)


def spr_list(n_tips, n_nodes, root, sons_ptr, sons, radius=0):
    """The canonical list of SPR moves of a tree in CSR form (paml_amd_spr_list, host only): int32 [n_moves][2] = s, x, the target
    branches within `radius` branches of the merged one (radius <= 0: no limit)."""
    L = lib()
    ptr, flat = np.ascontiguousarray(sons_ptr, dtype=np.int32), np.ascontiguousarray(sons, dtype=np.int32)
    L.paml_amd_spr_list.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    n = L.paml_amd_spr_list(int(n_tips), int(n_nodes), int(root), _p(ptr), _p(flat), int(radius), None, 0)
    if n < 0:
        raise EngineError("paml_amd_spr_list failed (%d): not a tree" % n)
    mv = np.zeros((n, 2), dtype=np.int32)
    if n and L.paml_amd_spr_list(int(n_tips), int(n_nodes), int(root), _p(ptr), _p(flat), int(radius), _p(mv), n) != n:
        raise EngineError("paml_amd_spr_list: the list changed its length")
    return mv


def nni_list(n_tips, n_nodes, root, sons_ptr, sons):
    """The canonical list of NNI swaps of a tree in CSR form (paml_amd_nni_list, host only): int32 [n_swaps][3] = v, s, x."""
    L = lib()
    ptr, flat = np.ascontiguousarray(sons_ptr, dtype=np.int32), np.ascontiguousarray(sons, dtype=np.int32)
    L.paml_amd_nni_list.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    n = L.paml_amd_nni_list(int(n_tips), int(n_nodes), int(root), _p(ptr), _p(flat), None, 0)
    if n < 0:
        raise EngineError("paml_amd_nni_list failed (%d): not a tree" % n)
    sw = np.zeros((n, 3), dtype=np.int32)
    if n and L.paml_amd_nni_list(int(n_tips), int(n_nodes), int(root), _p(ptr), _p(flat), _p(sw), n) != n:
        raise EngineError("paml_amd_nni_list: the list changed its length")
    return sw


def rell_replicates(lnf, w, gene_off=None, n_rep=10000, seed=1, arena_mb=None):
    """Bootstrap replicates of the tree comparison on the device (paml_amd_rell_replicates): lnf [n_trees][n_patt], w pattern counts,
    gene_off n_genes + 1 pattern offsets -> rep[n_rep][n_trees].  arena_mb: size of the chunk-sum workspace for this call (the
    library's PAML_AMD_RELL_ARENA_MB): a small one walks n_rep in several batches — same bits."""
    lnf = np.ascontiguousarray(np.atleast_2d(lnf), dtype=np.float64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    assert lnf.ndim == 2 and w.ndim == 1
    n_trees, n_patt = lnf.shape
    if w.shape[0] != n_patt:
        raise ValueError("rell_replicates: %d weights for %d patterns" % (w.shape[0], n_patt))
    go = None if gene_off is None else np.ascontiguousarray(gene_off, dtype=np.int32)
    rep = np.zeros((max(int(n_rep), 0), n_trees))
    L = lib()
    L.paml_amd_rell_replicates.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_ulonglong, C.c_void_p]
    old = os.environ.get("PAML_AMD_RELL_ARENA_MB")
    if arena_mb is not None:
        os.environ["PAML_AMD_RELL_ARENA_MB"] = repr(float(arena_mb))
    try:
        rc = L.paml_amd_rell_replicates(n_trees, n_patt, _p(w), _p(lnf), 1 if go is None else len(go) - 1, _p(go), int(n_rep), int(seed) & (2**64 - 1), _p(rep))
    finally:
        if arena_mb is not None:
            if old is None:
                del os.environ["PAML_AMD_RELL_ARENA_MB"]
            else:
                os.environ["PAML_AMD_RELL_ARENA_MB"] = old
    if rc != 0:
        raise EngineError("%s (code %d)" % (L.paml_amd_last_error(None).decode(), rc))
    return rep


def engine_for(pb: Problem, flags=0) -> Engine:
    return Engine(pb.n, pb.tree.n_tips, pb.n_patt, max_classes=pb.K, n_genes=pb.n_genes, flags=flags).load(pb)
