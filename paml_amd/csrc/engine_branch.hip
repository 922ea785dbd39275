// engine_branch.hip — the tree seen from another node: branch-local lnL(t), dlnL/dt, d2lnL/dt2 on resident partials
// (paml_amd_eval_branch: lfuntdd / minbranches, treesub.c:7826-8541) and the marginal posteriors at a node (paml_amd_node_posterior).
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_branch.h"

namespace paml_amd {
namespace {

// the contraction kernel's instantiations: [how A is obtained][B is a tip]
typedef void (*beig_fn)(BranchEigArgs);
#define BEIG_ROW(NS, S0, S1) {{branch_eig_kernel<NS, S0, S1, false, false>, branch_eig_kernel<NS, S0, S1, false, true>}, \
                              {branch_eig_kernel<NS, S0, S1, true, false>, branch_eig_kernel<NS, S0, S1, true, true>}}
beig_fn const beig_kernels[6][2][2] = {      // [how A is obtained][B is a tip][61 states]
   BEIG_ROW(0, false, false),      // A resident
   BEIG_ROW(1, true, false),       // one son, internal
   BEIG_ROW(1, false, false),      // one son, a tip
   BEIG_ROW(2, true, true),        // two internal sons
   BEIG_ROW(2, true, false),       // an internal son and a tip
   BEIG_ROW(2, false, false),      // two tips
};
#undef BEIG_ROW

// Run `prog` (its ops in d_ops_tmp) with the full-featured kernels (gather / valu) over all patterns and classes, reading the P(t)
// buffers of the last pmat launch.  `resident`: STOREs / LOADs address the branch cache's partials; OP_EXPORT writes to export_buf.
int run_prune_full(paml_amd_engine *e, const Program &prog, bool resident, double *export_buf, double *export_scale)
{
   const int n_blocks = e->n_tiles_full * e->K;
   int overflow = 0;
   if (int rc = check_stack_depth(e, prog)) return rc;
   if (int rc = stack_overflow(e, prog, n_blocks, GATHER_WAVES, &overflow)) return rc;
   PruneArgs pr = prune_args(e, prog, e->K, e->d_ops_tmp.p, true, resident ? e->tree.n_scale : 0, resident, resident ? e->d_bl_partials.p : nullptr,
                             resident ? e->d_bl_scalef.p : nullptr, overflow);
   pr.export_buf = export_buf; pr.export_scale = export_scale;
   launch_prune_full(e, prog.max_stack, n_blocks, pr, e->stream);
   HIPCHK(hipGetLastError());
   return 0;
}

// P(t) of every edge of the tree as re-oriented in d_label_eff / d_branch and rooted at `root`, in one batched launch
int reoriented_pmat(paml_amd_engine *e, int root, bool pcol)
{
   const int psets = e->n_genes * e->K;
   if (int rc = ensure_pmat_buffers(e, psets, false, pcol)) return rc;
   const PmatArgs pa = pmat_args(e, root, e->d_label_eff.p, e->kk == KK_MFMA64 ? 1 : 0, pcol ? e->d_pcol.p : nullptr);
   InlineVec iv;
   iv.n_branch = iv.n_rate = 0;
   launch_pmat(pa, iv, e->tree.n_nodes, psets, false, e->stream, pmat_on_matrix_cores(e, pa));
   e->prog_valid = false;      // d_branch / P buffers now hold the re-oriented edge data: the next eval rebuilds
   e->pmat_valid = false;
   return 0;
}

// the table of eigen systems, sent again when a set_eigen_* call has changed one
int send_eigen_table_if_dirty(paml_amd_engine *e, hipStream_t st)
{
   if (!e->eigen_dirty) return 0;
   std::vector<EigenDev> tab;
   if (int rc = eigen_table(e, tab)) return rc;
   HIPCHK(upload(e->d_eigen, tab.data(), tab.size(), st));
   e->eigen_dirty = false;
   return 0;
}

// Node posteriors look at the tree from another node: build the tree rooted at `new_root`
// (along the path new_root -> old root every node loses the son it came from and gains its father; the edge data —
// length, label — of node p moves to its father, now a son of p; cut_son >= 0: that son of new_root and its subtree are
// left out), send the re-oriented branch lengths / labels, and compute P(t) for every edge with one batched launch.
// What ReRootTree (treespace.c:236) + updateconP (treesub.c:7982) do on the host in the reference.
int rerooted_pmat(paml_amd_engine *e, int new_root, int cut_son, const double *branch, const double *gene_rate, TreeDesc *out)
{
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, K = e->K, G = e->n_genes, psets = G * K;
   std::vector<int> father(nn, -1);
   for (int i = 0; i < nn; i++)
      for (int j = T.sons_ptr[i]; j < T.sons_ptr[i + 1]; j++) father[T.sons[j]] = i;
   std::vector<std::vector<int>> sons(nn);
   for (int i = 0; i < nn; i++) sons[i].assign(T.sons.begin() + T.sons_ptr[i], T.sons.begin() + T.sons_ptr[i + 1]);
   std::vector<double> br(branch, branch + nn);
   std::vector<int> lab(T.label);
   for (int p = new_root, prev = cut_son; p >= 0; prev = p, p = father[p]) {
      auto &s = sons[p];
      if (prev >= 0) s.erase(std::find(s.begin(), s.end(), prev));
      if (father[p] >= 0) {
         s.push_back(father[p]);
         br[father[p]] = branch[p];
         lab[father[p]] = T.label[p];
      }
   }
   TreeDesc t;
   t.n_tips = T.n_tips; t.n_nodes = nn; t.root = new_root;
   t.sons_ptr.assign(nn + 1, 0);
   for (int i = 0; i < nn; i++) t.sons_ptr[i + 1] = t.sons_ptr[i] + (int)sons[i].size();
   for (int i = 0; i < nn; i++) t.sons.insert(t.sons.end(), sons[i].begin(), sons[i].end());
   t.label = lab;
   // the nodes SetNodeScale marked keep rescaling their partial, whichever subtree it now stands for; the factors
   // travel with the exported partials
   t.scale_node.assign(nn, 0);
   t.scale_slot.assign(nn, -1);
   if (T.n_scale > 0)
      for (int i = 0; i < nn; i++)
         if (T.scale_node[i] && !t.is_leaf(i)) { t.scale_node[i] = 1; t.scale_slot[i] = t.n_scale++; }
   *out = t;

   std::vector<double> gr(G, 1.0);
   if (gene_rate) gr.assign(gene_rate, gene_rate + G);
   HIPCHK(upload(e->d_branch, br.data(), br.size(), e->stream));
   HIPCHK(upload(e->d_gene_rate, gr.data(), gr.size(), e->stream));
   e->bl_gr_sent = false;
   HIPCHK(upload(e->d_label_eff, lab.data(), lab.size(), e->stream));
   if (int rc = send_eigen_table_if_dirty(e, e->stream)) return rc;
   HIPCHK(hipStreamSynchronize(e->stream));
   HIPCHK(e->d_fhK.ensure((size_t)K * e->n_patt));
   if (int rc = reoriented_pmat(e, new_root, false)) return rc;
   e->n_pmat += (long)psets * (nn - 1);
   e->partials_valid = false;
   return 0;
}

// ---- one branch-local evaluation, phase by phase (paml_amd_eval_branch, below, is the list) -------------------------------------------

// The arguments of paml_amd_eval_branch and the locals its phases share; lives on its stack.
struct BranchEval {
   int node_b, n_t;
   const double *t, *branch, *gene_rate;
   double *lnL, *dlnL, *ddlnL;
   int nn, n, K, G, psets, n_int;
   bool mfma, scaled;
   hipStream_t st;
   std::vector<double> gr;
   Adjacency adj;
   BranchPlan p;      // (branch_plan.h)
};

// The cache's bookkeeping (which partials, coefficients and operand tables are current) is updated where the kernels that fill them are
// queued; should anything after that fail — a launch, the exchange step, the final synchronisation — the call returns its error and the
// whole cache is dropped, so that the next call cannot take a "hit" on buffers that were never written.
struct DropCacheOnError {
   BranchCache &c;
   bool ok = false;
   ~DropCacheOnError() { if (!ok) c.valid = false; }
};

// the call is valid; the two ends of its branch
int check_args(paml_amd_engine *e, BranchEval &c)
{
   if (!e || !c.t || !c.branch || !c.lnL || !c.dlnL || !c.ddlnL || c.n_t < 1 || c.n_t > 64)
      return fail(e, PAML_AMD_EINVAL, "eval_branch: bad arguments");
   if (!(e->have_tips && e->have_tree && e->have_pi && e->have_classes) || e->eigen.empty())
      return fail(e, PAML_AMD_EINVAL, "eval_branch before set_tips/set_tree/set_pi/set_classes/set_eigen");
   const TreeDesc &T = e->tree;
   c.nn = T.n_nodes; c.n = e->n; c.K = e->K; c.G = e->n_genes; c.psets = c.G * c.K; c.n_int = c.nn - e->n_tips;
   c.mfma = e->kk == KK_MFMA64; c.scaled = T.n_scale > 0; c.st = e->stream;
   if (c.node_b < 0 || c.node_b >= c.nn || c.node_b == T.root) return fail(e, PAML_AMD_EINVAL, "eval_branch: node has no branch");
   for (size_t i = 0; i < e->eigen.size(); i++)
      if (e->eigen[i].kind == PAML_AMD_EIGEN_QMAT) return fail(e, PAML_AMD_EUNSUPPORTED, "eval_branch: not for rate-matrix (UNREST) sets");
   c.adj = adjacency(T);
   if (!branch_ends(T, c.adj, c.node_b, c.p)) return fail(e, PAML_AMD_EUNSUPPORTED, "eval_branch: a branch between two tips");
   return 0;
}

// the resident partials and their scale factors: a buffer that had to grow holds nothing
int size_partials(paml_amd_engine *e, const BranchEval &c)
{
   const size_t words = c.mfma ? (size_t)c.K * c.n_int * e->n_tiles_full * GATHER_WAVES * 1024 + 8 * 1024      // (+ PruneArgs::part_dump)
                               : (size_t)c.K * c.n_int * e->n_patt * c.n;
   if (words > e->d_bl_partials.cap) { HIPCHK(e->d_bl_partials.ensure(words)); e->bl.valid = false; }
   const size_t sf = (size_t)c.K * e->tree.n_scale * e->n_patt;
   if (c.scaled && sf > e->d_bl_scalef.cap) { HIPCHK(e->d_bl_scalef.ensure(sf)); e->bl.valid = false; }
   return 0;
}

// what of the cache serves this call, and the tree the rest is formed on (branch_plan.h: host only)
void plan_call(paml_amd_engine *e, BranchEval &c)
{
   c.gr.assign(c.G, 1.0);
   if (c.gene_rate) c.gr.assign(c.gene_rate, c.gene_rate + c.G);
   if (reset_if_stale(e->bl, c.nn, c.K, c.gr)) e->bl_gr_sent = false;
   invalidate(e->bl, e->tree, c.adj, c.branch);
   orient(e->bl, e->tree, c.adj, c.p);
   tree_seen_from(e->tree, c.adj, c.branch, c.p);
}

// the eigen systems and the gene rates, where the device does not hold them yet
int send_model(paml_amd_engine *e, const BranchEval &c)
{
   if (int rc = eigen_refs_ok(e, e->h_eigen_of.data(), e->h_eigen_of.size(), "eval_branch")) return rc;
   if (int rc = send_eigen_table_if_dirty(e, c.st)) return rc;
   // (d_gene_rate is shared with the ordinary evaluation, which rewrites it: sent again unless the last writer was this function with the same rates)
   if (!e->bl_gr_sent) { HIPCHK(upload(e->d_gene_rate, c.gr.data(), c.gr.size(), c.st)); }
   e->bl_gr_sent = true;
   return 0;
}

// P(t) of every edge in its orientation towards the branch (the lengths and labels are on their way)
int plan_pmat(paml_amd_engine *e, const BranchEval &c, bool pcol)
{
   if (int rc = reoriented_pmat(e, c.p.A, pcol)) return rc;
   e->n_pmat += (long)c.psets * (c.nn - 2);
   return 0;
}

// The dirty partials are queued: the cache's bookkeeping follows (DropCacheOnError takes it back if the call fails later)
void commit_plan(paml_amd_engine *e, const BranchEval &c) { e->n_branch_nodes += commit(e->bl, c.p, e->n_tips); }

// The exchange step of the branch-local evaluation, on the communicator's own stream like every collective
int exchange_partials(paml_amd_engine *e, hipStream_t st, size_t count)
{
   if (!e->comm) return 0;
   HIPCHK(hipEventRecord(e->ev_part[0], st));
   HIPCHK(hipStreamWaitEvent(e->sc, e->ev_part[0], 0));
   const ncclResult_t nr = rccl().AllReduce(e->d_bpartial.p, e->d_bpartial.p, count, ncclDouble, ncclSum, e->comm, e->sc);
   if (nr != ncclSuccess) return fail(e, PAML_AMD_EHIP, std::string("ncclAllReduce: ") + rccl().GetErrorString(nr));
   HIPCHK(hipEventRecord(e->ev_done[0], e->sc));
   HIPCHK(hipStreamWaitEvent(st, e->ev_done[0], 0));
   return 0;
}

// the 3 n_t results are on their way to h_out: wait for them and hand them out
int read_back(paml_amd_engine *e, const BranchEval &c)
{
   HIPCHK(hipStreamSynchronize(c.st));      // the one host synchronisation of the call
   if (int rc = eigen_fail_check(e)) return rc;
   for (int i = 0; i < c.n_t; i++) { c.lnL[i] = e->h_out[3 * i]; c.dlnL[i] = e->h_out[3 * i + 1]; c.ddlnL[i] = e->h_out[3 * i + 2]; }
   e->n_branch_eval++;
   return 0;
}

// ---- the eigen-basis form (kernels_branch.h): matrix-core engines with one gene and (U, V, Root) eigen systems -------------------------
bool eigen_form_applies(const paml_amd_engine *e, const BranchEval &c)
{
   bool eig = c.mfma && c.G == 1 && e->n_pi == 1 && !e->env.no_branch_eig && (size_t)(c.K * BEIG_NT * 192 + 8 * 3 * BEIG_NT) * 8 <= 150 * 1024;
   for (const EigenHost &h : e->eigen) eig = eig && (h.kind == PAML_AMD_EIGEN_UVROOT || h.kind < 0);
   return eig;
}

struct EigForm {
   int n_groups, n_out, cg, nb_local, nrows, lab_b;      // nrows: a row per wave and chunk (kernels_branch.h): the sums of an eighth of a reduction chunk
   bool hit;                                              // the coefficients of this branch are current: no contraction
   double *efrag, *ztab;
   int n_sons = 0, son[2] = {-1, -1};                     // A formed inside the contraction kernel from these
   Program prog;                                          // the other dirty subtrees
   bool run_pmat = false, run_prog = false;
};

int eig_buffers(paml_amd_engine *e, const BranchEval &c, EigForm &f)
{
   BranchCache &bc = e->bl;
   const int K = c.K, n_t = c.n_t, NL = e->n_labels;
   if (!e->beig_attr_set) {
      for (auto &row : beig_kernels)
         for (auto &r2 : row)
            for (auto fn : r2) HIPCHK(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      HIPCHK(hipFuncSetAttribute((const void *)branch_poly_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      e->beig_attr_set = true;
   }
   HIPCHK(e->d_bl_coef.ensure((size_t)K * f.n_groups * 1024));
   if ((size_t)NL * K * 2 * 4096 > e->d_bl_efrag.cap || (size_t)NL * K * e->n_codes * 64 > e->d_bl_ztab.cap || (size_t)NL * K * 128 > e->d_bl_ecol.cap ||
       (int)bc.frag_ok.size() != NL) {
      HIPCHK(e->d_bl_ecol.ensure((size_t)NL * K * 128));
      HIPCHK(e->d_bl_efrag.ensure((size_t)NL * K * 2 * 4096));
      HIPCHK(e->d_bl_ztab.ensure((size_t)NL * K * e->n_codes * 64));
      bc.frag_ok.assign(NL, 0);
   }
   if (f.lab_b < 0 || f.lab_b >= NL) return fail(e, PAML_AMD_EINVAL, "eval_branch: branch label out of range");
   f.efrag = e->d_bl_efrag.p + (size_t)f.lab_b * K * 2 * 4096; f.ztab = e->d_bl_ztab.p + (size_t)f.lab_b * K * e->n_codes * 64;
   HIPCHK(e->d_bl_etab.ensure((size_t)K * n_t * 192));
   HIPCHK(e->d_bpartial.ensure((size_t)f.nrows * f.n_out));
   HIPCHK(e->d_bout.ensure((size_t)f.n_out));
   HIPCHK(e->d_tt.ensure(n_t));
   e->bpart_rows = f.nrows; e->bpart_cols = f.n_out; e->bpart_colmajor = true;
   if (e->nb_global != f.nb_local || e->chunk * f.nb_local != e->n_patt)      // (the other ranks' rows; rows past the last pattern)
      HIPCHK(hipMemsetAsync(e->d_bpartial.p, 0, (size_t)f.nrows * f.n_out * sizeof(double), c.st));
   return 0;
}

// A itself is formed inside the contraction kernel when it has one or two sons in the tree seen from the branch (what changes when
// minbranches moves on to a neighbouring branch); everything else that is dirty goes through the interpreter.  Host only.
void eig_forest(const TreeDesc &T, const BranchPlan &p, bool scaled, EigForm &f)
{
   const TreeDesc &tr = p.tr;
   std::vector<int> roots;
   if (!p.clean[p.A]) {
      const int ns = tr.sons_ptr[p.A + 1] - tr.sons_ptr[p.A];
      if (!scaled && (ns == 1 || ns == 2)) {
         for (int j = tr.sons_ptr[p.A]; j < tr.sons_ptr[p.A + 1]; j++) f.son[f.n_sons++] = tr.sons[j];
         if (f.n_sons == 2 && T.is_leaf(f.son[0]) && !T.is_leaf(f.son[1])) std::swap(f.son[0], f.son[1]);      // (an internal son first: its product initialises the partial)
         for (int j = 0; j < f.n_sons; j++)
            if (!T.is_leaf(f.son[j]) && !p.clean[f.son[j]]) roots.push_back(f.son[j]);
      }
      else roots.push_back(p.A);
   }
   if (!p.b_tip && !p.clean[p.Bn]) roots.push_back(p.Bn);
   f.prog = forest_program(tr, roots, p.clean.data(), false);
   f.run_pmat = true;
   f.run_prog = !f.prog.ops.empty();
}

// A refill — every branch length moved since the partials were formed (minB's round after ming2 has moved kappa / omega, the first
// call of a search): the forest of dirty subtrees is most of the tree, and the program is the same every time it happens at this
// branch.  From the second time on it runs on a per-tree kernel of its own (round 6: STOREs in the resident layout, as a
// keep-partials evaluation — 128-pattern tiles, the operand ring — instead of the 64-pattern interpreter), compiled on the worker
// thread while the interpreter serves, or at once when the caller asked for per-tree kernels.  *done: the kernel is queued.
int eig_refill_jit(paml_amd_engine *e, const BranchEval &c, const EigForm &f, bool *done)
{
   const TreeDesc &T = e->tree;
   const int n = c.n, K = c.K;
   *done = false;
   if (!(f.run_prog && e->jit_enabled && e->n_tips <= 207 && (e->n_codes <= 64 || (e->amb_ascending && e->plain_codes >= n)))) return 0;      // (as launch_eval's)
   int n_store = 0;
   for (const Op &o : f.prog.ops) n_store += o.code == OP_STORE;
   Program full = f.prog;
   finish_program(full);
   if (!(2 * n_store >= c.n_int && jit_supported(full, e->n_tips, e->n_codes, e->n_pi, 6, 128, true))) return 0;
   const std::string key = "b" + std::to_string(n) + "c" + std::to_string(e->n_codes) + ":" + jit_program_key(full, e->n_tips);
   bool have = false;
   if (e->jit_forced || e->env.jit_sync || e->jit_recall(key) || e->jit_count_request(key) >= 2)
      if (int rc = obtain_kernel(e, e->bjit_slot, &e->jit, true, key, [&]() { return jit_generate(full, e->n_tips, n, e->n_codes); },
                                 (e->jit_forced || e->env.jit_sync) ? JIT_WAIT_CALLER : JIT_WAIT_WORKER, "refill", &have)) return rc;
   if (!have) return 0;
   e->kernel = PK_MFMA64_JIT;      // (kernel_name: the last pruning kernel was a per-tree one)
   e->last_ctab_n = e->last_ctab_bytes = 0;      // (... without cherry tables)
   e->last_stab_n = e->last_stab_bytes = 0; e->last_stab_blocks = -1;
   if (int rc = select_tiles(e, true, 8, true)) return rc;
   const int n_blocks = e->n_tiles * K;
   int overflow = 0;
   if (int rc = stack_overflow(e, full, n_blocks, 8, &overflow)) return rc;
   if (T.n_scale) HIPCHK(e->d_fscale.ensure((size_t)K * e->n_patt));
   HIPCHK(e->d_fhK.ensure((size_t)K * e->n_patt));
   PruneArgs pr = prune_args(e, full, K, nullptr, false, T.n_scale, true, e->d_bl_partials.p, e->d_bl_scalef.p, overflow);
   void *params[] = {&pr};
   HIPCHK(hipModuleLaunchKernel(e->jit.fn, std::min(n_blocks, e->n_cu), 1, 1, 8 * 64, 1, 1, 0, c.st, params, nullptr));
   *done = true;
   e->n_branch_refill_jit++;
   return 0;
}

// per class V and U^T diag(pi) in operand order and the tips' z rows (kept per branch label), e^{mu t} {1, mu, mu^2} per trial length
void launch_eigprep(paml_amd_engine *e, const BranchEval &c, const EigForm &f)
{
   BranchCache &bc = e->bl;
   const int n = c.n, K = c.K, lab_b = f.lab_b;
   EigPrepArgs ea{};
   ea.n = n; ea.K = K; ea.n_labels = e->n_labels; ea.n_t = c.n_t; ea.label = lab_b; ea.n_codes = e->n_codes;
   ea.rate_gs = e->rate_per_gene ? K : 0; ea.only_etab = (f.hit || bc.frag_ok[lab_b]) ? 1 : 0;      // (the operand-order matrices depend on the eigen systems only)
   bc.frag_ok[lab_b] = 1;
   ea.t = e->d_tt.p; ea.rate = e->d_rate.p; ea.gene_rate = e->d_gene_rate.p; ea.qfactor = e->d_qfactor.p; ea.pi = e->d_pi_plain.p;
   ea.eigen_of = e->d_eigen_of.p; ea.eigen = e->d_eigen.p; ea.code_mask = e->d_code_mask.p;
   ea.efrag = f.efrag; ea.ztab = f.ztab; ea.etab = e->d_bl_etab.p; ea.ecol = n == 61 ? e->d_bl_ecol.p + (size_t)lab_b * K * 128 : nullptr;
   hipLaunchKernelGGL(branch_eigprep_kernel, dim3(K), dim3(256), 0, c.st, ea);
}

// the contraction: A read or formed from its sons, the coefficients of this branch, and (`feval`) the results themselves
void launch_contraction(paml_amd_engine *e, const BranchEval &c, const EigForm &f, bool feval)
{
   const TreeDesc &T = e->tree;
   const int n = c.n, K = c.K;
   BranchEigArgs ba{};
   ba.n = n; ba.K = K; ba.n_patt = e->n_patt; ba.n_tips = e->n_tips; ba.n_int = c.n_int; ba.n_nodes = c.nn; ba.n_groups = f.n_groups;
   ba.n_scale = T.n_scale; ba.n_t = c.n_t; ba.n_codes = e->n_codes; ba.a_node = c.p.A; ba.b_node = c.p.Bn;
   ba.n_sons = f.n_sons; ba.son[0] = f.son[0]; ba.son[1] = f.son[1]; ba.feval = feval ? 1 : 0;
   ba.chunk_groups = f.cg; ba.nb_local = f.nb_local; ba.first_chunk = e->first_chunk; ba.n_out = f.n_out; ba.n_rows = f.nrows;
   ba.partials = e->d_bl_partials.p; ba.scalef = c.scaled ? e->d_bl_scalef.p : nullptr; ba.z = e->d_z.p;
   ba.pint = e->d_pint.p; ba.ptip = e->d_ptip.p; ba.tip_words = (long)tip_words(e);
   ba.efrag = f.efrag; ba.ztab = f.ztab; ba.etab = e->d_bl_etab.p;
   ba.ecol = e->d_bl_ecol.p + (size_t)f.lab_b * K * 128; ba.pcol = e->d_pcol.p;
   ba.freqK = e->d_freqK.p; ba.weights = e->d_weights.p; ba.coef = e->d_bl_coef.p; ba.partial = e->d_bpartial.p;
   const bool i0 = f.n_sons > 0 && !T.is_leaf(f.son[0]), i1 = f.n_sons > 1 && !T.is_leaf(f.son[1]);
   const int variant = f.n_sons == 0 ? 0 : (f.n_sons == 1 ? (i0 ? 1 : 2) : (i1 ? 3 : (i0 ? 4 : 5)));      // (two sons: the internal one, if any, comes first)
   beig_fn const fn = beig_kernels[variant][c.p.b_tip ? 1 : 0][n == 61 ? 1 : 0];
   hipLaunchKernelGGL(fn, dim3(std::min(f.nb_local, e->n_cu), K), dim3(512), BEIG_LDS_BYTES, c.st, ba);
}

// f, f', f'' from the stored coefficients, BEIG_NT trial lengths per launch
void launch_poly(paml_amd_engine *e, const BranchEval &c, const EigForm &f)
{
   const int K = c.K, n_t = c.n_t;
   BranchPolyArgs pa{};
   pa.K = K; pa.n_patt = e->n_patt; pa.n_groups = f.n_groups; pa.n_scale = e->tree.n_scale; pa.n_t = n_t;
   pa.chunk_groups = f.cg; pa.nb_local = f.nb_local; pa.first_chunk = e->first_chunk; pa.n_out = f.n_out; pa.n_rows = f.nrows;
   pa.coef = e->d_bl_coef.p; pa.etab = e->d_bl_etab.p; pa.scalef = c.scaled ? e->d_bl_scalef.p : nullptr; pa.weights = e->d_weights.p;
   pa.partial = e->d_bpartial.p;
   for (int it0 = 0; it0 < n_t; it0 += BEIG_NT) {
      pa.it0 = it0; pa.nt_here = std::min(BEIG_NT, n_t - it0);
      const size_t lds = ((size_t)K * pa.nt_here * 192 + 8 * 3 * BEIG_NT) * 8;
      hipLaunchKernelGGL(branch_poly_kernel, dim3(std::min(f.nb_local, 4 * e->n_cu)), dim3(512), lds, c.st, pa);
   }
}

int eigen_form(paml_amd_engine *e, const BranchEval &c)
{
   BranchCache &bc = e->bl;
   const BranchPlan &p = c.p;
   hipStream_t st = c.st;
   EigForm f;
   f.n_groups = e->n_tiles_full * GATHER_WAVES; f.n_out = 3 * c.n_t;
   f.cg = e->chunk / 16; f.nb_local = (e->n_patt + e->chunk - 1) / e->chunk; f.nrows = e->nb_global * 8;
   f.lab_b = e->tree.label[c.node_b];
   f.hit = bc.coef_ok && bc.coef_node == c.node_b && p.clean[p.A] && (p.b_tip || p.clean[p.Bn]) && !e->env.no_coef_cache;
   if (int rc = eig_buffers(e, c, f)) return rc;
   if (!f.hit && p.any_dirty) eig_forest(e->tree, p, c.scaled, f);
   // the call's small inputs: one pinned arena, asynchronous copies
   HIPCHK(e->stage.begin((size_t)c.n_t * 8 + (f.run_pmat ? (size_t)c.nn * 12 : 0) + (f.run_prog ? f.prog.ops.size() * sizeof(Op) : 0) + 256));
   HIPCHK(e->stage.send(e->d_tt, c.t, (size_t)c.n_t, st));
   if (f.run_pmat) {
      HIPCHK(e->stage.send(e->d_label_eff, p.lab_eff.data(), (size_t)c.nn, st));
      HIPCHK(e->stage.send(e->d_branch, p.br_eff.data(), (size_t)c.nn, st));
   }
   if (f.run_prog) HIPCHK(e->stage.send(e->d_ops_tmp, f.prog.ops.data(), f.prog.ops.size(), st));
   HIPCHK(e->stage.end(st));
   if (f.run_pmat)
      if (int rc = plan_pmat(e, c, true)) return rc;
   bool refill_done = false;
   if (int rc = eig_refill_jit(e, c, f, &refill_done)) return rc;
   if (f.run_prog && !refill_done) {
      HIPCHK(e->d_fhK.ensure((size_t)c.K * e->n_patt));
      if (int rc = run_prune_full(e, f.prog, true, nullptr, nullptr)) return rc;
   }
   launch_eigprep(e, c, f);
   const bool feval = !f.hit && c.K == 1 && c.n_t <= BEIG_NT;
   e->bk_timed = false;
   if (e->profiling) {
      for (DevEvent &ev : e->ev_bk) HIPCHK(ev.ensure());
      HIPCHK(hipEventRecord(e->ev_bk[0], st));
   }
   if (!f.hit) {
      launch_contraction(e, c, f, feval);
      commit_plan(e, c);
      bc.coef_ok = true;
      bc.coef_node = c.node_b;
   }
   else e->n_branch_coef_hits++;
   if (!feval) launch_poly(e, c, f);
   HIPCHK(hipGetLastError());
   if (e->profiling) { HIPCHK(hipEventRecord(e->ev_bk[1], st)); e->bk_timed = true; }
   if (int rc = exchange_partials(e, st, (size_t)f.nrows * f.n_out)) return rc;
   if (int rc = ensure_hout(e, (size_t)f.n_out)) return rc;
   hipLaunchKernelGGL(branch_total_kernel, dim3(f.n_out), dim3(256), 0, st, (const double *)e->d_bpartial.p, f.nrows, f.n_out, e->h_out);      // (pinned, device-visible: no copy)
   HIPCHK(hipGetLastError());
   return 0;
}

// ---- the P / dP / ddP form: every other engine -----------------------------------------------------------------------------------------
// the dirty partials: one program per side, run back to back in one launch of the full-featured kernels
int pdp_refill(paml_amd_engine *e, const BranchEval &c)
{
   const BranchPlan &p = c.p;
   std::vector<int> roots;
   for (int rt : {p.A, p.Bn})
      if (!e->tree.is_leaf(rt) && !p.clean[rt]) roots.push_back(rt);
   const Program prog = forest_program(p.tr, roots, p.clean.data(), true);
   if (int rc = check_stack_depth(e, prog)) return rc;
   HIPCHK(upload(e->d_label_eff, p.lab_eff.data(), p.lab_eff.size(), c.st));
   HIPCHK(upload(e->d_branch, p.br_eff.data(), p.br_eff.size(), c.st));
   if (int rc = plan_pmat(e, c, false)) return rc;
   HIPCHK(upload(e->d_ops_tmp, prog.ops.data(), prog.ops.size(), c.st));
   if (int rc = run_prune_full(e, prog, true, nullptr, nullptr)) return rc;
   commit_plan(e, c);
   return 0;
}

// P, dP, ddP of the branch for every trial length
int launch_deriv(paml_amd_engine *e, const BranchEval &c)
{
   const int n = c.n, n_t = c.n_t;
   HIPCHK(upload(e->d_tt, c.t, (size_t)n_t, c.st));
   HIPCHK(e->d_deriv.ensure((size_t)c.psets * n_t * 3 * n * n));
   if (c.mfma) HIPCHK(e->d_bl_frag.ensure((size_t)c.psets * n_t * 3 * 4096));
   DerivArgs da{};
   da.n = n; da.K = c.K; da.n_genes = c.G; da.n_labels = e->n_labels; da.n_t = n_t; da.label = e->tree.label[c.node_b];
   da.rate_gs = e->rate_per_gene ? c.K : 0;
   da.t = e->d_tt.p; da.rate = e->d_rate.p; da.gene_rate = e->d_gene_rate.p; da.qfactor = e->d_qfactor.p;
   da.eigen_of = e->d_eigen_of.p; da.eigen = e->d_eigen.p; da.out = e->d_deriv.p; da.frag = c.mfma ? e->d_bl_frag.p : nullptr;
   hipLaunchKernelGGL(pmat_deriv_kernel, dim3(n_t, c.psets), dim3(256), 0, c.st, da);
   return 0;
}

int pdp_form(paml_amd_engine *e, const BranchEval &c)
{
   const TreeDesc &T = e->tree;
   const int n = c.n, K = c.K, G = c.G, n_t = c.n_t, A = c.p.A, Bn = c.p.Bn;
   const bool mfma = c.mfma, b_tip = c.p.b_tip;
   hipStream_t st = c.st;
   e->bl.coef_ok = false;      // (this form recomputes partials without the coefficients)
   if (c.p.any_dirty)
      if (int rc = pdp_refill(e, c)) return rc;
   // P, dP, ddP for every trial length, then the per-pattern contraction and the three weighted sums
   if (int rc = launch_deriv(e, c)) return rc;
   HIPCHK(e->d_bout.ensure((size_t)n_t * 3));
   // The 3 n_t sums (lnL, dlnL, ddlnL per trial length) are formed like the evaluation's total: one partial per block of patterns
   // at the block's GLOBAL position, the ranks' (disjoint, zero elsewhere) arrays summed over RCCL, then one fixed-order pass —
   // the same bits whatever the number of ranks.  Blocks: 64 patterns (matrix-core contraction) or 256.
   const int blk = mfma ? 64 : 256, n_out = 3 * n_t;
   const long nb_local = mfma ? e->n_tiles_full : (e->n_patt + 255) / 256;
   const bool sharded = e->comm != nullptr || e->n_patt_global != e->n_patt;      // (also: shard geometry without a communicator, for tests)
   const long nbg = sharded ? (e->n_patt_global + blk - 1) / blk : nb_local, fb = sharded ? e->first_patt / blk : 0;
   HIPCHK(e->d_bpartial.ensure((size_t)nbg * n_out));
   e->bpart_rows = nbg; e->bpart_cols = n_out; e->bpart_colmajor = false;
   if (sharded) HIPCHK(hipMemsetAsync(e->d_bpartial.p, 0, (size_t)nbg * n_out * sizeof(double), st));
   double *const bpart = e->d_bpartial.p + (size_t)fb * n_out;
   if (mfma) {
      BranchMfmaArgs ba{};
      ba.n = n; ba.K = K; ba.n_genes = G; ba.n_patt = e->n_patt; ba.n_pi = e->n_pi; ba.n_tips = e->n_tips; ba.n_int = c.n_int;
      ba.n_tiles = e->n_tiles_full; ba.n_scale = T.n_scale; ba.n_t = n_t; ba.a_node = A; ba.b_node = Bn;
      ba.tiles = e->d_tiles_full.p; ba.gene_off = e->d_gene_off.p; ba.partials = e->d_bl_partials.p;
      ba.scalef = c.scaled ? e->d_bl_scalef.p : nullptr; ba.zb = b_tip ? e->d_z.p + (size_t)Bn * e->n_patt : nullptr;
      ba.code_mask = e->d_code_mask.p; ba.pi = e->d_pi.p; ba.freqK = e->d_freqK.p; ba.weights = e->d_weights.p;
      ba.frag = e->d_bl_frag.p; ba.partial = bpart;
      for (int it = 0; it < n_t; it++) {
         ba.it = it;
         hipLaunchKernelGGL(branch_mfma_kernel, dim3(e->n_tiles_full), dim3(256), 0, st, ba);
      }
   }
   else {
      BranchArgs ba{};
      ba.n = n; ba.K = K; ba.n_genes = G; ba.n_patt = e->n_patt; ba.n_t = n_t; ba.n_pi = e->n_pi; ba.b_is_tip = b_tip ? 1 : 0;
      ba.n_codes = e->n_codes; ba.cls_stride = (long)c.n_int * e->n_patt * n;
      ba.A = e->d_bl_partials.p + (size_t)(A - e->n_tips) * e->n_patt * n;
      ba.B = b_tip ? nullptr : e->d_bl_partials.p + (size_t)(Bn - e->n_tips) * e->n_patt * n;
      ba.SA = c.scaled ? e->d_bl_scalef.p : nullptr; ba.SB = nullptr; ba.n_scale = T.n_scale;
      ba.zb = b_tip ? e->d_z.p + (size_t)Bn * e->n_patt : nullptr;
      ba.n_chara = e->d_n_chara.p; ba.chara_map = e->d_chara_map.p; ba.freqK = e->d_freqK.p;
      ba.weights = e->d_weights.p; ba.PdP = e->d_deriv.p; ba.gene_off = e->d_gene_off.p; ba.partial = bpart;
      ba.pi = e->d_pi_plain.p;
      hipLaunchKernelGGL(branch_kernel, dim3((e->n_patt + 255) / 256), dim3(256), 0, st, ba);
   }
   HIPCHK(hipGetLastError());
   if (int rc = exchange_partials(e, st, (size_t)nbg * n_out)) return rc;
   hipLaunchKernelGGL(branch_reduce_kernel, dim3(1), dim3(256), 0, st, (const double *)e->d_bpartial.p, (int)nbg, n_out, e->d_bout.p);
   HIPCHK(hipGetLastError());
   if (int rc = ensure_hout(e, (size_t)n_t * 3)) return rc;
   HIPCHK(hipMemcpyAsync(e->h_out, e->d_bout.p, (size_t)n_t * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
   return 0;
}

}  // namespace
}  // namespace paml_amd

extern "C" {

int paml_amd_eval_branch(paml_amd_engine *e, int node_b, int n_t, const double *t, const double *branch,
                         const double *gene_rate, double *lnL, double *dlnL, double *ddlnL)
{
   enter(e);
   BranchEval c{node_b, n_t, t, branch, gene_rate, lnL, dlnL, ddlnL};
   if (int rc = check_args(e, c)) return rc;                  // the call is valid; the two ends of the branch
   DropCacheOnError cache_guard{e->bl};                       // from here on an error drops the whole cache
   if (int rc = size_partials(e, c)) return rc;               // (a buffer that grew: the cache starts over)
   plan_call(e, c);                                           // branch_plan.h: what is current, the tree seen from the branch
   if (int rc = send_model(e, c)) return rc;                  // eigen table, gene rates
   if (int rc = eigen_form_applies(e, c) ? eigen_form(e, c) : pdp_form(e, c)) return rc;      // Kernel D, the exchange step, the totals
   if (int rc = read_back(e, c)) return rc;
   cache_guard.ok = true;
   return 0;
}

int paml_amd_branch_counters(const paml_amd_engine *e, long *n_calls, long *n_nodes_recomputed)
{
   if (!e) return PAML_AMD_EINVAL;
   if (n_calls) *n_calls = e->n_branch_eval;
   if (n_nodes_recomputed) *n_nodes_recomputed = e->n_branch_nodes;
   return 0;
}

long paml_amd_branch_coef_hits(const paml_amd_engine *e) { return e ? e->n_branch_coef_hits : -1; }

long paml_amd_branch_refill_kernels(const paml_amd_engine *e) { return e ? e->n_branch_refill_jit : -1; }

double paml_amd_branch_kernel_ms(paml_amd_engine *e)
{
   float ms = -1;
   if (!e || !e->bk_timed || hipEventElapsedTime(&ms, e->ev_bk[0], e->ev_bk[1]) != hipSuccess) { (void)hipGetLastError(); return -1; }
   return ms;
}

int paml_amd_get_branch_partials(paml_amd_engine *e, double *out, long cap, long *rows, int *cols)
{
   if (!e || !rows || !cols) return PAML_AMD_EINVAL;
   *rows = e->bpart_rows; *cols = e->bpart_cols;
   if (!out) return 0;
   if (cap < e->bpart_rows * e->bpart_cols || !e->d_bpartial.p) return fail(e, PAML_AMD_EINVAL, "get_branch_partials: no branch evaluation yet, or the buffer is too small");
   if (!e->bpart_colmajor) { HIPCHK(hipMemcpy(out, e->d_bpartial.p, (size_t)e->bpart_rows * e->bpart_cols * sizeof(double), hipMemcpyDeviceToHost)); }
   else {
      std::vector<double> t((size_t)e->bpart_rows * e->bpart_cols);
      HIPCHK(hipMemcpy(t.data(), e->d_bpartial.p, t.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (long r = 0; r < e->bpart_rows; r++)
         for (int c = 0; c < e->bpart_cols; c++) out[r * e->bpart_cols + c] = t[(size_t)c * e->bpart_rows + r];
   }
   return 0;
}

int paml_amd_node_posterior(paml_amd_engine *e, int node, const double *branch, const double *gene_rate, double *post)
{
   enter(e);
   if (!e || !branch || !post) return fail(e, PAML_AMD_EINVAL, "node_posterior: null argument");
   if (!(e->have_tips && e->have_tree && e->have_pi && e->have_classes) || e->eigen.empty())
      return fail(e, PAML_AMD_EINVAL, "node_posterior before set_tips/set_tree/set_pi/set_classes/set_eigen");
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K;
   if (node < 0 || node >= nn || T.is_leaf(node)) return fail(e, PAML_AMD_EINVAL, "node_posterior: not an internal node");
   for (size_t i = 0; i < e->eigen.size(); i++)
      if (e->eigen[i].kind == PAML_AMD_EIGEN_QMAT)
         return fail(e, PAML_AMD_EUNSUPPORTED, "node_posterior: moving the root needs a reversible model");
   TreeDesc tr;
   int r = rerooted_pmat(e, node, -1, branch, gene_rate, &tr);
   if (r) return r;
   Program prog = build_program(tr, false, nullptr);
   for (Op &o : prog.ops)
      if (o.code == OP_ROOT) o.code = OP_EXPORT;
   const bool scaled = T.n_scale > 0;
   HIPCHK(e->d_expA.ensure((size_t)K * e->n_patt * n));
   if (scaled) HIPCHK(e->d_expSA.ensure((size_t)K * e->n_patt));
   HIPCHK(upload(e->d_ops_tmp, prog.ops.data(), prog.ops.size(), e->stream));
   HIPCHK(hipStreamSynchronize(e->stream));
   r = run_prune_full(e, prog, false, e->d_expA.p, scaled ? e->d_expSA.p : nullptr);
   if (r) return r;
   HIPCHK(e->d_expB.ensure((size_t)e->n_patt * n));
   PostArgs pa{};
   pa.n = n; pa.K = K; pa.n_genes = e->n_genes; pa.n_patt = e->n_patt; pa.n_pi = e->n_pi;
   pa.L = e->d_expA.p; pa.S = scaled ? e->d_expSA.p : nullptr; pa.pi = e->d_pi_plain.p; pa.freqK = e->d_freqK.p;
   pa.gene_off = e->d_gene_off.p; pa.post = e->d_expB.p;
   hipLaunchKernelGGL(posterior_kernel, dim3((e->n_patt + 255) / 256), dim3(256), 0, e->stream, pa);
   HIPCHK(hipGetLastError());
   HIPCHK(hipMemcpyAsync(post, e->d_expB.p, (size_t)e->n_patt * n * sizeof(double), hipMemcpyDeviceToHost, e->stream));
   HIPCHK(hipStreamSynchronize(e->stream));
   return eigen_fail_check(e);
}

}  // extern "C"
