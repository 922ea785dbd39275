// engine_ancestral.hip — ancestral reconstruction at every internal node in one call: marginal (AncestralMarginal / PostProbNode,
// treesub.c:6288, 6142) and joint (AncestralJointPPSG2000 treesub.c:6964); the definitions and the kernels in kernels_ancestral.h.
// P(t) comes from the evaluation's own builders (launch_pmat, engine_eval.hip).
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_ancestral.h"
#include "ancestral_host.h"

static thread_local int anc_last_batches = 0;
static thread_local double anc_last_kernel_ms = 0;      // HIP events around the P(t) kernels and every batch's passes, summed

extern "C" void paml_amd_ancestral_info(int *last_batches, double *last_kernel_ms)
{
   if (last_batches) *last_batches = anc_last_batches;
   if (last_kernel_ms) *last_kernel_ms = anc_last_kernel_ms;
}

namespace paml_amd {

// the tree as one int array: sons_ptr, sons, father, post, pre, scale (AncTree)
int anc_tree_pack(paml_amd_engine *e, const char *who, AncScratch &w, AncTree *out)
{
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n_tips = T.n_tips;
   for (int v = 0; v < nn; v++)
      if ((v < n_tips) != T.is_leaf(v) && v != T.root)
         return fail(e, PAML_AMD_EUNSUPPORTED, std::string(who) + ": the tips are expected to be the nodes 0 .. n_tips - 1");
   std::vector<int> father(nn, -1), pre, post, all_pre;
   std::vector<int> stack(1, T.root);
   while (!stack.empty()) {
      const int v = stack.back();
      stack.pop_back();
      all_pre.push_back(v);
      for (int j = T.sons_ptr[v + 1] - 1; j >= T.sons_ptr[v]; j--) {      // (pushed last to first: visited first to last)
         father[T.sons[j]] = v;
         stack.push_back(T.sons[j]);
      }
   }
   if ((int)all_pre.size() != nn) return fail(e, PAML_AMD_EINVAL, std::string(who) + ": the tree does not reach every node from its root");
   for (int v : all_pre)
      if (v >= n_tips && v != T.root) pre.push_back(v);
   // (the reverse of a pre-order is a post-order: every node after all of its subtree)
   post.assign(pre.rbegin(), pre.rend());
   post.push_back(T.root);
   std::vector<int> pack;
   const size_t o_sons = nn + 1, o_father = o_sons + T.sons.size(), o_post = o_father + nn, o_pre = o_post + post.size(), o_scale = o_pre + pre.size();
   pack.insert(pack.end(), T.sons_ptr.begin(), T.sons_ptr.begin() + nn + 1);
   pack.insert(pack.end(), T.sons.begin(), T.sons.end());
   pack.insert(pack.end(), father.begin(), father.end());
   pack.insert(pack.end(), post.begin(), post.end());
   pack.insert(pack.end(), pre.begin(), pre.end());
   for (int v = 0; v < nn; v++) pack.push_back(T.n_scale > 0 && !T.scale_node.empty() && T.scale_node[v] ? 1 : 0);
   HIPCHK(upload(w.tree, pack.data(), pack.size(), e->stream));
   HIPCHK(hipStreamSynchronize(e->stream));      // (`pack` is on this stack)
   const int *d = w.tree.p;
   *out = AncTree{d, d + o_sons, d + o_father, d + o_post, d + o_pre, d + o_scale, (int)post.size(), (int)pre.size(), nn, n_tips, nn - n_tips, T.root};
   return 0;
}

// P(t) of every (gene, class, node), as an evaluation builds it: same kernels, same arguments (paml_amd_simulate does the same for one gene)
// (`d_label`: the nodes' labels on the device; null: the tree's own.  A call may build more than one family of matrices: the events are made once)
int anc_pmat(paml_amd_engine *e, const char *who, const double *branch, const double *gene_rate, AncScratch &w, const int *d_label)
{
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, K = e->K, G = e->n_genes, n = e->n;
   hipStream_t st = e->stream;
   if (int rc = eigen_refs_ok(e, e->h_eigen_of.data(), e->h_eigen_of.size(), who)) return rc;
   if (e->eigen_dirty) {
      std::vector<EigenDev> tab;
      if (int rc = eigen_table(e, tab)) return rc;
      HIPCHK(upload(e->d_eigen, tab.data(), tab.size(), st));
      HIPCHK(hipStreamSynchronize(st));
      e->eigen_dirty = false;
   }
   {
      std::vector<double> gr(G, 1.0);
      if (gene_rate) gr.assign(gene_rate, gene_rate + G);
      HIPCHK(upload(e->d_branch, branch, (size_t)nn, st));
      HIPCHK(upload(e->d_gene_rate, gr.data(), (size_t)G, st));
      HIPCHK(hipStreamSynchronize(st));      // (`gr` is on this stack)
      e->bl_gr_sent = false;
   }
   if (!w.ev0) HIPCHK(hipEventCreate(&w.ev0));
   if (!w.ev1) HIPCHK(hipEventCreate(&w.ev1));
   if (int rc = ensure_pmat_buffers(e, G * K, false, false)) return rc;
   // (from here on the P(t) buffers are this call's: whatever looked at an earlier evaluation's starts over)
   e->pmat_valid = false;
   e->bl.valid = false;
   HIPCHK(hipEventRecord(w.ev0, st));
   PmatArgs pa = pmat_args(e, T.root, d_label ? d_label : e->d_label.p, e->kk == KK_MFMA64 ? 1 : 0, nullptr);
   InlineVec iv;
   iv.n_branch = iv.n_rate = 0;
   bool small_pmat = e->kk != KK_MFMA64 && n <= 5;
   for (const EigenHost &h : e->eigen) small_pmat = small_pmat && h.kind != PAML_AMD_EIGEN_QMAT;
   launch_pmat(pa, iv, nn, G * K, small_pmat, st, pmat_on_matrix_cores(e, pa));
   HIPCHK(hipGetLastError());
   e->n_pmat += (long)G * K * (nn - 1);
   e->pmat_B = 1;
   e->rowmajor_valid = true;
   return 0;
}

// patterns per batch: what the workspace holds at `bytes_per_patt`, whole tiles, at least one (the variable `env`: MiB, default 256)
long anc_batch(double bytes_per_patt, long n_patt, const char *env)
{
   double arena_mb = 256;
   if (const char *s = getenv(env)) { const double v = atof(s); if (v > 0) arena_mb = v; }
   long batch = (long)(arena_mb * 1048576.0 / bytes_per_patt) / ANC_JTILE * ANC_JTILE;
   if (batch < ANC_JTILE) batch = (long)(arena_mb * 1048576.0 / bytes_per_patt) / ANC_TILE * ANC_TILE;
   if (batch > (1L << 24)) batch = 1L << 24;
   if (batch < ANC_TILE) batch = ANC_TILE;
   const long all = (n_patt + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   return batch > all ? all : batch;
}

int anc_common_checks(paml_amd_engine *e, const char *who)
{
   if (!(e->have_tips && e->have_tree && e->have_pi && e->have_classes) || e->eigen.empty())
      return fail(e, PAML_AMD_EINVAL, std::string(who) + " before set_tips/set_tree/set_pi/set_classes/set_eigen");
   if (e->n > 64) return fail(e, PAML_AMD_EUNSUPPORTED, std::string(who) + ": more than 64 states");
   return 0;
}

}  // namespace paml_amd

namespace {

// 4 / 5 / 20 states, the engines that are not on the matrix cores (paml_amd_create: every other state count is KK_MFMA64): the partial in registers
void anc_launch_lane(KernelKind kk, dim3 grid, hipStream_t st, const AncMargArgs &a, int outer)
{
   if (kk == KK_VALU4) hipLaunchKernelGGL(anc_lane_kernel<4>, grid, dim3(256), 0, st, a, outer);
   else if (kk == KK_VALU5) hipLaunchKernelGGL(anc_lane_kernel<5>, grid, dim3(256), 0, st, a, outer);
   else hipLaunchKernelGGL(anc_lane_kernel<20>, grid, dim3(256), 0, st, a, outer);
}

}  // namespace

extern "C" int paml_amd_ancestral_marginal(paml_amd_engine *e, const double *branch, const double *gene_rate, int n_query, const int *nodes,
                                           unsigned char *best, double *best_prob, double *post)
{
   enter(e);
   anc_last_batches = 0;
   anc_last_kernel_ms = 0;
   const char *who = "ancestral_marginal";
   if (!e || !branch || !best || !best_prob) return fail(e, PAML_AMD_EINVAL, "ancestral_marginal: null argument");
   if (int rc = anc_common_checks(e, who)) return rc;
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes, n_tips = e->n_tips, n_int = nn - n_tips;
   std::vector<int> query;
   if (nodes) {
      if (n_query < 1) return fail(e, PAML_AMD_EINVAL, "ancestral_marginal: n_query = " + std::to_string(n_query) + " < 1");
      std::vector<char> seen(nn, 0);
      for (int i = 0; i < n_query; i++) {
         const int v = nodes[i];
         if (v < 0 || v >= nn || v < n_tips || T.is_leaf(v)) return fail(e, PAML_AMD_EINVAL, "ancestral_marginal: node " + std::to_string(v) + " is not an internal node");
         if (seen[v]) return fail(e, PAML_AMD_EINVAL, "ancestral_marginal: node " + std::to_string(v) + " is listed twice");
         seen[v] = 1;
         query.push_back(v - n_tips);
      }
   }
   else
      for (int v = n_tips; v < nn; v++) query.push_back(v - n_tips);
   const int nq = (int)query.size();
   if (nq < 1) return fail(e, PAML_AMD_EINVAL, "ancestral_marginal: the tree has no internal node");
   for (size_t i = 0; i < e->eigen.size(); i++)
      if (e->eigen[i].kind == PAML_AMD_EIGEN_QMAT)
         return fail(e, PAML_AMD_EUNSUPPORTED, "ancestral_marginal: moving the root needs a reversible model");
   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   AncScratch w;
   AncMargArgs a{};
   if (int rc = anc_tree_pack(e, who, w, &a.t)) return rc;
   HIPCHK(upload(w.query, query.data(), query.size(), st));
   HIPCHK(hipStreamSynchronize(st));
   if (int rc = anc_pmat(e, who, branch, gene_rate, w)) return rc;
   HIPCHK(hipEventRecord(w.ev1, st));
   HIPCHK(hipStreamSynchronize(st));
   if (int rc = eigen_fail_check(e)) return rc;
   { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); anc_last_kernel_ms += ms; }

   const int ns = mfma ? 64 : n;      // doubles a partial takes per pattern
   const double per_patt = 2.0 * K * n_int * (ns + 1) * 8 + (double)nq * (n * 8 + 9);
   long batch = anc_batch(per_patt, e->n_patt);
   for (;;) {      // halve the batch until it fits
      const size_t part = (size_t)K * n_int * ns * batch, sc = (size_t)K * n_int * batch;
      if (w.L.ensure(part) == hipSuccess && w.G.ensure(part) == hipSuccess && w.SL.ensure(sc) == hipSuccess && w.SG.ensure(sc) == hipSuccess &&
          w.post.ensure((size_t)nq * batch * n) == hipSuccess && w.prob.ensure((size_t)nq * batch) == hipSuccess && w.best.ensure((size_t)nq * batch) == hipSuccess)
         break;
      (void)hipGetLastError();
      w.L.release(); w.G.release(); w.post.release();
      if (batch <= ANC_TILE) return fail(e, PAML_AMD_ENOMEM, "ancestral_marginal: no device memory for one tile of patterns");
      batch = (batch / 2 + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   }
   a.n = n; a.K = K; a.scaled = T.n_scale > 0 ? 1 : 0; a.n_pi = e->n_pi; a.n_query = nq; a.stride = batch;
   a.z = e->d_z.p; a.z_stride = e->n_patt; a.code_mask = e->d_code_mask.p;
   a.P = e->d_rowmajor.p; a.pint = e->d_pint.p; a.ptip = e->d_ptip.p; a.tip_words = (long)tip_words(e);
   a.pi = e->d_pi_plain.p; a.freqK = e->d_freqK.p; a.query = w.query.p;
   a.L = w.L.p; a.G = w.G.p; a.SL = w.SL.p; a.SG = w.SG.p; a.post = w.post.p; a.best_prob = w.prob.p; a.best = w.best.p; a.mfma = mfma ? 1 : 0;
   const long n_patt = e->n_patt;
   for (int g = 0; g < G; g++)
      for (long h0 = e->gene_off[g]; h0 < e->gene_off[g + 1]; h0 += batch) {
         const long nb = std::min<long>(batch, e->gene_off[g + 1] - h0);
         a.gene = g; a.h0 = h0; a.nb = nb;
         HIPCHK(hipEventRecord(w.ev0, st));
         for (int outer = 0; outer < 2; outer++) {
            if (mfma) hipLaunchKernelGGL(anc_mfma_kernel, dim3((unsigned)((nb + ANC_TILE - 1) / ANC_TILE), K), dim3(256), 0, st, a, outer);
            else anc_launch_lane(e->kk, dim3((unsigned)((nb + 255) / 256), K), st, a, outer);
            HIPCHK(hipGetLastError());
         }
         hipLaunchKernelGGL(anc_posterior_kernel, dim3((unsigned)((nb + 255) / 256), nq), dim3(256), 0, st, a);
         HIPCHK(hipGetLastError());
         HIPCHK(hipEventRecord(w.ev1, st));
         // the batch's rows to the caller's [n_query][n_patt]( [n] ): one plain copy per queried node (no pitch that n_patt could outgrow)
         for (int qi = 0; qi < nq; qi++) {
            HIPCHK(hipMemcpyAsync(best + (size_t)qi * n_patt + h0, w.best.p + (size_t)qi * batch, (size_t)nb, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(best_prob + (size_t)qi * n_patt + h0, w.prob.p + (size_t)qi * batch, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
            if (post)
               HIPCHK(hipMemcpyAsync(post + ((size_t)qi * n_patt + h0) * n, w.post.p + (size_t)qi * batch * n, (size_t)nb * n * 8, hipMemcpyDeviceToHost, st));
         }
         HIPCHK(hipStreamSynchronize(st));
         { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); anc_last_kernel_ms += ms; }
         anc_last_batches++;
      }
   return 0;
}

extern "C" int paml_amd_ancestral_joint(paml_amd_engine *e, const double *branch, const double *gene_rate, unsigned char *states, double *ln_best)
{
   enter(e);
   anc_last_batches = 0;
   anc_last_kernel_ms = 0;
   const char *who = "ancestral_joint";
   if (!e || !branch || !states || !ln_best) return fail(e, PAML_AMD_EINVAL, "ancestral_joint: null argument");
   if (int rc = anc_common_checks(e, who)) return rc;
   if (e->K != 1) return fail(e, PAML_AMD_EUNSUPPORTED, "ancestral_joint: one class only (this model has " + std::to_string(e->K) + ")");
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, G = e->n_genes, n_tips = e->n_tips, n_int = nn - n_tips;
   if (n_int < 1) return fail(e, PAML_AMD_EINVAL, "ancestral_joint: the tree has no internal node");
   hipStream_t st = e->stream;
   AncScratch w;
   AncJointArgs a{};
   if (int rc = anc_tree_pack(e, who, w, &a.t)) return rc;
   if (int rc = anc_pmat(e, who, branch, gene_rate, w)) return rc;
   const long n_p = (long)G * nn * n * n, n_q = (long)e->n_pi * n;
   HIPCHK(w.lnP.ensure((size_t)(n_p + n_q)));
   hipLaunchKernelGGL(anc_log_kernel, dim3((unsigned)((n_p + n_q + 255) / 256)), dim3(256), 0, st, (const double *)e->d_rowmajor.p, n_p, (const double *)e->d_pi_plain.p, n_q, w.lnP.p, w.lnP.p + n_p);
   HIPCHK(hipGetLastError());
   HIPCHK(hipEventRecord(w.ev1, st));
   HIPCHK(hipStreamSynchronize(st));
   if (int rc = eigen_fail_check(e)) return rc;
   e->pmat_valid = true;
   { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); anc_last_kernel_ms += ms; }

   const double per_patt = (double)n_int * n * 9 + n_int + 1 + 8;
   long batch = anc_batch(per_patt, e->n_patt);
   for (;;) {      // halve the batch until it fits
      if (w.L.ensure((size_t)n_int * n * batch) == hipSuccess && w.C.ensure((size_t)n_int * n * batch) == hipSuccess &&
          w.state.ensure((size_t)n_int * batch) == hipSuccess && w.rootstate.ensure((size_t)batch) == hipSuccess && w.lnbest.ensure((size_t)batch) == hipSuccess)
         break;
      (void)hipGetLastError();
      w.L.release(); w.C.release();
      if (batch <= ANC_TILE) return fail(e, PAML_AMD_ENOMEM, "ancestral_joint: no device memory for one tile of patterns");
      batch = (batch / 2 + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   }
   a.n = n; a.stride = batch; a.z = e->d_z.p; a.z_stride = e->n_patt; a.code_mask = e->d_code_mask.p;
   a.lnP = w.lnP.p; a.L = w.L.p; a.C = w.C.p; a.state = w.state.p; a.rootstate = w.rootstate.p; a.ln_best = w.lnbest.p;
   const long n_patt = e->n_patt;
   const size_t lds = (size_t)n * n * sizeof(double);
   for (int g = 0; g < G; g++)
      for (long h0 = e->gene_off[g]; h0 < e->gene_off[g + 1]; h0 += batch) {
         const long nb = std::min<long>(batch, e->gene_off[g + 1] - h0);
         a.gene = g; a.h0 = h0; a.nb = nb;
         a.lnpi = w.lnP.p + n_p + (long)(e->n_pi > 1 ? g : 0) * n;
         const dim3 grid((unsigned)((nb + ANC_JTILE - 1) / ANC_JTILE));
         HIPCHK(hipEventRecord(w.ev0, st));
         hipLaunchKernelGGL(anc_joint_kernel, grid, dim3(ANC_JTILE), lds, st, a);
         HIPCHK(hipGetLastError());
         HIPCHK(hipEventRecord(w.ev1, st));
         for (int vi = 0; vi < n_int; vi++)
            HIPCHK(hipMemcpyAsync(states + (size_t)vi * n_patt + h0, w.state.p + (size_t)vi * batch, (size_t)nb, hipMemcpyDeviceToHost, st));
         HIPCHK(hipMemcpyAsync(ln_best + h0, w.lnbest.p, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
         HIPCHK(hipStreamSynchronize(st));
         { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); anc_last_kernel_ms += ms; }
         anc_last_batches++;
      }
   return 0;
}
