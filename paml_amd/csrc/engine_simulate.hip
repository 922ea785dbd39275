// engine_simulate.hip — alignments drawn under the engine's model (Evolve / Simulate, evolver.c:737-805 and 818) on the device; the draw's
// definition and the kernels in kernels_simulate.h.  P(t) comes from the evaluation's own builders (launch_pmat, engine_eval.hip).
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_simulate.h"

static thread_local int sim_last_batches = 0;
static thread_local double sim_last_kernel_ms = 0;      // HIP events around the P(t), table and walk kernels of every batch, summed

extern "C" void paml_amd_simulate_info(int *last_batches, double *last_kernel_ms)
{
   if (last_batches) *last_batches = sim_last_batches;
   if (last_kernel_ms) *last_kernel_ms = sim_last_kernel_ms;
}

namespace {

// what a call allocates for itself; released on every way out
struct SimScratch {
   DevBuf<double> cdf;
   DevBuf<unsigned char> last, state, cls;
   DevBuf<int2> order;
   DevEvent ev0, ev1;
};

}  // namespace

extern "C" int paml_amd_simulate(paml_amd_engine *e, const double *branch, const double *gene_rate, long n_sites, long first_site,
                                 unsigned long long seed, unsigned replicate, unsigned char *z, unsigned char *cls, unsigned char *anc)
{
   enter(e);
   sim_last_batches = 0;
   sim_last_kernel_ms = 0;
   if (!e || !branch || !z) return fail(e, PAML_AMD_EINVAL, "simulate: null argument");
   if (n_sites < 1) return fail(e, PAML_AMD_EINVAL, "simulate: n_sites = " + std::to_string(n_sites) + " < 1");
   if (first_site < 0) return fail(e, PAML_AMD_EINVAL, "simulate: first_site = " + std::to_string(first_site) + " < 0");
   if (e->n_genes > 1) return fail(e, PAML_AMD_EUNSUPPORTED, "simulate: one gene only (this engine has " + std::to_string(e->n_genes) + ")");
   if (!(e->have_tree && e->have_pi && e->have_classes)) return fail(e, PAML_AMD_EINVAL, "simulate before set_tree/set_pi/set_classes");
   if (e->eigen.empty()) return fail(e, PAML_AMD_EINVAL, "simulate before any set_eigen_*");
   if (e->rate_per_gene) return fail(e, PAML_AMD_EUNSUPPORTED, "simulate: class rates per gene");
   const TreeDesc &T = e->tree;
   const int n = e->n, K = e->K, nn = T.n_nodes, n_tips = e->n_tips;
   if (K > 256 || n > 256) return fail(e, PAML_AMD_EUNSUPPORTED, "simulate: classes and states are bytes");
   if (int rc = eigen_refs_ok(e, e->h_eigen_of.data(), e->h_eigen_of.size(), "simulate")) return rc;
   hipStream_t st = e->stream;

   // (node, parent) pairs in pre-order from the root
   std::vector<int2> order;
   {
      std::vector<int> father(nn, -1), stack(1, T.root);
      while (!stack.empty()) {
         const int v = stack.back();
         stack.pop_back();
         if (v != T.root) order.push_back(make_int2(v, father[v]));
         for (int j = T.sons_ptr[v + 1] - 1; j >= T.sons_ptr[v]; j--) {      // (pushed last to first: visited first to last)
            father[T.sons[j]] = v;
            stack.push_back(T.sons[j]);
         }
      }
   }
   if ((int)order.size() != nn - 1) return fail(e, PAML_AMD_EINVAL, "simulate: the tree does not reach every node from its root");

   // P(t) of every (class, node), as an evaluation builds it: same kernels, same arguments; the row-major copies are what is read here
   // and what paml_amd_get_pmat hands out afterwards
   if (e->eigen_dirty) {
      std::vector<EigenDev> tab;
      if (int rc = eigen_table(e, tab)) return rc;
      HIPCHK(upload(e->d_eigen, tab.data(), tab.size(), st));
      HIPCHK(hipStreamSynchronize(st));
      e->eigen_dirty = false;
   }
   {
      const double one = 1.0;
      HIPCHK(upload(e->d_branch, branch, (size_t)nn, st));
      HIPCHK(upload(e->d_gene_rate, gene_rate ? gene_rate : &one, (size_t)1, st));
      HIPCHK(hipStreamSynchronize(st));      // (`one` is on this stack)
      e->bl_gr_sent = false;
   }
   SimScratch w;
   HIPCHK(w.ev0.ensure());
   HIPCHK(w.ev1.ensure());
   if (int rc = ensure_pmat_buffers(e, K, false, false)) return rc;
   // (from here on the P(t) buffers are this call's: whatever looked at an earlier evaluation's starts over)
   e->pmat_valid = false;
   e->bl.valid = false;
   const long n_rows = (long)K * nn * n;
   HIPCHK(w.cdf.ensure((size_t)n_rows * n + n + K));
   HIPCHK(w.last.ensure((size_t)n_rows + 2));
   HIPCHK(upload(w.order, order.data(), order.size(), st));
   HIPCHK(hipStreamSynchronize(st));
   HIPCHK(hipEventRecord(w.ev0, st));
   {
      PmatArgs pa = pmat_args(e, T.root, e->d_label.p, e->kk == KK_MFMA64 ? 1 : 0, nullptr);
      InlineVec iv;
      iv.n_branch = iv.n_rate = 0;
      bool small_pmat = e->kk != KK_MFMA64 && n <= 5;
      for (const EigenHost &h : e->eigen) small_pmat = small_pmat && h.kind != PAML_AMD_EIGEN_QMAT;
      launch_pmat(pa, iv, nn, K, small_pmat, st, pmat_on_matrix_cores(e, pa));
      HIPCHK(hipGetLastError());
      e->n_pmat += (long)K * (nn - 1);
      e->pmat_B = 1;
      e->rowmajor_valid = true;
   }
   hipLaunchKernelGGL(sim_cdf_kernel, dim3((unsigned)((n_rows + 2 + 255) / 256)), dim3(256), 0, st, e->d_rowmajor.p, e->d_pi_plain.p, e->d_freqK.p, n, K, nn,
                      T.root, w.cdf.p, w.last.p);
   HIPCHK(hipGetLastError());
   HIPCHK(hipEventRecord(w.ev1, st));
   HIPCHK(hipStreamSynchronize(st));
   if (int rc = eigen_fail_check(e)) return rc;
   e->pmat_valid = true;
   { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); sim_last_kernel_ms += ms; }

   // sites per batch: what the workspace of state bytes holds (default 256 MiB; PAML_AMD_SIM_ARENA_MB gives another size), a whole
   // number of tiles, at most 2^30 sites per launch, at least one tile
   double arena_mb = 256;
   if (const char *s = getenv("PAML_AMD_SIM_ARENA_MB")) { const double v = atof(s); if (v > 0) arena_mb = v; }
   long batch = (long)(arena_mb * 1048576.0 / (double)(nn + 1)) / SIM_TILE * SIM_TILE;
   if (batch > (1L << 30)) batch = 1L << 30;
   if (batch < SIM_TILE) batch = SIM_TILE;
   if (batch > n_sites) batch = (n_sites + SIM_TILE - 1) / SIM_TILE * SIM_TILE;
   for (;;) {      // halve the batch until it fits
      if (w.state.ensure((size_t)nn * batch) == hipSuccess && w.cls.ensure((size_t)batch) == hipSuccess) break;
      (void)hipGetLastError();
      w.state.release();
      if (batch <= SIM_TILE) return fail(e, PAML_AMD_ENOMEM, "simulate: no device memory for one tile of sites");
      batch = (batch / 2 + SIM_TILE - 1) / SIM_TILE * SIM_TILE;
   }
   SimArgs a{};
   a.cdf = w.cdf.p; a.last = w.last.p; a.order = w.order.p; a.state = w.state.p; a.cls = w.cls.p;
   a.stream = rell_stream(seed, replicate, 0u);
   a.stride = batch; a.n = n; a.K = K; a.n_nodes = nn; a.root = T.root;
   a.lds_cdf = (long)K * n * n <= SIM_LDS_CDF ? 1 : 0;
   a.lds_state = nn <= SIM_LDS_NODES ? 1 : 0;
   const size_t lds = (a.lds_cdf ? (size_t)K * n * n * sizeof(double) : 0) + (a.lds_state ? (size_t)nn * SIM_TILE : 0);
   for (long s0 = 0; s0 < n_sites; s0 += batch) {
      const long nb = n_sites - s0 < batch ? n_sites - s0 : batch;
      a.site0 = first_site + s0; a.n_sites = nb;
      const dim3 grid((unsigned)((nb + SIM_TILE - 1) / SIM_TILE));
      HIPCHK(hipEventRecord(w.ev0, st));
      if (n <= 5) hipLaunchKernelGGL(sim_walk_kernel<true>, grid, dim3(SIM_TILE), lds, st, a);
      else hipLaunchKernelGGL(sim_walk_kernel<false>, grid, dim3(SIM_TILE), lds, st, a);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(w.ev1, st));
      // rows of the batch's state array to the caller's [n_tips][n_sites] / [n_nodes - n_tips][n_sites]
      HIPCHK(hipMemcpy2DAsync(z + s0, (size_t)n_sites, w.state.p, (size_t)batch, (size_t)nb, (size_t)n_tips, hipMemcpyDeviceToHost, st));
      if (anc && nn > n_tips)
         HIPCHK(hipMemcpy2DAsync(anc + s0, (size_t)n_sites, w.state.p + (size_t)n_tips * batch, (size_t)batch, (size_t)nb, (size_t)(nn - n_tips),
                                 hipMemcpyDeviceToHost, st));
      if (cls) HIPCHK(hipMemcpyAsync(cls + s0, w.cls.p, (size_t)nb, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, w.ev0, w.ev1)); sim_last_kernel_ms += ms; }
      sim_last_batches++;
   }
   return 0;
}
