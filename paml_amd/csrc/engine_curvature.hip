// engine_curvature.hip — lnL, its derivative and its second derivative along every branch length in one call (paml_amd_curvature); the
// definition in kernels_curvature.h, the kernels' bodies in kernels_gradient.h at CURV = true.  P(t) comes from the evaluation's own builders
// (anc_pmat, engine_ancestral.hip), the down pass is the ancestral module's, the rows' totals are grad_total_kernel's.
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_curvature.h"
#include "ancestral_host.h"

static thread_local AncCallInfo curv_info;

extern "C" void paml_amd_curvature_info(int *last_batches, double *last_kernel_ms) { curv_info.read(last_batches, last_kernel_ms); }

namespace paml_amd {

// dP, d2P and P^T of every (parameter set, node) in one launch: grid (n_nodes, gene x class)
__global__ __launch_bounds__(256) void curv_pmat_kernel(GradPmatArgs a)
{
   __shared__ double sE[64], sM[64];
   grad_pmat_body<true>(a, sE, sM);
}

// matrix cores: grid (stride / ANC_TILE, K), after anc_mfma_kernel's down pass
__global__ __launch_bounds__(256) void curv_mfma_kernel(GradArgs a)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   grad_mfma_body<true>(a, sP);
}

// grid (stride / 256, 2 n_nodes + 1)
__global__ __launch_bounds__(256) void curv_combine_kernel(GradArgs a) { grad_combine_body<true>(a); }

}  // namespace paml_amd

namespace {

struct CurvScratch : AncScratch {
   using AncScratch::AncScratch;
   DevBuf<double> dP, d2P, PT, num, den, cur, sig, lnf, partial, out;
};

}  // namespace

extern "C" int paml_amd_curvature(paml_amd_engine *e, const double *branch, const double *gene_rate, double *lnL, double *grad, double *curv, double *lnf)
{
   enter(e);
   curv_info = AncCallInfo{};
   const char *who = "curvature";
   if (!e || !branch || !lnL || !grad || !curv) return fail(e, PAML_AMD_EINVAL, "curvature: null argument");
   if (!(e->have_tips && e->have_tree && e->have_pi && e->have_classes) || e->eigen.empty())      // (anc_common_checks' first test, with this call's prefix)
      return fail(e, PAML_AMD_EINVAL, "curvature: called before set_tips/set_tree/set_pi/set_classes/set_eigen");
   if (int rc = anc_begin(e, who, "the derivatives of a rate-matrix (UNREST) set's P(t) need matrix products of their own")) return rc;
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes, n_int = nn - e->n_tips;
   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   CurvScratch w(curv_info);
   GradArgs a{};
   AncMargArgs &m = a.m;
   if (int rc = anc_tree_pack(e, who, w, &m.t)) return rc;
   if (int rc = anc_pmat(e, who, branch, gene_rate, w)) return rc;
   if (int rc = grad_dpmat(e, w.dP, &w.d2P, w.PT)) return rc;
   if (int rc = anc_pmat_wait(e, w)) return rc;
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) in the tree's own orientation, as after paml_amd_gradient)

   const long n_chunks = anc_chunk_base(e)[G];
   const int rows = 2 * nn + 1;      // w s_v, w c_v, w lnf
   HIPCHK(w.partial.ensure((size_t)rows * std::max<long>(n_chunks, 1)));
   HIPCHK(w.out.ensure((size_t)rows));

   long batch = anc_batch(curv_bytes_per_pattern(K, n_int, nn, mfma ? 64 : n), e->n_patt, "PAML_AMD_CURV_ARENA_MB");
   {
      const size_t part = (size_t)K * n_int * (mfma ? 64 : n), sc = (size_t)K * n_int, cl = (size_t)K * nn;
      if (int rc = anc_alloc(e, who, {{&w.L, part}, {&w.G, part}, {&w.SL, sc}, {&w.SG, sc}, {&w.num, cl}, {&w.den, cl}, {&w.cur, cl}, {&w.sig, cl}, {&w.lnf, 1}}, &batch))
         return rc;
   }
   anc_fill(e, w, batch, m);
   a.dP = w.dP.p; a.d2P = w.d2P.p; a.PT = w.PT.p; a.num = w.num.p; a.den = w.den.p; a.cur = w.cur.p; a.sig = w.sig.p; a.weights = e->d_weights.p;
   a.lnf = w.lnf.p; a.partial = w.partial.p; a.n_chunks = n_chunks;
   a.ref_node = T.sons[T.sons_ptr[T.root]];
   if (int rc = anc_batches(
          e, w, m, &a.chunk0, batch, [&](const AncBatch &b) { hipLaunchKernelGGL(curv_mfma_kernel, b.tiles, dim3(256), 0, st, a); },
          [&](const AncBatch &b, int pass) { anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(curv_lane_kernel<N()>, b.lanes, dim3(256), 0, st, a, pass); }); },
          [&](const AncBatch &b) {
             hipLaunchKernelGGL(curv_combine_kernel, dim3(b.lanes.x, rows), dim3(256), 0, st, a);
             HIPCHK(hipGetLastError());
             return 0;
          },
          [&](const AncBatch &b) {
             if (lnf) HIPCHK(hipMemcpyAsync(lnf + b.h0, w.lnf.p, (size_t)b.nb * 8, hipMemcpyDeviceToHost, st));
             return 0;
          }))
      return rc;
   std::vector<double> out((size_t)rows);
   if (int rc = anc_totals(e, w, w.partial.p, n_chunks, w.out.p, out)) return rc;
   for (int v = 0; v < nn; v++) {
      grad[v] = v == T.root ? 0.0 : out[v];
      curv[v] = v == T.root ? 0.0 : out[nn + v];
   }
   *lnL = out[2 * nn];
   return 0;
}
