// engine_gradient.hip — the derivative of lnL with respect to every branch length and the per-pattern scores in one call
// (paml_amd_gradient); the definition in kernels_gradient.h, the kernels here.  P(t) comes from the evaluation's own builders (anc_pmat,
// engine_ancestral.hip), the down pass is the ancestral module's.
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_gradient.h"
#include "ancestral_host.h"

static thread_local AncCallInfo grad_info;

extern "C" void paml_amd_gradient_info(int *last_batches, double *last_kernel_ms) { grad_info.read(last_batches, last_kernel_ms); }

namespace paml_amd {

// the kernels' bodies are kernels_gradient.h's, at CURV = false (engine_curvature.hip holds the other instantiation)
__global__ __launch_bounds__(256) void grad_pmat_kernel(GradPmatArgs a)
{
   __shared__ double sE[64], sM[64];
   grad_pmat_body<false>(a, sE, sM);
}

// one pattern per lane: grid (patterns / 256, K); pass 0: the down pass, 1: the outer + derivative pass
template <int N> __global__ __launch_bounds__(256) void grad_lane_kernel(GradArgs a, int pass)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.m.nb) return;
   if (pass) grad_lane_outer<N>(a, blockIdx.y, p);
   else anc_lane_down<N>(a.m, blockIdx.y, p);
}

__global__ __launch_bounds__(256) void grad_mfma_kernel(GradArgs a)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   grad_mfma_body<false>(a, sP);
}

__global__ __launch_bounds__(256) void grad_combine_kernel(GradArgs a) { grad_combine_body<false>(a); }

// row v's chunks added in a fixed order: grid (n_nodes + 1)
__global__ __launch_bounds__(256) void grad_total_kernel(const double *partial, long n_chunks, double *out)
{
   __shared__ double sw4[4];
   const double s = red_total256(partial + (long)blockIdx.x * n_chunks, (int)n_chunks, false, sw4);
   if (threadIdx.x == 0) out[blockIdx.x] = s;
}
}  // namespace paml_amd

namespace {

struct GradScratch : AncScratch {
   using AncScratch::AncScratch;
   DevBuf<double> dP, PT, num, den, sig, scores, lnf, partial, out;
};

}  // namespace

extern "C" int paml_amd_gradient(paml_amd_engine *e, const double *branch, const double *gene_rate, double *lnL, double *grad, double *lnf, double *scores)
{
   enter(e);
   grad_info = AncCallInfo{};
   const char *who = "gradient";
   if (!e || !branch || !lnL || !grad) return fail(e, PAML_AMD_EINVAL, "gradient: null argument");
   if (int rc = anc_begin(e, who, "the derivative of a rate-matrix (UNREST) set's P(t) needs a matrix product of its own")) return rc;
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes, n_int = nn - e->n_tips;
   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   GradScratch w(grad_info);
   GradArgs a{};
   AncMargArgs &m = a.m;
   if (int rc = anc_tree_pack(e, who, w, &m.t)) return rc;
   if (int rc = anc_pmat(e, who, branch, gene_rate, w)) return rc;
   if (int rc = grad_dpmat(e, w.dP, nullptr, w.PT)) return rc;
   if (int rc = anc_pmat_wait(e, w)) return rc;
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) in the tree's own orientation, as after the joint reconstruction)

   const long n_chunks = anc_chunk_base(e)[G];
   HIPCHK(w.partial.ensure((size_t)(nn + 1) * std::max<long>(n_chunks, 1)));
   HIPCHK(w.out.ensure((size_t)nn + 1));

   const int ns = mfma ? 64 : n;      // doubles a partial takes per pattern
   const double per_patt = 2.0 * K * n_int * (ns + 1) * 8 + 3.0 * K * nn * 8 + (nn + 1) * 8.0;
   long batch = anc_batch(per_patt, e->n_patt, "PAML_AMD_GRAD_ARENA_MB");
   {
      const size_t part = (size_t)K * n_int * ns, sc = (size_t)K * n_int, cl = (size_t)K * nn;
      if (int rc = anc_alloc(e, who, {{&w.L, part}, {&w.G, part}, {&w.SL, sc}, {&w.SG, sc}, {&w.num, cl}, {&w.den, cl}, {&w.sig, cl}, {&w.scores, (size_t)nn}, {&w.lnf, 1}}, &batch))
         return rc;
   }
   anc_fill(e, w, batch, m);
   a.dP = w.dP.p; a.PT = w.PT.p; a.num = w.num.p; a.den = w.den.p; a.sig = w.sig.p; a.weights = e->d_weights.p;
   a.scores = w.scores.p; a.lnf = w.lnf.p; a.partial = w.partial.p; a.n_chunks = n_chunks;
   a.ref_node = T.sons[T.sons_ptr[T.root]];
   const long n_patt = e->n_patt;
   if (int rc = anc_batches(
          e, w, m, &a.chunk0, batch, [&](const AncBatch &b) { hipLaunchKernelGGL(grad_mfma_kernel, b.tiles, dim3(256), 0, st, a); },
          [&](const AncBatch &b, int pass) { anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(grad_lane_kernel<N()>, b.lanes, dim3(256), 0, st, a, pass); }); },
          [&](const AncBatch &b) {
             hipLaunchKernelGGL(grad_combine_kernel, dim3(b.lanes.x, nn + 1), dim3(256), 0, st, a);
             HIPCHK(hipGetLastError());
             return 0;
          },
          [&](const AncBatch &b) {      // the batch's rows to the caller's [n_nodes][n_patt]: one plain copy per node
             if (scores)
                for (int v = 0; v < nn; v++)
                   HIPCHK(hipMemcpyAsync(scores + (size_t)v * n_patt + b.h0, w.scores.p + (size_t)v * batch, (size_t)b.nb * 8, hipMemcpyDeviceToHost, st));
             if (lnf) HIPCHK(hipMemcpyAsync(lnf + b.h0, w.lnf.p, (size_t)b.nb * 8, hipMemcpyDeviceToHost, st));
             return 0;
          }))
      return rc;
   std::vector<double> out((size_t)nn + 1);
   if (int rc = anc_totals(e, w, w.partial.p, n_chunks, w.out.p, out)) return rc;
   for (int v = 0; v < nn; v++) grad[v] = v == T.root ? 0.0 : out[v];
   *lnL = out[nn];
   return 0;
}
