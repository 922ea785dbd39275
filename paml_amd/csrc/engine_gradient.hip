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

// dP of every (parameter set, node): grid (n_nodes, gene x class).  The formulas are pmat_deriv_kernel's, term for term.
__global__ __launch_bounds__(256) void grad_pmat_kernel(GradPmatArgs a)
{
   const int node = blockIdx.x, pset = blockIdx.y, n = a.n;
   if (node == a.root) return;
   const int gene = pset / a.K, iclass = pset % a.K, lab = a.label[node];
   const EigenDev es = a.eigen[a.eigen_of[(gene * a.K + iclass) * a.n_labels + lab]];
   const double t = a.branch[node];
   const double qf = es.kind == PAML_AMD_EIGEN_UVROOT ? a.qfactor[iclass * a.n_labels + lab] : 1.0;
   const double base = a.gene_rate[gene] * a.rate[gene * a.rate_gs + iclass] * qf;
   const int nroot = es.kind == PAML_AMD_EIGEN_CIJK ? es.nR : n;
   const bool closed = es.kind == PAML_AMD_EIGEN_K80 || es.kind == PAML_AMD_EIGEN_JC69LIKE, k80 = es.kind == PAML_AMD_EIGEN_K80;
   __shared__ double sE[64], sM[64];
   double m1 = 0, m2 = 0, e1 = 0, e2 = 0;
   if (closed) {
      m1 = base * (k80 ? -4 / (es.kappa + 2) : -(double)n / (n - 1));
      m2 = base * (k80 ? -2 * (es.kappa + 1) / (es.kappa + 2) : 0.0);
      e1 = exp(t * m1);
      e2 = k80 ? exp(t * m2) : 0.0;
   }
   else {
      for (int k = threadIdx.x; k < nroot; k += 256) {
         const double mu = base * es.Root[k];
         sM[k] = mu;
         sE[k] = k ? exp(t * mu) : 1.0;
      }
      __syncthreads();
   }
   auto entry = [&](int i, int j) -> double {
      if (closed) {
         double c1, c2;
         if (k80) { c1 = (i == j || (i ^ j) == 1) ? 0.25 : -0.25; c2 = i == j ? 0.5 : ((i ^ j) == 1 ? -0.5 : 0.0); }
         else { c1 = i == j ? 1 - 1.0 / n : -1.0 / n; c2 = 0; }
         return c1 * e1 * m1 + c2 * e2 * m2;
      }
      double dp = 0;
      for (int k = 1; k < nroot; k++) {
         const double c0 = es.kind == PAML_AMD_EIGEN_CIJK ? es.Cijk[((long)i * n + j) * nroot + k] * sE[k] : (es.U[i * n + k] * sE[k]) * es.V[k * n + j];
         dp += c0 * sM[k];
      }
      return dp;
   };
   const long slot = (long)pset * a.n_nodes + node;
   if (!a.mfma) {
      double *dP = a.dP + slot * n * n;
      for (int idx = threadIdx.x; idx < n * n; idx += 256) dP[idx] = entry(idx / n, idx % n);
      return;
   }
   // A-operand order: element ((kb2*4 + jb)*64 + lane)*2 + e  =  M[jb*16 + (lane&15)][4*(2*kb2+e) + (lane>>4)], zero padded
   const double *P = a.P + slot * n * n;
   double *df = a.dP + slot * 4096, *tf = a.PT + slot * 4096;
   for (int idx = threadIdx.x; idx < 4096; idx += 256) {
      const int e = idx & 1, lane = (idx >> 1) & 63, jb = (idx >> 7) & 3, kb2 = idx >> 9;
      const int r = jb * 16 + (lane & 15), c = 4 * (2 * kb2 + e) + (lane >> 4);
      const bool in = r < n && c < n;
      df[idx] = in ? entry(r, c) : 0.0;
      if (node >= a.n_tips) tf[idx] = in ? P[c * n + r] : 0.0;
   }
}

// one pattern per lane: grid (patterns / 256, K); pass 0: the down pass, 1: the outer + derivative pass
template <int N> __global__ __launch_bounds__(256) void grad_lane_kernel(GradArgs a, int pass)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.m.nb) return;
   if (pass) grad_lane_outer<N>(a, blockIdx.y, p);
   else anc_lane_down<N>(a.m, blockIdx.y, p);
}

// Matrix cores, the outer + derivative pass: a workgroup of four waves owns ANC_TILE patterns of one class, as anc_mfma_kernel (whose
// down pass runs first): lane = q * 16 + pattern, register m = state 4 m + q.  Grid (stride / ANC_TILE, K).
__global__ __launch_bounds__(256) void grad_mfma_kernel(GradArgs a)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   const AncMargArgs &m = a.m;
   const AncTree &t = m.t;
   const int tid = threadIdx.x, lane = tid & 63, n = m.n;
   const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
   const int q = lane >> 4, k = blockIdx.y;
   const AncMfma w{sP, lane, wave, q};
   const long g16 = (long)blockIdx.x * 4 + wave, p = g16 * 16 + (lane & 15);
   const long pc = p < m.nb ? p : m.nb - 1;      // (lanes past the batch's end read the last pattern and write into the padding: p < stride)
   const long pset = (long)m.gene * m.K + k;
   const double *pi = m.pi + (long)(m.n_pi > 1 ? m.gene : 0) * n;
   if (t.root >= t.n_tips) {
      const int ri = t.root - t.n_tips;
      double x[16];
#pragma unroll
      for (int i = 0; i < 16; i++) x[i] = 4 * i + q < n ? pi[4 * i + q] : 0.0;
      part_store(m.G + (((long)k * t.n_int + ri) * (m.stride >> 4) + g16) * 1024, lane, x);
      if (q == 0) m.SG[((long)k * t.n_int + ri) * m.stride + p] = 0;
   }
   const int n_walk = t.n_pre + t.n_tips;
   for (int i = 0; i < n_walk; i++) {
      const int v = i < t.n_pre ? t.pre[i] : i - t.n_pre;      // the internal nodes father first, then the tips
      if (v == t.root) continue;
      const int f = t.father[v];
      double h[16], ls = 0;
      __syncthreads();      // (SG of the father was stored by the pattern's q = 0 lane: a workgroup-scope fence before the other lanes read it)
      if (f >= t.n_tips) {
         const int fi = f - t.n_tips;
         part_load(m.G + (((long)k * t.n_int + fi) * (m.stride >> 4) + g16) * 1024, lane, h);      // (this lane's own stores)
         ls = m.SG[((long)k * t.n_int + fi) * m.stride + pc];
      }
      else {
         const unsigned long long mask = m.code_mask[m.z[(long)f * m.z_stride + m.h0 + pc]];
#pragma unroll
         for (int j = 0; j < 16; j++) h[j] = (4 * j + q < n && ((mask >> (4 * j + q)) & 1ull)) ? pi[4 * j + q] : 0.0;
      }
      for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
         if (t.sons[j] != v) anc_mfma_mul_son(m, w, k, g16, pc, t.sons[j], h, &ls);
      const long slot = pset * t.n_nodes + v;
      const long oi = grad_out_idx(a, k, v, p);
      double x[16], y[16];
      v4d acc[4];
      if (v < t.n_tips) {
         const int code = (int)m.z[(long)v * m.z_stride + m.h0 + pc];
         const unsigned long long mask = m.code_mask[code];
#pragma unroll
         for (int j = 0; j < 16; j++) x[j] = (mask >> (4 * j + q)) & 1ull ? 1.0 : 0.0;
         w.product(a.dP + slot * 4096, x, acc);
#pragma unroll
         for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
         const double num = grad_mfma_dot(h, y);
         double2 tv[8];
         tip_gather(m.ptip + pset * t.n_nodes * m.tip_words, m.tip_words, v, code, q, tv);
#pragma unroll
         for (int j = 0; j < 8; j++) { y[2 * j] = tv[j].x; y[2 * j + 1] = tv[j].y; }
         const double den = grad_mfma_dot(h, y);
         if (q == 0) { a.num[oi] = num; a.den[oi] = den; a.sig[oi] = ls; }
         continue;
      }
      const int vi = v - t.n_tips;
      part_load(m.L + (((long)k * t.n_int + vi) * (m.stride >> 4) + g16) * 1024, lane, x);
      w.product(a.dP + slot * 4096, x, acc);
#pragma unroll
      for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
      const double num = grad_mfma_dot(h, y);
      w.product(a.PT + slot * 4096, h, acc);      // A_v = P_v^T H_v
#pragma unroll
      for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
      const double den = grad_mfma_dot(y, x);
      if (q == 0) { a.num[oi] = num; a.den[oi] = den; a.sig[oi] = ls + m.SL[((long)k * t.n_int + vi) * m.stride + pc]; }
      if (m.scaled) {
         const double mx = anc_mfma_max(y);
         if (mx > 0) {
#pragma unroll
            for (int j = 0; j < 16; j++) y[j] /= mx;
            ls += log(mx);
         }
      }
      part_store(m.G + (((long)k * t.n_int + vi) * (m.stride >> 4) + g16) * 1024, lane, y);
      if (q == 0) m.SG[((long)k * t.n_int + vi) * m.stride + p] = ls;
   }
}

// the classes of every (node, pattern) and the chunks' sums: grid (stride / 256, n_nodes + 1); a wave = one chunk of GRAD_CHUNK patterns
__global__ __launch_bounds__(256) void grad_combine_kernel(GradArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   const int v = blockIdx.y;
   double acc = p < a.m.nb ? grad_combine(a, v, p) : 0.0;
#pragma unroll
   for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
   const long chunk = a.chunk0 + (p >> 6);
   if ((threadIdx.x & 63) == 0 && (p & ~63L) < a.m.nb) a.partial[(long)v * a.n_chunks + chunk] = acc;
}

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
   ~GradScratch()
   {
      for (DevBuf<double> *b : {&dP, &PT, &num, &den, &sig, &scores, &lnf, &partial, &out}) b->release();
   }
};

}  // namespace

extern "C" int paml_amd_gradient(paml_amd_engine *e, const double *branch, const double *gene_rate, double *lnL, double *grad, double *lnf, double *scores)
{
   enter(e);
   grad_info = AncCallInfo{};
   const char *who = "gradient";
   if (!e || !branch || !lnL || !grad) return fail(e, PAML_AMD_EINVAL, "gradient: null argument");
   if (int rc = anc_common_checks(e, who)) return rc;
   if (e->world > 1) return fail(e, PAML_AMD_EUNSUPPORTED, "gradient: one rank only (this engine's communicator has " + std::to_string(e->world) + ")");
   for (size_t i = 0; i < e->eigen.size(); i++)
      if (e->eigen[i].kind == PAML_AMD_EIGEN_QMAT)
         return fail(e, PAML_AMD_EUNSUPPORTED, "gradient: the derivative of a rate-matrix (UNREST) set's P(t) needs a matrix product of its own");
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes, n_tips = e->n_tips, n_int = nn - n_tips;
   if (nn < 2) return fail(e, PAML_AMD_EINVAL, "gradient: the tree has no branch");
   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   GradScratch w(grad_info);
   GradArgs a{};
   AncMargArgs &m = a.m;
   if (int rc = anc_tree_pack(e, who, w, &m.t)) return rc;
   if (int rc = anc_pmat(e, who, branch, gene_rate, w)) return rc;
   {
      const size_t pn = (size_t)G * K * nn;
      HIPCHK(w.dP.ensure(pn * (mfma ? 4096 : n * n)));
      if (mfma) HIPCHK(w.PT.ensure(pn * 4096));
      GradPmatArgs ga{};
      ga.n = n; ga.K = K; ga.n_nodes = nn; ga.n_tips = n_tips; ga.root = T.root; ga.n_labels = e->n_labels; ga.rate_gs = e->rate_per_gene ? K : 0; ga.mfma = mfma ? 1 : 0;
      ga.label = e->d_label.p; ga.eigen_of = e->d_eigen_of.p; ga.eigen = e->d_eigen.p;
      ga.branch = e->d_branch.p; ga.rate = e->d_rate.p; ga.gene_rate = e->d_gene_rate.p; ga.qfactor = e->d_qfactor.p;
      ga.P = e->d_rowmajor.p; ga.dP = w.dP.p; ga.PT = w.PT.p;
      hipLaunchKernelGGL(grad_pmat_kernel, dim3(nn, G * K), dim3(256), 0, st, ga);
      HIPCHK(hipGetLastError());
   }
   if (int rc = anc_pmat_wait(e, w)) return rc;
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) in the tree's own orientation, as after the joint reconstruction)

   const std::vector<long> chunk_base = anc_chunk_base(e);
   const long n_chunks = chunk_base[G];
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
   for (int g = 0; g < G; g++)
      for (long h0 = e->gene_off[g]; h0 < e->gene_off[g + 1]; h0 += batch) {
         const long nb = std::min<long>(batch, e->gene_off[g + 1] - h0);
         m.gene = g; m.h0 = h0; m.nb = nb;
         a.chunk0 = chunk_base[g] + (h0 - e->gene_off[g]) / GRAD_CHUNK;
         HIPCHK(hipEventRecord(w.ev0, st));
         if (mfma) {
            const dim3 grid((unsigned)((nb + ANC_TILE - 1) / ANC_TILE), K);
            hipLaunchKernelGGL(anc_mfma_kernel, grid, dim3(256), 0, st, m, 0);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(grad_mfma_kernel, grid, dim3(256), 0, st, a);
            HIPCHK(hipGetLastError());
         }
         else
            for (int pass = 0; pass < 2; pass++) {
               anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(grad_lane_kernel<N()>, dim3((unsigned)((nb + 255) / 256), K), dim3(256), 0, st, a, pass); });
               HIPCHK(hipGetLastError());
            }
         hipLaunchKernelGGL(grad_combine_kernel, dim3((unsigned)((nb + 255) / 256), nn + 1), dim3(256), 0, st, a);
         HIPCHK(hipGetLastError());
         HIPCHK(hipEventRecord(w.ev1, st));
         // the batch's rows to the caller's [n_nodes][n_patt]: one plain copy per node
         if (scores)
            for (int v = 0; v < nn; v++)
               HIPCHK(hipMemcpyAsync(scores + (size_t)v * n_patt + h0, w.scores.p + (size_t)v * batch, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
         if (lnf) HIPCHK(hipMemcpyAsync(lnf + h0, w.lnf.p, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
         HIPCHK(w.lap(st));
         grad_info.batches++;
      }
   std::vector<double> out((size_t)nn + 1);
   if (int rc = anc_totals(e, w, w.partial.p, n_chunks, w.out.p, out)) return rc;
   for (int v = 0; v < nn; v++) grad[v] = v == T.root ? 0.0 : out[v];
   *lnL = out[nn];
   return 0;
}
