// engine_counts.hip — posterior expected labelled substitution counts and dwell times per branch and per pattern in one call
// (paml_amd_subst_counts): the definition in kernels_counts.h, the kernels here.  P(t) comes from the evaluation's own builders (anc_pmat,
// engine_ancestral.hip), the down pass is the ancestral module's, the outer pass is the model gradient's (H_v stored); the label-matrix
// kernel and the product kernels are this unit's.  Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_counts.h"
#include "ancestral_host.h"

static thread_local AncCallInfo counts_info;

extern "C" void paml_amd_subst_counts_info(int *last_batches, double *last_kernel_ms) { counts_info.read(last_batches, last_kernel_ms); }

namespace paml_amd {

// I_lkv of one (queried node, gene x class, label): grid (n_query, gene x class, n_lab); a thread owns the entries tid, tid + 256, ... of
// every n x n intermediate (sixteen at most), which pass through one LDS buffer, as in mg_pull_kernel (whose adjoint this is).
__global__ __launch_bounds__(256) void counts_label_kernel(CountsLabelArgs a)
{
   __shared__ double sA[4096], sLam[64];
   const int qi = blockIdx.x, pset = blockIdx.y, l = blockIdx.z, n = a.n, tid = threadIdx.x, n2 = n * n;
   const int node = a.nodes[qi], gene = pset / a.K, iclass = pset % a.K, lab = a.label[node];
   const EigenDev es = a.eigen[a.eigen_of[(gene * a.K + iclass) * a.n_labels + lab]];
   const bool uv = es.kind == PAML_AMD_EIGEN_UVROOT;
   const double qf = uv ? a.qfactor[iclass * a.n_labels + lab] : 1.0;
   const double tau = a.branch[node] * (a.gene_rate[gene] * a.rate[gene * a.rate_gs + iclass] * qf);
   const double dwell = tau > 0 ? a.branch[node] / tau : 0.0;      // the diagonal's unit: branch[v] per unit of tau
   const int R = uv ? n : (es.kind == PAML_AMD_EIGEN_CIJK ? es.nR : (es.kind == PAML_AMD_EIGEN_K80 ? 3 : 2));
   const double *M = a.M + (long)l * n2;
   if (tid < R) sLam[tid] = mg_lambda(es, n, tid);
   __syncthreads();
   double reg[16];
   if (uv) {
      // B[a][b] = A[a][b] M[a][b], A = U diag(Root) V;  B[a][a] = M[a][a] branch / tau
#pragma unroll
      for (int j = 0; j < 16; j++) {
         const int idx = tid + 256 * j, r = idx / n, c = idx % n;
         if (idx >= n2) continue;
         double s = 0;
         if (r != c)
            for (int i = 0; i < n; i++) s += (es.U[r * n + i] * sLam[i]) * es.V[i * n + c];
         sA[idx] = r == c ? M[idx] * dwell : s * M[idx];
      }
      __syncthreads();
      // T1[i][b] = sum_a V[i][a] B[a][b]
#pragma unroll
      for (int j = 0; j < 16; j++) {
         const int idx = tid + 256 * j, i = idx / n, c = idx % n;
         double s = 0;
         if (idx < n2)
            for (int x = 0; x < n; x++) s += es.V[i * n + x] * sA[x * n + c];
         reg[j] = s;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 16; j++)
         if (tid + 256 * j < n2) sA[tid + 256 * j] = reg[j];
      __syncthreads();
      // Z[i][j] = Psi_ij sum_b T1[i][b] U[b][j]
#pragma unroll
      for (int j = 0; j < 16; j++) {
         const int idx = tid + 256 * j, i = idx / n, c = idx % n;
         double s = 0;
         if (idx < n2) {
            for (int x = 0; x < n; x++) s += sA[i * n + x] * es.U[x * n + c];
            s *= mg_psi(sLam[i], sLam[c], tau);
         }
         reg[j] = s;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 16; j++)
         if (tid + 256 * j < n2) sA[tid + 256 * j] = reg[j];
      __syncthreads();
      // T2[a][j] = sum_i U[a][i] Z[i][j]
#pragma unroll
      for (int j = 0; j < 16; j++) {
         const int idx = tid + 256 * j, r = idx / n, c = idx % n;
         double s = 0;
         if (idx < n2)
            for (int i = 0; i < n; i++) s += es.U[r * n + i] * sA[i * n + c];
         reg[j] = s;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 16; j++)
         if (tid + 256 * j < n2) sA[tid + 256 * j] = reg[j];
      __syncthreads();
      // I[a][b] = sum_j T2[a][j] V[j][b]
#pragma unroll
      for (int j = 0; j < 16; j++) {
         const int idx = tid + 256 * j, r = idx / n, c = idx % n;
         double s = 0;
         if (idx < n2)
            for (int i = 0; i < n; i++) s += sA[r * n + i] * es.V[i * n + c];
         reg[j] = s;
      }
   }
   else {
      // projector form: I = sum_{r,s} Psi_rs Pi_r B Pi_s, B formed where it is read (A = sum_r lambda_r Pi_r: two or three terms, nR of a CIJK set)
      auto B = [&](int r, int c) -> double {
         if (r == c) return M[r * n + r] * dwell;
         double s = 0;
         for (int i = 0; i < R; i++) s += sLam[i] * mg_proj(es, n, i, r, c);
         return s * M[r * n + c];
      };
      double out[16];
#pragma unroll
      for (int j = 0; j < 16; j++) out[j] = 0;
      for (int s = 0; s < R; s++) {
         // T_s[a][b] = sum_x B[a][x] Pi_s[x][b]
#pragma unroll
         for (int j = 0; j < 16; j++) {
            const int idx = tid + 256 * j, r = idx / n, c = idx % n;
            double t = 0;
            if (idx < n2)
               for (int x = 0; x < n; x++) t += B(r, x) * mg_proj(es, n, s, x, c);
            reg[j] = t;
         }
         __syncthreads();      // (every thread is done reading the last T)
#pragma unroll
         for (int j = 0; j < 16; j++)
            if (tid + 256 * j < n2) sA[tid + 256 * j] = reg[j];
         __syncthreads();
         for (int r = 0; r < R; r++) {
            const double psi = mg_psi(sLam[r], sLam[s], tau);
#pragma unroll
            for (int j = 0; j < 16; j++) {
               const int idx = tid + 256 * j, ra = idx / n, c = idx % n;
               double t = 0;
               if (idx < n2)
                  for (int y = 0; y < n; y++) t += mg_proj(es, n, r, ra, y) * sA[y * n + c];
               out[j] += psi * t;
            }
         }
      }
#pragma unroll
      for (int j = 0; j < 16; j++) reg[j] = out[j];
   }
   const long slot = ((long)pset * a.n_query + qi) * a.n_lab + l;
   if (!a.mfma) {
#pragma unroll
      for (int j = 0; j < 16; j++)
         if (tid + 256 * j < n2) a.I[slot * n2 + tid + 256 * j] = reg[j];
      return;
   }
   __syncthreads();      // (every thread is done reading the last intermediate)
#pragma unroll
   for (int j = 0; j < 16; j++)
      if (tid + 256 * j < n2) sA[tid + 256 * j] = reg[j];
   __syncthreads();
   // A-operand order: element ((kb2*4 + jb)*64 + lane)*2 + e  =  I[jb*16 + (lane&15)][4*(2*kb2+e) + (lane>>4)], zero padded
   for (int idx = tid; idx < 4096; idx += 256) {
      const int e = idx & 1, lane = (idx >> 1) & 63, jb = (idx >> 7) & 3, kb2 = idx >> 9;
      const int r = jb * 16 + (lane & 15), c = 4 * (2 * kb2 + e) + (lane >> 4);
      a.I[slot * 4096 + idx] = r < n && c < n ? sA[r * n + c] : 0.0;
   }
}

// one pattern per lane: grid (patterns / 256, K); pass 0: the down pass, 1: the model gradient's outer pass
template <int N> __global__ __launch_bounds__(256) void counts_pass_kernel(ModelGradArgs a, int pass)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.m.nb) return;
   if (pass) mg_lane_outer<N>(a, blockIdx.y, p);
   else anc_lane_down<N>(a.m, blockIdx.y, p);
}

// lnf and the pattern's scalar rows at the root's first son (mg_coef's statements): grid (patterns / 256)
__global__ __launch_bounds__(256) void counts_scalar_kernel(ModelGradArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p < a.m.nb) mg_coef(a, a.m.t.n_nodes, p);
}

// one pattern per lane: grid (patterns / 256, n_query)
template <int N> __global__ __launch_bounds__(256) void counts_lane_kernel(CountsArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p < a.g.m.nb) counts_lane<N>(a, blockIdx.y, p);
}

// Matrix cores: a workgroup of four waves owns ANC_TILE patterns of one queried node; lane = q * 16 + pattern, register m = state 4 m + q
// (the passes' layout).  Per class, ascending: H_v and L_v of the wave's sixteen patterns are loaded once and stay in registers while the
// labels' matrices stream through LDS, one product and one dot product each.  Grid (stride / ANC_TILE, n_query).
__global__ __launch_bounds__(256) void counts_mfma_kernel(CountsArgs a)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   const ModelGradArgs &g = a.g;
   const AncMargArgs &m = g.m;
   const AncTree &t = m.t;
   const int tid = threadIdx.x, lane = tid & 63;
   const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
   const int q = lane >> 4, qi = blockIdx.y, v = a.nodes[qi], K = m.K;
   const AncMfma w{sP, lane, wave, q};
   const long g16 = (long)blockIdx.x * 4 + wave, p = g16 * 16 + (lane & 15);
   const long pc = p < m.nb ? p : m.nb - 1;      // (lanes past the batch's end compute the last pattern again and store zeros into the padding: p < stride)
   const long groups = m.stride >> 4;
   const bool tip = v < t.n_tips;
   double smax = -1e300;
   for (int k = 0; k < K; k++) {
      const double s = g.sig[mg_out_idx(g, k, v, pc)];
      smax = s > smax ? s : smax;
   }
   double den = 0, num[COUNTS_MAX_LABELS];
#pragma unroll
   for (int l = 0; l < COUNTS_MAX_LABELS; l++) num[l] = 0;
   unsigned long long mask = 0;
   if (tip) mask = m.code_mask[m.z[(long)v * m.z_stride + m.h0 + pc]];
   for (int k = 0; k < K; k++) {
      const long oi = mg_out_idx(g, k, v, pc);
      const double rho = m.freqK[k] * exp(g.sig[oi] - smax);
      den += rho * g.den[oi];
      double h[16], x[16];
      part_load(g.H + (((long)k * t.n_nodes + v) * groups + g16) * 1024, lane, h);
      if (tip) {
#pragma unroll
         for (int j = 0; j < 16; j++) x[j] = (mask >> (4 * j + q)) & 1ull ? 1.0 : 0.0;
      }
      else part_load(m.L + (((long)k * t.n_int + (v - t.n_tips)) * groups + g16) * 1024, lane, x);
      const double *Ik = a.I + (((long)m.gene * K + k) * a.n_query + qi) * a.n_lab * 4096;
#pragma unroll
      for (int l = 0; l < COUNTS_MAX_LABELS; l++)
         if (l < a.n_lab) {      // (uniform over the workgroup: the product's barriers are met by every thread)
            v4d acc[4];
            w.product(Ik + (long)l * 4096, x, acc);
            double y[16];
#pragma unroll
            for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
            num[l] += rho * grad_mfma_dot(h, y);
         }
   }
   const bool live = p < m.nb && g.weights[m.h0 + pc] > 0;
   if (q == 0) {
#pragma unroll
      for (int l = 0; l < COUNTS_MAX_LABELS; l++)
         if (l < a.n_lab) a.site[counts_site_idx(a, l, qi, p)] = live ? num[l] / den : 0.0;
   }
}

// the chunks' sums of w_h n_lv(h): grid (stride / 256, n_lab x n_query); a wave = one chunk of GRAD_CHUNK patterns; row 0 of partial is lnL's
__global__ __launch_bounds__(256) void counts_rows_kernel(CountsArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   const int r = blockIdx.y;
   double acc = p < a.g.m.nb ? counts_row_term(a, r, p) : 0.0;
#pragma unroll
   for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
   const long chunk = a.g.chunk0 + (p >> 6);
   if ((threadIdx.x & 63) == 0 && (p & ~63L) < a.g.m.nb) a.g.partial[(long)(1 + r) * a.g.n_chunks + chunk] = acc;
}

}  // namespace paml_amd

namespace {

struct CountsScratch : AncScratch {
   using AncScratch::AncScratch;
   DevBuf<double> PT, H, den, sig, R, SR, croot, rows, lnf, partial, out, M, I, site;
};

}  // namespace

extern "C" int paml_amd_subst_counts(paml_amd_engine *e, const double *branch, const double *gene_rate, int n_lab, const double *labels, int n_query, const int *nodes,
                                     double *lnL, double *counts, double *site_counts, double *lnf)
{
   enter(e);
   counts_info = AncCallInfo{};
   const char *who = "subst_counts";
   if (!e || !branch || !labels || !lnL || !counts) return fail(e, PAML_AMD_EINVAL, "subst_counts: null argument");
   if (int rc = anc_begin(e, who, "a rate-matrix (UNREST) set has no spectral form for the integral of the label matrices")) return rc;
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes, n_int = nn - e->n_tips;
   if (n_lab < 1 || n_lab > COUNTS_MAX_LABELS)
      return fail(e, PAML_AMD_EINVAL, "subst_counts: n_lab = " + std::to_string(n_lab) + " is not in 1 .. " + std::to_string(COUNTS_MAX_LABELS));
   for (size_t i = 0; i < (size_t)n_lab * n * n; i++)
      if (!std::isfinite(labels[i])) return fail(e, PAML_AMD_EINVAL, "subst_counts: label " + std::to_string(i / ((size_t)n * n)) + " has an entry that is not finite");
   // the queried nodes and the column of the caller's arrays each one fills (no list: every node in node order, the root's column zero)
   std::vector<int> query, col;
   if (nodes) {
      if (n_query < 1) return fail(e, PAML_AMD_EINVAL, "subst_counts: n_query = " + std::to_string(n_query) + " < 1");
      std::vector<char> seen(nn, 0);
      for (int i = 0; i < n_query; i++) {
         const int v = nodes[i];
         if (v < 0 || v >= nn) return fail(e, PAML_AMD_EINVAL, "subst_counts: node " + std::to_string(v) + " is out of range");
         if (v == T.root) return fail(e, PAML_AMD_EINVAL, "subst_counts: node " + std::to_string(v) + " is the root: no branch above it");
         if (seen[v]) return fail(e, PAML_AMD_EINVAL, "subst_counts: node " + std::to_string(v) + " is listed twice");
         seen[v] = 1;
         query.push_back(v);
         col.push_back(i);
      }
   }
   else
      for (int v = 0; v < nn; v++)
         if (v != T.root) { query.push_back(v); col.push_back(v); }
   const int nq = (int)query.size(), n_out = nodes ? n_query : nn, n_rows = n_lab * nq;
   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   CountsScratch w(counts_info);
   CountsArgs a{};
   ModelGradArgs &ga = a.g;
   AncMargArgs &m = ga.m;
   if (int rc = anc_tree_pack(e, who, w, &m.t)) return rc;
   if (int rc = anc_pmat(e, who, branch, gene_rate, w)) return rc;
   const size_t pn = (size_t)G * K * nn, isz = mfma ? 4096 : (size_t)n * n;
   if (mfma) {
      HIPCHK(w.PT.ensure(pn * 4096));
      hipLaunchKernelGGL(nni_pt_all_kernel, dim3(nn, (unsigned)(G * K)), dim3(256), 0, st, (const double *)e->d_rowmajor.p, w.PT.p, n, nn, T.root);
      HIPCHK(hipGetLastError());
   }
   {
      HIPCHK(upload(w.query, query.data(), query.size(), st));
      HIPCHK(upload(w.M, labels, (size_t)n_lab * n * n, st));
      HIPCHK(w.I.ensure((size_t)G * K * nq * n_lab * isz));
      CountsLabelArgs la{};
      la.n = n; la.K = K; la.n_labels = e->n_labels; la.rate_gs = e->rate_per_gene ? K : 0; la.mfma = mfma ? 1 : 0; la.n_query = nq; la.n_lab = n_lab;
      la.nodes = w.query.p; la.label = e->d_label.p; la.eigen_of = e->d_eigen_of.p; la.eigen = e->d_eigen.p;
      la.branch = e->d_branch.p; la.rate = e->d_rate.p; la.gene_rate = e->d_gene_rate.p; la.qfactor = e->d_qfactor.p;
      la.M = w.M.p; la.I = w.I.p;
      hipLaunchKernelGGL(counts_label_kernel, dim3(nq, G * K, n_lab), dim3(256), 0, st, la);
      HIPCHK(hipGetLastError());
   }
   if (int rc = anc_pmat_wait(e, w)) return rc;      // (also: `query` and the caller's labels are read)
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) in the tree's own orientation, as after paml_amd_gradient)

   const long n_chunks = anc_chunk_base(e)[G];
   const int ns = mfma ? 64 : n;
   HIPCHK(w.partial.ensure((size_t)(1 + n_rows) * std::max<long>(n_chunks, 1)));
   HIPCHK(w.out.ensure((size_t)1 + n_rows));
   long batch = anc_batch(counts_bytes_per_pattern(K, n_int, nn, ns, n_lab, nq), e->n_patt, "PAML_AMD_COUNTS_ARENA_MB");
   {
      const size_t part = (size_t)K * n_int * ns, sc = (size_t)K * n_int, cl = (size_t)K * nn;
      if (int rc = anc_alloc(e, who, {{&w.L, part}, {&w.G, part}, {&w.SL, sc}, {&w.SG, sc}, {&w.H, cl * ns}, {&w.den, cl}, {&w.sig, cl}, {&w.R, (size_t)K * ns},
                                      {&w.SR, (size_t)K}, {&w.croot, (size_t)K}, {&w.rows, (size_t)1 + K}, {&w.lnf, 1}, {&w.site, (size_t)n_rows}}, &batch))
         return rc;
   }
   anc_fill(e, w, batch, m);
   ga.PT = w.PT.p; ga.H = w.H.p; ga.den = w.den.p; ga.sig = w.sig.p; ga.R = w.R.p; ga.SR = w.SR.p; ga.croot = w.croot.p; ga.rows = w.rows.p;
   ga.lnf = w.lnf.p; ga.weights = e->d_weights.p; ga.partial = w.partial.p; ga.n_chunks = n_chunks; ga.ref_node = T.sons[T.sons_ptr[T.root]];
   a.I = w.I.p; a.nodes = w.query.p; a.n_query = nq; a.n_lab = n_lab; a.site = w.site.p;
   if (site_counts && !nodes)      // (the root's rows)
      for (int l = 0; l < n_lab; l++) std::fill_n(site_counts + ((size_t)l * nn + T.root) * e->n_patt, (size_t)e->n_patt, 0.0);
   if (int rc = anc_batches(
          e, w, m, &ga.chunk0, batch, [&](const AncBatch &b) { hipLaunchKernelGGL(mg_mfma_outer_kernel, b.tiles, dim3(256), 0, st, ga); },
          [&](const AncBatch &b, int pass) { anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(counts_pass_kernel<N()>, b.lanes, dim3(256), 0, st, ga, pass); }); },
          [&](const AncBatch &b) {
             const unsigned lanes = b.lanes.x;
             hipLaunchKernelGGL(counts_scalar_kernel, dim3(lanes), dim3(256), 0, st, ga);
             HIPCHK(hipGetLastError());
             hipLaunchKernelGGL(mg_rows_kernel, dim3(lanes, 1), dim3(256), 0, st, ga);      // (row 0: w lnf)
             HIPCHK(hipGetLastError());
             if (mfma) hipLaunchKernelGGL(counts_mfma_kernel, dim3(b.tiles.x, nq), dim3(256), 0, st, a);
             else anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(counts_lane_kernel<N()>, dim3(lanes, nq), dim3(256), 0, st, a); });
             HIPCHK(hipGetLastError());
             hipLaunchKernelGGL(counts_rows_kernel, dim3(lanes, n_rows), dim3(256), 0, st, a);
             HIPCHK(hipGetLastError());
             return 0;
          },
          [&](const AncBatch &b) {
             if (lnf) HIPCHK(hipMemcpyAsync(lnf + b.h0, w.lnf.p, (size_t)b.nb * 8, hipMemcpyDeviceToHost, st));
             if (site_counts)      // runs of rows that are consecutive on both sides, one strided copy each
                for (int r0 = 0; r0 < n_rows;) {
                   const int l0 = r0 / nq, q0 = r0 % nq;
                   const long d0 = (long)l0 * n_out + col[q0];
                   int r1 = r0 + 1;
                   while (r1 < n_rows && (long)(r1 / nq) * n_out + col[r1 % nq] == d0 + (r1 - r0)) r1++;
                   HIPCHK(hipMemcpy2DAsync(site_counts + (size_t)d0 * e->n_patt + b.h0, (size_t)e->n_patt * 8, w.site.p + (size_t)r0 * batch, (size_t)batch * 8, (size_t)b.nb * 8,
                                           (size_t)(r1 - r0), hipMemcpyDeviceToHost, st));
                   r0 = r1;
                }
             return 0;
          }))
      return rc;
   std::vector<double> out((size_t)1 + n_rows);
   if (int rc = anc_totals(e, w, w.partial.p, n_chunks, w.out.p, out)) return rc;
   *lnL = out[0];
   std::fill_n(counts, (size_t)n_lab * n_out, 0.0);
   for (int l = 0; l < n_lab; l++)
      for (int qi = 0; qi < nq; qi++) counts[(size_t)l * n_out + col[qi]] = out[(size_t)1 + (size_t)l * nq + qi];
   return 0;
}
