// engine_ancestral.hip — ancestral reconstruction at every internal node in one call: marginal (AncestralMarginal / PostProbNode,
// treesub.c:6288, 6142) and joint (AncestralJointPPSG2000 treesub.c:6964); the definitions in kernels_ancestral.h, the kernels here.
// P(t) comes from the evaluation's own builders (launch_pmat, engine_eval.hip).  Also the host side every whole-tree call shares
// (ancestral_host.h) and the one the score calls share on top of it (score_host.h).
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "kernels_ancestral.h"
#include "kernels_curvature.h"
#include "score_host.h"

static thread_local AncCallInfo anc_info;

extern "C" void paml_amd_ancestral_info(int *last_batches, double *last_kernel_ms) { anc_info.read(last_batches, last_kernel_ms); }

namespace paml_amd {

// lnP = log(max(P, 1e-300)) of n_p entries, then lnpi of n_q
__global__ __launch_bounds__(256) void anc_log_kernel(const double *P, long n_p, const double *pi, long n_q, double *lnP, double *lnpi)
{
   const long i = (long)blockIdx.x * 256 + threadIdx.x;
   if (i < n_p) lnP[i] = log(fmax(P[i], 1e-300));
   else if (i < n_p + n_q) lnpi[i - n_p] = log(fmax(pi[i - n_p], 1e-300));
}

// one pattern per lane: grid (patterns / 256, K)
template <int N> __global__ __launch_bounds__(256) void anc_lane_kernel(AncMargArgs a, int outer)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.nb) return;
   if (outer) anc_lane_outer<N>(a, blockIdx.y, p);
   else anc_lane_down<N>(a, blockIdx.y, p);
}

// grid (patterns / 256, n_query)
__global__ __launch_bounds__(256) void anc_posterior_kernel(AncMargArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.nb) return;
   anc_posterior(a, blockIdx.y, p);
}

// grid (stride / ANC_TILE, K); outer = 0: the down pass, 1: the outer pass
__global__ __launch_bounds__(256) void anc_mfma_kernel(AncMargArgs a, int outer)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   const AncTree &t = a.t;
   const int tid = threadIdx.x, lane = tid & 63, n = a.n;
   const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
   const int q = lane >> 4, k = blockIdx.y;
   const AncMfma w{sP, lane, wave, q};
   const long g16 = (long)blockIdx.x * 4 + wave, p = g16 * 16 + (lane & 15);
   const bool valid = p < a.nb;
   const long pc = valid ? p : a.nb - 1;
   const long pset = (long)a.gene * a.K + k;
   if (!outer) {
      for (int i = 0; i < t.n_post; i++) {
         const int v = t.post[i];
         if (v < t.n_tips) continue;
         double x[16], ls = 0;
#pragma unroll
         for (int m = 0; m < 16; m++) x[m] = 4 * m + q < n ? 1.0 : 0.0;
         for (int j = t.sons_ptr[v]; j < t.sons_ptr[v + 1]; j++) anc_mfma_mul_son(a, w, k, g16, pc, t.sons[j], x, &ls);
         if (a.scaled && t.scale[v]) {
            const double mx = anc_mfma_max(x);
            if (mx < 1e-300) {
#pragma unroll
               for (int m = 0; m < 16; m++) x[m] = 4 * m + q < n ? 1.0 : 0.0;
               ls += -800;
            }
            else {
#pragma unroll
               for (int m = 0; m < 16; m++) x[m] /= mx;
               ls += log(mx);
            }
         }
         const int vi = v - t.n_tips;
         part_store(a.L + (((long)k * t.n_int + vi) * (a.stride >> 4) + g16) * 1024, lane, x);
         if (q == 0) a.SL[((long)k * t.n_int + vi) * a.stride + p] = ls;      // (p < stride: the padding takes the lanes past the end)
      }
      return;
   }
   if (t.root >= t.n_tips) {
      const int ri = t.root - t.n_tips;
      double x[16];
#pragma unroll
      for (int m = 0; m < 16; m++) x[m] = 4 * m + q < n ? 1.0 : 0.0;
      part_store(a.G + (((long)k * t.n_int + ri) * (a.stride >> 4) + g16) * 1024, lane, x);
      if (q == 0) a.SG[((long)k * t.n_int + ri) * a.stride + p] = 0;
   }
   for (int i = 0; i < t.n_pre; i++) {
      const int v = t.pre[i], f = t.father[v], vi = v - t.n_tips;
      double h[16], ls = 0;
      __syncthreads();      // (SG of the father was stored by the pattern's q = 0 lane: a workgroup-scope fence before the other lanes read it)
      if (f >= t.n_tips) {
         const int fi = f - t.n_tips;
         part_load(a.G + (((long)k * t.n_int + fi) * (a.stride >> 4) + g16) * 1024, lane, h);      // (this lane's own stores)
         ls = a.SG[((long)k * t.n_int + fi) * a.stride + pc];
      }
      else {
         const unsigned long long mask = a.code_mask[a.z[(long)f * a.z_stride + a.h0 + pc]];
#pragma unroll
         for (int m = 0; m < 16; m++) h[m] = (mask >> (4 * m + q)) & 1ull ? 1.0 : 0.0;
      }
      for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
         if (t.sons[j] != v) anc_mfma_mul_son(a, w, k, g16, pc, t.sons[j], h, &ls);
      v4d acc[4];
      w.product(a.pint + (pset * t.n_nodes + v) * 4096, h, acc);
      double g[16];
#pragma unroll
      for (int m = 0; m < 16; m++) g[m] = acc[m >> 2][m & 3];
      if (a.scaled) {
         const double mx = anc_mfma_max(g);
         if (mx > 0) {
#pragma unroll
            for (int m = 0; m < 16; m++) g[m] /= mx;
            ls += log(mx);
         }
      }
      part_store(a.G + (((long)k * t.n_int + vi) * (a.stride >> 4) + g16) * 1024, lane, g);
      if (q == 0) a.SG[((long)k * t.n_int + vi) * a.stride + p] = ls;
   }
}

// joint: grid (patterns / ANC_JTILE); dynamic LDS: the node's n^2 doubles (n <= 64: 32 KB at most)
__global__ __launch_bounds__(ANC_JTILE) void anc_joint_kernel(AncJointArgs a)
{
   extern __shared__ __attribute__((aligned(16))) double anc_lds[];
   const AncTree &t = a.t;
   const int tid = threadIdx.x, n2 = a.n * a.n;
   const long p = (long)blockIdx.x * ANC_JTILE + tid;
   const bool on = p < a.nb;      // (lanes past the end keep to the barriers and touch no memory)
   for (int i = 0; i + 1 < t.n_post; i++) {      // (the root is the last entry)
      const int v = t.post[i];
      const double *lnPv = a.lnP + ((long)a.gene * t.n_nodes + v) * n2;
      __syncthreads();      // (the previous node's table is no longer read)
      for (int idx = tid; idx < n2; idx += ANC_JTILE) anc_lds[idx] = lnPv[idx];
      __syncthreads();
      if (on) anc_joint_up(a, v, p, anc_lds);
   }
   if (on) anc_joint_root_down(a, p);
}

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
   HIPCHK(w.ev0.ensure());
   HIPCHK(w.ev1.ensure());
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

// the end of what a call queued behind anc_pmat's ev0: waited for, its kernel time added to the call's, then the builder's verdict
int anc_pmat_wait(paml_amd_engine *e, AncScratch &w)
{
   HIPCHK(hipEventRecord(w.ev1, e->stream));
   HIPCHK(w.lap(e->stream));
   return eigen_fail_check(e);
}

// anc_pmat, waited for
int anc_pmat_waited(paml_amd_engine *e, const char *who, const double *branch, const double *gene_rate, AncScratch &w, const int *d_label)
{
   if (int rc = anc_pmat(e, who, branch, gene_rate, w, d_label)) return rc;
   return anc_pmat_wait(e, w);
}

// Keeps what the kernels need of the builder's present output before the builder runs again, waited for.  Matrix cores: the A-operand
// blocks with the tips' column tables (pint with ptip) and / or the transposed blocks of every node but the root (PT); a null buffer:
// not kept.  Lanes: the row-major matrices (P).
int anc_keep_pmat(paml_amd_engine *e, DevBuf<double> *pint, DevBuf<double> *ptip, DevBuf<double> *PT, DevBuf<double> &P)
{
   const int nn = e->tree.n_nodes, n = e->n;
   const size_t psets = (size_t)e->n_genes * e->K, pn = psets * nn, tw = tip_words(e);
   hipStream_t st = e->stream;
   if (e->kk != KK_MFMA64) {
      HIPCHK(P.ensure(pn * n * n));
      HIPCHK(hipMemcpyAsync(P.p, e->d_rowmajor.p, pn * n * n * 8, hipMemcpyDeviceToDevice, st));
   }
   else {
      if (pint) {
         HIPCHK(pint->ensure(pn * 4096));
         HIPCHK(ptip->ensure(pn * tw));
      }
      if (PT) HIPCHK(PT->ensure(pn * 4096));
      if (pint) {
         HIPCHK(hipMemcpyAsync(pint->p, e->d_pint.p, pn * 4096 * 8, hipMemcpyDeviceToDevice, st));
         HIPCHK(hipMemcpyAsync(ptip->p, e->d_ptip.p, pn * tw * 8, hipMemcpyDeviceToDevice, st));
      }
      if (PT) {
         hipLaunchKernelGGL(nni_pt_all_kernel, dim3(nn, (unsigned)psets), dim3(256), 0, st, (const double *)e->d_rowmajor.p, PT->p, n, nn, e->tree.root);
         HIPCHK(hipGetLastError());
      }
   }
   HIPCHK(hipStreamSynchronize(st));
   return 0;
}

// the workspace a call may take, in MiB (the variable `env`; default 256)
double anc_arena_mb(const char *env)
{
   double arena_mb = 256;
   if (const char *s = getenv(env)) { const double v = atof(s); if (v > 0) arena_mb = v; }
   return arena_mb;
}

// patterns per batch: what the workspace holds at `bytes_per_patt`, whole tiles, at least one
long anc_batch(double bytes_per_patt, long n_patt, const char *env)
{
   const double arena_mb = anc_arena_mb(env);
   long batch = (long)(arena_mb * 1048576.0 / bytes_per_patt) / ANC_JTILE * ANC_JTILE;
   if (batch < ANC_JTILE) batch = (long)(arena_mb * 1048576.0 / bytes_per_patt) / ANC_TILE * ANC_TILE;
   if (batch > (1L << 24)) batch = 1L << 24;
   if (batch < ANC_TILE) batch = ANC_TILE;
   const long all = (n_patt + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   return batch > all ? all : batch;
}

// the batch workspace, in the order listed: the batch is halved until all of it fits
int anc_alloc(paml_amd_engine *e, const char *who, const std::vector<AncBatchBuf> &bufs, long *batch)
{
   for (;;) {
      bool ok = true;
      for (const AncBatchBuf &b : bufs) ok = ok && b.ensure(b.buf, b.per_patt * *batch) == hipSuccess;
      if (ok) return 0;
      (void)hipGetLastError();
      for (const AncBatchBuf &b : bufs) b.release(b.buf);      // (ensure only grows: the retry starts from nothing)
      if (*batch <= ANC_TILE) return fail(e, PAML_AMD_ENOMEM, std::string(who) + ": no device memory for one tile of patterns");
      *batch = (*batch / 2 + ANC_TILE - 1) / ANC_TILE * ANC_TILE;
   }
}

// what the down pass and the outer passes read of the engine, and the call's partials (the batch itself is the batch loop's to name)
void anc_fill(const paml_amd_engine *e, const AncScratch &w, long batch, AncMargArgs &m)
{
   m.n = e->n; m.K = e->K; m.scaled = e->tree.n_scale > 0 ? 1 : 0; m.n_pi = e->n_pi; m.stride = batch;
   m.z = e->d_z.p; m.z_stride = e->n_patt; m.code_mask = e->d_code_mask.p;
   m.P = e->d_rowmajor.p; m.pint = e->d_pint.p; m.ptip = e->d_ptip.p; m.tip_words = (long)tip_words(e);
   m.pi = e->d_pi_plain.p; m.freqK = e->d_freqK.p;
   m.L = w.L.p; m.G = w.G.p; m.SL = w.SL.p; m.SG = w.SG.p; m.mfma = e->kk == KK_MFMA64 ? 1 : 0;
}

// chunks of GRAD_CHUNK patterns counted from each gene's first pattern (a batch is whole chunks of one gene): [g] = gene g's first
// chunk, [n_genes] = the chunks of the engine
std::vector<long> anc_chunk_base(const paml_amd_engine *e)
{
   std::vector<long> chunk_base(e->n_genes + 1, 0);
   for (int g = 0; g < e->n_genes; g++) chunk_base[g + 1] = chunk_base[g] + (e->gene_off[g + 1] - e->gene_off[g] + GRAD_CHUNK - 1) / GRAD_CHUNK;
   return chunk_base;
}

// out[i] = the chunks of row i of `partial` added in a fixed order (grad_total_kernel), for out.size() rows: downloaded and waited for
int anc_totals(paml_amd_engine *e, AncScratch &w, const double *partial, long n_chunks, double *d_out, std::vector<double> &out)
{
   hipStream_t st = e->stream;
   HIPCHK(hipEventRecord(w.ev0, st));
   hipLaunchKernelGGL(grad_total_kernel, dim3((unsigned)out.size()), dim3(256), 0, st, partial, n_chunks, d_out);
   HIPCHK(hipGetLastError());
   HIPCHK(hipEventRecord(w.ev1, st));
   HIPCHK(hipMemcpyAsync(out.data(), d_out, out.size() * 8, hipMemcpyDeviceToHost, st));
   HIPCHK(w.lap(st));
   return 0;
}

int anc_common_checks(paml_amd_engine *e, const char *who)
{
   if (!(e->have_tips && e->have_tree && e->have_pi && e->have_classes) || e->eigen.empty())
      return fail(e, PAML_AMD_EINVAL, std::string(who) + " before set_tips/set_tree/set_pi/set_classes/set_eigen");
   if (e->n > 64) return fail(e, PAML_AMD_EUNSUPPORTED, std::string(who) + ": more than 64 states");
   return 0;
}


// What the score calls refuse before they allocate, in this order: anc_common_checks, more than one rank, a rate-matrix (UNREST) set
// with the caller's sentence for it (`unrest_reason`; null: such sets are allowed).
int score_begin(paml_amd_engine *e, const char *who, const char *unrest_reason)
{
   if (int rc = anc_common_checks(e, who)) return rc;
   if (e->world > 1) return fail(e, PAML_AMD_EUNSUPPORTED, std::string(who) + ": one rank only (this engine's communicator has " + std::to_string(e->world) + ")");
   for (size_t i = 0; unrest_reason && i < e->eigen.size(); i++)
      if (e->eigen[i].kind == PAML_AMD_EIGEN_QMAT) return fail(e, PAML_AMD_EUNSUPPORTED, std::string(who) + ": " + unrest_reason);
   return 0;
}

// What the derivative calls refuse: the same, then a tree without a branch.
int anc_begin(paml_amd_engine *e, const char *who, const char *unrest_reason)
{
   if (int rc = score_begin(e, who, unrest_reason)) return rc;
   if (e->tree.n_nodes < 2) return fail(e, PAML_AMD_EINVAL, std::string(who) + ": the tree has no branch");
   return 0;
}

// what the kernels that build P(t) and its derivatives read of the engine (a call adds its own outputs)
GradPmatArgs grad_pmat_args(const paml_amd_engine *e)
{
   GradPmatArgs ga{};
   ga.n = e->n; ga.K = e->K; ga.n_nodes = e->tree.n_nodes; ga.n_tips = e->n_tips; ga.root = e->tree.root; ga.n_labels = e->n_labels;
   ga.rate_gs = e->rate_per_gene ? e->K : 0; ga.mfma = e->kk == KK_MFMA64 ? 1 : 0;
   ga.label = e->d_label.p; ga.eigen_of = e->d_eigen_of.p; ga.eigen = e->d_eigen.p;
   ga.branch = e->d_branch.p; ga.rate = e->d_rate.p; ga.gene_rate = e->d_gene_rate.p; ga.qfactor = e->d_qfactor.p;
   ga.P = e->d_rowmajor.p;
   return ga;
}

// dP (and d2P when asked for: curv_pmat_kernel instead of grad_pmat_kernel) of every (parameter set, node) behind anc_pmat's P(t), and on
// the matrix cores P^T: the buffers sized, one launch
int grad_dpmat(paml_amd_engine *e, DevBuf<double> &dP, DevBuf<double> *d2P, DevBuf<double> &PT)
{
   const int nn = e->tree.n_nodes, n = e->n, K = e->K, G = e->n_genes;
   const bool mfma = e->kk == KK_MFMA64;
   const size_t pn = (size_t)G * K * nn, each = mfma ? 4096 : (size_t)n * n;
   HIPCHK(dP.ensure(pn * each));
   if (d2P) HIPCHK(d2P->ensure(pn * each));
   if (mfma) HIPCHK(PT.ensure(pn * 4096));
   GradPmatArgs ga = grad_pmat_args(e);
   ga.dP = dP.p; ga.PT = PT.p; ga.d2P = d2P ? d2P->p : nullptr;
   if (d2P) hipLaunchKernelGGL(curv_pmat_kernel, dim3(nn, G * K), dim3(256), 0, e->stream, ga);
   else hipLaunchKernelGGL(grad_pmat_kernel, dim3(nn, G * K), dim3(256), 0, e->stream, ga);
   HIPCHK(hipGetLastError());
   return 0;
}

// ---- the score calls' host side (score_host.h) ----------------------------------------------------------------------------------

// [v] = the father of v (-1: none)
std::vector<int> score_fathers(const TreeDesc &T)
{
   std::vector<int> father(T.n_nodes, -1);
   for (int v = 0; v < T.n_nodes; v++)
      for (int j = T.sons_ptr[v]; j < T.sons_ptr[v + 1]; j++) father[T.sons[j]] = v;
   return father;
}

bool score_son_of(const TreeDesc &T, int s, int v)
{
   for (int j = T.sons_ptr[v]; j < T.sons_ptr[v + 1]; j++)
      if (T.sons[j] == s) return true;
   return false;
}

// the node v of a row (`at`: the message's prefix, "call: row i: "): refused out of range, as a tip where the call has no use for one, and
// as the root (`father`: a node without a father counts as one; null: the tree's root only)
int score_check_node(paml_amd_engine *e, const std::string &at, int v, const std::vector<int> *father, bool tips_refused)
{
   const TreeDesc &T = e->tree;
   if (v < 0 || v >= T.n_nodes) return fail(e, PAML_AMD_EINVAL, at + "node " + std::to_string(v) + " is out of range");
   if (tips_refused && T.is_leaf(v)) return fail(e, PAML_AMD_EINVAL, at + "node " + std::to_string(v) + " is a tip");
   if (v == T.root || (father && (*father)[v] < 0)) return fail(e, PAML_AMD_EINVAL, at + "node " + std::to_string(v) + " is the root");
   return 0;
}

// query qi's row of character codes ([.][n_patt] in qz) in the engine's own numbering, into the same place of dst
int score_query_codes(paml_amd_engine *e, const std::string &prefix, int qi, const unsigned char *qz, unsigned char *dst)
{
   const long n_patt = e->n_patt;
   for (long h = 0; h < n_patt; h++) {
      const int c = qz[(size_t)qi * n_patt + h];
      if (c >= e->n_codes || e->code_nch[c] < 1)
         return fail(e, PAML_AMD_EINVAL, prefix + "query " + std::to_string(qi) + ", pattern " + std::to_string(h) + ": character code " + std::to_string(c) +
                                             (c >= e->n_codes ? " >= n_codes" : " has an empty state set"));
      dst[(size_t)qi * n_patt + h] = e->code_new_of[c];
   }
   return 0;
}

// The present tree's matrices: anc_pmat, and on the matrix cores P^T of the internal nodes (all_nodes: of every node but the root) behind
// it.  The caller queues its own uploads and kernels, then anc_pmat_wait (what it uploads is on its stack), then sets pmat_valid.
int score_present_pmat(paml_amd_engine *e, const char *who, const double *branch, const double *gene_rate, ScoreScratch &w, const int *d_label, bool all_nodes)
{
   if (int rc = anc_pmat(e, who, branch, gene_rate, w, d_label)) return rc;
   if (e->kk != KK_MFMA64) return 0;
   const int nn = e->tree.n_nodes, psets = e->n_genes * e->K;
   HIPCHK(w.PT.ensure((size_t)psets * nn * 4096));
   if (all_nodes) hipLaunchKernelGGL(nni_pt_all_kernel, dim3(nn, psets), dim3(256), 0, e->stream, (const double *)e->d_rowmajor.p, w.PT.p, e->n, nn, e->tree.root);
   else hipLaunchKernelGGL(nni_pt_kernel, dim3(nn, psets), dim3(256), 0, e->stream, (const double *)e->d_rowmajor.p, w.PT.p, e->n, nn, e->n_tips, e->tree.root);
   HIPCHK(hipGetLastError());
   return 0;
}

// bytes per pattern of the partials and the messages of the tree (L, G, SL, SG); a partial takes 64 doubles on the matrix cores, else n
double score_fixed(const paml_amd_engine *e)
{
   return 2.0 * e->K * (e->tree.n_nodes - e->n_tips) * ((e->kk == KK_MFMA64 ? 64 : e->n) + 1) * 8;
}

// The workspace plan of a score call, and `partial` / `out` ([n_out + 1] rows) sized.  Per pattern the workspace (`env` MiB) holds `fixed`
// bytes (0: score_fixed) and per_row bytes for every row of a group and for the extra rows (the present tree's).  One tile of patterns
// with all n_rows does not fit: groups of as many rows as one tile has room for, at least one; a group has 65535 rows at most (the lanes'
// row pass has a grid layer per row).  cap > 0: the rows of a group by the caller's own rule.
int score_plan(paml_amd_engine *e, ScoreScratch &w, ScorePlan *plan, const char *env, double per_row, int n_rows, long n_out, int extra_rows, double fixed, int cap)
{
   const int K = e->K, n_int = e->tree.n_nodes - e->n_tips;
   plan->n_chunks = anc_chunk_base(e)[e->n_genes];
   HIPCHK(w.partial.ensure((size_t)(n_out + 1) * std::max<long>(plan->n_chunks, 1)));
   HIPCHK(w.out.ensure((size_t)n_out + 1));
   if (fixed == 0) fixed = score_fixed(e);
   if (!cap) {
      const double arena_mb = anc_arena_mb(env);
      cap = n_rows;
      if ((fixed + per_row * (n_rows + extra_rows)) * ANC_TILE > arena_mb * 1048576.0)
         cap = (int)std::min<double>(n_rows, std::max(1.0, floor((arena_mb * 1048576.0 / ANC_TILE - fixed) / per_row) - extra_rows));
      cap = std::min(cap, 65535);
   }
   plan->cap = cap;
   plan->batch = anc_batch(fixed + per_row * (cap + extra_rows), e->n_patt, env);
   plan->part = (size_t)K * n_int * (e->kk == KK_MFMA64 ? 64 : e->n);
   plan->sc = (size_t)K * n_int;
   return 0;
}

// the batch workspace: L, G, SL, SG of the plan, then the call's own buffers (anc_alloc: the plan's batch is halved until all of it fits)
int score_alloc(paml_amd_engine *e, const char *who, ScoreScratch &w, ScorePlan &plan, std::initializer_list<AncBatchBuf> own)
{
   std::vector<AncBatchBuf> bufs{{&w.L, plan.part}, {&w.G, plan.part}, {&w.SL, plan.sc}, {&w.SG, plan.sc}};
   bufs.insert(bufs.end(), own.begin(), own.end());
   return anc_alloc(e, who, bufs, &plan.batch);
}

// what the passes of the present tree and the combining kernels read: anc_fill, and the rows' workspace ([K][cap + 1][batch], row `cap`
// the present tree's), the chunks' sums, the root's first son (where the present tree's f_hk is taken)
void score_fill(NniArgs &o, const ScoreScratch &w, const paml_amd_engine *e, const ScorePlan &plan, int n_rows)
{
   anc_fill(e, w, plan.batch, o.m);
   o.PT = w.PT.p; o.cap = plan.cap; o.n_swaps = n_rows; o.f = w.f.p; o.sig = w.sig.p; o.weights = e->d_weights.p;
   o.lnf = w.lnf.p; o.partial = w.partial.p; o.n_chunks = plan.n_chunks;
   o.ref_node = e->tree.sons[e->tree.sons_ptr[e->tree.root]];
}

// anc_totals of `partial` ([vals.size() n_rows + 1][n_chunks]: value d of row i at d n_rows + i, the present tree last), scattered:
// vals[d][index_of[i]] (null: [i]) and *lnL0
int score_totals(paml_amd_engine *e, ScoreScratch &w, const ScorePlan &plan, long n_rows, const int *index_of, double *lnL0, std::initializer_list<double *> vals)
{
   std::vector<double> out(vals.size() * (size_t)n_rows + 1);
   if (int rc = anc_totals(e, w, w.partial.p, plan.n_chunks, w.out.p, out)) return rc;
   size_t d = 0;
   for (double *dst : vals) {
      for (long i = 0; i < n_rows; i++) dst[index_of ? index_of[i] : i] = out[d * (size_t)n_rows + i];
      d++;
   }
   *lnL0 = out.back();
   return 0;
}

}  // namespace paml_amd

extern "C" int paml_amd_ancestral_marginal(paml_amd_engine *e, const double *branch, const double *gene_rate, int n_query, const int *nodes,
                                           unsigned char *best, double *best_prob, double *post)
{
   enter(e);
   anc_info = AncCallInfo{};
   const char *who = "ancestral_marginal";
   if (!e || !branch || !best || !best_prob) return fail(e, PAML_AMD_EINVAL, "ancestral_marginal: null argument");
   if (int rc = anc_common_checks(e, who)) return rc;
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, n_tips = e->n_tips, n_int = nn - n_tips;
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
   AncScratch w(anc_info);
   AncMargArgs a{};
   if (int rc = anc_tree_pack(e, who, w, &a.t)) return rc;
   HIPCHK(upload(w.query, query.data(), query.size(), st));
   HIPCHK(hipStreamSynchronize(st));
   if (int rc = anc_pmat_waited(e, who, branch, gene_rate, w)) return rc;

   const int ns = mfma ? 64 : n;      // doubles a partial takes per pattern
   const double per_patt = 2.0 * K * n_int * (ns + 1) * 8 + (double)nq * (n * 8 + 9);
   long batch = anc_batch(per_patt, e->n_patt);
   {
      const size_t part = (size_t)K * n_int * ns, sc = (size_t)K * n_int;
      if (int rc = anc_alloc(e, who, {{&w.L, part}, {&w.G, part}, {&w.SL, sc}, {&w.SG, sc}, {&w.post, (size_t)nq * n}, {&w.prob, (size_t)nq}, {&w.best, (size_t)nq}}, &batch)) return rc;
   }
   anc_fill(e, w, batch, a);
   a.n_query = nq; a.query = w.query.p; a.post = w.post.p; a.best_prob = w.prob.p; a.best = w.best.p;
   const long n_patt = e->n_patt;
   return anc_batches(
      e, w, a, nullptr, batch, [&](const AncBatch &b) { hipLaunchKernelGGL(anc_mfma_kernel, b.tiles, dim3(256), 0, st, a, 1); },
      [&](const AncBatch &b, int pass) { anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(anc_lane_kernel<N()>, b.lanes, dim3(256), 0, st, a, pass); }); },
      [&](const AncBatch &b) {
         hipLaunchKernelGGL(anc_posterior_kernel, dim3(b.lanes.x, nq), dim3(256), 0, st, a);
         HIPCHK(hipGetLastError());
         return 0;
      },
      [&](const AncBatch &b) {      // the batch's rows to the caller's [n_query][n_patt]( [n] ): one plain copy per queried node (no pitch that n_patt could outgrow)
         for (int qi = 0; qi < nq; qi++) {
            HIPCHK(hipMemcpyAsync(best + (size_t)qi * n_patt + b.h0, w.best.p + (size_t)qi * batch, (size_t)b.nb, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(best_prob + (size_t)qi * n_patt + b.h0, w.prob.p + (size_t)qi * batch, (size_t)b.nb * 8, hipMemcpyDeviceToHost, st));
            if (post)
               HIPCHK(hipMemcpyAsync(post + ((size_t)qi * n_patt + b.h0) * n, w.post.p + (size_t)qi * batch * n, (size_t)b.nb * n * 8, hipMemcpyDeviceToHost, st));
         }
         return 0;
      });
}

extern "C" int paml_amd_ancestral_joint(paml_amd_engine *e, const double *branch, const double *gene_rate, unsigned char *states, double *ln_best)
{
   enter(e);
   anc_info = AncCallInfo{};
   const char *who = "ancestral_joint";
   if (!e || !branch || !states || !ln_best) return fail(e, PAML_AMD_EINVAL, "ancestral_joint: null argument");
   if (int rc = anc_common_checks(e, who)) return rc;
   if (e->K != 1) return fail(e, PAML_AMD_EUNSUPPORTED, "ancestral_joint: one class only (this model has " + std::to_string(e->K) + ")");
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, G = e->n_genes, n_tips = e->n_tips, n_int = nn - n_tips;
   if (n_int < 1) return fail(e, PAML_AMD_EINVAL, "ancestral_joint: the tree has no internal node");
   hipStream_t st = e->stream;
   AncScratch w(anc_info);
   AncJointArgs a{};
   if (int rc = anc_tree_pack(e, who, w, &a.t)) return rc;
   if (int rc = anc_pmat(e, who, branch, gene_rate, w)) return rc;
   const long n_p = (long)G * nn * n * n, n_q = (long)e->n_pi * n;
   HIPCHK(w.lnP.ensure((size_t)(n_p + n_q)));
   hipLaunchKernelGGL(anc_log_kernel, dim3((unsigned)((n_p + n_q + 255) / 256)), dim3(256), 0, st, (const double *)e->d_rowmajor.p, n_p, (const double *)e->d_pi_plain.p, n_q, w.lnP.p, w.lnP.p + n_p);
   HIPCHK(hipGetLastError());
   if (int rc = anc_pmat_wait(e, w)) return rc;
   e->pmat_valid = true;

   const double per_patt = (double)n_int * n * 9 + n_int + 1 + 8;
   long batch = anc_batch(per_patt, e->n_patt);
   if (int rc = anc_alloc(e, who, {{&w.L, (size_t)n_int * n}, {&w.C, (size_t)n_int * n}, {&w.state, (size_t)n_int}, {&w.rootstate, 1}, {&w.lnbest, 1}}, &batch)) return rc;
   a.n = n; a.stride = batch; a.z = e->d_z.p; a.z_stride = e->n_patt; a.code_mask = e->d_code_mask.p;
   a.lnP = w.lnP.p; a.L = w.L.p; a.C = w.C.p; a.state = w.state.p; a.rootstate = w.rootstate.p; a.ln_best = w.lnbest.p;
   const long n_patt = e->n_patt;
   const size_t lds = (size_t)n * n * sizeof(double);
   return anc_batches(
      e, w, a, nullptr, batch, nullptr, nullptr,      // (one kernel walks the tree up and down: no two passes)
      [&](const AncBatch &b) {
         a.lnpi = w.lnP.p + n_p + (long)(e->n_pi > 1 ? b.gene : 0) * n;
         hipLaunchKernelGGL(anc_joint_kernel, dim3((unsigned)((b.nb + ANC_JTILE - 1) / ANC_JTILE)), dim3(ANC_JTILE), lds, st, a);
         HIPCHK(hipGetLastError());
         return 0;
      },
      [&](const AncBatch &b) {
         for (int vi = 0; vi < n_int; vi++)
            HIPCHK(hipMemcpyAsync(states + (size_t)vi * n_patt + b.h0, w.state.p + (size_t)vi * batch, (size_t)b.nb, hipMemcpyDeviceToHost, st));
         HIPCHK(hipMemcpyAsync(ln_best + b.h0, w.lnbest.p, (size_t)b.nb * 8, hipMemcpyDeviceToHost, st));
         return 0;
      });
}
