// engine_attach.hip — the lnL of the tree with a query tip hung on a branch at free lengths of the three branches around the new node,
// with the first and second derivative along one of them, for many rows in one call (paml_amd_attach_scores); the definition in
// kernels_attach.h, the kernels here.  The tree's own P(t) comes from the evaluation's builders (anc_pmat, engine_ancestral.hip), the
// rows' matrices from the edge call's formulas (edge_pmat_fill, kernels_edge.h), the down pass is the ancestral module's, the outer pass
// is the NNI call's, the classes meet in edge_combine.
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include <algorithm>

#include "engine_state.h"
#include "kernels_attach.h"
#include "ancestral_host.h"

static thread_local AncCallInfo attach_info;

extern "C" void paml_amd_attach_info(int *last_batches, double *last_kernel_ms) { attach_info.read(last_batches, last_kernel_ms); }

namespace paml_amd {

// where M[y][x] lives in a block of 4096 in the A-operand order (the index formula of edge_pmat_fill, inverted)
__device__ __forceinline__ int attach_aop_index(int y, int x)
{
   const int mm = x >> 2;
   return ((((mm >> 1) * 4 + (y >> 4)) * 64 + (y & 15) + 16 * (x & 3)) << 1) | (mm & 1);
}

// the column table of matrix M (A-operand order): T[c][y] = sum_{x in set(c)} M[y][x], ascending x, in the layout tip_gather reads
// (row = code * 4 + y % 4, sixteen doubles, piece i in slot i ^ TIP_SWZ(row)); states from n on: 0.  By a workgroup of 256.
__device__ __forceinline__ void attach_table_fill(const double *M, int n, int n_codes, const unsigned long long *code_mask, double *tab)
{
   for (int idx = threadIdx.x; idx < n_codes * 64; idx += 256) {
      const int code = idx >> 6, y = idx & 63;
      const unsigned long long mask = code_mask[code];
      double s = 0;
      if (y < n)
         for (int x = 0; x < n; x++)
            if ((mask >> x) & 1ull) s += M[attach_aop_index(y, x)];
      const int row = code * 4 + (y & 3), j = y >> 2;
      tab[row * 16 + ((((j >> 1) ^ TIP_SWZ(row)) << 1) | (j & 1))] = s;
   }
}

// P(t) of every (row, branch of the new node, parameter set), and dP, d^2P for the branch of the role: grid (rows x 3, gene x class).
// Matrix cores: the A-operand order, transposed for the up branch, and the column tables of the pendant and of a tip's dn branch.
__global__ __launch_bounds__(256) void attach_pmat_kernel(AttachPmatArgs a)
{
   const GradPmatArgs &g = a.g;
   const int row = blockIdx.x / 3, slot = blockIdx.x % 3, pset = blockIdx.y;
   const int v = a.rows[4L * row], role = a.rows[4L * row + 2];
   const bool with_d = role == slot;
   __shared__ double sE[64], sM[64];
   double *am = a.AM + ((long)row * a.psets + pset) * ATTACH_MATS * a.msz;
   double *P = am + slot * a.msz, *dP = am + 3 * a.msz, *ddP = am + 4 * a.msz;
   edge_pmat_fill<true>(g, pset, slot == 2 ? a.pendant_label : g.label[v], a.t3[3L * row + slot], with_d, g.mfma && slot == 0, sE, sM, P, dP, ddP);
   if (!g.mfma || slot == 0 || (slot == 1 && v >= g.n_tips)) return;      // (uniform over the workgroup)
   __syncthreads();      // (the tables read what the workgroup's other lanes stored)
   double *at = a.AT + ((long)row * a.psets + pset) * ATTACH_TABS * a.tip_words;
   attach_table_fill(P, g.n, a.n_codes, a.code_mask, at + (slot - 1) * a.tip_words);
   if (with_d) {
      attach_table_fill(dP, g.n, a.n_codes, a.code_mask, at + 2 * a.tip_words);
      attach_table_fill(ddP, g.n, a.n_codes, a.code_mask, at + 3 * a.tip_words);
   }
}

// one pattern per lane, the row pass: grid (patterns / 256, K, rows of the group); the block of a row that starts a node's run walks the run
template <int N> __global__ __launch_bounds__(256) void attach_lane_kernel(AttachArgs a)
{
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   if (p >= a.e.o.m.nb || !attach_run_start(a, blockIdx.z)) return;
   attach_lane_node<N>(a, blockIdx.y, p, blockIdx.z);
}

// Matrix cores, the row pass: four waves own ANC_TILE patterns of one class and loop over the group's rows; H_v (h) and L_v (l) are
// formed where the node changes and held in registers over the node's rows.  Grid (stride / ANC_TILE, K).
__global__ __launch_bounds__(256) void attach_mfma_kernel(AttachArgs a)
{
   __shared__ __attribute__((aligned(16))) double sP[4096];
   const NniArgs &o = a.e.o;
   const AncMargArgs &m = o.m;
   const AncTree &t = m.t;
   const int tid = threadIdx.x, lane = tid & 63;
   const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
   const int q = lane >> 4, k = blockIdx.y;
   const AncMfma w{sP, lane, wave, q};
   const long g16 = (long)blockIdx.x * 4 + wave, p = g16 * 16 + (lane & 15);
   const long pc = p < m.nb ? p : m.nb - 1;      // (lanes past the batch's end read the last pattern and write into the padding: p < stride)
   const long pset = (long)m.gene * m.K + k;
   double h[16], l[16], ls = 0;
   int v_held = -1, vcode = 0;
   auto gather = [&](const double *tab, int code, double (&x)[16]) {
      double2 tv[8];
      tip_gather(tab, m.tip_words, 0, code, q, tv);
#pragma unroll
      for (int j = 0; j < 8; j++) { x[2 * j] = tv[j].x; x[2 * j + 1] = tv[j].y; }
   };
   for (int i = 0; i < o.n_group; i++) {
      const int *rw = a.rows + 4L * (o.swap0 + i);
      const int v = rw[0], role = rw[2];
      const bool tip = v < t.n_tips;
      if (v != v_held) {
         const int f = t.father[v];
         nni_mfma_father(m, k, g16, pc, lane, q, f, h, &ls);
         for (int j = t.sons_ptr[f]; j < t.sons_ptr[f + 1]; j++)
            if (t.sons[j] != v) anc_mfma_mul_son(m, w, k, g16, pc, t.sons[j], h, &ls);
         if (tip) vcode = (int)m.z[(long)v * m.z_stride + m.h0 + pc];
         else {
            part_load(m.L + (((long)k * t.n_int + v - t.n_tips) * (m.stride >> 4) + g16) * 1024, lane, l);
            ls += m.SL[((long)k * t.n_int + v - t.n_tips) * m.stride + pc];
         }
         v_held = v;
      }
      const int qcode = (int)a.qz[(long)rw[1] * m.z_stride + m.h0 + pc];
      const double *am = a.AM + ((long)(o.swap0 + i) * a.psets + pset) * ATTACH_MATS * 4096;
      const double *at = a.AT + ((long)(o.swap0 + i) * a.psets + pset) * ATTACH_TABS * m.tip_words;
      auto product = [&](const double *blk, const double (&x)[16], double (&y)[16]) {
         v4d acc[4];
         w.product(blk, x, acc);
#pragma unroll
         for (int j = 0; j < 16; j++) y[j] = acc[j >> 2][j & 3];
      };
      double u[16], d[16], tq[16], x[16], y[16], fd[3] = {0, 0, 0};
      product(am, h, u);      // U = P_v(t_up)^T H_v
      if (tip) gather(at, vcode, d);      // (uniform over the workgroup) D of a tip: its column table of P_v(t_dn)
      else product(am + 4096, l, d);
      gather(at + m.tip_words, qcode, tq);
#pragma unroll
      for (int j = 0; j < 16; j++) y[j] = u[j] * d[j];
      fd[0] = grad_mfma_dot(y, tq);
      for (int dd = 1; dd <= 2 && role >= 0; dd++) {      // (the role is the row's: uniform over the workgroup)
         const double *dm = am + (2 + dd) * 4096, *dt = at + (1 + dd) * m.tip_words;
         if (role == 0) {
            product(dm, h, x);
#pragma unroll
            for (int j = 0; j < 16; j++) y[j] = x[j] * d[j];
            fd[dd] = grad_mfma_dot(y, tq);
         }
         else if (role == 1) {
            if (tip) gather(dt, vcode, x);
            else product(dm, l, x);
#pragma unroll
            for (int j = 0; j < 16; j++) y[j] = u[j] * x[j];
            fd[dd] = grad_mfma_dot(y, tq);
         }
         else {
            gather(dt, qcode, x);
#pragma unroll
            for (int j = 0; j < 16; j++) y[j] = u[j] * d[j];
            fd[dd] = grad_mfma_dot(y, x);
         }
      }
      const long oi = nni_out_idx(o, k, i, p);
      if (q == 0) { o.f[oi] = fd[0]; a.e.f1[oi] = fd[1]; a.e.f2[oi] = fd[2]; o.sig[oi] = ls; }
   }
}

// the classes of every (row, pattern) and the chunks' sums of w lnf, w g1, w g2: grid (stride / 256, rows); a wave = one chunk of
// GRAD_CHUNK patterns.  partial: [3 n_rows + 1][n_chunks] = lnL, d1, d2 of the rows at the caller's index, then the present tree.
__global__ __launch_bounds__(256) void attach_combine_kernel(AttachArgs a)
{
   const NniArgs &o = a.e.o;
   const long p = (long)blockIdx.x * 256 + threadIdx.x;
   const bool present = (int)blockIdx.y == o.n_group;      // (a batch's first group is launched with a row more: the present tree)
   double acc[3] = {0, 0, 0};
   if (p < o.m.nb) {
      if (present) acc[0] = nni_combine(o, o.cap, p);
      else edge_combine(a.e, (int)blockIdx.y, p, acc);
   }
#pragma unroll
   for (int off = 32; off >= 1; off >>= 1) {
      acc[0] += __shfl_xor(acc[0], off);
      acc[1] += __shfl_xor(acc[1], off);
      acc[2] += __shfl_xor(acc[2], off);
   }
   const long chunk = o.chunk0 + (p >> 6);
   if ((threadIdx.x & 63) != 0 || (p & ~63L) >= o.m.nb) return;
   const long nr = o.n_swaps;
   if (present) { o.partial[3 * nr * o.n_chunks + chunk] = acc[0]; return; }
   const long out_row = a.rows[4L * (o.swap0 + blockIdx.y) + 3];
   for (int d = 0; d < 3; d++) o.partial[(d * nr + out_row) * o.n_chunks + chunk] = acc[d];
}
}  // namespace paml_amd

namespace {

struct AttachScratch : AncScratch {
   using AncScratch::AncScratch;
   DevBuf<double> PT, AM, AT, t3, f, f1, f2, sig, lnf, g1, g2, partial, out;
   DevBuf<int> rows;
   DevBuf<unsigned char> qz;
};

}  // namespace

extern "C" int paml_amd_attach_scores(paml_amd_engine *e, const double *branch, const double *gene_rate, int n_q, const unsigned char *qz, int n_rows, const int *rows,
                                      const double *t3, int pendant_label, double *lnL0, double *lnL, double *d1, double *d2, double *lnf)
{
   enter(e);
   attach_info = AncCallInfo{};
   const char *who = "attach_scores";
   if (!e || !branch || !qz || !rows || !t3 || !lnL0 || !lnL || !d1 || !d2) return fail(e, PAML_AMD_EINVAL, "attach_scores: null argument");
   if (n_q < 1) return fail(e, PAML_AMD_EINVAL, "attach_scores: n_q < 1");
   if (n_rows < 1) return fail(e, PAML_AMD_EINVAL, "attach_scores: n_rows < 1");
   if (int rc = anc_common_checks(e, who)) return rc;
   if (e->world > 1) return fail(e, PAML_AMD_EUNSUPPORTED, "attach_scores: one rank only (this engine's communicator has " + std::to_string(e->world) + ")");
   for (size_t i = 0; i < e->eigen.size(); i++)
      if (e->eigen[i].kind == PAML_AMD_EIGEN_QMAT)
         return fail(e, PAML_AMD_EUNSUPPORTED, "attach_scores: the derivative of a rate-matrix (UNREST) set's P(t) needs a matrix product of its own");
   const TreeDesc &T = e->tree;
   const int nn = T.n_nodes, n = e->n, K = e->K, G = e->n_genes, n_tips = e->n_tips, n_int = nn - n_tips, psets = G * K;
   const long n_patt = e->n_patt;
   if (pendant_label < 0 || pendant_label >= e->n_labels)
      return fail(e, PAML_AMD_EINVAL, "attach_scores: pendant_label = " + std::to_string(pendant_label) + " is outside the class tables' " + std::to_string(e->n_labels) + " labels");
   // the queries' codes in the engine's own numbering; a query is checked at the first row that names it
   std::vector<unsigned char> qcodes((size_t)n_q * n_patt, 0);
   {
      std::vector<char> seen(n_q, 0);
      for (int i = 0; i < n_rows; i++) {
         const int qi = rows[3 * i], v = rows[3 * i + 1], role = rows[3 * i + 2];
         const std::string at = "attach_scores: row " + std::to_string(i) + ": ";
         if (qi < 0 || qi >= n_q) return fail(e, PAML_AMD_EINVAL, at + "query " + std::to_string(qi) + " is out of range");
         if (v < 0 || v >= nn) return fail(e, PAML_AMD_EINVAL, at + "node " + std::to_string(v) + " is out of range");
         if (v == T.root) return fail(e, PAML_AMD_EINVAL, at + "node " + std::to_string(v) + " is the root");
         if (role < -1 || role > 2) return fail(e, PAML_AMD_EINVAL, at + "role " + std::to_string(role) + " is outside -1..2");
         for (int j = 0; j < 3; j++)
            if (!(t3[3 * i + j] >= 0) || !std::isfinite(t3[3 * i + j]))
               return fail(e, PAML_AMD_EINVAL, at + "length " + std::to_string(j) + " is negative or not finite");
         if (seen[qi]) continue;
         seen[qi] = 1;
         for (long h = 0; h < n_patt; h++) {
            const int c = qz[(size_t)qi * n_patt + h];
            if (c >= e->n_codes || e->code_nch[c] < 1)
               return fail(e, PAML_AMD_EINVAL, at + "query " + std::to_string(qi) + ", pattern " + std::to_string(h) + ": character code " + std::to_string(c) +
                                                   (c >= e->n_codes ? " >= n_codes" : " has an empty state set"));
            qcodes[(size_t)qi * n_patt + h] = e->code_new_of[c];
         }
      }
   }
   // the rows sorted by node (then the caller's index)
   std::vector<int> order(n_rows);
   for (int i = 0; i < n_rows; i++) order[i] = i;
   std::sort(order.begin(), order.end(), [&](int x, int y) { return rows[3 * x + 1] != rows[3 * y + 1] ? rows[3 * x + 1] < rows[3 * y + 1] : x < y; });
   std::vector<int> srows((size_t)4 * n_rows);
   std::vector<double> st3((size_t)3 * n_rows);
   for (int i = 0; i < n_rows; i++) {
      const int c = order[i];
      srows[4 * i] = rows[3 * c + 1]; srows[4 * i + 1] = rows[3 * c]; srows[4 * i + 2] = rows[3 * c + 2]; srows[4 * i + 3] = c;
      for (int j = 0; j < 3; j++) st3[3 * i + j] = t3[3 * c + j];
   }

   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   AttachScratch w(attach_info);
   AttachArgs a{};
   NniArgs &o = a.e.o;
   AncMargArgs &m = o.m;
   if (int rc = anc_tree_pack(e, who, w, &m.t)) return rc;
   if (int rc = anc_pmat(e, who, branch, gene_rate, w)) return rc;
   if (mfma) {
      HIPCHK(w.PT.ensure((size_t)psets * nn * 4096));
      hipLaunchKernelGGL(nni_pt_kernel, dim3(nn, psets), dim3(256), 0, st, (const double *)e->d_rowmajor.p, w.PT.p, n, nn, n_tips, T.root);
      HIPCHK(hipGetLastError());
   }
   const long msz = mfma ? 4096 : (long)n * n;
   const size_t tw = tip_words(e);
   HIPCHK(upload(w.rows, srows.data(), srows.size(), st));
   HIPCHK(upload(w.t3, st3.data(), st3.size(), st));
   HIPCHK(upload(w.qz, qcodes.data(), qcodes.size(), st));
   HIPCHK(w.AM.ensure((size_t)n_rows * psets * ATTACH_MATS * msz));
   if (mfma) HIPCHK(w.AT.ensure((size_t)n_rows * psets * ATTACH_TABS * tw));
   {
      AttachPmatArgs pa{};
      GradPmatArgs &ga = pa.g;
      ga.n = n; ga.K = K; ga.n_nodes = nn; ga.n_tips = n_tips; ga.root = T.root; ga.n_labels = e->n_labels; ga.rate_gs = e->rate_per_gene ? K : 0; ga.mfma = mfma ? 1 : 0;
      ga.label = e->d_label.p; ga.eigen_of = e->d_eigen_of.p; ga.eigen = e->d_eigen.p;
      ga.rate = e->d_rate.p; ga.gene_rate = e->d_gene_rate.p; ga.qfactor = e->d_qfactor.p;
      pa.rows = w.rows.p; pa.t3 = w.t3.p; pa.code_mask = e->d_code_mask.p; pa.AM = w.AM.p; pa.AT = w.AT.p; pa.msz = msz; pa.tip_words = (long)tw;
      pa.psets = psets; pa.n_codes = e->n_codes; pa.pendant_label = pendant_label;
      hipLaunchKernelGGL(attach_pmat_kernel, dim3((unsigned)n_rows * 3, psets), dim3(256), 0, st, pa);
      HIPCHK(hipGetLastError());
   }
   if (int rc = anc_pmat_wait(e, w)) return rc;      // (the sorted lists are on this stack: waited for here)
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) of the tree at `branch`, in the tree's own orientation, as after nni_scores)

   const std::vector<long> chunk_base = anc_chunk_base(e);
   const long n_chunks = chunk_base[G];
   HIPCHK(w.partial.ensure((size_t)(3 * n_rows + 1) * std::max<long>(n_chunks, 1)));
   HIPCHK(w.out.ensure((size_t)3 * n_rows + 1));

   // the workspace per pattern: the partials and the messages, then (4 K + 3) doubles per row (the rows of a group and the present tree)
   const int ns = mfma ? 64 : n;      // doubles a partial takes per pattern
   const double fixed = 2.0 * K * n_int * (ns + 1) * 8, per_row = (4.0 * K + 3) * 8;
   const double arena_mb = anc_arena_mb("PAML_AMD_ATTACH_ARENA_MB");
   int cap = n_rows;
   if ((fixed + per_row * (n_rows + 1)) * ANC_TILE > arena_mb * 1048576.0)      // one tile with all rows does not fit: groups of rows
      cap = (int)std::min<double>(n_rows, std::max(1.0, floor((arena_mb * 1048576.0 / ANC_TILE - fixed) / per_row) - 1));
   cap = std::min(cap, 65535);      // (the lanes' row pass has a grid layer per row)
   long batch = anc_batch(fixed + per_row * (cap + 1), n_patt, "PAML_AMD_ATTACH_ARENA_MB");
   {
      const size_t part = (size_t)K * n_int * ns, sc = (size_t)K * n_int, kr = (size_t)K * (cap + 1), r1 = (size_t)cap + 1;
      if (int rc = anc_alloc(e, who, {{&w.L, part}, {&w.G, part}, {&w.SL, sc}, {&w.SG, sc}, {&w.f, kr}, {&w.f1, kr}, {&w.f2, kr}, {&w.sig, kr}, {&w.lnf, r1}, {&w.g1, r1}, {&w.g2, r1}}, &batch))
         return rc;
   }
   anc_fill(e, w, batch, m);
   o.PT = w.PT.p; o.cap = cap; o.n_swaps = n_rows; o.f = w.f.p; o.sig = w.sig.p; o.weights = e->d_weights.p;
   o.lnf = w.lnf.p; o.partial = w.partial.p; o.n_chunks = n_chunks;
   o.ref_node = T.sons[T.sons_ptr[T.root]];
   a.e.f1 = w.f1.p; a.e.f2 = w.f2.p; a.e.g1 = w.g1.p; a.e.g2 = w.g2.p; a.e.psets = psets;
   a.rows = w.rows.p; a.AM = w.AM.p; a.AT = w.AT.p; a.qz = w.qz.p; a.psets = psets;
   auto group = [&](int gi) { o.swap0 = gi * cap; o.n_group = std::min(cap, n_rows - o.swap0); };      // groups of `cap` rows of the sorted list
   if (int rc = anc_score_batches(
          e, w, o, batch, (n_rows + cap - 1) / cap,
          [&](dim3 lanes, int pass) { anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(nni_lane_kernel<N()>, lanes, dim3(256), 0, st, o, pass); }); },
          [](dim3) {},      // (the present tree's row is combined with the batch's first group)
          [&](int gi, dim3 tiles, dim3 lanes) {
             group(gi);
             if (mfma) hipLaunchKernelGGL(attach_mfma_kernel, tiles, dim3(256), 0, st, a);
             else anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(attach_lane_kernel<N()>, dim3(lanes.x, K, o.n_group), dim3(256), 0, st, a); });
          },
          [&](int gi, dim3 lanes) { hipLaunchKernelGGL(attach_combine_kernel, dim3(lanes.x, o.n_group + (gi == 0 ? 1 : 0)), dim3(256), 0, st, a); },
          [&](int, long h0, long nb) {      // the group's rows to the caller's [n_rows][n_patt], at the caller's index: one plain copy per row
             if (lnf)
                for (int i = 0; i < o.n_group; i++)
                   HIPCHK(hipMemcpyAsync(lnf + (size_t)srows[4 * (size_t)(o.swap0 + i) + 3] * n_patt + h0, w.lnf.p + (size_t)i * batch, (size_t)nb * 8, hipMemcpyDeviceToHost, st));
             return 0;
          }))
      return rc;
   std::vector<double> out((size_t)3 * n_rows + 1);
   if (int rc = anc_totals(e, w, w.partial.p, n_chunks, w.out.p, out)) return rc;
   for (int i = 0; i < n_rows; i++) {
      lnL[i] = out[i];
      d1[i] = out[(size_t)n_rows + i];
      d2[i] = out[(size_t)2 * n_rows + i];
   }
   *lnL0 = out[(size_t)3 * n_rows];
   return 0;
}
