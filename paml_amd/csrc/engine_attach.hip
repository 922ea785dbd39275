// engine_attach.hip — the lnL of the tree with a query tip hung on a branch at free lengths of the three branches around the new node,
// with the first and second derivative along one of them, for many rows in one call (paml_amd_attach_scores); the definition in
// kernels_attach.h, the kernels here.  The tree's own P(t) comes from the evaluation's builders (anc_pmat, engine_ancestral.hip), the
// rows' matrices from the edge call's formulas (edge_pmat_fill, kernels_edge.h), the down pass is the ancestral module's, the outer pass
// is the NNI call's, the classes meet in edge_combine.
// The host side that is not this call's own is the score calls' skeleton (score_host.h, defined in engine_ancestral.hip).
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include <algorithm>

#include "engine_state.h"
#include "kernels_attach.h"
#include "score_host.h"

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
   const ScoreTile c = score_tile(m);
   const int lane = c.lane, q = c.q, k = c.k;
   const long p = c.p, pc = c.pc, pset = c.pset;
   const AncMfma w{sP, lane, c.wave, q};
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
         score_mfma_hv(m, w, c, v, h, &ls);
         if (tip) vcode = (int)m.z[(long)v * m.z_stride + m.h0 + pc];
         else {
            score_mfma_lv(m, c, v, l, &ls);
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

// a row's chunks go to the caller's index of the row (edge_combine_rows, kernels_edge.h)
__global__ __launch_bounds__(256) void attach_combine_kernel(AttachArgs a)
{
   edge_combine_rows(a.e, [&](int row) { return a.rows[4L * (a.e.o.swap0 + row) + 3]; });
}
}  // namespace paml_amd

namespace {

struct AttachScratch : ScoreScratch {
   using ScoreScratch::ScoreScratch;
   DevBuf<double> AM, AT, t3, f1, f2, g1, g2;
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
   if (int rc = score_begin(e, who, "the derivative of a rate-matrix (UNREST) set's P(t) needs a matrix product of its own")) return rc;
   const int n = e->n, K = e->K, G = e->n_genes, psets = G * K;
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
         if (int rc = score_check_node(e, at, v, nullptr, false)) return rc;
         if (role < -1 || role > 2) return fail(e, PAML_AMD_EINVAL, at + "role " + std::to_string(role) + " is outside -1..2");
         for (int j = 0; j < 3; j++)
            if (!(t3[3 * i + j] >= 0) || !std::isfinite(t3[3 * i + j]))
               return fail(e, PAML_AMD_EINVAL, at + "length " + std::to_string(j) + " is negative or not finite");
         if (seen[qi]) continue;
         seen[qi] = 1;
         if (int rc = score_query_codes(e, at, qi, qz, qcodes.data())) return rc;
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
   if (int rc = score_present_pmat(e, who, branch, gene_rate, w)) return rc;
   const long msz = mfma ? 4096 : (long)n * n;
   const size_t tw = tip_words(e);
   HIPCHK(upload(w.rows, srows.data(), srows.size(), st));
   HIPCHK(upload(w.t3, st3.data(), st3.size(), st));
   HIPCHK(upload(w.qz, qcodes.data(), qcodes.size(), st));
   HIPCHK(w.AM.ensure((size_t)n_rows * psets * ATTACH_MATS * msz));
   if (mfma) HIPCHK(w.AT.ensure((size_t)n_rows * psets * ATTACH_TABS * tw));
   {
      AttachPmatArgs pa{};
      pa.g = grad_pmat_args(e);
      pa.rows = w.rows.p; pa.t3 = w.t3.p; pa.code_mask = e->d_code_mask.p; pa.AM = w.AM.p; pa.AT = w.AT.p; pa.msz = msz; pa.tip_words = (long)tw;
      pa.psets = psets; pa.n_codes = e->n_codes; pa.pendant_label = pendant_label;
      hipLaunchKernelGGL(attach_pmat_kernel, dim3((unsigned)n_rows * 3, psets), dim3(256), 0, st, pa);
      HIPCHK(hipGetLastError());
   }
   if (int rc = anc_pmat_wait(e, w)) return rc;      // (the sorted lists are on this stack: waited for here)
   e->pmat_valid = true;      // (d_rowmajor holds every branch's P(t) of the tree at `branch`, in the tree's own orientation, as after nni_scores)

   // the workspace per pattern: the partials and the messages, then (4 K + 3) doubles per row (the rows of a group and the present tree)
   ScorePlan plan;
   if (int rc = score_plan(e, w, &plan, "PAML_AMD_ATTACH_ARENA_MB", (4.0 * K + 3) * 8, n_rows, 3L * n_rows)) return rc;
   const int cap = plan.cap;
   const size_t kr = (size_t)K * (cap + 1), r1 = (size_t)cap + 1;
   if (int rc = score_alloc(e, who, w, plan, {{&w.f, kr}, {&w.f1, kr}, {&w.f2, kr}, {&w.sig, kr}, {&w.lnf, r1}, {&w.g1, r1}, {&w.g2, r1}})) return rc;
   score_fill(o, w, e, plan, n_rows);
   a.e.f1 = w.f1.p; a.e.f2 = w.f2.p; a.e.g1 = w.g1.p; a.e.g2 = w.g2.p; a.e.psets = psets;
   a.rows = w.rows.p; a.AM = w.AM.p; a.AT = w.AT.p; a.qz = w.qz.p; a.psets = psets;
   if (int rc = anc_score_batches(
          e, w, o, plan.batch, score_n_groups(n_rows, cap),
          [&](int gi, dim3 tiles, dim3 lanes) {
             score_group(o, cap, n_rows, gi);      // (of the sorted list)
             if (mfma) hipLaunchKernelGGL(attach_mfma_kernel, tiles, dim3(256), 0, st, a);
             else anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(attach_lane_kernel<N()>, dim3(lanes.x, K, o.n_group), dim3(256), 0, st, a); });
          },
          [&](int gi, dim3 lanes) { hipLaunchKernelGGL(attach_combine_kernel, dim3(lanes.x, o.n_group + (gi == 0 ? 1 : 0)), dim3(256), 0, st, a); },
          [&](int, long h0, long nb) {      // the group's rows to the caller's [n_rows][n_patt], at the caller's index
             return score_copy_rows(e, w.lnf.p, plan.batch, o.swap0, o.n_group, lnf, h0, nb, [&](long i) { return srows[4 * (size_t)i + 3]; });
          }))
      return rc;
   return score_totals(e, w, plan, n_rows, nullptr, lnL0, {lnL, d1, d2});      // (the combining kernel put a row's chunks at the caller's index)
}
