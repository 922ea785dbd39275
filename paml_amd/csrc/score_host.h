// score_host.h — the host side that the score calls share (paml_amd_{nni,edge,placement,spr,relabel,attach}_scores: many rows, each a
// variant of the tree, one lnL per row from one engine call), on top of ancestral_host.h; the functions that are not templates are
// defined in engine_ancestral.hip.  A call's body is its own argument checks, its own row preparation and matrices, then: score_begin,
// score_present_pmat, score_plan, score_alloc, score_fill, anc_score_batches over its row and combining kernels, score_totals.
#pragma once
#include <string>

#include "ancestral_host.h"

namespace paml_amd {

// what every score call allocates: P^T of the present tree (matrix cores), f_hk / sigma / lnf of the rows in the workspace, the chunks'
// sums and their totals.  A call's own struct adds only what is its own.
struct ScoreScratch : AncScratch {
   using AncScratch::AncScratch;
   DevBuf<double> PT, f, sig, lnf, partial, out;
};

// the workspace plan: rows of a group, chunks of the engine, patterns of a batch, and the elements per pattern of L / G (part) and SL / SG (sc)
struct ScorePlan {
   int cap;
   long n_chunks, batch;
   size_t part, sc;
};

int score_begin(paml_amd_engine *e, const char *who, const char *unrest_reason);
std::vector<int> score_fathers(const TreeDesc &T);
bool score_son_of(const TreeDesc &T, int s, int v);
int score_check_node(paml_amd_engine *e, const std::string &at, int v, const std::vector<int> *father, bool tips_refused);
int score_query_codes(paml_amd_engine *e, const std::string &prefix, int qi, const unsigned char *qz, unsigned char *dst);
GradPmatArgs grad_pmat_args(const paml_amd_engine *e);
int score_present_pmat(paml_amd_engine *e, const char *who, const double *branch, const double *gene_rate, ScoreScratch &w, const int *d_label = nullptr,
                       bool all_nodes = false);
double score_fixed(const paml_amd_engine *e);
int score_plan(paml_amd_engine *e, ScoreScratch &w, ScorePlan *plan, const char *env, double per_row, int n_rows, long n_out, int extra_rows = 1, double fixed = 0,
               int cap = 0);
int score_alloc(paml_amd_engine *e, const char *who, ScoreScratch &w, ScorePlan &plan, std::initializer_list<AncBatchBuf> own);
void score_fill(NniArgs &o, const ScoreScratch &w, const paml_amd_engine *e, const ScorePlan &plan, int n_rows);
int score_totals(paml_amd_engine *e, ScoreScratch &w, const ScorePlan &plan, long n_rows, const int *index_of, double *lnL0, std::initializer_list<double *> vals);

// groups of `cap` rows in list order: how many, and group gi named in the kernels' arguments
inline int score_n_groups(int n_rows, int cap) { return (n_rows + cap - 1) / cap; }
inline void score_group(NniArgs &o, int cap, int n_rows, int gi)
{
   o.swap0 = gi * cap;
   o.n_group = std::min(cap, n_rows - o.swap0);
}

// rows row0 .. row0 + n of the workspace's lnf (row i at d_lnf + i * batch) to the caller's [.][n_patt] at index_of(row0 + i), patterns
// h0 .. h0 + nb: one plain copy per row (no pitch that n_patt could outgrow); lnf null: not asked for
template <class IndexOf> int score_copy_rows(paml_amd_engine *e, const double *d_lnf, long batch, long row0, long n, double *lnf, long h0, long nb, IndexOf index_of)
{
   for (long i = 0; lnf && i < n; i++)
      HIPCHK(hipMemcpyAsync(lnf + (size_t)index_of(row0 + i) * e->n_patt + h0, d_lnf + (size_t)i * batch, (size_t)nb * 8, hipMemcpyDeviceToHost, e->stream));
   return 0;
}

// The batch loop of the score calls, on anc_batches.  The passes of the present tree are anc_mfma_kernel and nni_mfma_outer_kernel (matrix
// cores) or nni_lane_kernel at pass 0 and 1 (lanes; spr has a kernel of its own: lane_pass(lanes, pass)); then the caller's kernel for the
// present tree's row if it has one (placement: present(lanes); the others combine it with a batch's first group); then, as the batch's
// copies out, per group of rows the caller's row kernel (rows(gi, tiles, lanes), which also names the group in its arguments), its
// combining kernel (combine(gi, lanes)) and its copies to the caller's arrays (copy_out(gi, h0, nb), an error code).  A batch's first
// group is timed with its down and outer passes, every other by itself.
template <class Rows, class Combine, class CopyOut, class Present = std::nullptr_t, class LanePass = std::nullptr_t>
int anc_score_batches(paml_amd_engine *e, AncScratch &w, NniArgs &o, long batch, int n_groups, Rows rows, Combine combine, CopyOut copy_out, Present present = nullptr,
                      LanePass lane_pass = nullptr)
{
   hipStream_t st = e->stream;
   o.swap0 = 0; o.n_group = 0;      // (the passes and the present tree's row run with no group named)
   return anc_batches(
      e, w, o.m, &o.chunk0, batch, [&](const AncBatch &b) { hipLaunchKernelGGL(nni_mfma_outer_kernel, b.tiles, dim3(256), 0, st, o); },
      [&](const AncBatch &b, int pass) {
         if constexpr (std::is_same_v<LanePass, std::nullptr_t>)
            anc_lanes(e->kk, [&](auto N) { hipLaunchKernelGGL(nni_lane_kernel<N()>, b.lanes, dim3(256), 0, st, o, pass); });
         else lane_pass(b.lanes, pass);
      },
      [&](const AncBatch &b) {
         if constexpr (!std::is_same_v<Present, std::nullptr_t>) {
            present(b.lanes);
            HIPCHK(hipGetLastError());
         }
         return 0;
      },
      [&](const AncBatch &b) {
         for (int gi = 0; gi < n_groups; gi++) {
            if (gi) {
               HIPCHK(w.lap(st));
               HIPCHK(hipEventRecord(w.ev0, st));
            }
            rows(gi, b.tiles, b.lanes);
            HIPCHK(hipGetLastError());
            combine(gi, b.lanes);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(w.ev1, st));
            if (int rc = copy_out(gi, b.h0, b.nb)) return rc;
         }
         o.swap0 = 0; o.n_group = 0;
         return 0;
      });
}

}  // namespace paml_amd
