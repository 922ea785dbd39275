// ancestral_host.h — the host side that the calls walking a down pass and an outer pass over the whole tree share (defined in
// engine_ancestral.hip; used there, by engine_gradient.hip, engine_curvature.hip, engine_nni.hip, engine_place.hip and engine_spr.hip): the packed tree, P(t)
// from the evaluation's own builders, the batch size and its workspace, the batch loop of the score calls, the rows' totals.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "engine_state.h"
#include "kernels_nni.h"

namespace paml_amd {

// what paml_amd_*_info reports of the thread's last call: batches walked; HIP events around the P(t) kernels and every batch's passes, summed
struct AncCallInfo {
   int batches = 0;
   double kernel_ms = 0;
   void read(int *last_batches, double *last_kernel_ms) const
   {
      if (last_batches) *last_batches = batches;
      if (last_kernel_ms) *last_kernel_ms = kernel_ms;
   }
};

// what a call allocates for itself; released on every way out
struct AncScratch {
   AncCallInfo &info;
   DevBuf<int> tree, query;
   DevBuf<double> L, G, SL, SG, post, prob, lnP, lnbest;
   DevBuf<unsigned char> best, C, state, rootstate;
   hipEvent_t ev0 = nullptr, ev1 = nullptr;
   explicit AncScratch(AncCallInfo &i) : info(i) {}
   // waits for the stream and adds the time between ev0 and ev1 to the call's
   hipError_t lap(hipStream_t st)
   {
      float ms = 0;
      hipError_t r = hipStreamSynchronize(st);
      if (r == hipSuccess) r = hipEventElapsedTime(&ms, ev0, ev1);
      info.kernel_ms += ms;
      return r;
   }
   ~AncScratch()
   {
      tree.release(); query.release();
      for (DevBuf<double> *b : {&L, &G, &SL, &SG, &post, &prob, &lnP, &lnbest}) b->release();
      for (DevBuf<unsigned char> *b : {&best, &C, &state, &rootstate}) b->release();
      if (ev0) (void)hipEventDestroy(ev0);
      if (ev1) (void)hipEventDestroy(ev1);
   }
};

// a buffer of the batch workspace and the doubles it holds per pattern of the batch
struct AncBatchBuf {
   DevBuf<double> *buf;
   size_t per_patt;
};

int anc_tree_pack(paml_amd_engine *e, const char *who, AncScratch &w, AncTree *out);
int anc_pmat(paml_amd_engine *e, const char *who, const double *branch, const double *gene_rate, AncScratch &w, const int *d_label = nullptr);
int anc_pmat_wait(paml_amd_engine *e, AncScratch &w);
int anc_pmat_waited(paml_amd_engine *e, const char *who, const double *branch, const double *gene_rate, AncScratch &w, const int *d_label = nullptr);
int anc_keep_pmat(paml_amd_engine *e, DevBuf<double> *pint, DevBuf<double> *ptip, DevBuf<double> *PT, DevBuf<double> &P);
double anc_arena_mb(const char *env);
long anc_batch(double bytes_per_patt, long n_patt, const char *env = "PAML_AMD_ANC_ARENA_MB");
int anc_alloc(paml_amd_engine *e, const char *who, std::initializer_list<AncBatchBuf> bufs, long *batch);
void anc_fill(const paml_amd_engine *e, const AncScratch &w, long batch, AncMargArgs &m);
std::vector<long> anc_chunk_base(const paml_amd_engine *e);
int anc_totals(paml_amd_engine *e, AncScratch &w, const double *partial, long n_chunks, double *d_out, std::vector<double> &out);
int anc_common_checks(paml_amd_engine *e, const char *who);

// 4 / 5 / 20 states, the engines that are not on the matrix cores (paml_amd_create: every other state count is KK_MFMA64): f(N) with the
// state count a compile-time constant, for the lane kernels' template argument
template <class F> void anc_lanes(KernelKind kk, F &&f)
{
   if (kk == KK_VALU4) f(std::integral_constant<int, 4>{});
   else if (kk == KK_VALU5) f(std::integral_constant<int, 5>{});
   else f(std::integral_constant<int, 20>{});
}

// The batch loop of the score calls (NNI, placement, SPR).  Per gene and batch of patterns: the down pass and the outer pass of the
// present tree (matrix cores: anc_mfma_kernel and nni_mfma_outer_kernel; lanes: the caller's kernel, lane_pass(lanes, pass)), the caller's
// kernel for the present tree's row if it has one (present(lanes)), then per group of rows the caller's row kernel (rows(gi, tiles,
// lanes), which also names the group in its arguments), its combining kernel (combine(gi, lanes)) and its copies to the caller's arrays
// (copy_out(gi, h0, nb), an error code).  A batch's first group is timed with its down and outer passes, every other by itself.
template <class LanePass, class Present, class Rows, class Combine, class CopyOut>
int anc_score_batches(paml_amd_engine *e, AncScratch &w, NniArgs &o, const std::vector<long> &chunk_base, long batch, int n_groups, LanePass lane_pass, Present present,
                      Rows rows, Combine combine, CopyOut copy_out)
{
   AncMargArgs &m = o.m;
   const bool mfma = e->kk == KK_MFMA64;
   hipStream_t st = e->stream;
   for (int g = 0; g < e->n_genes; g++)
      for (long h0 = e->gene_off[g]; h0 < e->gene_off[g + 1]; h0 += batch) {
         const long nb = std::min<long>(batch, e->gene_off[g + 1] - h0);
         m.gene = g; m.h0 = h0; m.nb = nb;
         o.chunk0 = chunk_base[g] + (h0 - e->gene_off[g]) / GRAD_CHUNK;
         o.swap0 = 0; o.n_group = 0;
         const dim3 tiles((unsigned)((nb + ANC_TILE - 1) / ANC_TILE), m.K), lanes((unsigned)((nb + 255) / 256), m.K);
         HIPCHK(hipEventRecord(w.ev0, st));
         if (mfma) {
            hipLaunchKernelGGL(anc_mfma_kernel, tiles, dim3(256), 0, st, m, 0);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(nni_mfma_outer_kernel, tiles, dim3(256), 0, st, o);
            HIPCHK(hipGetLastError());
         }
         else
            for (int pass = 0; pass < 2; pass++) {
               lane_pass(lanes, pass);
               HIPCHK(hipGetLastError());
            }
         present(lanes);
         HIPCHK(hipGetLastError());
         HIPCHK(hipEventRecord(w.ev1, st));
         for (int gi = 0; gi < n_groups; gi++) {
            if (gi) {
               HIPCHK(w.lap(st));
               HIPCHK(hipEventRecord(w.ev0, st));
            }
            rows(gi, tiles, lanes);
            HIPCHK(hipGetLastError());
            combine(gi, lanes);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(w.ev1, st));
            if (int rc = copy_out(gi, h0, nb)) return rc;
         }
         HIPCHK(w.lap(st));
         w.info.batches++;
      }
   return 0;
}

}  // namespace paml_amd
