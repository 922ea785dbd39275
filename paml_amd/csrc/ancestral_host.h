// ancestral_host.h — the host side that the calls walking a down pass and an outer pass over the whole tree share (defined in
// engine_ancestral.hip; used there, by the derivative calls and, through score_host.h, by the six score calls): the packed tree, P(t)
// from the evaluation's own builders, the batch size and its workspace, the batch loop, the rows' totals.  What only the score calls
// share — their refusals, row checks, workspace plan, batch loop and totals — is in score_host.h.
#pragma once
#include <initializer_list>
#include <vector>
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

// what a call allocates for itself; released on every way out (the members free themselves, dev_buf.h: so do those a call's own struct adds)
struct AncScratch {
   AncCallInfo &info;
   DevBuf<int> tree, query;
   DevBuf<double> L, G, SL, SG, post, prob, lnP, lnbest;
   DevBuf<unsigned char> best, C, state, rootstate;
   DevEvent ev0, ev1;
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
};

// a buffer of the batch workspace, of any element type, and the elements it holds per pattern of the batch
struct AncBatchBuf {
   void *buf;
   size_t per_patt;
   hipError_t (*ensure)(void *, size_t);
   void (*release)(void *);
   template <class T>
   AncBatchBuf(DevBuf<T> *b, size_t per)
      : buf(b), per_patt(per), ensure([](void *p, size_t n) { return ((DevBuf<T> *)p)->ensure(n); }), release([](void *p) { ((DevBuf<T> *)p)->release(); })
   {
   }
};

// a batch of the batch loop: patterns [h0, h0 + nb) of `gene`, and the two grids over them (x: tiles of ANC_TILE patterns / blocks of 256
// lanes; y: the classes)
struct AncBatch {
   int gene;
   long h0, nb;
   dim3 tiles, lanes;
};

int anc_tree_pack(paml_amd_engine *e, const char *who, AncScratch &w, AncTree *out);
int anc_pmat(paml_amd_engine *e, const char *who, const double *branch, const double *gene_rate, AncScratch &w, const int *d_label = nullptr);
int anc_pmat_wait(paml_amd_engine *e, AncScratch &w);
int anc_pmat_waited(paml_amd_engine *e, const char *who, const double *branch, const double *gene_rate, AncScratch &w, const int *d_label = nullptr);
int anc_keep_pmat(paml_amd_engine *e, DevBuf<double> *pint, DevBuf<double> *ptip, DevBuf<double> *PT, DevBuf<double> &P);
double anc_arena_mb(const char *env);
long anc_batch(double bytes_per_patt, long n_patt, const char *env = "PAML_AMD_ANC_ARENA_MB");
int anc_alloc(paml_amd_engine *e, const char *who, const std::vector<AncBatchBuf> &bufs, long *batch);
void anc_fill(const paml_amd_engine *e, const AncScratch &w, long batch, AncMargArgs &m);
std::vector<long> anc_chunk_base(const paml_amd_engine *e);
int anc_totals(paml_amd_engine *e, AncScratch &w, const double *partial, long n_chunks, double *d_out, std::vector<double> &out);
int anc_common_checks(paml_amd_engine *e, const char *who);
int anc_begin(paml_amd_engine *e, const char *who, const char *unrest_reason);      // (score_begin, score_host.h, and a tree without a branch)
int grad_dpmat(paml_amd_engine *e, DevBuf<double> &dP, DevBuf<double> *d2P, DevBuf<double> &PT);

// 4 / 5 / 20 states, the engines that are not on the matrix cores (paml_amd_create: every other state count is KK_MFMA64): f(N) with the
// state count a compile-time constant, for the lane kernels' template argument
template <class F> void anc_lanes(KernelKind kk, F &&f)
{
   if (kk == KK_VALU4) f(std::integral_constant<int, 4>{});
   else if (kk == KK_VALU5) f(std::integral_constant<int, 5>{});
   else f(std::integral_constant<int, 20>{});
}

// The batch loop of every whole-tree call.  Per gene and batch of patterns, in this order: the batch named in `m` (gene, h0, nb; any
// argument structure with these members; AncMargArgs where the call has the two passes) and in *chunk0 (its first chunk of GRAD_CHUNK
// patterns, counted as anc_chunk_base counts; null: the call has no chunks); ev0; the down pass and the outer pass of the present tree —
// matrix cores: anc_mfma_kernel at 0 and the caller's kernel (mfma_outer(b)), lanes: the caller's kernel at pass 0 and 1 (lane_pass(b,
// pass)); both null: a call without the two passes —; the caller's other launches (rest(b), an error code); ev1; the caller's copies
// out (copy_out(b), an error code); the wait that adds the time between the events to the call's; the batch counted.  A callback that
// keeps per-batch bookkeeping in the kernels' arguments does it before its first launch (paml_amd_model_gradient's `place`).
template <class A, class MfmaOuter, class LanePass, class Rest, class CopyOut>
int anc_batches(paml_amd_engine *e, AncScratch &w, A &m, long *chunk0, long batch, MfmaOuter mfma_outer, LanePass lane_pass, Rest rest, CopyOut copy_out)
{
   hipStream_t st = e->stream;
   std::vector<long> chunk_base;
   if (chunk0) chunk_base = anc_chunk_base(e);
   for (int g = 0; g < e->n_genes; g++)
      for (long h0 = e->gene_off[g]; h0 < e->gene_off[g + 1]; h0 += batch) {
         const long nb = std::min<long>(batch, e->gene_off[g + 1] - h0);
         m.gene = g; m.h0 = h0; m.nb = nb;
         if (chunk0) *chunk0 = chunk_base[g] + (h0 - e->gene_off[g]) / GRAD_CHUNK;
         const AncBatch b{g, h0, nb, dim3((unsigned)((nb + ANC_TILE - 1) / ANC_TILE), e->K), dim3((unsigned)((nb + 255) / 256), e->K)};
         HIPCHK(hipEventRecord(w.ev0, st));
         if constexpr (!std::is_same_v<MfmaOuter, std::nullptr_t>) {
            if (e->kk == KK_MFMA64) {
               hipLaunchKernelGGL(anc_mfma_kernel, b.tiles, dim3(256), 0, st, m, 0);
               HIPCHK(hipGetLastError());
               mfma_outer(b);
               HIPCHK(hipGetLastError());
            }
            else
               for (int pass = 0; pass < 2; pass++) {
                  lane_pass(b, pass);
                  HIPCHK(hipGetLastError());
               }
         }
         if (int rc = rest(b)) return rc;
         HIPCHK(hipEventRecord(w.ev1, st));
         if (int rc = copy_out(b)) return rc;
         HIPCHK(w.lap(st));
         w.info.batches++;
      }
   return 0;
}

}  // namespace paml_amd
