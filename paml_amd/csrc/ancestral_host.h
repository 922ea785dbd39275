// ancestral_host.h — the host side that the calls walking a down pass and an outer pass over the whole tree share (defined in
// engine_ancestral.hip; used there, by engine_gradient.hip, engine_nni.hip, engine_place.hip and engine_spr.hip): the packed tree, P(t) from the evaluation's own builders, the batch size.
#pragma once
#include "engine_state.h"

namespace paml_amd {

struct AncTree;      // kernels_ancestral.h

// what a call allocates for itself; released on every way out
struct AncScratch {
   DevBuf<int> tree, query;
   DevBuf<double> L, G, SL, SG, post, prob, lnP, lnbest;
   DevBuf<unsigned char> best, C, state, rootstate;
   hipEvent_t ev0 = nullptr, ev1 = nullptr;
   ~AncScratch()
   {
      tree.release(); query.release();
      for (DevBuf<double> *b : {&L, &G, &SL, &SG, &post, &prob, &lnP, &lnbest}) b->release();
      for (DevBuf<unsigned char> *b : {&best, &C, &state, &rootstate}) b->release();
      if (ev0) (void)hipEventDestroy(ev0);
      if (ev1) (void)hipEventDestroy(ev1);
   }
};

int anc_tree_pack(paml_amd_engine *e, const char *who, AncScratch &w, AncTree *out);
int anc_pmat(paml_amd_engine *e, const char *who, const double *branch, const double *gene_rate, AncScratch &w, const int *d_label = nullptr);
long anc_batch(double bytes_per_patt, long n_patt, const char *env = "PAML_AMD_ANC_ARENA_MB");
int anc_common_checks(paml_amd_engine *e, const char *who);

}  // namespace paml_amd
