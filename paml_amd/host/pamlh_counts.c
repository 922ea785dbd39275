/* pamlh_counts.c — posterior expected numbers of labelled substitutions per branch and per site of a loaded analysis, from the engine call
 * that returns them for every branch and pattern at once (paml_amd_subst_counts; the definition is in csrc/kernels_counts.h).
 *
 * pamlh_count_labels builds the label matrices (n x n weights: off the diagonal of the jumps a -> b, on it of the time spent in a) that go
 * with the analysis's data type:
 *   codons        "synonymous", "nonsynonymous" by the analysis's genetic code (the stop codons are not states); every pair of sense codons
 *                 gets its weight, also the pairs the model gives rate 0 — the engine multiplies by the rate
 *   nucleotides   "transitions" (T <-> C, A <-> G), "transversions"
 *   amino acids   "changes"
 *   kind "total": every jump; kind "dwell": the identity, whose count is the branch length itself at every site
 * pamlh_subst_counts: the counts at x over x's branch-length block (pamlh_branch_order), summed over the alignment and, on request, per
 * site (the patterns' values expanded by pamlh_pose).
 * Refused by name, as pamlh_curvature refuses them: a clock (x holds ages), fix_blength = 2 or 3, rho != 0 (the sites are not
 * independent), a rate-matrix (UNREST) model, a pattern shard (the engine call is for one rank). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pamlh_internal.h"

static int counts_refused(pamlh *p, const char *who)
{
   int i;
   if (p->pairwise) return pamlh_fail(p, "%s: runmode = -2 has no tree", who);
   if (p->clock) return pamlh_fail(p, "%s: clock = %d: x holds node ages, not branch lengths", who, p->clock);
   if (p->fix_blength == 2 || p->fix_blength == 3 || !p->ntime || p->ntime != p->nbranch)
      return pamlh_fail(p, "%s: fix_blength = %d: the branch lengths are not parameters", who, p->fix_blength);
   if (!p->fix_rho || p->rho0 != 0) return pamlh_fail(p, "%s: rho models (auto-discrete-gamma): the sites are not independent", who);
   if (p->shard_world > 1) return pamlh_fail(p, "%s: a pattern shard (%d ranks): the engine call is for one rank", who, p->shard_world);
   for (i = 0; i < p->n_eigen; i++)
      if (p->eig[i].kind == PAML_AMD_EIGEN_QMAT) return pamlh_fail(p, "%s: a rate-matrix (UNREST) model has no spectral form for the label integrals", who);
   return 0;
}

static void set_name(char (*names)[32], int l, const char *s)
{
   if (names) { strncpy(names[l], s, 31); names[l][31] = 0; }
}

int pamlh_count_labels(pamlh *p, const char *kind, int *n_lab, double *M, char (*names)[32])
{
   const int n = p ? p->n : 0;
   int a, b, nl;
   if (!p || !n_lab) return p ? pamlh_fail(p, "pamlh_count_labels: null argument") : -1;
   if (p->pairwise) return pamlh_fail(p, "pamlh_count_labels: runmode = -2 has no tree");
   if (kind && (!strcmp(kind, "total") || !strcmp(kind, "dwell"))) {
      const int dwell = !strcmp(kind, "dwell");
      *n_lab = 1;
      set_name(names, 0, kind);
      if (M)
         for (a = 0; a < n; a++)
            for (b = 0; b < n; b++) M[a * n + b] = (a == b) == dwell ? 1.0 : 0.0;
      return 0;
   }
   if (kind && strcmp(kind, "standard")) return pamlh_fail(p, "pamlh_count_labels: kind \"%s\" is not standard, total or dwell", kind);
   nl = n == 20 ? 1 : 2;
   *n_lab = nl;
   if (M) memset(M, 0, (size_t)nl * n * n * sizeof(double));
   if (n == 4) {
      set_name(names, 0, "transitions"); set_name(names, 1, "transversions");
      if (M)
         for (a = 0; a < 4; a++)
            for (b = 0; b < 4; b++)
               if (a != b) M[((a ^ b) == 1 ? 0 : 1) * 16 + a * 4 + b] = 1;      /* (T C A G: T <-> C and A <-> G differ in the last bit) */
   }
   else if (n == 20) {
      set_name(names, 0, "changes");
      if (M)
         for (a = 0; a < 20; a++)
            for (b = 0; b < 20; b++) M[a * 20 + b] = a != b;
   }
   else {
      int from61[64], m = 0, c;
      for (c = 0; c < 64; c++) if (p->code[c] != '*') from61[m++] = c;
      if (m != n) return pamlh_fail(p, "pamlh_count_labels: %d states but %d sense codons", n, m);
      set_name(names, 0, "synonymous"); set_name(names, 1, "nonsynonymous");
      if (M)
         for (a = 0; a < n; a++)
            for (b = 0; b < n; b++)
               if (a != b) M[(p->code[from61[a]] == p->code[from61[b]] ? 0 : 1) * n * n + a * n + b] = 1;
   }
   return 0;
}

int pamlh_subst_counts(pamlh *p, const double *x, int n_lab, const double *M, double *counts, double *site_counts)
{
   double *cn = NULL, *sp = NULL, lnL = 0;
   int rc, l, i, h;
   if (!p || !x || !M || !counts) return p ? pamlh_fail(p, "pamlh_subst_counts: null argument") : -1;
   if ((rc = counts_refused(p, "pamlh_subst_counts"))) return rc;
   if ((rc = pamlh_set_x(p, x, p->np))) return rc < 0 ? rc : -1;
   if (!pamlh_model_feasible(p)) return pamlh_fail(p, "pamlh_subst_counts: the model rejects the parameter vector");
   if (p->adg) return pamlh_fail(p, "pamlh_subst_counts: rho models (auto-discrete-gamma): the sites are not independent");
   if ((rc = counts_refused(p, "pamlh_subst_counts"))) return rc;      /* (the eigen kinds are known once the model state is set) */
   if ((rc = pamlh_engine_model(p))) return rc < 0 ? rc : -1;
   cn = (double *)malloc((size_t)n_lab * p->ntime * sizeof(double));
   if (site_counts) sp = (double *)malloc((size_t)n_lab * p->ntime * p->npatt * sizeof(double));
   if (!cn || (site_counts && !sp)) { free(cn); free(sp); return pamlh_fail(p, "pamlh_subst_counts: out of memory"); }
   rc = paml_amd_subst_counts(p->eng, p->branch, p->ngene > 1 ? p->rgene : NULL, n_lab, M, p->ntime, p->branch_node, &lnL, cn, sp, NULL);
   if (rc) { pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); free(cn); free(sp); return rc < 0 ? rc : -1; }
   memcpy(counts, cn, (size_t)n_lab * p->ntime * sizeof(double));
   if (site_counts)
      for (l = 0; l < n_lab; l++)
         for (i = 0; i < p->ntime; i++) {
            const double *src = sp + ((size_t)l * p->ntime + i) * p->npatt;
            double *dst = site_counts + ((size_t)l * p->ntime + i) * p->n_pose;
            for (h = 0; h < p->n_pose; h++) dst[h] = src[p->pose[h]];
         }
   free(cn); free(sp);
   return 0;
}
