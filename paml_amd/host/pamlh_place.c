/* pamlh_place.c — query sequences placed on every branch of the analysis's tree: the lnL of the tree with one more tip hung on branch e,
 * for every query, every branch and every pendant length of a grid, from ONE engine call (pamlh_placement_scores ->
 * paml_amd_placement_scores); the primitive under the reference's stepwise addition (StepwiseAddition treesub.c:4866 on AddSpecies
 * treesub.c:4592, which sets and evaluates one enlarged tree after the other).  pamlh_load_placement reads an analysis whose tree names
 * only some of the sequences of the sequence file: the others are the queries.  pamlh_place picks the best (branch, pendant length) per
 * query and the likelihood weight ratios over the branches; pamlh_placement_newick writes the enlarged tree.
 * Refused by name: a clock (x holds node ages: a branch cannot be split without moving them), rho models (lfunAdG: the sites are not
 * independent, there is no per-pattern likelihood), runmode = -2 (no tree), an analysis without queries. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pamlh_internal.h"

/* pamlh_load_with, except that the tree may name only some of the sequence file's sequences — at least 3, by name or by 1-based number
 * in file order.  The sequences absent from the tree are the queries; the tree's sequences become the tips 0 .. m - 1 in file order.
 * Site patterns are compressed over ALL sequences together, so patterns that differ only in a query stay apart with their own weights
 * (the lnL of the tree is the same sum); with cleandata = 1 a site is dropped if ANY sequence has an ambiguity character there, the
 * queries included.  Everything counted from the data (observed frequencies, F3x4, ...) is counted on the tree's sequences only: a
 * parameter vector estimated without the queries means the same here. */
int pamlh_load_placement(pamlh **out, const char *ctl_path, const char *program, int tree_index, const char *overrides, char *err, int errcap)
{
   return pamlh_load_impl(out, ctl_path, program, tree_index, overrides, 1, err, errcap);
}

/* After pamlh_read_seqs: the tree is read once with the file's sequences as they stand, to see which it names; the others are taken out
 * of the tip rows (names, codes, raw characters) into the query arrays, and pamlh_read_tree then reads the tree on the tips that are left. */
int pamlh_split_queries(pamlh *p)
{
   const int ns_all = p->ns, np = p->npatt, w = p->n31;
   int rc, i, m = 0, nq = 0;
   int *row;
   if ((rc = pamlh_read_tree(p))) return rc;
   row = (int *)malloc(ns_all * sizeof(int));
   for (i = 0; i < ns_all; i++) row[i] = p->father[i] >= 0 ? m++ : -1;
   free(p->sons_ptr); free(p->sons); free(p->label); free(p->branch_node); free(p->father); free(p->tree_branch); free(p->scale);
   p->sons_ptr = p->sons = p->label = p->branch_node = p->father = NULL; p->tree_branch = NULL; p->scale = NULL;
   if (m < 3) { free(row); return pamlh_fail(p, "pamlh_load_placement: the tree names %d of the %d sequences: at least 3 are needed", m, ns_all); }
   nq = ns_all - m;
   p->file_row = row; p->ns_file = ns_all; p->n_query = nq;
   if (nq) {
      char **names = (char **)calloc(m, sizeof(char *));
      p->query_names = (char **)calloc(nq, sizeof(char *));
      p->query_z = (unsigned char *)malloc((size_t)nq * np);
      for (i = 0, nq = 0; i < ns_all; i++) {
         if (row[i] >= 0) {      /* (row[i] <= i: the rows move up in place) */
            names[row[i]] = p->names[i];
            memmove(p->z + (size_t)row[i] * np, p->z + (size_t)i * np, np);
            memmove(p->raw + (size_t)row[i] * np * w, p->raw + (size_t)i * np * w, (size_t)np * w);
         }
         else {
            p->query_names[nq] = p->names[i];
            memcpy(p->query_z + (size_t)nq * np, p->z + (size_t)i * np, np);
            nq++;
         }
      }
      free(p->names);
      p->names = names;
   }
   p->ns = m;
   return 0;
}

int pamlh_n_queries(const pamlh *p) { return p ? p->n_query : 0; }
const char *pamlh_query_name(const pamlh *p, int i) { return p && i >= 0 && i < p->n_query ? p->query_names[i] : NULL; }
const unsigned char *pamlh_query_codes(const pamlh *p) { return p ? p->query_z : NULL; }

static int place_refused(pamlh *p, const char *who)
{
   if (p->pairwise) return pamlh_fail(p, "%s: runmode = -2 has no tree to place sequences on", who);
   if (p->clock) return pamlh_fail(p, "%s: clock = %d: the parameters are node ages, a branch cannot be split without moving them", who, p->clock);
   if (!p->fix_rho || p->rho0 != 0) return pamlh_fail(p, "%s: rho models (auto-discrete-gamma) have no per-pattern likelihood to place sequences with", who);
   if (p->n_query < 1) return pamlh_fail(p, "%s: the analysis has no queries (pamlh_load_placement with a tree that leaves some of the sequences out)", who);
   if (p->shard_world > 1) return pamlh_fail(p, "%s: one GPU only (this analysis holds a pattern shard)", who);
   return 0;
}

/* lnL[n_q][nbranch][n_pend]: query q hung on the b-th branch of x's branch-length block (pamlh_branch_order) at `phi` of its length from
 * its lower end, with pendant length pendant[j] (label 0), at the branch lengths and parameters of x; *lnL0 the tree's own. */
int pamlh_placement_scores(pamlh *p, const double *x, int n_pend, const double *pendant, double phi, double *lnL0, double *lnL)
{
   int rc;
   if (!p) return -1;
   if ((rc = place_refused(p, "pamlh_placement_scores"))) return rc;
   if (!x || !pendant || !lnL0 || !lnL) return pamlh_fail(p, "pamlh_placement_scores: null argument");
   if ((rc = pamlh_set_x(p, x, p->np))) return rc < 0 ? rc : -1;
   if (!pamlh_model_feasible(p)) return pamlh_fail(p, "pamlh_placement_scores: the model rejects the parameter vector");
   if ((rc = pamlh_engine_model(p))) return rc < 0 ? rc : -1;
   rc = paml_amd_placement_scores(p->eng, p->branch, p->ngene > 1 ? p->rgene : NULL, p->n_query, p->query_z, p->nbranch, p->branch_node, n_pend, pendant, phi, 0,
                                  lnL0, lnL, NULL);
   if (rc) { pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); return rc < 0 ? rc : -1; }
   return 0;
}

/* Per query the best (branch, pendant length) of the grid and the likelihood weight ratios of the branches:
 * best_edge[n_q] (index into pamlh_branch_order), best_pendant[n_q], best_lnL[n_q]; lwr[n_q][nbranch] = exp(l_e - logsumexp_e' l_e'), l_e
 * the largest lnL of branch e over the pendant lengths.  Any of the four may be NULL.  Ties go to the first in (branch, pendant) order. */
int pamlh_place(pamlh *p, const double *x, int n_pend, const double *pendant, double phi, int *best_edge, double *best_pendant, double *best_lnL, double *lwr)
{
   int rc, q, e, j;
   double l0 = 0, *sc, *le;
   if (!p) return -1;
   if ((rc = place_refused(p, "pamlh_place"))) return rc;
   if (n_pend < 1) return pamlh_fail(p, "pamlh_place: n_pend < 1");
   sc = (double *)malloc((size_t)p->n_query * p->nbranch * n_pend * sizeof(double));
   le = (double *)malloc((size_t)p->nbranch * sizeof(double));
   if ((rc = pamlh_placement_scores(p, x, n_pend, pendant, phi, &l0, sc))) { free(sc); free(le); return rc; }
   for (q = 0; q < p->n_query; q++) {
      int be = 0, bj = 0;
      double top, tot = 0;
      for (e = 0; e < p->nbranch; e++) {
         const double *row = sc + ((size_t)q * p->nbranch + e) * n_pend;
         int mj = 0;
         for (j = 1; j < n_pend; j++) if (row[j] > row[mj]) mj = j;
         le[e] = row[mj];
         if (e == 0 || le[e] > le[be]) { be = e; bj = mj; }
      }
      top = le[be];
      for (e = 0; e < p->nbranch; e++) tot += exp(le[e] - top);
      if (best_edge) best_edge[q] = be;
      if (best_pendant) best_pendant[q] = pendant[bj];
      if (best_lnL) best_lnL[q] = top;
      if (lwr) for (e = 0; e < p->nbranch; e++) lwr[(size_t)q * p->nbranch + e] = exp(le[e] - top) / tot;
   }
   free(sc); free(le);
   return 0;
}

/* a length with as few digits as read back to the same double */
static int put_length(char *w, size_t room, double v)
{
   char tmp[40];
   snprintf(tmp, sizeof(tmp), "%.15g", v);
   if (strtod(tmp, NULL) != v) snprintf(tmp, sizeof(tmp), "%.17g", v);
   return snprintf(w, room, ": %s", tmp);
}

static void place_newick_rec(const pamlh *p, int node, int at, int q, double phi, double pendant, char **w, char *end)
{
   int j;
   if (node == at && node != p->root) *w += snprintf(*w, end - *w, "(");
   if (node < p->ns) *w += snprintf(*w, end - *w, "%s", p->names[node]);
   else {
      *w += snprintf(*w, end - *w, "(");
      for (j = p->sons_ptr[node]; j < p->sons_ptr[node + 1]; j++) {
         if (j > p->sons_ptr[node]) *w += snprintf(*w, end - *w, ", ");
         place_newick_rec(p, p->sons[j], at, q, phi, pendant, w, end);
      }
      *w += snprintf(*w, end - *w, ")");
   }
   if (node == p->root) return;
   if (p->label[node]) *w += snprintf(*w, end - *w, " #%d", p->label[node]);
   *w += put_length(*w, end - *w, node == at ? phi * p->branch[node] : p->branch[node]);
   if (node == at) {      /* the new node: (node, query), on the upper part of the branch */
      *w += snprintf(*w, end - *w, ", %s", p->query_names[q]);
      *w += put_length(*w, end - *w, pendant);
      *w += snprintf(*w, end - *w, ")");
      if (p->label[node]) *w += snprintf(*w, end - *w, " #%d", p->label[node]);
      *w += put_length(*w, end - *w, (1 - phi) * p->branch[node]);
   }
}

/* The tree with query q hung on the edge-th branch of pamlh_branch_order (split phi, pendant length `pendant`), in Newick form with the
 * branch lengths of the current model state (the last x; lengths written so that they read back to the same doubles) and the '#' labels
 * the tree was read with.  The new node takes the place of the branch's lower node in its father's list; its sons are (that node, the query). */
int pamlh_placement_newick(pamlh *p, int q, int edge, double phi, double pendant, char *buf, int cap)
{
   char *w = buf;
   if (!p || !buf) return -1;
   if (p->n_query < 1) return pamlh_fail(p, "pamlh_placement_newick: the analysis has no queries");
   if (q < 0 || q >= p->n_query) return pamlh_fail(p, "pamlh_placement_newick: query %d of %d", q, p->n_query);
   if (edge < 0 || edge >= p->nbranch) return pamlh_fail(p, "pamlh_placement_newick: branch %d of %d", edge, p->nbranch);
   if (!(phi >= 0 && phi <= 1) || !(pendant >= 0)) return pamlh_fail(p, "pamlh_placement_newick: phi outside [0, 1] or a negative pendant length");
   if (cap < 160 * (p->nnode + 2) + 256) return pamlh_fail(p, "pamlh_placement_newick: room for %d characters is needed", 160 * (p->nnode + 2) + 256);
   place_newick_rec(p, p->root, p->branch_node[edge], q, phi, pendant, &w, buf + cap);
   snprintf(w, buf + cap - w, ";");
   return 0;
}
