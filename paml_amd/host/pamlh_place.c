/* pamlh_place.c — query sequences placed on every branch of the analysis's tree: the lnL of the tree with one more tip hung on branch e,
 * for every query, every branch and every pendant length of a grid, from ONE engine call (pamlh_placement_scores ->
 * paml_amd_placement_scores); the primitive under the reference's stepwise addition (StepwiseAddition treesub.c:4866 on AddSpecies
 * treesub.c:4592, which sets and evaluates one enlarged tree after the other).  pamlh_load_placement reads an analysis whose tree names
 * only some of the sequences of the sequence file: the others are the queries.  pamlh_place picks the best (branch, pendant length) per
 * query and the likelihood weight ratios over the branches; pamlh_placement_newick writes the enlarged tree.  The second half of the
 * file is maximum-likelihood placement: the three lengths at the new node maximised per (query, branch) from one
 * paml_amd_attach_scores call per Newton step (pamlh_attach_scores, pamlh_place_optimize, pamlh_place_ml, pamlh_placement_newick3).
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

/* ---- maximum-likelihood placement: the three lengths at the new node are free ---------------------------------------------------------
 * pamlh_attach_scores is the engine call (paml_amd_attach_scores) at x's branch-length block; pamlh_place_optimize maximises every row
 * over (t_up, t_dn, t_pend) in lock step by the safeguarded cyclic Newton iteration of pamlh_edge_optimize (pamlh_support.c: the same
 * step, pamlh_newton_trial, the same trials per role, tolerance, sweeps and bounds) with ONE engine call per step for all unfinished
 * rows; pamlh_place_ml starts it from the grid call's best rows.  Refused by name: what pamlh_placement_scores refuses, and
 * fix_blength = 2 or 3 (the branch lengths are not parameters); rate-matrix (UNREST) models by the engine's own message. */
#define PLACE_TRIALS 4
#define PLACE_MAX_SWEEPS 30
#define PLACE_T_LO 4e-6
#define PLACE_T_HI 50.0

static int attach_refused(pamlh *p, const char *who)
{
   int rc;
   if ((rc = place_refused(p, who))) return rc;
   if (p->fix_blength == 2 || p->fix_blength == 3 || !p->ntime || p->ntime != p->nbranch)
      return pamlh_fail(p, "%s: fix_blength = %d: the branch lengths are not parameters", who, p->fix_blength);
   return 0;
}

static int attach_model(pamlh *p, const double *x, const char *who)
{
   int rc;
   if ((rc = pamlh_set_x(p, x, p->np))) return rc < 0 ? rc : -1;
   if (!pamlh_model_feasible(p)) return pamlh_fail(p, "%s: the model rejects the parameter vector", who);
   if ((rc = pamlh_engine_model(p))) return rc < 0 ? rc : -1;
   return 0;
}

/* rows[n_rows][3] = q, node, role of the engine call from the host's (q, edge index into pamlh_branch_order); role NULL: -1 */
static int attach_rows(pamlh *p, const char *who, int n_rows, const int *q, const int *edge, const int *role, int *rows)
{
   int i;
   for (i = 0; i < n_rows; i++) {
      if (q[i] < 0 || q[i] >= p->n_query) return pamlh_fail(p, "%s: row %d: query %d of %d", who, i, q[i], p->n_query);
      if (edge[i] < 0 || edge[i] >= p->nbranch) return pamlh_fail(p, "%s: row %d: branch %d of %d", who, i, edge[i], p->nbranch);
      rows[3 * i] = q[i];
      rows[3 * i + 1] = p->branch_node[edge[i]];
      rows[3 * i + 2] = role ? role[i] : -1;
   }
   return 0;
}

/* lnL[n_rows], d1[n_rows], d2[n_rows] of query q[i] hung on the edge[i]-th branch of x's branch-length block (pamlh_branch_order) at the
 * lengths t3[i] = (t_up, t_dn, t_pend) (pendant label 0), the derivatives along the branch role[i] names (-1: none, 0: up, 1: dn, 2:
 * pendant); *lnL0 the tree's own.  One engine call. */
int pamlh_attach_scores(pamlh *p, const double *x, int n_rows, const int *q, const int *edge, const int *role, const double *t3, double *lnL0, double *lnL, double *d1,
                        double *d2)
{
   int rc, *rows;
   if (!p) return -1;
   if ((rc = attach_refused(p, "pamlh_attach_scores"))) return rc;
   if (!x || !q || !edge || !role || !t3 || !lnL0 || !lnL || !d1 || !d2) return pamlh_fail(p, "pamlh_attach_scores: null argument");
   if (n_rows < 1) return pamlh_fail(p, "pamlh_attach_scores: n_rows < 1");
   if ((rc = attach_model(p, x, "pamlh_attach_scores"))) return rc;
   rows = (int *)malloc((size_t)3 * n_rows * sizeof(int));
   if (!(rc = attach_rows(p, "pamlh_attach_scores", n_rows, q, edge, role, rows))) {
      rc = paml_amd_attach_scores(p->eng, p->branch, p->ngene > 1 ? p->rgene : NULL, p->n_query, p->query_z, n_rows, rows, t3, 0, lnL0, lnL, d1, d2, NULL);
      if (rc) { pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); rc = rc < 0 ? rc : -1; }
   }
   free(rows);
   return rc;
}

/* Every row (q[i], edge[i]) maximised over its three lengths, started at t3[i] (clipped to the bounds of a branch length, 4e-6 and 50)
 * and ending in t3[i]; lnL[i] the maximum.  A sweep takes the roles up, dn, pendant in turn; a role is one call at the accepted lengths
 * and at most PLACE_TRIALS calls at trial lengths; a row that gained no more than 1e-6 in a sweep is finished and stays in the calls
 * without a derivative.  No row's lnL ever falls.  stats[3] (or NULL) = sweeps, engine calls, rows that ended with a length at a bound. */
int pamlh_place_optimize(pamlh *p, const double *x, int n_rows, const int *q, const int *edge, double *t3, double *lnL, int *stats)
{
   int rc, i, j, sweep = 0, calls = 0, role, trial, at_bound = 0, active;
   int *rows = NULL;
   unsigned char *done = NULL, *wait = NULL;
   double *t = t3, *tt = NULL, *l = lnL, *l_sweep = NULL, *step = NULL, *ln = NULL, *d1 = NULL, *d2 = NULL, l0 = 0;
   if (!p) return -1;
   if ((rc = attach_refused(p, "pamlh_place_optimize"))) return rc;
   if (!x || !q || !edge || !t3 || !lnL) return pamlh_fail(p, "pamlh_place_optimize: null argument");
   if (n_rows < 1) return pamlh_fail(p, "pamlh_place_optimize: n_rows < 1");
   for (i = 0; i < 3 * n_rows; i++)
      if (!(t3[i] >= 0) || !isfinite(t3[i])) return pamlh_fail(p, "pamlh_place_optimize: row %d: length %d is negative or not finite", i / 3, i % 3);
   if ((rc = attach_model(p, x, "pamlh_place_optimize"))) return rc;
   rows = (int *)malloc((size_t)3 * n_rows * sizeof(int));
   if ((rc = attach_rows(p, "pamlh_place_optimize", n_rows, q, edge, NULL, rows))) { free(rows); return rc; }
   done = (unsigned char *)calloc(n_rows, 1); wait = (unsigned char *)calloc(n_rows, 1);
   tt = (double *)malloc((size_t)3 * n_rows * sizeof(double));
   l_sweep = (double *)malloc(n_rows * sizeof(double)); step = (double *)calloc(n_rows, sizeof(double));
   ln = (double *)malloc(n_rows * sizeof(double)); d1 = (double *)malloc(n_rows * sizeof(double)); d2 = (double *)malloc(n_rows * sizeof(double));
   for (i = 0; i < 3 * n_rows; i++) t[i] = fmin(fmax(t[i], PLACE_T_LO), PLACE_T_HI);
#define PLACE_CALL(lengths)                                                                                                                             \
   do {                                                                                                                                                 \
      rc = paml_amd_attach_scores(p->eng, p->branch, p->ngene > 1 ? p->rgene : NULL, p->n_query, p->query_z, n_rows, rows, lengths, 0, &l0, ln, d1, d2, NULL); \
      calls++;                                                                                                                                          \
      if (rc) { pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); rc = rc < 0 ? rc : -1; goto done; }                                                   \
   } while (0)
   PLACE_CALL(t);
   memcpy(l, ln, n_rows * sizeof(double));
   for (sweep = 0; sweep < PLACE_MAX_SWEEPS;) {
      memcpy(l_sweep, l, n_rows * sizeof(double));
      for (role = 0; role < 3; role++) {
         /* the derivatives along this role's branch at the accepted lengths, then the trials */
         for (i = 0; i < n_rows; i++) { rows[3 * i + 2] = done[i] ? -1 : role; wait[i] = done[i]; step[i] = 0; }
         memcpy(tt, t, (size_t)3 * n_rows * sizeof(double));
         for (trial = 0; trial <= PLACE_TRIALS; trial++) {
            PLACE_CALL(tt);
            active = 0;
            for (i = 0; i < n_rows; i++) {
               if (wait[i]) continue;
               if (!pamlh_newton_trial(trial, PLACE_TRIALS, PLACE_T_LO, PLACE_T_HI, ln[i], d1[i], d2[i], l + i, t + 3 * i + role, tt + 3 * i + role, step + i)) {
                  wait[i] = 1;
                  rows[3 * i + 2] = -1;
                  continue;
               }
               active++;
            }
            if (!active) break;
         }
      }
      sweep++;
      active = 0;
      for (i = 0; i < n_rows; i++) {
         if (!done[i] && l[i] - l_sweep[i] <= 1e-6) done[i] = 1;
         active += !done[i];
      }
      if (!active) break;
   }
#undef PLACE_CALL
   for (i = 0; i < n_rows; i++) {
      int b = 0;
      for (j = 0; j < 3; j++) b |= t[3 * i + j] <= PLACE_T_LO || t[3 * i + j] >= PLACE_T_HI;
      at_bound += b;
   }
   if (stats) { stats[0] = sweep; stats[1] = calls; stats[2] = at_bound; }
   rc = 0;
done:
   free(rows); free(done); free(wait); free(tt); free(l_sweep); free(step); free(ln); free(d1); free(d2);
   return rc;
}

/* The grid call first (pamlh_placement_scores at n_pend pendant lengths and the split phi), then per query its `keep` best branches
 * (keep <= 0 or > nbranch: all; a branch's grid value is its largest over the pendant lengths; best first, ties to the first in branch
 * order), each started at ((1 - phi) t_v, phi t_v, its best grid pendant) and maximised by pamlh_place_optimize.  Row i of the output:
 * rows_q[i], rows_edge[i] (index into pamlh_branch_order), t3[i] the maximising lengths, lnL[i] the maximum, lwr[i] the likelihood weight
 * ratio exp(l_i - logsumexp l_j) over the query's kept rows; *n_rows = n_queries x the branches kept, the queries in order.  The outputs
 * need room for n_queries x nbranch rows. */
int pamlh_place_ml(pamlh *p, const double *x, int keep, int n_pend, const double *pendant, double phi, int *rows_q, int *rows_edge, double *t3, double *lnL,
                   double *lwr, int *n_rows)
{
   int rc, q, e, j, k, nb, n = 0;
   double l0 = 0, *sc, *le;
   int *lj;
   unsigned char *taken;
   if (!p) return -1;
   if ((rc = attach_refused(p, "pamlh_place_ml"))) return rc;
   if (!x || !pendant || !rows_q || !rows_edge || !t3 || !lnL || !lwr || !n_rows) return pamlh_fail(p, "pamlh_place_ml: null argument");
   if (n_pend < 1) return pamlh_fail(p, "pamlh_place_ml: n_pend < 1");
   nb = p->nbranch;
   if (keep <= 0 || keep > nb) keep = nb;
   sc = (double *)malloc((size_t)p->n_query * nb * n_pend * sizeof(double));
   le = (double *)malloc((size_t)nb * sizeof(double)); lj = (int *)malloc((size_t)nb * sizeof(int)); taken = (unsigned char *)malloc(nb);
   if ((rc = pamlh_placement_scores(p, x, n_pend, pendant, phi, &l0, sc))) goto done;
   for (q = 0; q < p->n_query; q++) {
      for (e = 0; e < nb; e++) {
         const double *row = sc + ((size_t)q * nb + e) * n_pend;
         int mj = 0;
         for (j = 1; j < n_pend; j++) if (row[j] > row[mj]) mj = j;
         le[e] = row[mj]; lj[e] = mj; taken[e] = 0;
      }
      for (k = 0; k < keep; k++, n++) {
         int be = -1;
         for (e = 0; e < nb; e++) if (!taken[e] && (be < 0 || le[e] > le[be])) be = e;
         taken[be] = 1;
         rows_q[n] = q; rows_edge[n] = be;
         t3[3 * n] = (1 - phi) * p->branch[p->branch_node[be]];
         t3[3 * n + 1] = phi * p->branch[p->branch_node[be]];
         t3[3 * n + 2] = pendant[lj[be]];
      }
   }
   *n_rows = n;
   if ((rc = pamlh_place_optimize(p, x, n, rows_q, rows_edge, t3, lnL, NULL))) goto done;
   for (q = 0; q < p->n_query; q++) {
      const double *lq = lnL + (size_t)q * keep;
      double top = lq[0], tot = 0;
      for (k = 1; k < keep; k++) if (lq[k] > top) top = lq[k];
      for (k = 0; k < keep; k++) tot += exp(lq[k] - top);
      for (k = 0; k < keep; k++) lwr[(size_t)q * keep + k] = exp(lq[k] - top) / tot;
   }
done:
   free(sc); free(le); free(lj); free(taken);
   return rc;
}

static void place_newick3_rec(const pamlh *p, int node, int at, int q, const double *t3, char **w, char *end)
{
   int j;
   if (node == at) *w += snprintf(*w, end - *w, "(");
   if (node < p->ns) *w += snprintf(*w, end - *w, "%s", p->names[node]);
   else {
      *w += snprintf(*w, end - *w, "(");
      for (j = p->sons_ptr[node]; j < p->sons_ptr[node + 1]; j++) {
         if (j > p->sons_ptr[node]) *w += snprintf(*w, end - *w, ", ");
         place_newick3_rec(p, p->sons[j], at, q, t3, w, end);
      }
      *w += snprintf(*w, end - *w, ")");
   }
   if (node == p->root) return;
   if (p->label[node]) *w += snprintf(*w, end - *w, " #%d", p->label[node]);
   *w += put_length(*w, end - *w, node == at ? t3[1] : p->branch[node]);
   if (node == at) {      /* the new node: (node, query), on the upper part of the branch */
      *w += snprintf(*w, end - *w, ", %s", p->query_names[q]);
      *w += put_length(*w, end - *w, t3[2]);
      *w += snprintf(*w, end - *w, ")");
      if (p->label[node]) *w += snprintf(*w, end - *w, " #%d", p->label[node]);
      *w += put_length(*w, end - *w, t3[0]);
   }
}

/* pamlh_placement_newick with the three attachment lengths written in: the branch above the new node t_up, the branch above the
 * branch's lower node t_dn, the query's branch t_pend; every other length is the current model state's (the last x).  cap as there. */
int pamlh_placement_newick3(pamlh *p, int q, int edge, double t_up, double t_dn, double t_pend, char *buf, int cap)
{
   char *w = buf;
   const double t3[3] = {t_up, t_dn, t_pend};
   if (!p || !buf) return -1;
   if (p->n_query < 1) return pamlh_fail(p, "pamlh_placement_newick3: the analysis has no queries");
   if (q < 0 || q >= p->n_query) return pamlh_fail(p, "pamlh_placement_newick3: query %d of %d", q, p->n_query);
   if (edge < 0 || edge >= p->nbranch) return pamlh_fail(p, "pamlh_placement_newick3: branch %d of %d", edge, p->nbranch);
   if (!(t_up >= 0) || !(t_dn >= 0) || !(t_pend >= 0)) return pamlh_fail(p, "pamlh_placement_newick3: a negative length");
   if (cap < 160 * (p->nnode + 2) + 256) return pamlh_fail(p, "pamlh_placement_newick3: room for %d characters is needed", 160 * (p->nnode + 2) + 256);
   place_newick3_rec(p, p->root, p->branch_node[edge], q, t3, &w, buf + cap);
   snprintf(w, buf + cap - w, ";");
   return 0;
}
