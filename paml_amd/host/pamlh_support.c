/* pamlh_support.c — branch supports of the analysis's tree by the approximate likelihood-ratio test (aLRT, Anisimova & Gascuel 2006)
 * in its SH-like, non-parametric form (Guindon et al. 2010).  Per internal edge that has them (paml_amd_edge_list), the present
 * resolution and its two NNI alternatives are each maximised over the five branches around the edge with everything else held fixed
 * (pamlh_edge_optimize: every row of every edge in lock step, ONE paml_amd_edge_scores call per Newton step — no tree is set and no
 * kernel is built per neighbour); delta = 2 (l0 - max(l1, l2)); the support is the share of RELL replicates
 * (paml_amd_rell_replicates over the three configurations' per-pattern log likelihoods, genes respected) whose centred statistic
 * stays below delta (pamlh_branch_supports_from_replicates).
 *
 * The iteration of pamlh_edge_optimize, per row (a configuration of an edge with its own five lengths t, started at the tree's): a
 * cyclic, safeguarded Newton iteration.  A sweep takes the five roles (s1, s2, v, then c and f, or c1 and c2) in turn.  A role starts
 * with one call that gives every row's lnL, d1 and d2 along that branch at its accepted lengths, then makes at most EDGE_TRIALS = 4
 * calls at trial lengths: a row proposes t - d1 / d2 where d2 < 0, otherwise a step in the gradient's direction (t doubled for d1 > 0,
 * halved for d1 < 0), clipped to the bounds pamlh_optimize uses for a branch length (4e-6, 50); the next call shows the trial's lnL,
 * d1 and d2: if the lnL did not fall the trial is accepted and the next Newton step is proposed from its derivatives, otherwise the
 * step is halved from the accepted length.  A row whose step is below 1e-10 or that sits at a bound with the gradient pointing outwards
 * waits for the next role (u = -1).  No damping.  The iteration ends after a sweep in which no row gained more than 1e-6, or after
 * EDGE_MAX_SWEEPS = 30 sweeps; a row that gained no more than 1e-6 in a sweep is finished and stays in the calls with u = -1.
 * Refused by name: a clock, rho models, runmode = -2, fix_blength = 2 or 3 (the branch lengths are not parameters), a tree whose root
 * has two sons. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pamlh_internal.h"

#define EDGE_TRIALS 4
#define EDGE_MAX_SWEEPS 30
#define EDGE_T_LO 4e-6
#define EDGE_T_HI 50.0

static int support_refused(pamlh *p, const char *who)
{
   if (p->pairwise) return pamlh_fail(p, "%s: runmode = -2 has no tree whose branches to support", who);
   if (p->clock) return pamlh_fail(p, "%s: clock = %d: the five branches around an edge are not free under a clock", who, p->clock);
   if (!p->fix_rho || p->rho0 != 0) return pamlh_fail(p, "%s: rho models (auto-discrete-gamma) have no per-pattern likelihood to resample", who);
   if (p->fix_blength == 2 || p->fix_blength == 3 || !p->ntime || p->ntime != p->nbranch)
      return pamlh_fail(p, "%s: fix_blength = %d: the branch lengths are not parameters", who, p->fix_blength);
   if (p->sons_ptr[p->root + 1] - p->sons_ptr[p->root] == 2)
      return pamlh_fail(p, "%s: the root has two sons: the two branches at the root are one branch of the unrooted tree (unroot the tree)", who);
   return 0;
}

static int support_model(pamlh *p, const double *x, const char *who)
{
   int rc;
   if ((rc = pamlh_set_x(p, x, p->np))) return rc < 0 ? rc : -1;
   if (!pamlh_model_feasible(p)) return pamlh_fail(p, "%s: the model rejects the parameter vector", who);
   if ((rc = pamlh_engine_model(p))) return rc < 0 ? rc : -1;
   return 0;
}

/* The edges of the tree as it stands that have three configurations (paml_amd_edge_list): edges[*n_edges][3][3], five[*n_edges][5];
 * both NULL: the count only. */
int pamlh_edge_list(pamlh *p, int *n_edges, int *edges, int *five)
{
   int n, rc;
   if (!p || !n_edges) return -1;
   if ((rc = support_refused(p, "pamlh_edge_list"))) return rc;
   n = paml_amd_edge_list(p->ns, p->nnode, p->root, p->sons_ptr, p->sons, NULL, NULL, 0);
   if (n < 0) return pamlh_fail(p, "pamlh_edge_list: the tree has no list of edges (%d)", n);
   *n_edges = n;
   if ((edges || five) && n && paml_amd_edge_list(p->ns, p->nnode, p->root, p->sons_ptr, p->sons, edges, five, n) != n)
      return pamlh_fail(p, "pamlh_edge_list: internal: the list changed its length");
   return 0;
}

/* One row's move in the safeguarded Newton iteration along one length (pamlh_edge_optimize, pamlh_place_optimize), after the call that
 * showed ln, d1 and d2 at the trial length *tn (trial 0: at the accepted length itself).  A trial that did not fall is accepted (*ti,
 * *l) and Newton's step is proposed from its derivatives where d2 < 0, otherwise the length doubled or halved along the gradient; one
 * that fell halves the step from the accepted length; the target is clipped to [lo, hi].  Returns 1 with the next trial in *tn, or 0
 * with *tn = *ti when the row waits: the trials are used up or the step is below 1e-10. */
int pamlh_newton_trial(int trial, int max_trials, double lo, double hi, double ln, double d1, double d2, double *l, double *ti, double *tn, double *step)
{
   double s, target;
   if (trial == 0 || ln >= *l) {      /* the trial did not fall: accepted, and the next step comes from its derivatives */
      *ti = *tn;
      if (trial) *l = ln;
      if (d2 < 0) s = -d1 / d2;
      else s = d1 > 0 ? *ti : d1 < 0 ? -0.5 * *ti : 0.0;
   }
   else s = 0.5 * *step;                 /* it fell: half the step from the accepted length */
   target = fmin(fmax(*ti + s, lo), hi);
   *step = s = target - *ti;
   if (trial == max_trials || fabs(s) < 1e-10) { *tn = *ti; return 0; }
   *tn = target;
   return 1;
}

int pamlh_edge_optimize(pamlh *p, const double *x, int n_edges, const int *edges, const int *five, double *t5_out, double *l_out, int *stats)
{
   int rc, i, j, sweep = 0, calls = 0, n_rows = 3 * n_edges, role, trial, at_bound = 0, active;
   int *rows = NULL, *on = NULL;
   unsigned char *done = NULL, *wait = NULL;
   double *t = NULL, *tt = NULL, *l = NULL, *l_sweep = NULL, *step = NULL, *ln = NULL, *d1 = NULL, *d2 = NULL, l0 = 0;
   if (!p || !x || !edges || !five || !t5_out || !l_out) return p ? pamlh_fail(p, "pamlh_edge_optimize: null argument") : -1;
   if (n_edges < 1) return pamlh_fail(p, "pamlh_edge_optimize: n_edges < 1");
   if ((rc = support_refused(p, "pamlh_edge_optimize"))) return rc;
   if ((rc = support_model(p, x, "pamlh_edge_optimize"))) return rc;
   rows = (int *)malloc((size_t)4 * n_rows * sizeof(int)); on = (int *)malloc((size_t)5 * n_rows * sizeof(int));
   done = (unsigned char *)calloc(n_rows, 1); wait = (unsigned char *)calloc(n_rows, 1);
   t = (double *)malloc((size_t)5 * n_rows * sizeof(double)); tt = (double *)malloc((size_t)5 * n_rows * sizeof(double));
   l = (double *)malloc(n_rows * sizeof(double)); l_sweep = (double *)malloc(n_rows * sizeof(double)); step = (double *)calloc(n_rows, sizeof(double));
   ln = (double *)malloc(n_rows * sizeof(double)); d1 = (double *)malloc(n_rows * sizeof(double)); d2 = (double *)malloc(n_rows * sizeof(double));
   for (i = 0; i < n_rows; i++) {
      for (j = 0; j < 3; j++) rows[4 * i + j] = edges[3 * i + j];
      rows[4 * i + 3] = -1;
      for (j = 0; j < 5; j++) {
         const int c = five[5 * (i / 3) + j];
         if (c < 0 || c >= p->nnode) { rc = pamlh_fail(p, "pamlh_edge_optimize: edge %d: node %d is out of range", i / 3, c); goto done; }
         on[5 * i + j] = c;
         t[5 * i + j] = fmin(fmax(p->branch[c], EDGE_T_LO), EDGE_T_HI);
      }
   }
#define EDGE_CALL(lengths)                                                                                                                          \
   do {                                                                                                                                             \
      rc = paml_amd_edge_scores(p->eng, p->branch, p->ngene > 1 ? p->rgene : NULL, n_rows, rows, on, lengths, &l0, ln, d1, d2, NULL);               \
      calls++;                                                                                                                                      \
      if (rc) { pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); rc = rc < 0 ? rc : -1; goto done; }                                               \
   } while (0)
   EDGE_CALL(t);
   memcpy(l, ln, n_rows * sizeof(double));
   for (sweep = 0; sweep < EDGE_MAX_SWEEPS;) {
      memcpy(l_sweep, l, n_rows * sizeof(double));
      for (role = 0; role < 5; role++) {
         /* the derivatives along this role's branch at the accepted lengths, then the trials */
         for (i = 0; i < n_rows; i++) { rows[4 * i + 3] = done[i] ? -1 : on[5 * i + role]; wait[i] = done[i]; step[i] = 0; }
         memcpy(tt, t, (size_t)5 * n_rows * sizeof(double));
         for (trial = 0; trial <= EDGE_TRIALS; trial++) {
            EDGE_CALL(tt);
            active = 0;
            for (i = 0; i < n_rows; i++) {
               if (wait[i]) continue;
               if (!pamlh_newton_trial(trial, EDGE_TRIALS, EDGE_T_LO, EDGE_T_HI, ln[i], d1[i], d2[i], l + i, t + 5 * i + role, tt + 5 * i + role, step + i)) {
                  wait[i] = 1;
                  rows[4 * i + 3] = -1;
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
#undef EDGE_CALL
   for (i = 0; i < n_rows; i++) {
      int b = 0;
      for (j = 0; j < 5; j++) b |= t[5 * i + j] <= EDGE_T_LO || t[5 * i + j] >= EDGE_T_HI;
      at_bound += b;
      l_out[i] = l[i];
   }
   memcpy(t5_out, t, (size_t)5 * n_rows * sizeof(double));
   if (stats) { stats[0] = sweep; stats[1] = calls; stats[2] = at_bound; }
   rc = 0;
done:
   free(rows); free(on); free(done); free(wait); free(t); free(tt); free(l); free(l_sweep); free(step); free(ln); free(d1); free(d2);
   return rc;
}

/* lnL[n_edges][3] and lnf[n_edges][3][npatt] of every configuration at the lengths t5[n_edges][3][5] (in the order of five) and the
 * parameters of x: one engine call with u = -1 for all rows. */
int pamlh_edge_lnf(pamlh *p, const double *x, int n_edges, const int *edges, const int *five, const double *t5, double *lnL, double *lnf)
{
   int rc, i, j, n_rows = 3 * n_edges, *rows, *on;
   double *d, l0 = 0;
   if (!p || !x || !edges || !five || !t5 || !lnL || !lnf) return p ? pamlh_fail(p, "pamlh_edge_lnf: null argument") : -1;
   if (n_edges < 1) return pamlh_fail(p, "pamlh_edge_lnf: n_edges < 1");
   if ((rc = support_refused(p, "pamlh_edge_lnf"))) return rc;
   if ((rc = support_model(p, x, "pamlh_edge_lnf"))) return rc;
   rows = (int *)malloc((size_t)4 * n_rows * sizeof(int)); on = (int *)malloc((size_t)5 * n_rows * sizeof(int)); d = (double *)malloc((size_t)2 * n_rows * sizeof(double));
   for (i = 0; i < n_rows; i++) {
      for (j = 0; j < 3; j++) rows[4 * i + j] = edges[3 * i + j];
      rows[4 * i + 3] = -1;
      for (j = 0; j < 5; j++) on[5 * i + j] = five[5 * (i / 3) + j];
   }
   rc = paml_amd_edge_scores(p->eng, p->branch, p->ngene > 1 ? p->rgene : NULL, n_rows, rows, on, t5, &l0, lnL, d, d + n_rows, lnf);
   if (rc) { pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); rc = rc < 0 ? rc : -1; }
   free(rows); free(on); free(d);
   return rc;
}

/* Host only.  rep[n_rep][3 n_edges]: the replicates' sums of the rows' per-pattern log likelihoods; l3[n_edges][3]: the rows' lnL.
 * delta = 2 (l0 - max(l1, l2)).  Per row its mean over the replicates (added in replicate order) is subtracted — the centring of the
 * S-H column of the tree comparison; per edge and replicate delta*_r = 2 (largest - second largest of the three centred sums);
 * support = #{r : delta*_r < delta} / n_rep, and 0 where delta <= 0 (a better NNI neighbour exists). */
int pamlh_branch_supports_from_replicates(int n_edges, int n_rep, const double *rep, const double *l3, double *delta, double *support)
{
   int e, r, j;
   if (n_edges < 1 || n_rep < 1 || !rep || !l3 || !delta || !support) return -1;
   for (e = 0; e < n_edges; e++) {
      double mean[3] = {0, 0, 0};
      int count = 0;
      const double d = 2 * (l3[3 * e] - fmax(l3[3 * e + 1], l3[3 * e + 2]));
      delta[e] = d;
      support[e] = 0;
      if (!(d > 0)) continue;
      for (j = 0; j < 3; j++) {
         for (r = 0; r < n_rep; r++) mean[j] += rep[(size_t)r * 3 * n_edges + 3 * e + j];
         mean[j] /= n_rep;
      }
      for (r = 0; r < n_rep; r++) {
         double c[3], hi, mid;
         for (j = 0; j < 3; j++) c[j] = rep[(size_t)r * 3 * n_edges + 3 * e + j] - mean[j];
         hi = fmax(c[0], fmax(c[1], c[2]));
         mid = fmax(fmin(c[0], c[1]), fmin(fmax(c[0], c[1]), c[2]));      /* the second largest: the median of three */
         count += 2 * (hi - mid) < d;
      }
      support[e] = (double)count / n_rep;
   }
   return 0;
}

/* The list, the optimisation, one last call with the per-pattern values of all rows at the maximised lengths, the replicates, the
 * table.  edge_node = delta = support = l3 = NULL: the count only.  edge_node[*n_edges] = v (the branch above v), l3[*n_edges][3]. */
int pamlh_branch_supports(pamlh *p, const double *x, int n_rep, unsigned long long seed, int *n_edges, int *edge_node, double *delta, double *support, double *l3)
{
   int rc, n = 0, i, n_rows, stats[3];
   int *edges = NULL, *five = NULL, *goff = NULL;
   double *t5 = NULL, *l = NULL, *lnf = NULL, *rep = NULL;
   if (!p || !n_edges) return -1;
   if ((rc = pamlh_edge_list(p, &n, NULL, NULL))) return rc;
   *n_edges = n;
   if (!edge_node && !delta && !support && !l3) return 0;
   if (!x || !edge_node || !delta || !support || !l3) return pamlh_fail(p, "pamlh_branch_supports: null argument");
   if (n < 1) return pamlh_fail(p, "pamlh_branch_supports: the tree has no internal edge with three configurations");
   if (n_rep < 1) return pamlh_fail(p, "pamlh_branch_supports: n_rep < 1");
   n_rows = 3 * n;
   edges = (int *)malloc((size_t)9 * n * sizeof(int)); five = (int *)malloc((size_t)5 * n * sizeof(int));
   t5 = (double *)malloc((size_t)5 * n_rows * sizeof(double)); l = (double *)malloc(n_rows * sizeof(double));
   lnf = (double *)malloc((size_t)n_rows * p->npatt * sizeof(double)); rep = (double *)malloc((size_t)n_rep * n_rows * sizeof(double));
   goff = (int *)malloc((p->ngene + 2) * sizeof(int));
   if ((rc = pamlh_edge_list(p, &n, edges, five))) goto done;
   if ((rc = pamlh_edge_optimize(p, x, n, edges, five, t5, l, stats))) goto done;
   if ((rc = pamlh_edge_lnf(p, x, n, edges, five, t5, l, lnf))) goto done;
   for (i = 0; i < p->ngene; i++) goff[i] = p->ngene > 1 ? p->posG[i] : 0;
   goff[p->ngene] = p->npatt;
   rc = paml_amd_rell_replicates(n_rows, p->npatt, p->w, lnf, p->ngene, goff, n_rep, seed, rep);
   if (rc) { pamlh_fail(p, "%s", paml_amd_last_error(NULL)); rc = rc < 0 ? rc : -1; goto done; }
   for (i = 0; i < n; i++) edge_node[i] = edges[9 * i];
   memcpy(l3, l, n_rows * sizeof(double));
   if (pamlh_branch_supports_from_replicates(n, n_rep, rep, l3, delta, support)) rc = pamlh_fail(p, "pamlh_branch_supports: internal: the table's arguments");
done:
   free(edges); free(five); free(t5); free(l); free(lnf); free(rep); free(goff);
   return rc;
}

static void support_newick_rec(const pamlh *p, int node, const double *sup_of, char **w, char *end)
{
   int j;
   if (node < p->ns) *w += snprintf(*w, end - *w, "%s", p->names[node]);
   else {
      *w += snprintf(*w, end - *w, "(");
      for (j = p->sons_ptr[node]; j < p->sons_ptr[node + 1]; j++) {
         if (j > p->sons_ptr[node]) *w += snprintf(*w, end - *w, ", ");
         support_newick_rec(p, p->sons[j], sup_of, w, end);
      }
      *w += snprintf(*w, end - *w, ")");
      if (sup_of[node] >= 0) *w += snprintf(*w, end - *w, "%.3f", sup_of[node]);
   }
   if (node != p->root) {
      if (p->label[node]) *w += snprintf(*w, end - *w, " #%d", p->label[node]);
      *w += snprintf(*w, end - *w, ": %.6f", p->branch[node]);
   }
}

/* pamlh_newick with the supports as the labels of the internal nodes below the supported branches (buf needs 80 bytes per node + 128) */
int pamlh_newick_supports(const pamlh *p, int n_edges, const int *edge_node, const double *support, char *buf, int cap)
{
   char *w = buf;
   int i;
   double *sup_of;
   if (!p || !buf || cap < 80 * p->nnode + 128 || (n_edges > 0 && (!edge_node || !support))) return -1;
   sup_of = (double *)malloc(p->nnode * sizeof(double));
   for (i = 0; i < p->nnode; i++) sup_of[i] = -1;
   for (i = 0; i < n_edges; i++)
      if (edge_node[i] >= 0 && edge_node[i] < p->nnode) sup_of[edge_node[i]] = support[i];
   support_newick_rec(p, p->root, sup_of, &w, buf + cap);
   snprintf(w, buf + cap - w, ";");
   free(sup_of);
   return 0;
}
