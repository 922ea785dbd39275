/* pamlh_newton.c — branch-length maximisation by Newton steps on EVERY branch at once, from the engine call that returns lnL, the
 * gradient and the curvature along every branch (paml_amd_curvature).  Where pamlh_minbranches walks the tree one branch at a time on
 * paml_amd_eval_branch — at least 2 (n - 1) dependent engine calls per sweep — a sweep here is ONE call.
 *
 * pamlh_newton_branches, per sweep, with t the accepted lengths and L, g, h the call's results there:
 *   step      d_v = -g_v / h_v where h_v < 0; otherwise a step of the gradient's sign and of the size b_v = max(t_v, NEWTON_FLOOR)
 *   trust     |d_v| <= trust_v b_v upwards and 0.75 trust_v b_v downwards (a branch is never cut below a quarter of its length in one
 *             sweep), trust_v = 1 at the start; then t_v + d_v is clipped to the box of pamlh_bounds
 *   test      the next call, at t + d, is also the test of the step.  lnL fell: t stays, every trust_v is halved, and those of the branches
 *             whose gradient changed sign (they overshot) are quartered; the call's derivatives are dropped.  lnL did not fall: t + d is
 *             accepted with its L, g, h; trust_v doubles up to 1, except where the gradient changed sign — it stays, and is halved where
 *             the new |g_v| is still more than half the old one
 *   end       an accepted sweep that gained less than e with max |d| < sqrt(e), no branch able to move, or max_sweeps sweeps (accepted
 *             and rejected both count)
 * The diagonal of the Hessian ignores the cross derivatives, so near the maximum the iteration converges linearly (measured on random
 * 9-tip trees: a factor of about six per sweep), not quadratically; profiles/curvature_times.txt has what that costs and gains.
 * lnL never decreases from entry to exit: only accepted points replace x.
 * Refused by name: a clock (x holds ages), fix_blength = 2 or 3 (the branch lengths are not parameters), rho != 0 (the sites are not
 * independent), a rate-matrix (UNREST) model, a pattern shard (the engine call is for one rank). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pamlh_internal.h"

#define NEWTON_FLOOR 0.01

static int newton_refused(pamlh *p, const char *who)
{
   int i;
   if (p->pairwise) return pamlh_fail(p, "%s: runmode = -2 has no tree", who);
   if (p->clock) return pamlh_fail(p, "%s: clock = %d: x holds node ages, not branch lengths", who, p->clock);
   if (p->fix_blength == 2 || p->fix_blength == 3 || !p->ntime || p->ntime != p->nbranch)
      return pamlh_fail(p, "%s: fix_blength = %d: the branch lengths are not parameters", who, p->fix_blength);
   if (!p->fix_rho || p->rho0 != 0) return pamlh_fail(p, "%s: rho models (auto-discrete-gamma): the sites are not independent", who);
   if (p->shard_world > 1) return pamlh_fail(p, "%s: a pattern shard (%d ranks): the engine call is for one rank", who, p->shard_world);
   for (i = 0; i < p->n_eigen; i++)
      if (p->eig[i].kind == PAML_AMD_EIGEN_QMAT) return pamlh_fail(p, "%s: a rate-matrix (UNREST) model has no analytic branch derivatives", who);
   return 0;
}

/* the model state and the engine's model at x */
static int newton_model(pamlh *p, const double *x, const char *who)
{
   int rc;
   if ((rc = pamlh_set_x(p, x, p->np))) return rc < 0 ? rc : -1;
   if (!pamlh_model_feasible(p)) return pamlh_fail(p, "%s: the model rejects the parameter vector", who);
   if (p->adg) return pamlh_fail(p, "%s: rho models (auto-discrete-gamma): the sites are not independent", who);
   if ((rc = newton_refused(p, who))) return rc;      /* (the eigen kinds are known once the model state is set) */
   if ((rc = pamlh_engine_model(p))) return rc < 0 ? rc : -1;
   return 0;
}

/* one paml_amd_curvature call at the lengths t[ntime] (NULL: the model state's own): L, g[ntime], h[ntime] in pamlh_branch_order.
 * gn: room for 2 nnode doubles, br: for nnode. */
static int newton_call(pamlh *p, const double *t, double *br, double *gn, double *L, double *g, double *h)
{
   int i, rc;
   memcpy(br, p->branch, p->nnode * sizeof(double));
   if (t) for (i = 0; i < p->ntime; i++) br[p->branch_node[i]] = t[i];
   rc = paml_amd_curvature(p->eng, br, p->ngene > 1 ? p->rgene : NULL, L, gn, gn + p->nnode, NULL);
   if (rc) { pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); return rc < 0 ? rc : -1; }
   for (i = 0; i < p->ntime; i++) { g[i] = gn[p->branch_node[i]]; h[i] = gn[p->nnode + p->branch_node[i]]; }
   return 0;
}

int pamlh_curvature(pamlh *p, const double *x, double *lnL, double *g, double *h)
{
   double *w;
   int rc;
   if (!p || !x || !lnL || !g || !h) return p ? pamlh_fail(p, "pamlh_curvature: null argument") : -1;
   if ((rc = newton_refused(p, "pamlh_curvature"))) return rc;
   if ((rc = newton_model(p, x, "pamlh_curvature"))) return rc;
   w = (double *)malloc((size_t)3 * p->nnode * sizeof(double));
   rc = newton_call(p, NULL, w + 2 * p->nnode, w, lnL, g, h);
   free(w);
   return rc;
}

int pamlh_newton_branches(pamlh *p, double *x, double e, int max_sweeps, double *lnL, int verbose, int *stats)
{
   int rc, i, nt, sweep = 0, calls = 0, rejected = 0;
   double *w = NULL, *t, *tn, *g, *h, *g1, *h1, *trust, *lo, *hi, *br, *gn, L = 0, L1 = 0;
   if (!p || !x || !lnL) return p ? pamlh_fail(p, "pamlh_newton_branches: null argument") : -1;
   if ((rc = newton_refused(p, "pamlh_newton_branches"))) return rc;
   if ((rc = newton_model(p, x, "pamlh_newton_branches"))) return rc;
   nt = p->ntime;
   w = (double *)malloc(((size_t)7 * nt + 2 * p->np + 3 * p->nnode + 8) * sizeof(double));
   t = w; tn = t + nt; g = tn + nt; h = g + nt; g1 = h + nt; h1 = g1 + nt; trust = h1 + nt; lo = trust + nt; hi = lo + p->np; br = hi + p->np; gn = br + p->nnode;
   if (pamlh_bounds(p, lo, hi)) { rc = pamlh_fail(p, "internal: bounds do not match np"); goto done; }
   for (i = 0; i < nt; i++) { t[i] = fmin(fmax(x[i], lo[i]), hi[i]); trust[i] = 1; }
   if ((rc = newton_call(p, t, br, gn, &L, g, h))) goto done;
   calls++;
   if (verbose) fprintf(stderr, "\tnewton sweep  0: lnL %.6f\n", L);
   while (sweep < max_sweeps) {
      double maxstep = 0, gain;
      for (i = 0; i < nt; i++) {
         const double b = fmax(t[i], NEWTON_FLOOR), cap = trust[i] * b;
         double s = h[i] < 0 ? -g[i] / h[i] : g[i] > 0 ? b : g[i] < 0 ? -b : 0.0;
         if (!(s == s)) s = 0;      /* (NaN) */
         s = fmin(fmax(s, -0.75 * cap), cap);
         tn[i] = fmin(fmax(t[i] + s, lo[i]), hi[i]);
         maxstep = fmax(maxstep, fabs(tn[i] - t[i]));
      }
      if (maxstep == 0) break;
      if ((rc = newton_call(p, tn, br, gn, &L1, g1, h1))) goto done;
      calls++; sweep++;
      if (L1 >= L) {      /* the step stands */
         gain = L1 - L;
         for (i = 0; i < nt; i++) {
            if (g1[i] * g[i] < 0) { if (fabs(g1[i]) > 0.5 * fabs(g[i])) trust[i] *= 0.5; }
            else trust[i] = fmin(2 * trust[i], 1.0);
         }
         memcpy(t, tn, nt * sizeof(double)); memcpy(g, g1, nt * sizeof(double)); memcpy(h, h1, nt * sizeof(double));
         L = L1;
         if (verbose) fprintf(stderr, "\tnewton sweep %2d: lnL %.6f (gain %.3g, largest step %.3g)\n", sweep, L, gain, maxstep);
         if (gain < e && maxstep < sqrt(e)) break;
      }
      else {              /* lnL fell: the previous lengths stay, shorter steps from them */
         rejected++;
         for (i = 0; i < nt; i++) trust[i] *= g1[i] * g[i] < 0 ? 0.25 : 0.5;
         if (verbose) fprintf(stderr, "\tnewton sweep %2d: rejected (lnL %.6f < %.6f, largest step %.3g)\n", sweep, L1, L, maxstep);
      }
   }
   for (i = 0; i < nt; i++) x[i] = t[i];
   *lnL = L;
   if ((rc = pamlh_set_x(p, x, p->np))) rc = rc < 0 ? rc : -1;      /* (the state is left at the x returned) */
done:
   if (stats) { stats[0] = sweep; stats[1] = calls; stats[2] = rejected; }
   free(w);
   return rc;
}

/* pamlh_optimize_minb with pamlh_newton_branches in the place of pamlh_minbranches: the same alternation, tolerances and ending.
 * n_eval: evaluations spent on the other parameters plus the engine calls of the branch steps, one each. */
int pamlh_optimize_newton(pamlh *p, double *x, double *lnL, double e0, int verbose, int *n_eval_out)
{
   int np, npcom, maxr, ir, i, rc = 0, status = 1, n_eval = 0, ne, calm = 0, st[3] = {0, 0, 0};
   double e, e_nb, L = 0, L0 = -1e300, dl;
   unsigned char *frozen;
   if (!p || !x || !lnL) return p ? pamlh_fail(p, "pamlh_optimize_newton: null argument") : -1;
   if ((rc = newton_refused(p, "pamlh_optimize_newton"))) return rc;
   np = p->np; npcom = np - p->ntime; maxr = npcom ? 200 : 1;
   e = npcom ? 5.0 : e0; e_nb = e;
   frozen = (unsigned char *)calloc(np ? np : 1, 1);
   for (i = 0; i < p->ntime; i++) frozen[i] = 1;
   for (ir = 0; ir < maxr; ir++) {
      if (npcom) {
         p->frozen = frozen; p->opt_lean = calm ? 2 : 1; p->opt_abs_tol = e;
         rc = pamlh_optimize(p, x, &L, e > 0.05 ? 2 : 30, 1e-10, 0, &ne);
         p->frozen = NULL; p->opt_lean = 0; p->opt_abs_tol = 0;
         n_eval += ne;
         if (rc < 0) goto done;
         if (verbose) fprintf(stderr, "round %da: parameters, lnL %.6f (%d evaluations)\n", ir + 1, L, ne);
      }
      if ((rc = pamlh_newton_branches(p, x, e_nb, 50, &L, verbose > 1, st))) { n_eval += st[1]; goto done; }
      n_eval += st[1];
      if (verbose) fprintf(stderr, "round %db: branch lengths, lnL %.6f (e = %.3g, %d sweeps, %d rejected)\n", ir + 1, L, e_nb, st[0], st[2]);
      dl = fabs(L - L0);
      calm = (dl < e0 && e <= 0.02) ? calm + 1 : 0;
      if (calm >= 2 || (calm && !npcom)) { status = 0; break; }
      e /= 2; if (dl < 1) e /= 2;
      if (dl < 0.5) e = fmin(e, 1e-3);
      else if (dl > 10) e = fmax(e, 0.1);
      e_nb = fmax(e, 1e-6);
      e = fmax(e, 1e-6);
      L0 = L;
   }
   if (!npcom) status = 0;
   /* one ordinary evaluation at the estimate (also leaves the model state there), as minB */
   if (pamlh_set_x(p, x, np)) { rc = -1; goto done; }
   if ((rc = pamlh_eval_gpu(p, lnL, NULL))) goto done;
   n_eval++;
   if (fabs(*lnL - L) > 1e-6 * (fabs(L) + 1)) rc = pamlh_fail(p, "optimize_newton: lnL %.9f after the last round, %.9f on re-evaluation", L, *lnL);
done:
   free(frozen);
   p->frozen = NULL; p->opt_lean = 0; p->opt_abs_tol = 0;
   if (n_eval_out) *n_eval_out = n_eval;
   return rc ? rc : status;
}
