/* pamlh_hessian.c — what the exact Hessian of lnL over the branch lengths (paml_amd_hessian: one engine call) serves on the host.
 *
 * pamlh_branch_hessian_exact   lnL, g and the ntime x ntime block H_ij = d2 lnL / d t_i d t_j in pamlh_branch_order.  (pamlh_branch_hessian
 *                              is the outer product of scores, an estimate of the information; this is the Hessian itself.)
 * pamlh_write_bv_exact         the block pamlh_write_bv writes for mcmctree's in.BV, with this Hessian.
 * pamlh_standard_errors_exact  the observed information over all free parameters in three blocks: branch x branch from the call; branch x
 *                              model parameter from central differences of the branch gradient (paml_amd_gradient, the engine call under
 *                              pamlh_gradient's branch block) at x +- h e_i, two calls per model parameter; model x model by
 *                              pamlh_standard_errors method 1's second-difference stencil restricted to the model parameters
 *                              (2 m^2 + 1 evaluations in one batch).  h = 1e-4 (|x_i| + 1) as there; the parameters method 1 leaves out
 *                              at a bound are left out here too and get se = -1; the matrix is inverted as a whole.
 * pamlh_newton_full            pamlh_newton_branches with the step from the whole block: on the branches inside the box, or pushed inwards
 *                              by their gradient, (-H + lambda I) d = g by Cholesky, lambda = 0 first and raised (1e-3 of the largest
 *                              diagonal entry, then tenfold) until the factorisation succeeds.  The trust-factor cap, the clipping, the
 *                              accept / reject rule and the termination test are those of pamlh_newton_branches; a sweep is one engine
 *                              call; lnL never decreases from entry to exit.
 * Refused by name, as pamlh_curvature refuses them: a clock (x holds ages), fix_blength = 2 or 3, rho != 0, a rate-matrix (UNREST)
 * model, a pattern shard. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pamlh_internal.h"

#define NEWTON_FLOOR 0.01

static int hess_refused(pamlh *p, const char *who)
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
static int hess_model(pamlh *p, const double *x, const char *who)
{
   int rc;
   if ((rc = pamlh_set_x(p, x, p->np))) return rc < 0 ? rc : -1;
   if (!pamlh_model_feasible(p)) return pamlh_fail(p, "%s: the model rejects the parameter vector", who);
   if (p->adg) return pamlh_fail(p, "%s: rho models (auto-discrete-gamma): the sites are not independent", who);
   if ((rc = hess_refused(p, who))) return rc;      /* (the eigen kinds are known once the model state is set) */
   if ((rc = pamlh_engine_model(p))) return rc < 0 ? rc : -1;
   return 0;
}

/* one paml_amd_hessian call at the lengths t[ntime] (NULL: the model state's own): L, g[ntime], H[ntime][ntime] in pamlh_branch_order.
 * br, gn: room for nnode doubles each. */
static int hess_call(pamlh *p, const double *t, double *br, double *gn, double *L, double *g, double *H)
{
   int i, rc;
   memcpy(br, p->branch, p->nnode * sizeof(double));
   if (t) for (i = 0; i < p->ntime; i++) br[p->branch_node[i]] = t[i];
   rc = paml_amd_hessian(p->eng, br, p->ngene > 1 ? p->rgene : NULL, p->branch_node, p->ntime, L, gn, H, NULL);
   if (rc) { pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); return rc < 0 ? rc : -1; }
   for (i = 0; i < p->ntime; i++) g[i] = gn[p->branch_node[i]];
   return 0;
}

int pamlh_branch_hessian_exact(pamlh *p, const double *x, double *lnL, double *g, double *H)
{
   double *w;
   int rc;
   if (!p || !x || !lnL || !g || !H) return p ? pamlh_fail(p, "pamlh_branch_hessian_exact: null argument") : -1;
   if ((rc = hess_refused(p, "pamlh_branch_hessian_exact"))) return rc;
   if ((rc = hess_model(p, x, "pamlh_branch_hessian_exact"))) return rc;
   w = (double *)malloc((size_t)2 * p->nnode * sizeof(double));
   rc = hess_call(p, NULL, w, w + p->nnode, lnL, g, H);
   free(w);
   return rc;
}

/* pamlh_write_bv's block (baseml.c:581-596) with the exact Hessian */
int pamlh_write_bv_exact(pamlh *p, const double *x, const char *path)
{
   int nt, i, j, rc;
   double *g, *H, lnL;
   char *nw;
   FILE *f;
   if (!p || !x || !path) return p ? pamlh_fail(p, "pamlh_write_bv_exact: null argument") : -1;
   if ((rc = hess_refused(p, "pamlh_write_bv_exact"))) return rc;
   nt = p->ntime;
   if (p->sons_ptr[p->root + 1] - p->sons_ptr[p->root] != 3)
      return pamlh_fail(p, "--bv: the gradient and Hessian of the branch lengths are written for an unrooted tree (three sons at the root) without a clock, as the reference does");
   g = (double *)malloc(((size_t)nt * (nt + 1) + 1) * sizeof(double)); H = g + nt;
   if ((rc = pamlh_branch_hessian_exact(p, x, &lnL, g, H))) { free(g); return rc; }
   nw = (char *)malloc((size_t)160 * p->nnode + 256);
   if (pamlh_set_x(p, x, p->np) || pamlh_newick(p, nw, 160 * p->nnode + 256)) { free(g); free(nw); return pamlh_fail(p, "--bv: no tree to write"); }
   if (!(f = fopen(path, "w"))) { free(g); free(nw); return pamlh_fail(p, "--bv: cannot write %s", path); }
   fprintf(f, "\n %d\n\n%s\n\n", p->ns, nw);
   for (i = 0; i < nt; i++) if (x[i] > 0.0004 && fabs(g[i]) < 0.005) g[i] = 0;
   for (i = 0; i < nt; i++) fprintf(f, " %9.6f", x[i]);
   fprintf(f, "\n\n");
   for (i = 0; i < nt; i++) fprintf(f, " %9.6f", g[i]);
   fprintf(f, "\n\n\nHessian\n\n");
   for (i = 0; i < nt; i++) {
      for (j = 0; j < nt; j++) fprintf(f, " %10.4g", H[i * nt + j]);
      fprintf(f, "\n");
   }
   fclose(f);
   free(g); free(nw);
   return 0;
}

/* Cholesky factor of the nf x nf matrix A (row-major, lower triangle written in place); returns 0, or -1 when A is not positive definite */
static int cholesky(double *A, int nf)
{
   int i, j, k;
   for (j = 0; j < nf; j++) {
      double d = A[j * nf + j];
      for (k = 0; k < j; k++) d -= A[j * nf + k] * A[j * nf + k];
      if (!(d > 0) || !(d < 1e300)) return -1;
      d = sqrt(d);
      A[j * nf + j] = d;
      for (i = j + 1; i < nf; i++) {
         double s = A[i * nf + j];
         for (k = 0; k < j; k++) s -= A[i * nf + k] * A[j * nf + k];
         A[i * nf + j] = s / d;
      }
   }
   return 0;
}

/* b := A^-1 b from A's Cholesky factor */
static void cholesky_solve(const double *A, int nf, double *b)
{
   int i, k;
   for (i = 0; i < nf; i++) {
      double s = b[i];
      for (k = 0; k < i; k++) s -= A[i * nf + k] * b[k];
      b[i] = s / A[i * nf + i];
   }
   for (i = nf - 1; i >= 0; i--) {
      double s = b[i];
      for (k = i + 1; k < nf; k++) s -= A[k * nf + i] * b[k];
      b[i] = s / A[i * nf + i];
   }
}

/* Gauss-Jordan inverse of the nf x nf matrix M (row-major, destroyed) with partial pivoting; returns 0, or -1 when singular */
static int invert(double *M, int nf, double *inv)
{
   int i, j, k;
   for (i = 0; i < nf; i++)
      for (j = 0; j < nf; j++) inv[i * nf + j] = (i == j);
   for (k = 0; k < nf; k++) {
      int piv = k;
      double d;
      for (i = k + 1; i < nf; i++)
         if (fabs(M[i * nf + k]) > fabs(M[piv * nf + k])) piv = i;
      if (fabs(M[piv * nf + k]) < 1e-300) return -1;
      if (piv != k)
         for (j = 0; j < nf; j++) {
            d = M[k * nf + j]; M[k * nf + j] = M[piv * nf + j]; M[piv * nf + j] = d;
            d = inv[k * nf + j]; inv[k * nf + j] = inv[piv * nf + j]; inv[piv * nf + j] = d;
         }
      d = M[k * nf + k];
      for (j = 0; j < nf; j++) { M[k * nf + j] /= d; inv[k * nf + j] /= d; }
      for (i = 0; i < nf; i++)
         if (i != k && M[i * nf + k] != 0) {
            d = M[i * nf + k];
            for (j = 0; j < nf; j++) { M[i * nf + j] -= d * M[k * nf + j]; inv[i * nf + j] -= d * inv[k * nf + j]; }
         }
   }
   return 0;
}

int pamlh_standard_errors_exact(pamlh *p, const double *x, double *se, double *hess)
{
   const char *who = "pamlh_standard_errors_exact";
   int n, nt, nm, i, j, rc, nf = 0, *freev = NULL;
   double *lo = NULL, *hi, *h, *H = NULL, *Hb = NULL, *gb, *gp, *gm, *br, *gn, *xt = NULL, *xs = NULL, *ls = NULL, *A = NULL, *Ai = NULL, lnL;
   if (!p || !x || !se) return p ? pamlh_fail(p, "%s: null argument", who) : -1;
   if ((rc = hess_refused(p, who))) return rc;
   n = p->np; nt = p->ntime; nm = n - nt;
   lo = (double *)malloc(((size_t)3 * n + 3) * sizeof(double)); hi = lo + n + 1; h = hi + n + 1;
   H = (double *)calloc((size_t)n * n + 1, sizeof(double));
   Hb = (double *)malloc(((size_t)nt * nt + 3 * nt + 2 * p->nnode + 1) * sizeof(double)); gb = Hb + (size_t)nt * nt; gp = gb + nt; gm = gp + nt; br = gm + nt; gn = br + p->nnode;
   xt = (double *)malloc(((size_t)n + 1) * sizeof(double));
   freev = (int *)malloc(((size_t)n + 1) * sizeof(int));
   if (pamlh_bounds(p, lo, hi)) { rc = pamlh_fail(p, "internal: bounds do not match np"); goto done; }
   for (i = 0; i < n; i++) {
      se[i] = -1;
      h[i] = 1e-4 * (fabs(x[i]) + 1);
      if (x[i] - h[i] >= lo[i] && x[i] + h[i] <= hi[i]) freev[nf++] = i;
   }
   /* branch x branch: the call */
   if ((rc = hess_model(p, x, who))) goto done;
   if ((rc = hess_call(p, NULL, br, gn, &lnL, gb, Hb))) goto done;
   for (i = 0; i < nt; i++)
      for (j = 0; j < nt; j++) H[i * n + j] = -Hb[i * nt + j];
   /* branch x model parameter: central differences of the branch gradient, two engine calls per model parameter */
   for (i = nt; i < n; i++) {
      int side;
      if (!(x[i] - h[i] >= lo[i] && x[i] + h[i] <= hi[i])) continue;
      for (side = 0; side < 2; side++) {
         double *gs = side ? gm : gp;
         memcpy(xt, x, n * sizeof(double));
         xt[i] = x[i] + (side ? -h[i] : h[i]);
         if ((rc = hess_model(p, xt, who))) goto done;
         rc = paml_amd_gradient(p->eng, p->branch, p->ngene > 1 ? p->rgene : NULL, &lnL, gn, NULL, NULL);
         if (rc) { pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); rc = rc < 0 ? rc : -1; goto done; }
         for (j = 0; j < nt; j++) gs[j] = gn[p->branch_node[j]];
      }
      for (j = 0; j < nt; j++) H[i * n + j] = H[j * n + i] = -(gp[j] - gm[j]) / (2 * h[i]);
   }
   if (nm) { if ((rc = pamlh_set_x(p, x, n))) { rc = rc < 0 ? rc : -1; goto done; } }
   /* model x model: method 1's stencil over the model parameters, one batch */
   {
      int nfm = 0, *fm;      /* the model parameters among the free ones */
      size_t q = 0, npts;
      for (i = 0; i < nf; i++) if (freev[i] >= nt) nfm++;
      fm = (int *)malloc(((size_t)nfm + 1) * sizeof(int));
      for (i = 0, nfm = 0; i < nf; i++) if (freev[i] >= nt) fm[nfm++] = freev[i];
      npts = (size_t)2 * nfm * nfm + 1;
      if (nfm) {
         xs = (double *)malloc(npts * n * sizeof(double));
         ls = (double *)malloc(npts * sizeof(double));
#define PT(di, si, dj, sj)                                                                                       \
   do {                                                                                                          \
      double *v = xs + q * n;                                                                                    \
      memcpy(v, x, n * sizeof(double));                                                                          \
      v[di] += (si) * h[di];                                                                                     \
      if ((dj) >= 0) v[dj] += (sj) * h[dj];                                                                      \
      q++;                                                                                                       \
   } while (0)
         memcpy(xs, x, n * sizeof(double));
         q = 1;
         for (i = 0; i < nfm; i++) { PT(fm[i], +1, -1, 0); PT(fm[i], -1, -1, 0); }
         for (i = 0; i < nfm; i++)
            for (j = i + 1; j < nfm; j++) { PT(fm[i], +1, fm[j], +1); PT(fm[i], +1, fm[j], -1); PT(fm[i], -1, fm[j], +1); PT(fm[i], -1, fm[j], -1); }
#undef PT
         if ((rc = pamlh_eval_batch_gpu(p, (int)q, xs, ls))) { free(fm); goto done; }
         q = 1;
         for (i = 0; i < nfm; i++, q += 2) {
            const int a = fm[i];
            H[a * n + a] = -(ls[q] - 2 * ls[0] + ls[q + 1]) / (h[a] * h[a]);
         }
         for (i = 0; i < nfm; i++)
            for (j = i + 1; j < nfm; j++, q += 4) {
               const int a = fm[i], b = fm[j];
               H[a * n + b] = H[b * n + a] = -(ls[q] - ls[q + 1] - ls[q + 2] + ls[q + 3]) / (4 * h[a] * h[b]);
            }
      }
      free(fm);
   }
   if (hess) memcpy(hess, H, (size_t)n * n * sizeof(double));
   A = (double *)malloc((size_t)nf * nf * sizeof(double) + 8);
   Ai = (double *)malloc((size_t)nf * nf * sizeof(double) + 8);
   for (i = 0; i < nf; i++)
      for (j = 0; j < nf; j++) A[i * nf + j] = H[freev[i] * n + freev[j]];
   if (invert(A, nf, Ai)) { rc = pamlh_fail(p, "%s: the information matrix is singular", who); goto done; }
   for (i = 0; i < nf; i++) se[freev[i]] = Ai[i * nf + i] > 0 ? sqrt(Ai[i * nf + i]) : -1;
   if ((rc = pamlh_set_x(p, x, n))) rc = rc < 0 ? rc : -1;
done:
   free(lo); free(H); free(Hb); free(xt); free(freev); free(xs); free(ls); free(A); free(Ai);
   return rc;
}

int pamlh_newton_full(pamlh *p, double *x, double e, int max_sweeps, double *lnL, int verbose, int *stats)
{
   const char *who = "pamlh_newton_full";
   int rc, i, j, nt, sweep = 0, calls = 0, rejected = 0, *fr = NULL;
   double *w = NULL, *t, *tn, *g, *g1, *trust, *lo, *hi, *br, *gn, *d, *H = NULL, *H1 = NULL, *A = NULL, L = 0, L1 = 0;
   if (!p || !x || !lnL) return p ? pamlh_fail(p, "%s: null argument", who) : -1;
   if ((rc = hess_refused(p, who))) return rc;
   if ((rc = hess_model(p, x, who))) return rc;
   nt = p->ntime;
   w = (double *)malloc(((size_t)6 * nt + 2 * p->np + 2 * p->nnode + 8) * sizeof(double));
   t = w; tn = t + nt; g = tn + nt; g1 = g + nt; trust = g1 + nt; d = trust + nt; lo = d + nt; hi = lo + p->np; br = hi + p->np; gn = br + p->nnode;
   H = (double *)malloc(((size_t)3 * nt * nt + 1) * sizeof(double)); H1 = H + (size_t)nt * nt; A = H1 + (size_t)nt * nt;
   fr = (int *)malloc(((size_t)nt + 1) * sizeof(int));
   if (pamlh_bounds(p, lo, hi)) { rc = pamlh_fail(p, "internal: bounds do not match np"); goto done; }
   for (i = 0; i < nt; i++) { t[i] = fmin(fmax(x[i], lo[i]), hi[i]); trust[i] = 1; }
   if ((rc = hess_call(p, t, br, gn, &L, g, H))) goto done;
   calls++;
   if (verbose) fprintf(stderr, "\tnewton-full sweep  0: lnL %.6f\n", L);
   while (sweep < max_sweeps) {
      double maxstep = 0, gain, lambda = 0, dmax = 0;
      int nf = 0;
      /* the branches that can move: inside the box, or on it and pushed inwards by the gradient */
      for (i = 0; i < nt; i++) {
         d[i] = 0;
         if ((t[i] <= lo[i] && !(g[i] > 0)) || (t[i] >= hi[i] && !(g[i] < 0))) continue;
         fr[nf++] = i;
         dmax = fmax(dmax, fabs(H[i * nt + i]));
      }
      for (;;) {      /* (-H + lambda I) d = g on them */
         for (i = 0; i < nf; i++)
            for (j = 0; j < nf; j++) A[i * nf + j] = -H[fr[i] * nt + fr[j]] + (i == j ? lambda : 0.0);
         if (!nf || !cholesky(A, nf)) break;
         lambda = lambda > 0 ? 10 * lambda : 1e-3 * fmax(dmax, 1e-6);
         if (!(lambda < 1e300)) { nf = 0; break; }
      }
      if (nf) {
         for (i = 0; i < nf; i++) tn[i] = g[fr[i]];      /* (tn as the right-hand side, before it holds the new lengths) */
         cholesky_solve(A, nf, tn);
         for (i = 0; i < nf; i++) d[fr[i]] = tn[i];
      }
      for (i = 0; i < nt; i++) {
         const double b = fmax(t[i], NEWTON_FLOOR), cap = trust[i] * b;
         double s = d[i];
         if (!(s == s)) s = 0;      /* (NaN) */
         s = fmin(fmax(s, -0.75 * cap), cap);
         tn[i] = fmin(fmax(t[i] + s, lo[i]), hi[i]);
         maxstep = fmax(maxstep, fabs(tn[i] - t[i]));
      }
      if (maxstep == 0) break;
      if ((rc = hess_call(p, tn, br, gn, &L1, g1, H1))) goto done;
      calls++; sweep++;
      if (L1 >= L) {      /* the step stands */
         gain = L1 - L;
         for (i = 0; i < nt; i++) {
            if (g1[i] * g[i] < 0) { if (fabs(g1[i]) > 0.5 * fabs(g[i])) trust[i] *= 0.5; }
            else trust[i] = fmin(2 * trust[i], 1.0);
         }
         memcpy(t, tn, nt * sizeof(double)); memcpy(g, g1, nt * sizeof(double)); memcpy(H, H1, (size_t)nt * nt * sizeof(double));
         L = L1;
         if (verbose) fprintf(stderr, "\tnewton-full sweep %2d: lnL %.6f (gain %.3g, largest step %.3g, lambda %.3g)\n", sweep, L, gain, maxstep, lambda);
         if (gain < e && maxstep < sqrt(e)) break;
      }
      else {              /* lnL fell: the previous lengths stay, shorter steps from them */
         rejected++;
         for (i = 0; i < nt; i++) trust[i] *= g1[i] * g[i] < 0 ? 0.25 : 0.5;
         if (verbose) fprintf(stderr, "\tnewton-full sweep %2d: rejected (lnL %.6f < %.6f, largest step %.3g)\n", sweep, L1, L, maxstep);
      }
   }
   for (i = 0; i < nt; i++) x[i] = t[i];
   *lnL = L;
   if ((rc = pamlh_set_x(p, x, p->np))) rc = rc < 0 ? rc : -1;      /* (the state is left at the x returned) */
done:
   if (stats) { stats[0] = sweep; stats[1] = calls; stats[2] = rejected; }
   free(w); free(H); free(fr);
   return rc;
}
