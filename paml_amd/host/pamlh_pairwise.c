/* pamlh_pairwise.c — codeml runmode = -2: maximum-likelihood t, kappa, omega and from them dN, dS for every pair of sequences
 * (PairwiseCodon codeml.c:4344-4604; Goldman & Yang 1994).
 *
 * The reference runs the ns (ns - 1) / 2 searches one after another.  Here they run IN LOCK STEP: every pair carries its own bounded
 * quasi-Newton state (BFGS on the free parameters among t, kappa, omega; the method of pamlh_opt.c cut down to three parameters and
 * many independent problems, which that file's single-model driver cannot hold), and each round gathers the points all unfinished
 * pairs want evaluated — the 2 np central-difference points of their gradients, then the trial steps of their line searches — into ONE
 * paml_amd_pairset_eval call.  Bounds as in the reference: t in [1e-5, 50], kappa in [0.4, 999], omega in [0.001, 99]
 * (codeml.c:4359-4360, 4468); fix_kappa / fix_omega are honoured.
 *
 * Starting values.  The reference's are random (codeml.c:4461-4480); these are a fixed rule:
 *   t0     = 3 d, d the Jukes-Cantor distance of the pair's proportion of differing nucleotides (from the pair's count table), kept in [0.01, 3];
 *   kappa0 = the control file's kappa when it lies in [0.4, 10], else 2;   omega0 = the control file's omega kept in [0.05, 2].
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pamlh_internal.h"

#define PW_OUT 9      /* t, kappa, omega, lnL, S, N, dN, dS, evaluations */

int pamlh_is_pairwise(const pamlh *p) { return p ? p->pairwise : 0; }
const char *pamlh_seq_name(const pamlh *p, int i) { return p && i >= 0 && i < p->ns ? p->names[i] : NULL; }
int pamlh_pairwise_n(const pamlh *p) { return p && p->pairwise ? p->ns * (p->ns - 1) / 2 : 0; }

/* pi of a pair from its count table fp[n][n] (row = the larger state) by GetCodonFreqs2 (codeml.c:4169-4216) after the observed
 * frequencies of codeml.c:4448-4451; CodonFreq 0 (equal), 1 (F1x4), 2 (F3x4), 3 (the observed codon frequencies). */
int pamlh_pairwise_freqs(const pamlh *p, const double *fp, double ls, double *pi)
{
   const int n = p->n;
   int from61[64], i, j, k, m = 0;
   double fb3x4[12] = {0}, fb4[4] = {0}, s = 0;
   if (!p->pairwise || !(ls > 0)) return -1;
   for (i = 0; i < 64; i++) if (p->code[i] != '*') from61[m++] = i;
   for (i = 0; i < n; i++) pi[i] = 0;
   for (j = 0; j < n; j++)
      for (k = 0; k <= j; k++)
         if (fp[j * n + k] != 0) { pi[j] += fp[j * n + k] / (2. * ls); pi[k] += fp[j * n + k] / (2. * ls); }
   if (p->codonfreq == 0) { for (i = 0; i < n; i++) pi[i] = 1. / n; return 0; }
   if (p->codonfreq == 3) return 0;
   for (i = 0; i < n; i++) {
      const int ic = from61[i], b[3] = {ic / 16, (ic / 4) % 4, ic % 4};
      for (j = 0; j < 3; j++) { fb3x4[j * 4 + b[j]] += pi[i]; fb4[b[j]] += pi[i] / 3.; }
   }
   for (i = 0; i < n; i++) {
      const int ic = from61[i], b[3] = {ic / 16, (ic / 4) % 4, ic % 4};
      pi[i] = p->codonfreq == 2 ? fb3x4[b[0]] * fb3x4[4 + b[1]] * fb3x4[8 + b[2]] : fb4[b[0]] * fb4[b[1]] * fb4[b[2]];
      s += pi[i];
   }
   for (i = 0; i < n; i++) pi[i] *= 1. / s;
   return 0;
}

/* lfun2dSdN on the host (codeml.c:4219-4264; +lnL): where the device's Jacobi did not converge (PAML_AMD_ENOCONV) */
static double host_lnl(const pamlh *p, const double *fp, const double *pi, double t, double kappa, double omega)
{
   const int n = p->n;
   double *Q = (double *)malloc((size_t)(3 * n * n + 2 * n) * sizeof(double)), *U = Q + n * n, *V = U + n * n, *Root = V + n * n, *ex = Root + n;
   double mr = pamlh_codon_q(p, pi, kappa, omega, Q), lnL = 0;
   int j, k, x;
   pamlh_eigen_qrev(Q, pi, n, Root, U, V);
   for (x = 0; x < n; x++) ex[x] = exp(t * Root[x] / mr);
   for (j = 0; j < n; j++)
      for (k = 0; k <= j; k++)
         if (fp[j * n + k] > 0) {
            double f = 0;
            for (x = 0; x < n; x++) f += U[j * n + x] * ex[x] * V[x * n + k];
            f *= pi[j];
            if (f <= 0) f = 1e-70;
            lnL += fp[j * n + k] * log(f);
         }
   free(Q);
   return lnL;
}

typedef struct {
   double x[3], f, g[3], H[9], d[3], xn[3], fn, gold[3], amax;
   int phase, iter, fails, fresh, nev, done;      /* fresh: H is the scaled start, not yet updated */
} pw_state;

enum { LS_N = 7 };
static const double LS_STEP[LS_N] = {1. / 64, 1. / 16, 1. / 4, 1. / 2, 1, 2, 4};

/* out[n_pairs][9] = t, kappa, omega, lnL, S, N, dN, dS, likelihood evaluations used; pairs in the reference's order (2,1), (3,1), (3,2), (4,1) ...:
 * pair (is, js), js < is, at index is (is - 1) / 2 + js (0-based sequences).  counters (may be NULL): [0] elements evaluated, [1]
 * decompositions done, [2] evaluate calls, [3] elements redone on the host. */
int pamlh_pairwise(pamlh *p, double *out, long *counters, int verbose)
{
   const double lo3[3] = {1e-5, 0.4, 0.001}, hi3[3] = {50, 999, 99}, floor3[3] = {0.002, 0.1, 0.02};
   const int n = p->n, ns = p->ns, npair = ns * (ns - 1) / 2;
   int fidx[3], np = 0, i, k, q, is, js, rc = 0, nnz, round = 0, active;
   const int *row, *col;
   unsigned char flags[704];
   int *sa, *sb, *epair, *eown;
   double *fp, *ls, *pi, *et, *ek, *ew, *el, lo[3], hi[3];
   long *failed, redone = 0, ncalls = 0;
   paml_amd_pairset *ps = NULL;
   pw_state *st;
   if (!p->pairwise) return pamlh_fail(p, "pamlh_pairwise: the control file does not ask for runmode = -2");
   if (!p->eng) {
      if ((rc = paml_amd_create(&p->eng, n, ns, p->npatt, 1, 1, 0))) return pamlh_fail(p, "paml_amd_create failed (%d): no GPU?", rc);
      if ((rc = paml_amd_set_tips(p->eng, p->z, 1, n, NULL, NULL, p->w, NULL))) return pamlh_fail(p, "%s", paml_amd_last_error(p->eng));
   }
   fidx[np++] = 0;
   if (!p->fix_kappa) fidx[np++] = 1;
   if (!p->fix_omega) fidx[np++] = 2;
   for (i = 0; i < np; i++) { lo[i] = lo3[fidx[i]]; hi[i] = hi3[fidx[i]]; }
   sa = (int *)malloc((size_t)2 * npair * sizeof(int)); sb = sa + npair;
   for (is = 1, q = 0; is < ns; is++) for (js = 0; js < is; js++, q++) { sa[q] = is; sb[q] = js; }
   fp = (double *)malloc(((size_t)npair * n * n + npair + (size_t)npair * n) * sizeof(double)); ls = fp + (size_t)npair * n * n; pi = ls + npair;
   st = (pw_state *)calloc(npair, sizeof(pw_state));
   {
      const size_t cap = (size_t)npair * (LS_N > 2 * np ? LS_N : 2 * np);
      epair = (int *)malloc(2 * cap * sizeof(int)); eown = epair + cap;
      et = (double *)malloc(4 * cap * sizeof(double)); ek = et + cap; ew = ek + cap; el = ew + cap;
      failed = (long *)malloc(cap * sizeof(long));
   }
   if ((rc = paml_amd_pairset_create(p->eng, &ps, npair, sa, sb)) || (rc = paml_amd_pairset_get_counts(ps, fp, ls))) { rc = pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); goto end; }
   for (q = 0; q < npair; q++)
      if (pamlh_pairwise_freqs(p, fp + (size_t)q * n * n, ls[q], pi + (size_t)q * n)) { rc = pamlh_fail(p, "pair %d has no sites", q); goto end; }
   nnz = pamlh_codon_pattern_flags(p, &row, &col, flags);
   if ((rc = paml_amd_pairset_set_pi(ps, pi)) || (rc = paml_amd_pairset_set_pattern(ps, nnz, row, col, flags))) { rc = pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); goto end; }
   /* the fixed starting rule (see the head of this file) */
   {
      int from61[64], m = 0;
      for (i = 0; i < 64; i++) if (p->code[i] != '*') from61[m++] = i;
      for (q = 0; q < npair; q++) {
         const double *f = fp + (size_t)q * n * n;
         double nd = 0, pd, d;
         int j;
         for (j = 0; j < n; j++)
            for (k = 0; k < j; k++)
               if (f[j * n + k] > 0) {
                  const int c1 = from61[j], c2 = from61[k];
                  nd += f[j * n + k] * ((c1 / 16 != c2 / 16) + ((c1 / 4) % 4 != (c2 / 4) % 4) + (c1 % 4 != c2 % 4));
               }
         pd = nd / (3 * ls[q]);
         d = pd < 0.7 ? -0.75 * log(1 - 4 * pd / 3) : 3;
         st[q].x[0] = 3 * d < 0.01 ? 0.01 : 3 * d > 3 ? 3 : 3 * d;
         st[q].x[1] = p->fix_kappa ? p->kappa0 : (p->kappa0 >= 0.4 && p->kappa0 <= 10 ? p->kappa0 : 2);
         st[q].x[2] = p->fix_omega ? p->omega0 : (p->omega0 < 0.05 ? 0.05 : p->omega0 > 2 ? 2 : p->omega0);
         st[q].phase = -1;      /* -1: the start's lnL is wanted; 0: gradient; 1: line search */
      }
   }
   /* lock step: one evaluate call per round for everything the unfinished pairs want */
   for (active = npair; active > 0 && round < 2000; round++) {
      long ne = 0, nfail = 0, e;
      for (q = 0; q < npair; q++) {
         pw_state *s = &st[q];
         if (s->done) continue;
#define PW_PUT(X) do { epair[ne] = q; eown[ne] = q; et[ne] = (X)[0]; ek[ne] = (X)[1]; ew[ne] = (X)[2]; ne++; } while (0)
         if (s->phase == -1) PW_PUT(s->x);
         else if (s->phase == 0) {
            /* central differences inside the box: a point beyond a bound is moved onto it and the quotient taken over the distance left */
            for (i = 0; i < np; i++) {
               const int v = fidx[i];
               const double h = 1e-6 * (fabs(s->x[v]) + 1);
               double y[3];
               memcpy(y, s->x, sizeof(y)); y[v] = s->x[v] + h > hi[i] ? hi[i] : s->x[v] + h; PW_PUT(y);
               memcpy(y, s->x, sizeof(y)); y[v] = s->x[v] - h < lo[i] ? lo[i] : s->x[v] - h; PW_PUT(y);
            }
         }
         else
            for (k = 0; k < LS_N; k++) {
               const double a = LS_STEP[k] < s->amax ? LS_STEP[k] : s->amax;
               double y[3];
               memcpy(y, s->x, sizeof(y));
               for (i = 0; i < np; i++) {
                  const int v = fidx[i];
                  y[v] = s->x[v] + a * s->d[i];
                  if (y[v] < lo[i]) y[v] = lo[i];
                  if (y[v] > hi[i]) y[v] = hi[i];
               }
               PW_PUT(y);
            }
#undef PW_PUT
      }
      rc = paml_amd_pairset_eval(ps, ne, epair, et, ek, ew, el);
      ncalls++;
      if (rc == PAML_AMD_ENOCONV) {      /* those elements alone are done again on the host */
         nfail = paml_amd_pairset_failed(ps, failed, ne);
         for (e = 0; e < nfail; e++) {
            const long x = failed[e];
            el[x] = host_lnl(p, fp + (size_t)epair[x] * n * n, pi + (size_t)epair[x] * n, et[x], ek[x], ew[x]);
         }
         redone += nfail;
         rc = 0;
      }
      if (rc) { rc = pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); goto end; }
      for (e = 0; e < ne;) {
         pw_state *s = &st[q = eown[e]];
         if (s->phase == -1) { s->f = el[e++]; s->nev++; s->phase = 0; s->fresh = 1; continue; }
         if (s->phase == 0) {
            double gn = 0, dg = 0, sc[3], nrm = 0;
            int free_dir = 0;
            for (i = 0; i < np; i++, e += 2) {
               const int v = fidx[i];
               const double h = 1e-6 * (fabs(s->x[v]) + 1);
               const double xp = s->x[v] + h > hi[i] ? hi[i] : s->x[v] + h, xm = s->x[v] - h < lo[i] ? lo[i] : s->x[v] - h;
               s->g[i] = (el[e] - el[e + 1]) / (xp - xm);      /* gradient of +lnL: the search climbs */
            }
            s->nev += 2 * np;
            /* BFGS update of the inverse Hessian with the step just taken (skipped when the curvature condition fails) */
            if (s->iter > 0 && s->fresh != 1) {
               double sv[3], yv[3], Hy[3], sy = 0, yHy = 0;
               for (i = 0; i < np; i++) { sv[i] = s->xn[i]; yv[i] = -(s->g[i] - s->gold[i]); sy += sv[i] * yv[i]; }
               if (sy > 1e-14) {
                  int a, b;
                  for (a = 0; a < np; a++) { Hy[a] = 0; for (b = 0; b < np; b++) Hy[a] += s->H[a * 3 + b] * yv[b]; yHy += yv[a] * Hy[a]; }
                  if (s->fresh == 2 && yHy > 0) {      /* first update after a (re)start: bring the start's scale to the curvature seen */
                     const double ga = sy / yHy;
                     for (a = 0; a < 9; a++) s->H[a] *= ga;
                     for (a = 0; a < np; a++) Hy[a] *= ga;
                     yHy *= ga;
                  }
                  for (a = 0; a < np; a++)
                     for (b = 0; b < np; b++)
                        s->H[a * 3 + b] += (1 + yHy / sy) * sv[a] * sv[b] / sy - (Hy[a] * sv[b] + sv[a] * Hy[b]) / sy;
               }
            }
            /* variables on a bound whose gradient points outward are held */
            for (i = 0; i < np; i++) {
               const int v = fidx[i];
               const int held = (s->x[v] <= lo[i] && s->g[i] < 0) || (s->x[v] >= hi[i] && s->g[i] > 0);
               sc[i] = held ? 0 : 0.3 * (fabs(s->x[v]) > floor3[v] ? fabs(s->x[v]) : floor3[v]);      /* the scale of a variable: 30 % of its size */
               if (!held) { gn += s->g[i] * s->g[i] * sc[i] * sc[i]; free_dir++; }
            }
            if (!free_dir || sqrt(gn) < 3e-7 * (1 + fabs(s->f) / 1000)) { s->done = 1; active--; continue; }      /* (the gain a 30 % step could bring at first order: at the differences' noise) */
            if (s->fresh == 1) {      /* scaled steepest ascent of unit scaled length */
               memset(s->H, 0, sizeof(s->H));
               for (i = 0; i < np; i++) s->H[i * 3 + i] = sc[i] * sc[i] / sqrt(gn);
               s->fresh = 2;
            }
            else if (s->fresh == 2) s->fresh = 0;
            for (i = 0; i < np; i++) {
               s->d[i] = 0;
               if (sc[i] == 0) continue;
               for (k = 0; k < np; k++) if (sc[k] != 0) s->d[i] += s->H[i * 3 + k] * s->g[k];
            }
            for (i = 0; i < np; i++) dg += s->d[i] * s->g[i];
            if (!(dg > 0)) {      /* not an ascent direction: start over from the scaled gradient */
               memset(s->H, 0, sizeof(s->H));
               for (i = 0; i < np; i++) { s->H[i * 3 + i] = sc[i] * sc[i] / sqrt(gn); s->d[i] = s->H[i * 3 + i] * s->g[i]; }
               s->fresh = 2;
            }
            /* a scaled step of more than 2 is cut.  The trial points are PROJECTED into the box (each variable clipped on its own): a
             * variable that reaches its bound stays there while the others go on — pairs without synonymous differences end at
             * omega = 99 and kappa = 0.4 with a small t, and a step cut short at the first bound met would stall there */
            for (i = 0; i < np; i++) if (sc[i] != 0) nrm += s->d[i] * s->d[i] / (sc[i] * sc[i]);
            nrm = sqrt(nrm) * 0.3;
            if (nrm > 2) for (i = 0; i < np; i++) s->d[i] *= 2 / nrm;
            s->amax = 1e300;
            memcpy(s->gold, s->g, sizeof(s->g));
            s->phase = 1;
            continue;
         }
         /* line search: the best of the trial steps */
         {
            int best = -1;
            double fb = s->f;
            for (k = 0; k < LS_N; k++) if (el[e + k] > fb) { fb = el[e + k]; best = k; }
            s->nev += LS_N;
            if (best < 0) {
               /* no trial step gains: from an updated H, start over once from the scaled gradient; from there, the search is over */
               if (s->fresh == 0 && s->fails < 2) { s->fails++; s->fresh = 1; s->phase = 0; s->iter = 0; }
               else { s->done = 1; active--; }
            }
            else {
               const double a = LS_STEP[best] < s->amax ? LS_STEP[best] : s->amax, gain = fb - s->f;
               for (i = 0; i < np; i++) {
                  const int v = fidx[i];
                  double y = s->x[v] + a * s->d[i];
                  if (y < lo[i]) y = lo[i];
                  if (y > hi[i]) y = hi[i];
                  s->xn[i] = y - s->x[v];      /* the step, for the next update */
                  s->x[v] = y;
               }
               s->f = fb;
               s->iter++;
               s->phase = 0;
               if (gain < 1e-10 * (fabs(fb) + 1)) {
                  if (s->fresh == 0 && s->fails < 2) { s->fails++; s->fresh = 1; s->iter = 0; }      /* make sure with one fresh start */
                  else { s->done = 1; active--; }
               }
               else if (s->iter >= 300) { s->done = 1; active--; }
            }
            e += LS_N;
         }
      }
      if (verbose) fprintf(stderr, "pairwise round %d: %ld elements, %d pairs still searching\n", round, ne, active);
   }
   for (q = 0; q < npair; q++) {
      double *o = out + (size_t)q * PW_OUT;
      o[0] = st[q].x[0]; o[1] = st[q].x[1]; o[2] = st[q].x[2]; o[3] = st[q].f; o[8] = st[q].nev;
      pamlh_dnds_one(p, pi + (size_t)q * n, o[1], o[2], o[0], p->ls, &o[5], &o[4], &o[6], &o[7]);
   }
   if (counters) {
      long a = 0, b = 0;
      paml_amd_pairset_counters(ps, &a, &b, NULL, NULL);
      counters[0] = a; counters[1] = b; counters[2] = ncalls; counters[3] = redone;
   }
end:
   if (ps) paml_amd_pairset_destroy(ps);
   free(sa); free(fp); free(st); free(epair); free(et); free(failed);
   return rc;
}

/* 2ML.t, 2ML.dN, 2ML.dS in the reference's layout (first line "%6d" ns; per sequence "%-15s " name, then " %7.4f" per earlier sequence:
 * codeml.c:4384-4394, 4531-4533, 4594) and the pair table of `rst` (codeml.c:4386-4388, 4404, 4539-4549 without the SE column), written
 * into the directory `dir` from out[n_pairs][9] as pamlh_pairwise fills it. */
int pamlh_pairwise_write(pamlh *p, const double *out, const char *dir)
{
   static const char *const name[3] = {"2ML.t", "2ML.dN", "2ML.dS"};
   static const int column[3] = {0, 6, 7};
   const int np = 1 + !p->fix_kappa + !p->fix_omega;
   char path[1200];
   FILE *f;
   int k, is, js, q;
   if (!p->pairwise) return pamlh_fail(p, "pamlh_pairwise_write: not a runmode = -2 analysis");
   for (k = 0; k < 3; k++) {
      snprintf(path, sizeof(path), "%s/%s", dir, name[k]);
      if (!(f = fopen(path, "w"))) return pamlh_fail(p, "cannot write %s", path);
      fprintf(f, "%6d\n", p->ns);
      for (is = 0, q = 0; is < p->ns; is++) {
         fprintf(f, "%-*s ", 15, p->names[is]);
         for (js = 0; js < is; js++, q++) fprintf(f, " %7.4f", out[(size_t)q * PW_OUT + column[k]]);
         fprintf(f, "\n");
      }
      fclose(f);
   }
   snprintf(path, sizeof(path), "%s/rst", dir);
   if (!(f = fopen(path, "w"))) return pamlh_fail(p, "cannot write %s", path);
   fprintf(f, "\n\npairwise comparison (Goldman & Yang 1994)");
   fprintf(f, "\nseq seq        N       S       dN       dS     dN/dS   Paras.\n");
   for (is = 0, q = 0; is < p->ns; is++)
      for (js = 0; js < is; js++, q++) {
         const double *o = out + (size_t)q * PW_OUT;
         fprintf(f, "%3d %3d ", is + 1, js + 1);
         fprintf(f, "%8.1f %8.1f %8.4f %8.4f %8.4f", o[5], o[4], o[6], o[7], o[2]);
         fprintf(f, " %8.4f", o[0]);
         if (!p->fix_kappa) fprintf(f, " %8.4f", o[1]);
         if (!p->fix_omega) fprintf(f, " %8.4f", o[2]);
         fprintf(f, " %9.3f\n", o[3]);
      }
   fclose(f);
   (void)np;
   return 0;
}
