/* pamlh_scan.c — every branch of the tree as the foreground of codeml's branch-site model A (model = 2, NSsites = 2, fix_omega = 0) in
 * turn, from ONE engine call (pamlh_foreground_scan -> paml_amd_relabel_scores) instead of a tree file, a model set-up and a search per
 * branch; the maximisation of the site-class proportions at fixed class likelihoods that the scan rests on (pamlh_mixture_max, host
 * only); the parameter vector of a row of the scan (pamlh_foreground_point) and the relabelling of the analysis's tree
 * (pamlh_set_foreground).
 *
 * Model A gives a branch type its own time scale, and the scale depends on the proportions (pamlh_set_x): Qfactor_bg = 1 / mr(kappa,
 * r w0 + 1 - r), Qfactor_fg = 1 / mr(kappa, p0 w0 + p1 + (1 - p0 - p1) w2), r = p0 / (p0 + p1).  With the EFFECTIVE lengths tau_v =
 * t_v Qfactor held fixed instead of t_v, the likelihoods of the four site classes do not depend on the proportions: the mixture
 *    sum_h w_h log(s r f0 + s (1 - r) f1 + (1 - s) r f2a + (1 - s)(1 - r) f2b),     s = p0 + p1,
 * re-mixed on the host, is an exact point of model A (at branch lengths t = tau / Qfactor, pamlh_foreground_point), not an
 * approximation; what the scan does not do is maximise the lengths, kappa and w0 again.  Classes 0 and 1 never see the foreground
 * branch: f0 and f1 are the present tree's (the engine hands their bytes through), f2a and f2b are the row's.
 * Refused by name: models other than branch-site A, fix_omega = 1, a clock, rho, several genes, a pattern shard. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifndef PAMLH_MIXTURE_ONLY
#include "pamlh_internal.h"
#endif

#define MIX_LO 1e-6
#define MIX_HI (1 - 1e-6)
#define MIX_EM_STEPS 30
#define MIX_NEWTON_STEPS 200

typedef struct {
   int n;              /* patterns of weight > 0 */
   double *w, *F;      /* [n], [n][4]: the class likelihoods over the pattern's largest */
   double c;           /* sum_h w_h (the pattern's largest log) */
} mix_t;

static double mix_clip(double x) { return x < MIX_LO ? MIX_LO : x > MIX_HI ? MIX_HI : x; }

/* the mixture's log likelihood without the constant; g, H (may be NULL): its gradient (s, r) and Hessian (ss, sr, rr) */
static double mix_value(const mix_t *m, double s, double r, double *g, double *H)
{
   double l = 0, gs = 0, gr = 0, hss = 0, hsr = 0, hrr = 0;
   int h;
   for (h = 0; h < m->n; h++) {
      const double *F = m->F + 4 * h, w = m->w[h];
      const double D = s * (r * F[0] + (1 - r) * F[1]) + (1 - s) * (r * F[2] + (1 - r) * F[3]);
      l += w * log(D);
      if (g) {
         const double Ds = (r * F[0] + (1 - r) * F[1]) - (r * F[2] + (1 - r) * F[3]), Dr = s * (F[0] - F[1]) + (1 - s) * (F[2] - F[3]);
         const double Dsr = (F[0] - F[1]) - (F[2] - F[3]), a = Ds / D, b = Dr / D;
         gs += w * a; gr += w * b;
         hss -= w * a * a; hrr -= w * b * b; hsr += w * (Dsr / D - a * b);
      }
   }
   if (g) { g[0] = gs; g[1] = gr; H[0] = hss; H[1] = hsr; H[2] = hrr; }
   return l;
}

/* Maximises sum_h w_h log(s r f0 + s (1 - r) f1 + (1 - s) r f2a + (1 - s)(1 - r) f2b) over (s, r) in [1e-6, 1 - 1e-6]^2 from (s0, r0);
 * lnf4[4][n_patt]: the logs of f0, f1, f2a, f2b (-inf allowed; a pattern of weight > 0 with all four -inf: -1).  Thirty EM steps (the
 * classes are pairs of two independent choices, so the M step is the two posterior means, clipped into the box), then a projected
 * Newton iteration: variables at a bound whose derivative points outwards are held, the others take the Newton step where the
 * Hessian on them is negative definite and the gradient's direction otherwise, and the step is halved along the clipped path until
 * lnL does not decrease — it never does.  *p0 = s r, *p1 = s (1 - r), *lnL the mixture's value. */
int pamlh_mixture_max(int n_patt, const double *w, const double *lnf4, double s0, double r0, double *p0, double *p1, double *lnL)
{
   mix_t m;
   double s = mix_clip(s0), r = mix_clip(r0), l, g[2], H[3];
   int h, c, it, rc = 0;
   if (n_patt < 1 || !w || !lnf4 || !p0 || !p1 || !lnL) return -1;
   m.n = 0; m.c = 0;
   m.w = (double *)malloc((size_t)n_patt * sizeof(double)); m.F = (double *)malloc((size_t)4 * n_patt * sizeof(double));
   if (!m.w || !m.F) { free(m.w); free(m.F); return -1; }
   for (h = 0; h < n_patt; h++) {
      double mx = -INFINITY;
      if (!(w[h] > 0)) continue;
      for (c = 0; c < 4; c++) if (lnf4[(size_t)c * n_patt + h] > mx) mx = lnf4[(size_t)c * n_patt + h];
      if (!(mx > -INFINITY) || !isfinite(mx)) { rc = -1; break; }
      for (c = 0; c < 4; c++) m.F[4 * m.n + c] = exp(lnf4[(size_t)c * n_patt + h] - mx);      /* (exp(-inf) = 0) */
      m.w[m.n++] = w[h];
      m.c += w[h] * mx;
   }
   if (rc) { free(m.w); free(m.F); return rc; }
   for (it = 0; it < MIX_EM_STEPS; it++) {
      double sw = 0, ss = 0, sr = 0;
      for (h = 0; h < m.n; h++) {
         const double *F = m.F + 4 * h;
         const double q0 = s * r * F[0], q1 = s * (1 - r) * F[1], q2 = (1 - s) * r * F[2], q3 = (1 - s) * (1 - r) * F[3], D = q0 + q1 + q2 + q3;
         sw += m.w[h]; ss += m.w[h] * (q0 + q1) / D; sr += m.w[h] * (q0 + q2) / D;
      }
      if (!(sw > 0)) break;
      s = mix_clip(ss / sw); r = mix_clip(sr / sw);
   }
   l = mix_value(&m, s, r, g, H);
   for (it = 0; it < MIX_NEWTON_STEPS; it++) {
      const int fs = !((s <= MIX_LO && g[0] < 0) || (s >= MIX_HI && g[0] > 0)), fr = !((r <= MIX_LO && g[1] < 0) || (r >= MIX_HI && g[1] > 0));
      double ds = 0, dr = 0, a = 1, ln = l, sn = s, rn = r;
      int k;
      if (!fs && !fr) break;
      if (fs && fr) {
         const double det = H[0] * H[2] - H[1] * H[1];
         if (H[0] < 0 && det > 1e-14 * H[0] * H[2]) { ds = -(H[2] * g[0] - H[1] * g[1]) / det; dr = -(H[0] * g[1] - H[1] * g[0]) / det; }
         else { const double q = fabs(H[0]) + fabs(H[2]) + 1e-300; ds = g[0] / q; dr = g[1] / q; }
      }
      else if (fs) ds = H[0] < 0 ? -g[0] / H[0] : g[0];
      else dr = H[2] < 0 ? -g[1] / H[2] : g[1];
      for (k = 0; k < 60; k++, a *= 0.5) {
         sn = mix_clip(s + a * ds); rn = mix_clip(r + a * dr);
         if (sn == s && rn == r) break;
         ln = mix_value(&m, sn, rn, NULL, NULL);
         if (ln > l) break;
      }
      if (!(ln > l) || (sn == s && rn == r)) break;      /* no point along the path is better: the maximum to rounding */
      {
         const double gain = ln - l;
         s = sn; r = rn;
         l = mix_value(&m, s, r, g, H);
         if (gain <= 1e-15 * fabs(l)) break;
      }
   }
   *p0 = s * r; *p1 = s * (1 - r); *lnL = l + m.c;
   free(m.w); free(m.F);
   return 0;
}

#ifndef PAMLH_MIXTURE_ONLY

static int scan_refused(pamlh *p, const char *who)
{
   if (p->pairwise) return pamlh_fail(p, "%s: runmode = -2 has no tree", who);
   if (p->clock) return pamlh_fail(p, "%s: clock = %d: the scan holds effective branch lengths, which a clock does not have", who, p->clock);
   if (!p->fix_rho || p->rho0 != 0) return pamlh_fail(p, "%s: rho models (auto-discrete-gamma) have no per-pattern class likelihoods to re-mix", who);
   if (p->ngene > 1) return pamlh_fail(p, "%s: several genes (%d) are not supported", who, p->ngene);
   if (p->shard_world > 0) return pamlh_fail(p, "%s: a pattern shard holds a part of the patterns only", who);
   if (!(p->seqtype == 1 && p->model == 2 && p->nssites == 2 && !p->m2a_rel && !p->aadist))
      return pamlh_fail(p, "%s: the analysis is not branch-site model A (model = 2, NSsites = 2)", who);
   if (p->fix_omega) return pamlh_fail(p, "%s: fix_omega = 1: the scan is of the alternative model, w2 free", who);
   if (p->ntime != p->nbranch) return pamlh_fail(p, "%s: the branch lengths are not parameters (fix_blength = 2)", who);
   return 0;
}

/* index of p0 in the parameter vector: branch lengths, kappa, frequency parameters, then p0 p1 w0 w2 */
static int scan_ip0(const pamlh *p) { return p->ntime + !p->fix_kappa + p->npi; }

static double scan_qfactor(const pamlh *p, double wmean)
{
   double *Q = (double *)malloc((size_t)p->n * p->n * sizeof(double));
   const double mr = pamlh_codon_q(p, p->pi, p->kappa, wmean, Q);
   free(Q);
   return 1 / mr;
}

/* Every non-root node of the tree in node order as the only foreground branch, at every omega2[g] of an ascending grid with omega2[0] =
 * 1: lnL[*n_br][n_grid], p0, p1 the same shape — the mixture maximised over the proportions (pamlh_mixture_max from x's) at the
 * effective lengths tau_v = t_v Qfactor_bg(r_x) of EVERY branch and x's kappa and w0; x's w2 and the tree's own '#' labels are not
 * used.  delta[*n_br] = 2 (max_{g >= 1} lnL - lnL at g = 0), best[*n_br] that g; node[*n_br] the nodes; *lnL_base the mixture at s -> 1
 * (no foreground class).  ONE paml_amd_relabel_scores call covers all (node, g) — K = 2 classes (w0 and 1) and 1 + n_grid labels, label
 * 1 + g the unscaled Q at omega2[g], every Qfactor 1, base labels 0 — in sub-lists of rows where the class values would pass 256 MB.
 * node = lnL = ... = NULL: *n_br only.  The analysis and its engine are left as they were. */
int pamlh_foreground_scan(pamlh *p, const double *x, int n_grid, const double *omega2, int *n_br, int *node, double *lnL_base, double *lnL, double *p0,
                          double *p1, double *delta, int *best)
{
   int rc, g, v, i, nb, n2, np_, chunk, r0, K = 2;
   pamlh *q = NULL;
   double *Q = NULL, *tau = NULL, *lk0 = NULL, *lk = NULL, *rl = NULL, l0 = 0, px0, px1, sx, rx, qf;
   int *rows = NULL, *base = NULL;
   if (!p || !n_br) return -1;
   if ((rc = scan_refused(p, "pamlh_foreground_scan"))) return rc;
   nb = p->nnode - 1;
   *n_br = nb;
   if (!node && !lnL) return 0;
   if (!x || !omega2 || !node || !lnL_base || !lnL || !p0 || !p1 || !delta || !best) return pamlh_fail(p, "pamlh_foreground_scan: null argument");
   if (n_grid < 1 || omega2[0] != 1) return pamlh_fail(p, "pamlh_foreground_scan: the grid starts at omega2 = 1");
   for (g = 1; g < n_grid; g++) if (!(omega2[g] > omega2[g - 1])) return pamlh_fail(p, "pamlh_foreground_scan: the grid is not ascending");
   if (2 + n_grid > PAMLH_MAXEIG) return pamlh_fail(p, "pamlh_foreground_scan: at most %d grid points", PAMLH_MAXEIG - 2);
   if ((rc = pamlh_set_x(p, x, p->np))) return rc < 0 ? rc : -1;
   if (!pamlh_model_feasible(p)) return pamlh_fail(p, "pamlh_foreground_scan: the model rejects the parameter vector");
   if ((rc = pamlh_engine_ready(p))) return rc;
   px0 = p->freqK[0]; px1 = p->freqK[1]; sx = px0 + px1; rx = px0 / sx;
   qf = p->qfactor[0];      /* class 0, background: Qfactor_bg(r_x) */
   n2 = p->n * p->n; np_ = p->npatt;
   /* the scan's model on a private copy of the model state that shares the engine */
   if (!(q = pamlh_state_clone(p))) return pamlh_fail(p, "pamlh_foreground_scan: out of memory");
   q->eng = p->eng;
   memcpy(q->pi, p->pi, p->n * sizeof(double));
   q->kappa = p->kappa;
   Q = (double *)malloc((size_t)n2 * sizeof(double));
   tau = (double *)malloc(p->nnode * sizeof(double));
   for (v = 0; v < p->nnode; v++) tau[v] = p->branch[v] * qf;
   for (i = 0; i < 2 + n_grid; i++) {
      pamlh_codon_q(q, q->pi, q->kappa, i == 0 ? p->class_w[0] : i == 1 ? 1.0 : omega2[i - 2], Q);
      pamlh_set_eig_uvroot(q, i, Q, q->pi, 1.0);
   }
   q->K = K; q->n_eigen = 2 + n_grid; q->n_labels = 1 + n_grid; q->mode = PAML_AMD_MODE_LFUNDG; q->use_qf = 0; q->n_pi = 1;
   for (i = 0; i < K; i++) {
      q->freqK[i] = 0.5; q->rate[i] = 1;      /* (the proportions are the host's: lnfk carries none) */
      q->eigen_of[i * q->n_labels] = i;
      for (g = 0; g < n_grid; g++) q->eigen_of[i * q->n_labels + 1 + g] = 2 + g;
   }
   if ((rc = pamlh_engine_model(q))) { pamlh_fail(p, "%s", q->err); goto done; }
   rows = (int *)malloc((size_t)2 * nb * n_grid * sizeof(int));
   base = (int *)calloc(p->nnode, sizeof(int));
   for (v = 0, i = 0; v < p->nnode; v++) {
      if (v == p->root) continue;
      node[i] = v;
      for (g = 0; g < n_grid; g++) { rows[2 * (i * n_grid + g)] = v; rows[2 * (i * n_grid + g) + 1] = 1 + g; }
      i++;
   }
   chunk = (int)(268435456.0 / ((double)K * np_ * 8));
   if (chunk < 1) chunk = 1;
   if (chunk > nb * n_grid) chunk = nb * n_grid;
   lk0 = (double *)malloc((size_t)K * np_ * sizeof(double));
   lk = (double *)malloc((size_t)chunk * K * np_ * sizeof(double));
   rl = (double *)malloc((size_t)chunk * sizeof(double));
   for (r0 = 0; r0 < nb * n_grid; r0 += chunk) {
      const int nr = r0 + chunk <= nb * n_grid ? chunk : nb * n_grid - r0;
      int bad = 0;
      rc = paml_amd_relabel_scores(p->eng, tau, NULL, base, nr, rows + 2 * r0, &l0, rl, NULL, lk0, lk);
      if (rc) { pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); goto done; }
#pragma omp parallel for schedule(dynamic)
      for (i = 0; i < nr; i++) {
         double *f4 = (double *)malloc((size_t)4 * np_ * sizeof(double));
         memcpy(f4, lk0, (size_t)2 * np_ * sizeof(double));
         memcpy(f4 + (size_t)2 * np_, lk + (size_t)i * K * np_, (size_t)2 * np_ * sizeof(double));
         if (pamlh_mixture_max(np_, p->w, f4, sx, rx, &p0[r0 + i], &p1[r0 + i], &lnL[r0 + i])) {
#pragma omp atomic write
            bad = 1;
         }
         free(f4);
      }
      if (bad) { rc = pamlh_fail(p, "pamlh_foreground_scan: a pattern has no likelihood under any class"); goto done; }
   }
   {      /* s -> 1: classes 0 and 1 only */
      double s = 0;
      int h;
      for (h = 0; h < np_; h++) {
         const double a = lk0[h], b = lk0[np_ + h], mx = a > b ? a : b;
         if (p->w[h] > 0) s += p->w[h] * (mx + log(rx * exp(a - mx) + (1 - rx) * exp(b - mx)));
      }
      *lnL_base = s;
   }
   for (i = 0; i < nb; i++) {
      best[i] = n_grid > 1 ? 1 : 0;
      for (g = 2; g < n_grid; g++) if (lnL[i * n_grid + g] > lnL[i * n_grid + best[i]]) best[i] = g;
      delta[i] = 2 * (lnL[i * n_grid + best[i]] - lnL[i * n_grid]);
   }
   rc = 0;
done:
   free(Q); free(tau); free(rows); free(base); free(lk0); free(lk); free(rl);
   if (q) { q->eng = NULL; pamlh_state_free(q); }
   /* the analysis's own model on the engine again (pamlh_eval_gpu sends it anyway; the other calls find it) */
   if (!rc && (rc = pamlh_engine_model(p))) return rc < 0 ? rc : -1;
   return rc < 0 ? rc : rc ? -1 : 0;
}

/* The model-A parameter vector, in x's layout, of the scan's row (node, omega2, p0, p1) for the tree with `node` as the only
 * foreground branch: t'_u = tau_u / Qfactor_bg(r') for u != node, t'_node = tau_node / Qfactor_fg(p0, p1, omega2), kappa and w0 from
 * x, then p0, p1, omega2; tau_u = t_u(x) Qfactor_bg(r_x).  No clamping into pamlh_bounds. */
int pamlh_foreground_point(pamlh *p, const double *x, int node, double omega2, double p0, double p1, double *xA)
{
   int rc, i, ip0;
   double qx, qb, qfg, w0, s = p0 + p1;
   if (!p || !x || !xA) return -1;
   if ((rc = scan_refused(p, "pamlh_foreground_point"))) return rc;
   if (node < 0 || node >= p->nnode || node == p->root) return pamlh_fail(p, "pamlh_foreground_point: node %d is the root or out of range", node);
   if (!(p0 > 0 && p1 > 0 && s <= 1) || !(omega2 > 0)) return pamlh_fail(p, "pamlh_foreground_point: proportions or omega2 out of range");
   if ((rc = pamlh_set_x(p, x, p->np))) return rc < 0 ? rc : -1;
   ip0 = scan_ip0(p);
   w0 = x[ip0 + 2];
   qx = p->qfactor[0];
   qb = scan_qfactor(p, (p0 * w0 + p1) / s);
   qfg = scan_qfactor(p, p0 * w0 + p1 + (1 - s) * omega2);
   memcpy(xA, x, p->np * sizeof(double));
   for (i = 0; i < p->ntime; i++) xA[i] = x[i] * qx / (p->branch_node[i] == node ? qfg : qb);
   xA[ip0] = p0; xA[ip0 + 1] = p1; xA[ip0 + 3] = omega2;
   return 0;
}

/* Relabels the analysis's tree in place: label 1 on the branch above `node`, 0 elsewhere (the precedent: pamlh_apply_nni); the engine,
 * if there is one, gets the tree again.  pamlh_newick then prints #1 there. */
int pamlh_set_foreground(pamlh *p, int node)
{
   int rc, v;
   if (!p) return -1;
   if ((rc = scan_refused(p, "pamlh_set_foreground"))) return rc;
   if (node < 0 || node >= p->nnode || node == p->root) return pamlh_fail(p, "pamlh_set_foreground: node %d is the root or out of range", node);
   for (v = 0; v < p->nnode; v++) p->label[v] = v == node;
   if (p->eng && (rc = paml_amd_set_tree(p->eng, p->nnode, p->root, p->sons_ptr, p->sons, p->label, p->scale)))
      return pamlh_fail(p, "%s", paml_amd_last_error(p->eng));
   return 0;
}

#endif
