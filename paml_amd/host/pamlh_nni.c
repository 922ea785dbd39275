/* pamlh_nni.c — nearest-neighbour interchange on the analysis's tree: the lnL of every NNI neighbour at a parameter vector from ONE
 * engine call (pamlh_nni_scores -> paml_amd_nni_scores), a rearrangement applied to the tree in place (pamlh_apply_nni), and the hill
 * climb of the reference's runmode = 5 (Perturbation treesub.c:4642 on NeighborNNI treespace.c:283) with the screening call deciding
 * the order in which the neighbours are maximised (pamlh_nni_search).
 * Refused by name: a clock (the reference refuses it too, treesub.c:4653), rho models (lfunAdG: the sites are not independent, there
 * is no per-pattern likelihood to rearrange) and runmode = -2 (no tree). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pamlh_internal.h"

static int nni_refused(pamlh *p, const char *who)
{
   if (p->pairwise) return pamlh_fail(p, "%s: runmode = -2 has no tree to rearrange", who);
   if (p->clock) return pamlh_fail(p, "%s: clock = %d: tree rearrangement does not work with a clock (nor does the reference's, treesub.c:4653)", who, p->clock);
   if (!p->fix_rho || p->rho0 != 0) return pamlh_fail(p, "%s: rho models (auto-discrete-gamma) have no per-pattern likelihood to rearrange", who);
   return 0;
}

/* The canonical list (paml_amd_nni_list) of the tree as it stands, scored at x: swaps[*n_swaps][3] = v, s, x (0-based nodes), lnL[*n_swaps]
 * the neighbours' lnL at the branch lengths and parameters of x (each subtree keeps the branch above it), *lnL0 the present tree's.
 * swaps = lnL = NULL: the list's length only (host only; room for it is the caller's). */
int pamlh_nni_scores(pamlh *p, const double *x, int *n_swaps, int *swaps, double *lnL0, double *lnL)
{
   int n, rc;
   if (!p || !n_swaps) return -1;
   if ((rc = nni_refused(p, "pamlh_nni_scores"))) return rc;
   n = paml_amd_nni_list(p->ns, p->nnode, p->root, p->sons_ptr, p->sons, NULL, 0);
   if (n < 0) return pamlh_fail(p, "pamlh_nni_scores: the tree has no list of swaps (%d)", n);
   *n_swaps = n;
   if (!swaps && !lnL) return 0;
   if (!x || !swaps || !lnL || !lnL0) return pamlh_fail(p, "pamlh_nni_scores: null argument");
   if (n < 1) return pamlh_fail(p, "pamlh_nni_scores: the tree has no internal branch to rearrange");
   if ((rc = pamlh_set_x(p, x, p->np))) return rc < 0 ? rc : -1;
   if (!pamlh_model_feasible(p)) return pamlh_fail(p, "pamlh_nni_scores: the model rejects the parameter vector");
   if ((rc = pamlh_engine_model(p))) return rc < 0 ? rc : -1;
   if (paml_amd_nni_list(p->ns, p->nnode, p->root, p->sons_ptr, p->sons, swaps, n) != n) return pamlh_fail(p, "pamlh_nni_scores: internal: the list changed its length");
   rc = paml_amd_nni_scores(p->eng, p->branch, p->ngene > 1 ? p->rgene : NULL, n, swaps, lnL0, lnL, NULL);
   if (rc) { pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); return rc < 0 ? rc : -1; }
   return 0;
}

/* Son s of v and son x of the father of v change places in the two son lists; the scaling marks are those of the new tree
 * (SetNodeScale, as for a tree just read) and the engine, if there is one, gets the tree again.  Node ids, labels and the order of the
 * branch lengths in the parameter vector stay: the same x describes the new tree, every subtree with the branch above it.
 * (v, x, s) afterwards undoes it. */
int pamlh_apply_nni(pamlh *p, int v, int s, int x)
{
   int j, js = -1, jx = -1, f, rc;
   if (!p) return -1;
   if ((rc = nni_refused(p, "pamlh_apply_nni"))) return rc;
   if (v < 0 || v >= p->nnode || v == p->root || p->sons_ptr[v + 1] == p->sons_ptr[v])
      return pamlh_fail(p, "pamlh_apply_nni: node %d is not an internal node other than the root", v);
   f = p->father[v];
   for (j = p->sons_ptr[v]; j < p->sons_ptr[v + 1]; j++) if (p->sons[j] == s) js = j;
   for (j = p->sons_ptr[f]; j < p->sons_ptr[f + 1]; j++) if (p->sons[j] == x && x != v) jx = j;
   if (js < 0) return pamlh_fail(p, "pamlh_apply_nni: %d is not a son of %d", s, v);
   if (jx < 0) return pamlh_fail(p, "pamlh_apply_nni: %d is not a son of the father of %d other than it", x, v);
   p->sons[js] = x; p->sons[jx] = s;
   p->father[x] = v; p->father[s] = f;
   pamlh_set_node_scale(p);
   if (p->eng && (rc = paml_amd_set_tree(p->eng, p->nnode, p->root, p->sons_ptr, p->sons, p->label, p->scale)))
      return pamlh_fail(p, "%s", paml_amd_last_error(p->eng));
   return 0;
}

static const double *nni_key;
static int nni_by_score(const void *a, const void *b)      /* descending lnL, ties in list order */
{
   const int i = *(const int *)a, j = *(const int *)b;
   if (nni_key[i] != nni_key[j]) return nni_key[i] > nni_key[j] ? -1 : 1;
   return i - j;
}

/* NNI hill climb from the tree as it stands: maximise it (pamlh_optimize from x), then per step ONE screening call at the estimates,
 * the neighbours taken in descending order of their screened lnL, each applied and maximised from the present x; the first whose
 * maximised lnL is higher by more than 1e-4 (the four decimals the reference prints its search's lnL with, treesub.c:4709) is kept,
 * every other is undone.  The search ends after a step in which every neighbour was maximised and none was better — the tree is then
 * an NNI-local optimum, as the reference's; the screening only decides the order — or after max_moves moves (<= 0: no limit).
 * x: start in, estimates on the final tree out; *lnL its lnL.  stats (may be NULL): moves, screening calls, neighbours maximised (the
 * starting tree's own maximisation not counted).  verbose: every accepted move on stdout. */
int pamlh_nni_search(pamlh *p, double *x, double *lnL, int max_moves, int verbose, int *stats)
{
   int rc, n = 0, moves = 0, screens = 0, opts = 0, n_eval = 0, cap = 0, i, k;
   int *swaps = NULL, *order = NULL;
   double cur = 0, l0 = 0, *sc = NULL, *xt = NULL;
   if (!p || !x || !lnL) return -1;
   if ((rc = nni_refused(p, "pamlh_nni_search"))) return rc;
   if (p->np > 0 && (rc = pamlh_optimize(p, x, &cur, 500, 1e-10, 0, &n_eval)) < 0) return rc;
   if (p->np <= 0 && ((rc = pamlh_set_x(p, x, p->np)) || (rc = pamlh_eval_gpu(p, &cur, NULL)))) return rc < 0 ? rc : -1;
   xt = (double *)malloc((p->np + 1) * sizeof(double));
   for (;;) {
      int improved = 0;
      if (max_moves > 0 && moves >= max_moves) break;
      if ((rc = pamlh_nni_scores(p, NULL, &n, NULL, NULL, NULL))) goto done;
      if (n < 1) break;      /* (a star tree, three tips: nothing to rearrange) */
      if (n > cap) {
         cap = n;
         swaps = (int *)realloc(swaps, (size_t)3 * cap * sizeof(int)); order = (int *)realloc(order, cap * sizeof(int)); sc = (double *)realloc(sc, cap * sizeof(double));
      }
      if ((rc = pamlh_nni_scores(p, x, &n, swaps, &l0, sc))) goto done;
      screens++;
      for (i = 0; i < n; i++) order[i] = i;
      nni_key = sc;
      qsort(order, n, sizeof(int), nni_by_score);
      for (k = 0; k < n && !improved; k++) {
         const int *sw = swaps + 3 * order[k];
         double l = 0;
         if ((rc = pamlh_apply_nni(p, sw[0], sw[1], sw[2]))) goto done;
         memcpy(xt, x, p->np * sizeof(double));
         if (p->np > 0 ? (rc = pamlh_optimize(p, xt, &l, 500, 1e-10, 0, &n_eval)) < 0 : ((rc = pamlh_set_x(p, xt, p->np)) || (rc = pamlh_eval_gpu(p, &l, NULL)))) goto done;
         rc = 0;
         opts++;
         if (l > cur + 1e-4) {
            memcpy(x, xt, p->np * sizeof(double));
            moves++;
            improved = 1;
            if (verbose) printf("move %d: nodes %d and %d change places across %d..%d (screened lnL %.4f, rank %d of %d): lnL %.4f -> %.4f\n", moves, sw[1] + 1, sw[2] + 1,
                                p->father[sw[0]] + 1, sw[0] + 1, sc[order[k]], k + 1, n, cur, l);
            cur = l;
         }
         else if ((rc = pamlh_apply_nni(p, sw[0], sw[2], sw[1]))) goto done;
      }
      if (!improved) break;
   }
   rc = pamlh_set_x(p, x, p->np);      /* (the model state of the estimates on the final tree: what pamlh_newick prints) */
   *lnL = cur;
   if (stats) { stats[0] = moves; stats[1] = screens; stats[2] = opts; }
done:
   free(swaps); free(order); free(sc); free(xt);
   return rc < 0 ? rc : rc ? -1 : 0;
}
