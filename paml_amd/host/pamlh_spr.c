/* pamlh_spr.c — subtree prune and regraft on the analysis's tree: the lnL of every SPR neighbour within a radius at a parameter vector
 * from ONE engine call (pamlh_spr_scores -> paml_amd_spr_scores), a move applied to the tree and to the parameter vector in place
 * (pamlh_apply_spr), and a hill climb over the SPR neighbourhood with the screening call deciding which neighbours are maximised and in
 * which order (pamlh_spr_search).  A move is (s, x), 0-based nodes, with a split phi: the definition is in include/paml_amd.h.
 * Refused by name, as the NNI calls: a clock, rho models (lfunAdG: the sites are not independent, there is no per-pattern likelihood to
 * rearrange) and runmode = -2 (no tree). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pamlh_internal.h"

static int spr_refused(pamlh *p, const char *who)
{
   if (p->pairwise) return pamlh_fail(p, "%s: runmode = -2 has no tree to rearrange", who);
   if (p->clock) return pamlh_fail(p, "%s: clock = %d: tree rearrangement does not work with a clock (nor does the reference's, treesub.c:4653)", who, p->clock);
   if (!p->fix_rho || p->rho0 != 0) return pamlh_fail(p, "%s: rho models (auto-discrete-gamma) have no per-pattern likelihood to rearrange", who);
   return 0;
}

/* The canonical list (paml_amd_spr_list) of the tree as it stands within `radius` branches (<= 0: no limit), scored at x with the split
 * phi: moves[*n_moves][2] = s, x (0-based nodes), lnL[*n_moves] the neighbours' lnL at the branch lengths of the definition and the
 * parameters of x, *lnL0 the present tree's.  moves = lnL = NULL: the list's length only (host only; room for it is the caller's). */
int pamlh_spr_scores(pamlh *p, const double *x, int radius, double phi, int *n_moves, int *moves, double *lnL0, double *lnL)
{
   int n, rc;
   if (!p || !n_moves) return -1;
   if ((rc = spr_refused(p, "pamlh_spr_scores"))) return rc;
   n = paml_amd_spr_list(p->ns, p->nnode, p->root, p->sons_ptr, p->sons, radius, NULL, 0);
   if (n < 0) return pamlh_fail(p, "pamlh_spr_scores: the tree has no list of moves (%d)", n);
   *n_moves = n;
   if (!moves && !lnL) return 0;
   if (!x || !moves || !lnL || !lnL0) return pamlh_fail(p, "pamlh_spr_scores: null argument");
   if (n < 1) return pamlh_fail(p, "pamlh_spr_scores: the tree has no subtree to prune and regraft");
   if ((rc = pamlh_set_x(p, x, p->np))) return rc < 0 ? rc : -1;
   if (!pamlh_model_feasible(p)) return pamlh_fail(p, "pamlh_spr_scores: the model rejects the parameter vector");
   if ((rc = pamlh_engine_model(p))) return rc < 0 ? rc : -1;
   if (paml_amd_spr_list(p->ns, p->nnode, p->root, p->sons_ptr, p->sons, radius, moves, n) != n) return pamlh_fail(p, "pamlh_spr_scores: internal: the list changed its length");
   rc = paml_amd_spr_scores(p->eng, p->branch, p->ngene > 1 ? p->rgene : NULL, n, moves, phi, lnL0, lnL, NULL);
   if (rc) { pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); return rc < 0 ? rc : -1; }
   return 0;
}

/* why (s, x) is not a move of the tree (sons_ptr, sons, father); NULL: it is one */
static const char *spr_invalid(int nnode, int root, const int *sons_ptr, const int *father, int s, int x)
{
   int f, u;
   if (s < 0 || s >= nnode || x < 0 || x >= nnode) return "a node is out of range";
   if (s == root) return "the pruned node is the root";
   f = father[s];
   if (f == root) return "the father of the pruned node is the root";
   if (sons_ptr[f + 1] - sons_ptr[f] != 2) return "the father of the pruned node does not have exactly two sons";
   if (x == root) return "the target is the root";
   if (x == f) return "the target is the father of the pruned node";
   if (father[x] == f) return "the target is the sibling of the pruned node: the same topology";
   for (u = x; u != root; u = father[u])
      if (u == s) return "the target lies in the subtree below the pruned node";
   return NULL;
}

/* the son lists and fathers of a valid move, in place: c takes f's place under g, f takes x's place under x's father, sons[f] = (x, s) */
static void spr_edit(const int *sons_ptr, int *sons, int *father, int s, int x)
{
   const int f = father[s], g = father[f], c = sons[sons_ptr[f]] == s ? sons[sons_ptr[f] + 1] : sons[sons_ptr[f]];
   int j, fx;
   for (j = sons_ptr[g]; j < sons_ptr[g + 1]; j++) if (sons[j] == f) { sons[j] = c; break; }
   father[c] = g;
   fx = father[x];
   for (j = sons_ptr[fx]; j < sons_ptr[fx + 1]; j++) if (sons[j] == x) { sons[j] = f; break; }
   father[f] = fx;
   sons[sons_ptr[f]] = x; sons[sons_ptr[f] + 1] = s;
   father[x] = f; father[s] = f;
}

static int spr_branch_index(const pamlh *p, int node)
{
   int i;
   for (i = 0; i < p->nbranch; i++) if (p->branch_node[i] == node) return i;
   return -1;
}

/* The move (s, x) on the analysis's tree: son lists, fathers and label[f] in place, and in xvec the three branch lengths the definition
 * changes — t_c + t_f at c, (1 - phi) t_x at f, phi t_x at x.  Node ids and the order of the branch lengths in the parameter vector
 * stay (node f travels with s), the tree's length is unchanged.  The scaling marks are those of the new tree (SetNodeScale, as for a
 * tree just read) and the engine, if there is one, gets the tree again. */
int pamlh_apply_spr(pamlh *p, int s, int x, double phi, double *xvec)
{
   int rc, f, c, ic, jf, ix;
   const char *why;
   double tx;
   if (!p || !xvec) return -1;
   if ((rc = spr_refused(p, "pamlh_apply_spr"))) return rc;
   if (!(phi >= 0 && phi <= 1)) return pamlh_fail(p, "pamlh_apply_spr: phi = %g is outside [0, 1]", phi);
   if (p->ntime != p->nbranch || p->fix_blength == 3) return pamlh_fail(p, "pamlh_apply_spr: the branch lengths are not parameters of this analysis (fix_blength)");
   if ((why = spr_invalid(p->nnode, p->root, p->sons_ptr, p->father, s, x))) return pamlh_fail(p, "pamlh_apply_spr: (%d, %d): %s", s, x, why);
   f = p->father[s];
   c = p->sons[p->sons_ptr[f]] == s ? p->sons[p->sons_ptr[f] + 1] : p->sons[p->sons_ptr[f]];
   ic = spr_branch_index(p, c); jf = spr_branch_index(p, f); ix = spr_branch_index(p, x);
   if (ic < 0 || jf < 0 || ix < 0) return pamlh_fail(p, "pamlh_apply_spr: internal: a node without a branch");
   spr_edit(p->sons_ptr, p->sons, p->father, s, x);
   p->label[f] = p->label[x];
   xvec[ic] += xvec[jf];
   tx = xvec[ix];
   xvec[jf] = (1 - phi) * tx;
   xvec[ix] = phi * tx;
   pamlh_set_node_scale(p);
   if (p->eng && (rc = paml_amd_set_tree(p->eng, p->nnode, p->root, p->sons_ptr, p->sons, p->label, p->scale)))
      return pamlh_fail(p, "%s", paml_amd_last_error(p->eng));
   return 0;
}

/* The unrooted topology of the tree (sons_ptr, sons) as a key: its non-trivial splits, each the set of tips on the side without tip 0,
 * sorted; key[nnode][words], unused rows zero.  Two trees have the same key exactly when they are the same unrooted topology. */
static void spr_topology_key(int ns, int nnode, int root, const int *sons_ptr, const int *sons, const int *father, int words, uint64_t *key, uint64_t *set, int *order)
{
   int i, j, w, n = 0, top = 0, n_key = 0;
   memset(set, 0, (size_t)nnode * words * sizeof(uint64_t));
   memset(key, 0, (size_t)nnode * words * sizeof(uint64_t));
   order[top++] = root;      /* a pre-order; walked backwards every node comes after its subtree */
   while (n < top) {
      const int v = order[n++];
      for (j = sons_ptr[v]; j < sons_ptr[v + 1]; j++) order[top++] = sons[j];
   }
   for (i = nnode - 1; i >= 0; i--) {
      const int v = order[i];
      int count = 0, has0;
      uint64_t *sv = set + (size_t)v * words;
      if (v < ns && sons_ptr[v + 1] == sons_ptr[v]) sv[v >> 6] |= 1ull << (v & 63);
      if (v == root) continue;
      for (w = 0; w < words; w++) { set[(size_t)father[v] * words + w] |= sv[w]; count += __builtin_popcountll(sv[w]); }
      if (count < 2 || count > ns - 2) continue;
      has0 = (int)(sv[0] & 1ull);
      for (w = 0; w < words; w++) {
         uint64_t bits = has0 ? ~sv[w] : sv[w];
         if (has0 && w == words - 1 && (ns & 63)) bits &= (1ull << (ns & 63)) - 1;
         key[(size_t)n_key * words + w] = bits;
      }
      n_key++;
   }
   /* sorted, without repeats (a root with two sons names one split twice): insertion sort, the lists are short */
   for (i = 1; i < n_key; i++) {
      uint64_t tmp[64];
      uint64_t *row = key + (size_t)i * words;
      if (words > 64) break;      /* (more than 4096 tips: left unsorted; the search then maximises some topologies twice) */
      memcpy(tmp, row, words * sizeof(uint64_t));
      for (j = i; j > 0 && memcmp(key + (size_t)(j - 1) * words, tmp, words * sizeof(uint64_t)) > 0; j--)
         memcpy(key + (size_t)j * words, key + (size_t)(j - 1) * words, words * sizeof(uint64_t));
      memcpy(key + (size_t)j * words, tmp, words * sizeof(uint64_t));
   }
   for (i = 1, j = 0; i < n_key; i++)
      if (memcmp(key + (size_t)j * words, key + (size_t)i * words, words * sizeof(uint64_t))) { j++; if (j != i) memcpy(key + (size_t)j * words, key + (size_t)i * words, words * sizeof(uint64_t)); }
   for (i = j + 1; i < n_key; i++) memset(key + (size_t)i * words, 0, words * sizeof(uint64_t));
}

typedef struct { double lnL; int i; } spr_ranked;      /* a move of the list with its screened lnL: sorted as pairs, no state outside the call */
static int spr_by_score(const void *a, const void *b)      /* descending lnL, ties in list order */
{
   const spr_ranked *u = (const spr_ranked *)a, *v = (const spr_ranked *)b;
   if (u->lnL != v->lnL) return u->lnL > v->lnL ? -1 : 1;
   return u->i - v->i;
}

/* the saved tree back on the analysis and on its engine (the scaling marks follow the tree); nonzero: the engine refused it */
static int spr_restore(pamlh *p, const int *sons0, const int *father0, const int *label0)
{
   memcpy(p->sons, sons0, p->sons_ptr[p->nnode] * sizeof(int)); memcpy(p->father, father0, p->nnode * sizeof(int)); memcpy(p->label, label0, p->nnode * sizeof(int));
   pamlh_set_node_scale(p);
   return p->eng ? paml_amd_set_tree(p->eng, p->nnode, p->root, p->sons_ptr, p->sons, p->label, p->scale) : 0;
}

/* SPR hill climb from the tree as it stands: maximise it (pamlh_optimize from x), then per step ONE screening call (radius, phi = 0.5) at
 * the estimates; the candidates in descending order of their screened lnL, at most one per distinct unrooted topology and at most
 * `top` of them (<= 0: all), each applied and maximised from the x the move rewrites; the first whose maximised lnL is higher by more
 * than 1e-4 is kept, every other is undone from a saved copy of the tree and of x.  The search ends after a step in which none of the
 * tried candidates was better, or after max_moves moves (<= 0: no limit).  x: start in, estimates on the final tree out; *lnL its lnL.
 * stats (may be NULL): moves, screening calls, neighbours maximised (the starting tree's own maximisation not counted).  verbose: every
 * accepted move on stdout.  Where a candidate cannot be applied or maximised the search ends with that error, on the last tree it kept:
 * the candidate is undone, x holds that tree's estimates, *lnL and stats say how far the search came. */
int pamlh_spr_search(pamlh *p, double *x, double *lnL, int radius, int top, int max_moves, int verbose, int *stats)
{
   int rc, n = 0, moves = 0, screens = 0, opts = 0, n_eval = 0, cap = 0, i, k, words, n_sons;
   int *mv = NULL, *sons0 = NULL, *father0 = NULL, *label0 = NULL, *sons1 = NULL, *father1 = NULL, *walk = NULL;
   uint64_t *keys = NULL, *set = NULL;
   double cur = 0, l0 = 0, *sc = NULL, *xt = NULL;
   spr_ranked *order = NULL;
   size_t key_len;
   if (!p || !x || !lnL) return -1;
   if ((rc = spr_refused(p, "pamlh_spr_search"))) return rc;
   if (p->ntime != p->nbranch || p->fix_blength == 3) return pamlh_fail(p, "pamlh_spr_search: the branch lengths are not parameters of this analysis (fix_blength)");
   if ((rc = pamlh_optimize(p, x, &cur, 500, 1e-10, 0, &n_eval)) < 0) return rc;      /* (np >= nbranch > 0: the branch lengths are parameters) */
   words = (p->ns + 63) / 64;
   n_sons = p->sons_ptr[p->nnode];
   key_len = (size_t)p->nnode * words;
   xt = (double *)malloc((p->np + 1) * sizeof(double));
   sons0 = (int *)malloc((n_sons + 1) * sizeof(int)); sons1 = (int *)malloc((n_sons + 1) * sizeof(int));
   father0 = (int *)malloc(p->nnode * sizeof(int)); father1 = (int *)malloc(p->nnode * sizeof(int));
   label0 = (int *)malloc(p->nnode * sizeof(int)); walk = (int *)malloc(p->nnode * sizeof(int));
   set = (uint64_t *)malloc(key_len * sizeof(uint64_t));
   for (;;) {
      int improved = 0, tried = 0, n_keys = 1;
      if (max_moves > 0 && moves >= max_moves) break;
      if ((rc = pamlh_spr_scores(p, NULL, radius, 0.5, &n, NULL, NULL, NULL))) goto failed;
      if (n < 1) break;      /* (nothing to prune: a star tree, four tips) */
      if (n > cap) {
         cap = n;
         mv = (int *)realloc(mv, (size_t)2 * cap * sizeof(int)); order = (spr_ranked *)realloc(order, cap * sizeof(spr_ranked)); sc = (double *)realloc(sc, cap * sizeof(double));
      }
      if ((rc = pamlh_spr_scores(p, x, radius, 0.5, &n, mv, &l0, sc))) goto failed;
      screens++;
      for (i = 0; i < n; i++) { order[i].lnL = sc[i]; order[i].i = i; }
      qsort(order, n, sizeof(spr_ranked), spr_by_score);
      memcpy(sons0, p->sons, n_sons * sizeof(int)); memcpy(father0, p->father, p->nnode * sizeof(int)); memcpy(label0, p->label, p->nnode * sizeof(int));
      keys = (uint64_t *)realloc(keys, key_len * sizeof(uint64_t));      /* the first key: the present tree's own (a move around a root with two sons can give it back) */
      spr_topology_key(p->ns, p->nnode, p->root, p->sons_ptr, sons0, father0, words, keys, set, walk);
      for (k = 0; k < n && !improved && (top <= 0 || tried < top); k++) {
         const int *m = mv + 2 * order[k].i;
         uint64_t *key;
         double l = 0;
         int seen = 0;
         /* the candidate's topology: one per distinct unrooted tree, the best screened first */
         keys = (uint64_t *)realloc(keys, (size_t)(n_keys + 1) * key_len * sizeof(uint64_t));
         key = keys + (size_t)n_keys * key_len;
         memcpy(sons1, sons0, n_sons * sizeof(int)); memcpy(father1, father0, p->nnode * sizeof(int));
         spr_edit(p->sons_ptr, sons1, father1, m[0], m[1]);
         spr_topology_key(p->ns, p->nnode, p->root, p->sons_ptr, sons1, father1, words, key, set, walk);
         for (i = 0; i < n_keys && !seen; i++) seen = !memcmp(keys + (size_t)i * key_len, key, key_len * sizeof(uint64_t));
         if (seen) continue;
         n_keys++;
         tried++;
         memcpy(xt, x, p->np * sizeof(double));
         if ((rc = pamlh_apply_spr(p, m[0], m[1], 0.5, xt)) || (rc = pamlh_optimize(p, xt, &l, 500, 1e-10, 0, &n_eval)) < 0) {
            spr_restore(p, sons0, father0, label0);      /* (the error stands as the failed call left it) */
            goto failed;
         }
         rc = 0;
         opts++;
         if (l > cur + 1e-4) {
            memcpy(x, xt, p->np * sizeof(double));
            moves++;
            improved = 1;
            if (verbose) printf("move %d: the subtree below node %d regrafted on the branch above node %d (screened lnL %.4f, rank %d of %d): lnL %.4f -> %.4f\n", moves, m[0] + 1,
                                m[1] + 1, order[k].lnL, k + 1, n, cur, l);
            cur = l;
         }
         else {      /* undone from the saved copy */
            if ((rc = spr_restore(p, sons0, father0, label0))) { pamlh_fail(p, "%s", paml_amd_last_error(p->eng)); goto failed; }
         }
      }
      if (!improved) break;
   }
   rc = pamlh_set_x(p, x, p->np);      /* (the model state of the estimates on the final tree: what pamlh_newick prints) */
failed:
   *lnL = cur;
   if (stats) { stats[0] = moves; stats[1] = screens; stats[2] = opts; }
   free(mv); free(order); free(sc); free(xt); free(sons0); free(sons1); free(father0); free(father1); free(label0); free(walk); free(keys); free(set);
   return rc < 0 ? rc : rc ? -1 : 0;
}
