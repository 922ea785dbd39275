/* pamlh_lnl — command-line driver: one likelihood evaluation of a codeml/baseml analysis on the MI355X.
 *   usage: pamlh_lnl <codeml|baseml> <file.ctl> [--optimize [--analytic-gradient | --analytic-gradient-all | --newton-branches] [--newton-full]] [--nni-scores | --nni-search [--max-moves N]] [--branch-supports [--replicates N] [--seed S]] [--spr-scores [--radius R] [--split PHI] | --spr-search [--radius R] [--top N] [--max-moves N]] [--place [--pendant a,b,c] [--split PHI]] [--bv FILE [--exact-hessian]] [--se-exact] [--subst-counts [--per-site]] [--ancestral | --ancestral-all] [--gpus N [--devices a,b,...]] [--tree K] [x0 x1 ...]
 *   (--set "key = value": replaces an option of the control file, e.g. one of the site models of an "NSsites = 0 1 2 7 8" list;
 *    --tree K: the K-th tree of the tree file, 1-based; --all-trees: every tree in turn — the reference's loop, Forestry codeml.c:635 —
 *    each optimised from the control file's initial values, then the comparison table of rell(), treesub.c:5844;
 *    --all-trees --rell-gpu [--replicates N]: the table's bootstrap replicates drawn on the device, 10 000 (or N) at every alignment
 *    length, their number printed under the table;
 *    --simulate OUT [--sites N] [--seed S] [--replicates R]: instead of the evaluation, R (default 1) alignments of N sites (default: the
 *    alignment's own length) drawn on the GPU under the model at the parameter vector the driver would otherwise evaluate — the control
 *    file's initial values, in.codeml / in.baseml, the command line's, or the estimates after --optimize — written as sequential PHYLIP
 *    to OUT, or OUT.0000, OUT.0001 ... for R > 1: the parametric bootstrap's data sets, the job of evolver (evolver.c:818))
 *    --nni-scores: the table of the tree's nearest-neighbour-interchange neighbours (v, s, x: son s of node v changes places with son x
 *    of v's father), their lnL at the parameter vector from one engine call and the difference to the present tree's;
 *    --nni-search [--max-moves N]: the NNI hill climb of the reference's runmode = 5 from the tree of the tree file (pamlh_nni_search):
 *    every accepted move, then the tree found with its estimates and lnL)
 *    --branch-supports [--replicates N] [--seed S]: the SH-like aLRT support of every internal branch that has three configurations
 *    (pamlh_branch_supports) at the parameter vector, or at the estimates after --optimize: one row per branch — father..node, the lnL
 *    of the present resolution and of its two NNI alternatives, each maximised over the five branches around the edge, delta = 2 (l0 -
 *    max(l1, l2)) and the support from N (default 1000) RELL replicates drawn on the GPU — then the tree with the supports as
 *    internal-node labels;
 *    --spr-scores [--radius R] [--split PHI]: the table of the tree's subtree-prune-and-regraft neighbours (s, x: the subtree below node s
 *    regrafted on the branch above node x, which the new node splits at PHI) within R branches (default: no limit), their lnL at the
 *    parameter vector from one engine call and the difference to the present tree's;
 *    --spr-search [--radius R] [--top N] [--max-moves N]: the SPR hill climb from the tree of the tree file (pamlh_spr_search), at most N
 *    candidates maximised per step: every accepted move, then the tree found with its estimates and lnL
 *    --place [--pendant a,b,c] [--split PHI]: the tree of the tree file may name only some of the sequences; the others are queries
 *    (pamlh_load_placement).  Per query one table row per branch — father..node, the best pendant length of the grid (default 0.05, 0.1,
 *    0.2, 0.4), the lnL of the tree with the query hung there at PHI (default 0.5) of the branch above the node, the difference to the
 *    tree's own lnL, the likelihood weight ratio — from one engine call, then the best placement's tree.  The parameter vector is the
 *    one the driver would evaluate, or the estimates after --optimize on the tree's sequences)
 *    --place --place-ml [--keep N]: maximum-likelihood placement (pamlh_place_ml): per query its N best branches of the grid (default:
 *    all) are maximised over the three lengths at the new node, one engine call per Newton step for all of them.  Per query one table
 *    row per kept branch — father..node, t_up, t_dn and the pendant length at the maximum, the lnL, the difference to the tree's own
 *    lnL, the likelihood weight ratio over the kept branches — then the best placement's tree with the three lengths written in
 *    --subst-counts [--per-site]: after the evaluation (or the estimates of --optimize), the posterior expected numbers of substitutions
 *    on every branch from one engine call (pamlh_subst_counts): one row per branch — father..node, t, then a column per label of the
 *    data type (codons: synonymous, nonsynonymous; nucleotides: transitions, transversions; amino acids: changes) and the total;
 *    --per-site adds, per label, the table site x branch
 * Reads the control file, the sequence and tree files it names, and the parameter vector from the command line,
 * else from in.codeml / in.baseml beside the ctl (the reference's "-1 x..." single-evaluation recipe, treesub.c:4057),
 * else the ctl's initial values; evaluates lnL through libpaml_amd.so; prints `lnL = ...` like the reference and
 * writes the per-pattern `lnf` file in the reference's layout.  With --optimize the vector is the starting point of a
 * maximum-likelihood search (pamlh_optimize: BFGS with batched finite differences) and the estimates are printed.
 * A control file with runmode = -2 (codeml) is the pairwise comparison instead: the estimates of every pair are printed and 2ML.t,
 * 2ML.dN, 2ML.dS and rst are written into the working directory in the reference's layout (pamlh_pairwise). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <signal.h>
#include <sys/wait.h>
#include <unistd.h>

#include "../../include/paml_amd.h"
#include "../../include/pamlh.h"

/* --gpus N: one process per GPU.  The parent becomes rank 0; it forks ranks 1 .. N-1 BEFORE anything touches the GPU, obtains the
 * RCCL id and hands it to them through pipes.  Every rank reads the same files, keeps its block of site patterns
 * (pamlh_set_shard) and runs the same code: the all-reduced lnL has the same bits on every rank, so the ranks stay in step
 * without further communication.  Only rank 0 prints.  --devices a,b,...: the GPU of each rank (default: rank r on GPU r).
 * What can go wrong is checked where every rank sees the same answer (more ranks than GPUs: before the fork, by a probe process,
 * since the parent must not initialise HIP before forking; more ranks than reduction chunks: paml_amd_shard_bounds refuses for every
 * rank alike).  A rank that dies on its own (its GPU fails) takes the job with it: rank 0 ends the others and exits non-zero
 * instead of waiting in a collective call for ever. */
#define MAX_RANKS 64
static pid_t child_pid[MAX_RANKS];
static int n_children = 0, ranks_done = 0;

static void end_children(void)      /* atexit of rank 0: an error path left ranks behind */
{
   int i, st;
   if (ranks_done) return;
   for (i = 0; i < n_children; i++) if (child_pid[i] > 0) kill(child_pid[i], SIGTERM);
   for (i = 0; i < n_children; i++) if (child_pid[i] > 0) waitpid(child_pid[i], &st, 0);
   n_children = 0;
}

static void on_sigchld(int sig)     /* a rank ended: fine when it is over, fatal while rank 0 is still working */
{
   int st, i;
   pid_t pid;
   (void)sig;
   while ((pid = waitpid(-1, &st, WNOHANG)) > 0) {
      for (i = 0; i < n_children; i++) if (child_pid[i] == pid) child_pid[i] = 0;
      if (!ranks_done && (!WIFEXITED(st) || WEXITSTATUS(st))) {
         static const char msg[] = "error: a rank ended abnormally; stopping the others\n";
         if (write(2, msg, sizeof(msg) - 1) < 0) {}
         for (i = 0; i < n_children; i++) if (child_pid[i] > 0) kill(child_pid[i], SIGTERM);
         _exit(1);
      }
   }
}

static int probe_device_count(void)      /* in a short-lived process: the parent stays clear of HIP until it has forked its ranks */
{
   int st = 0;
   const pid_t pid = fork();
   if (pid < 0) return -1;
   if (pid == 0) { int n = paml_amd_device_count(); _exit(n > 250 ? 250 : n); }
   if (waitpid(pid, &st, 0) != pid || !WIFEXITED(st)) return -1;
   return WEXITSTATUS(st);
}

static int spawn_ranks(int world, const int *device, int *rank_out, unsigned char *id)
{
   int r, fds[MAX_RANKS][2];
   const int ndev = probe_device_count();
   pid_t pid;
   *rank_out = 0;
   if (world > MAX_RANKS) { fprintf(stderr, "error: --gpus %d: at most %d ranks\n", world, MAX_RANKS); return -1; }
   for (r = 0; r < world; r++)
      if (device[r] < 0 || device[r] >= ndev) { fprintf(stderr, "error: rank %d wants GPU %d but %d are visible\n", r, device[r], ndev); return -1; }
   for (r = 1; r < world; r++) {
      if (pipe(fds[r])) return -1;
      pid = fork();
      if (pid < 0) return -1;
      if (pid == 0) {            /* child = rank r: wait for the id */
         int k;
         n_children = 0;
         for (k = 1; k <= r; k++) close(fds[k][1]);
         *rank_out = r;
         if (paml_amd_set_device(device[r])) { fprintf(stderr, "rank %d: no GPU %d\n", r, device[r]); _exit(1); }
         if (read(fds[r][0], id, PAML_AMD_COMM_ID_BYTES) != PAML_AMD_COMM_ID_BYTES) _exit(1);
         close(fds[r][0]);
         if (!freopen("/dev/null", "w", stdout)) _exit(1);
         return 0;
      }
      child_pid[n_children++] = pid;
      close(fds[r][0]);
   }
   atexit(end_children);
   signal(SIGCHLD, on_sigchld);
   if (paml_amd_set_device(device[0])) return -1;
   if (paml_amd_comm_unique_id(id)) return -1;
   for (r = 1; r < world; r++) {
      if (write(fds[r][1], id, PAML_AMD_COMM_ID_BYTES) != PAML_AMD_COMM_ID_BYTES) return -1;
      close(fds[r][1]);
   }
   return 0;
}

int main(int argc, char **argv)
{
   pamlh *p;
   char err[512];
   double x[4096], lnL, *lnf;
   int fg_scan = 0, fg_ngrid = 0;
   double fg_grid[64];
   int np, ntime, npatt, i, nx = 0, optimize = 0, ancestral = 0, ancestral_all = 0, gpus = 0, rank = 0, itree = 0, all_trees = 0, rell_gpu = 0, replicates = 0, analytic = 0, nni_scores = 0, nni_search = 0, max_moves = 0, spr_scores = 0, spr_search = 0, radius = 0, top = 0, place = 0, place_ml = 0, keep = 0, n_pend = 4, supports = 0, newton = 0, newton_full = 0, exact_hessian = 0, se_exact = 0, subst_counts = 0, per_site = 0;
   double pend[64] = {0.05, 0.1, 0.2, 0.4}, split = 0.5;
   char over[2048] = "";
   const char *sim_out = NULL, *bv_out = NULL;
   long sim_sites = 0;
   unsigned long long sim_seed = 1;
   unsigned char comm_id[PAML_AMD_COMM_ID_BYTES];
   int device[MAX_RANKS];
   for (i = 0; i < MAX_RANKS; i++) device[i] = i;
   if (argc < 3) { fprintf(stderr, "usage: %s <codeml|baseml> <ctl> [--optimize [--analytic-gradient | --analytic-gradient-all | --newton-branches] [--newton-full]] [--nni-scores | --nni-search [--max-moves N]] [--branch-supports [--replicates N] [--seed S]] [--spr-scores [--radius R] [--split PHI] | --spr-search [--radius R] [--top N] [--max-moves N]] [--place [--pendant a,b,c] [--split PHI]] [--bv FILE] [--subst-counts [--per-site]] [--ancestral | --ancestral-all] [--gpus N] [--tree K | --all-trees [--rell-gpu [--replicates N]]] [--simulate OUT [--sites N] [--seed S] [--replicates R]] [--set 'key = value'] [x...]\n", argv[0]); return 2; }
   for (i = 3; i < argc && nx < 4096; i++) {
      if (!strcmp(argv[i], "--optimize")) optimize = 1;
      else if (!strcmp(argv[i], "--analytic-gradient-all")) analytic = 2;  /* with --optimize: every parameter's derivative from one engine call per gradient */
      else if (!strcmp(argv[i], "--analytic-gradient")) analytic = 1;      /* with --optimize: the branch lengths' derivatives from one engine call per gradient */
      else if (!strcmp(argv[i], "--newton-branches")) newton = 1;          /* with --optimize: the branch lengths by Newton steps on every branch at once, one engine call per sweep (pamlh_optimize_newton); prints the sweeps */
      else if (!strcmp(argv[i], "--newton-full")) newton_full = 1;         /* with --optimize: first the branch lengths by Newton steps from the whole Hessian block, one engine call per sweep (pamlh_newton_full), the other parameters held; prints the sweeps; then the optimiser chosen */
      else if (!strcmp(argv[i], "--exact-hessian")) exact_hessian = 1;     /* with --bv: the Hessian itself from one engine call (pamlh_write_bv_exact), not the outer product of scores */
      else if (!strcmp(argv[i], "--se-exact")) se_exact = 1;               /* standard errors from the observed information with the exact branch block (pamlh_standard_errors_exact) */
      else if (!strcmp(argv[i], "--subst-counts")) subst_counts = 1;       /* posterior expected substitution counts per branch (pamlh_subst_counts) */
      else if (!strcmp(argv[i], "--per-site")) per_site = 1;               /* with --subst-counts: the site x branch table of every label as well */
      else if (!strcmp(argv[i], "--nni-scores")) nni_scores = 1;
      else if (!strcmp(argv[i], "--foreground-scan")) fg_scan = 1;        /* every branch as the foreground of branch-site model A in turn, one engine call (pamlh_foreground_scan); --top N: the N best maximised */
      else if (!strcmp(argv[i], "--omega-grid") && i + 1 < argc) {      /* the grid of w2, ascending from 1, e.g. "1,2,5,20" */
         char *s2 = argv[++i];
         for (fg_ngrid = 0; fg_ngrid < 64 && *s2; ) { fg_grid[fg_ngrid++] = strtod(s2, &s2); if (*s2 == ',') s2++; else break; }
      }
      else if (!strcmp(argv[i], "--branch-supports")) supports = 1;      /* SH-like aLRT supports of the internal branches (N replicates, default 1000; --seed S) */
      else if (!strcmp(argv[i], "--nni-search")) nni_search = 1;
      else if (!strcmp(argv[i], "--max-moves") && i + 1 < argc) max_moves = atoi(argv[++i]);
      else if (!strcmp(argv[i], "--spr-scores")) spr_scores = 1;
      else if (!strcmp(argv[i], "--spr-search")) spr_search = 1;
      else if (!strcmp(argv[i], "--radius") && i + 1 < argc) radius = atoi(argv[++i]);
      else if (!strcmp(argv[i], "--top") && i + 1 < argc) top = atoi(argv[++i]);
      else if (!strcmp(argv[i], "--place")) place = 1;
      else if (!strcmp(argv[i], "--place-ml")) place_ml = 1;
      else if (!strcmp(argv[i], "--keep") && i + 1 < argc) keep = atoi(argv[++i]);
      else if (!strcmp(argv[i], "--pendant") && i + 1 < argc) {      /* the grid of pendant lengths, e.g. "0.05,0.1,0.2" */
         char *tok = strtok(argv[++i], ",");
         for (n_pend = 0; tok && n_pend < 64; tok = strtok(NULL, ",")) pend[n_pend++] = atof(tok);
      }
      else if (!strcmp(argv[i], "--split") && i + 1 < argc) split = atof(argv[++i]);
      else if (!strcmp(argv[i], "--bv") && i + 1 < argc) bv_out = argv[++i];      /* gradient and Hessian of the branch lengths, the reference's rst2 block (mcmctree's in.BV) */
      else if (!strcmp(argv[i], "--ancestral")) ancestral = 1;
      else if (!strcmp(argv[i], "--ancestral-all")) ancestral_all = 1;
      else if (!strcmp(argv[i], "--gpus") && i + 1 < argc) gpus = atoi(argv[++i]);
      else if (!strcmp(argv[i], "--devices") && i + 1 < argc) {      /* the GPU of each rank, e.g. "4,5,6,7" */
         int k = 0;
         char *tok = strtok(argv[++i], ",");
         for (; tok && k < MAX_RANKS; tok = strtok(NULL, ",")) device[k++] = atoi(tok);
      }
      else if (!strcmp(argv[i], "--tree") && i + 1 < argc) itree = atoi(argv[++i]) - 1;
      else if (!strcmp(argv[i], "--all-trees")) all_trees = 1;
      else if (!strcmp(argv[i], "--rell-gpu")) rell_gpu = 1;      /* with --all-trees: the bootstrap replicates of the table on the device */
      else if (!strcmp(argv[i], "--replicates") && i + 1 < argc) replicates = atoi(argv[++i]);
      else if (!strcmp(argv[i], "--simulate") && i + 1 < argc) sim_out = argv[++i];
      else if (!strcmp(argv[i], "--sites") && i + 1 < argc) sim_sites = atol(argv[++i]);
      else if (!strcmp(argv[i], "--seed") && i + 1 < argc) sim_seed = strtoull(argv[++i], NULL, 10);
      else if (!strcmp(argv[i], "--set") && i + 1 < argc) {      /* --set "NSsites = 2": replaces the control file's option */
         if (strlen(over) + strlen(argv[i + 1]) + 2 >= sizeof(over)) { fprintf(stderr, "error: too many --set options\n"); return 2; }
         strcat(over, argv[++i]); strcat(over, "\n");
      }
      else x[nx++] = atof(argv[i]);
   }
   if (all_trees) {      /* every tree of the file: maximum likelihood on each, then the comparison of rell() from the per-pattern values */
      int nt = 1, t, npt = 0, ng = 1;
      double *all = NULL, *w = NULL, *res;
      const int *goff = NULL;
      for (t = 0; t < nt; t++) {
         int n_eval = 0;
         if (pamlh_load_with(&p, argv[2], argv[1], t, over, err, sizeof(err))) { fprintf(stderr, "error: %s\n", err); return 1; }
         pamlh_dims(p, NULL, NULL, &npatt, NULL, NULL, NULL, NULL, NULL, &np, &ntime);
         if (t == 0) {
            nt = pamlh_n_trees(p); npt = npatt;
            all = (double *)malloc((size_t)nt * npt * sizeof(double)); w = (double *)malloc(npt * sizeof(double));
            memcpy(w, pamlh_weights(p), npt * sizeof(double));
            ng = pamlh_genes(p, &goff, NULL, NULL, NULL);
            if (ng > 1) { int *cp = (int *)malloc((ng + 1) * sizeof(int)); memcpy(cp, goff, (ng + 1) * sizeof(int)); goff = cp; } else goff = NULL;
         }
         pamlh_default_x(p, x, 4096);
         if (np > 0 && pamlh_optimize(p, x, &lnL, 500, 1e-10, 0, &n_eval) < 0) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
         if (pamlh_set_x(p, x, np) || pamlh_eval_gpu(p, &lnL, all + (size_t)t * npt)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
         printf("TREE # %2d:  lnL(ntime:%3d  np:%3d): %13.6f\n", t + 1, ntime, np, lnL);
         for (i = 0; i < np; i++) printf(" %.6f", x[i]);
         printf("\n");
         pamlh_free(p);
      }
      if (nt > 1) {
         int best = 0;
         res = (double *)malloc((size_t)6 * nt * sizeof(double));
         if (rell_gpu) {
            if (pamlh_tree_comparison_gpu(nt, npt, w, all, ng, goff, replicates, 20260927ULL, res, res + nt, res + 2 * nt, res + 3 * nt, res + 4 * nt, res + 5 * nt, &best)) {
               fprintf(stderr, "error: %s\n", paml_amd_last_error(NULL));
               return 1;
            }
         }
         else if (pamlh_tree_comparison(nt, npt, w, all, ng, goff, 0, 20260927ULL, res, res + nt, res + 2 * nt, res + 3 * nt, res + 4 * nt, res + 5 * nt, &best)) return 1;
         printf("\nTree comparisons (Kishino & Hasegawa 1989; Shimodaira & Hasegawa 1999)\n\n%6s %12s %9s %9s%8s%10s%9s\n\n", "tree", "li", "Dli", " +- SE", "pKH", "pSH", "pRELL");
         for (t = 0; t < nt; t++)
            printf("%6d%c%12.3f %9.3f %9.3f%8.3f%10.3f%9.3f\n", t + 1, t == best ? '*' : ' ', res[t], res[nt + t], res[2 * nt + t], res[3 * nt + t], res[4 * nt + t], res[5 * nt + t]);
         if (rell_gpu) printf("\npSH and pRELL from %d bootstrap replicates drawn on the GPU\n", replicates > 0 ? replicates : 10000);
         free(res);
      }
      free(all); free(w);
      return 0;
   }
   if (gpus > 0 && spawn_ranks(gpus, device, &rank, comm_id)) { fprintf(stderr, "error: could not start %d ranks (GPUs visible: %d; librccl.so.1 present?)\n", gpus, paml_amd_device_count()); return 1; }
   if (place && (gpus > 0 || all_trees)) { fprintf(stderr, "error: --place runs on one GPU, on one tree\n"); return 1; }
   if (place_ml && !place) { fprintf(stderr, "error: --place-ml goes with --place\n"); return 1; }
   if ((place ? pamlh_load_placement : pamlh_load_with)(&p, argv[2], argv[1], itree, over, err, sizeof(err))) { fprintf(stderr, "error: %s\n", err); return 1; }
   if (gpus > 0 && pamlh_set_shard(p, rank, gpus, comm_id)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
   if (pamlh_is_pairwise(p)) {      /* runmode = -2: all pairs' searches in lock step; 2ML.t, 2ML.dN, 2ML.dS and rst as the reference writes them */
      const int npair = pamlh_pairwise_n(p);
      double *res = (double *)malloc((size_t)npair * 9 * sizeof(double));
      long cnt[4] = {0, 0, 0, 0};
      int q, is, js;
      if (gpus > 0) { fprintf(stderr, "error: --gpus does not apply to runmode = -2 (pairs are not sharded yet)\n"); return 1; }
      if (pamlh_pairwise(p, res, cnt, 0) || pamlh_pairwise_write(p, res, ".")) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
      printf("pairwise comparison (Goldman & Yang 1994): %d pairs, %ld likelihood elements in %ld calls, %ld decompositions\n", npair, cnt[0], cnt[2], cnt[1]);
      for (is = 1, q = 0; q < npair; is++)
         for (js = 0; js < is; js++, q++) {
            const double *o = res + (size_t)q * 9;
            printf("\n%d (%s) ... %d (%s)\nlnL =%12.6f\n %8.5f %8.5f %8.5f\nt= %6.4f  S= %7.1f  N= %7.1f  dN/dS= %7.4f  dN =%7.4f  dS =%7.4f\n",
                   is + 1, pamlh_seq_name(p, is), js + 1, pamlh_seq_name(p, js), o[3], o[0], o[1], o[2], o[0], o[4], o[5], o[2], o[6], o[7]);
         }
      free(res);
      pamlh_free(p);
      return 0;
   }
   pamlh_dims(p, NULL, NULL, &npatt, NULL, NULL, NULL, NULL, NULL, &np, &ntime);
   if (gpus > 0 && (ancestral || ancestral_all || pamlh_mgene(p) == 1)) { fprintf(stderr, "error: --gpus gives lnL and estimates; per-site outputs and Mgene = 1 need the whole alignment on one GPU\n"); return 1; }
   if (pamlh_mgene(p) == 1) {      /* separate analyses: every gene on its own (start values: the control file's), lnL summed */
      const int ng = pamlh_genes(p, NULL, NULL, NULL, NULL);
      double sum = 0;
      int g;
      for (g = 0; g < ng; g++) {
         pamlh *q;
         int npg, n_eval = 0, lsg, npattg;
         if (pamlh_gene_subset(p, g, &q)) { fprintf(stderr, "error: gene %d\n", g + 1); return 1; }
         pamlh_dims(q, NULL, NULL, &npattg, NULL, NULL, NULL, NULL, &lsg, &npg, NULL);
         pamlh_default_x(q, x, 4096);
         if (optimize ? pamlh_optimize(q, x, &lnL, 500, 1e-10, 0, &n_eval) < 0 : (pamlh_set_x(q, x, npg) || pamlh_eval_gpu(q, &lnL, NULL))) {
            fprintf(stderr, "error: %s\n", pamlh_error(q)); return 1;
         }
         printf("Gene %2d  ls:%5d  npatt:%4d  lnL = %.6f\nx:", g + 1, lsg, npattg, lnL);
         for (i = 0; i < npg; i++) printf(" %.6f", x[i]);
         printf("\n");
         sum += lnL;
         pamlh_free(q);
      }
      printf("Sum of lnL over the %d genes = %.6f\n", ng, sum);
      pamlh_free(p);
      return 0;
   }
   if (!nx) nx = pamlh_read_inx(p, x, 4096);
   if (!nx) nx = pamlh_default_x(p, x, 4096);
   if (nx != np) { fprintf(stderr, "error: the model has %d parameters (ntime %d) but %d values were given\n", np, ntime, nx); return 1; }
   if (analytic) pamlh_use_analytic_gradient(p, analytic);
   if (supports) {      /* SH-like aLRT supports of the internal branches at x (after --optimize: at the estimates); instead of the evaluation */
      int nnode = 0, n = 0, n_eval = 0, *node, *fa_of;
      double *delta, *sup, *l3;
      char *nw;
      if (gpus > 0) { fprintf(stderr, "error: --branch-supports runs on one GPU\n"); return 1; }
      pamlh_dims(p, NULL, NULL, NULL, &nnode, NULL, NULL, NULL, NULL, NULL, NULL);
      if (optimize && pamlh_optimize(p, x, &lnL, 500, 1e-10, 0, &n_eval) < 0) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
      if (pamlh_branch_supports(p, NULL, 0, 0, &n, NULL, NULL, NULL, NULL)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
      node = (int *)malloc((n + 1) * sizeof(int)); delta = (double *)malloc((n + 1) * sizeof(double)); sup = (double *)malloc((n + 1) * sizeof(double));
      l3 = (double *)malloc((size_t)(3 * n + 3) * sizeof(double));
      if (pamlh_branch_supports(p, x, replicates > 0 ? replicates : 1000, sim_seed, &n, node, delta, sup, l3)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
      fa_of = (int *)malloc(nnode * sizeof(int));
      {
         const int *sp = pamlh_sons_ptr(p), *so = pamlh_sons(p);
         int v, j;
         for (v = 0; v < nnode; v++) fa_of[v] = -1;
         for (v = 0; v < nnode; v++)
            for (j = sp[v]; j < sp[v + 1]; j++) fa_of[so[j]] = v;
      }
      printf("Branch supports (SH-like aLRT, %d replicates, seed %llu): every configuration maximised over the five branches around the edge\n%10s %16s %16s %16s %12s %9s\n",
             replicates > 0 ? replicates : 1000, sim_seed, "branch", "l0", "l1", "l2", "delta", "support");
      for (i = 0; i < n; i++) printf("%4d..%-4d %16.6f %16.6f %16.6f %12.6f %9.3f\n", fa_of[node[i]] + 1, node[i] + 1, l3[3 * i], l3[3 * i + 1], l3[3 * i + 2], delta[i], sup[i]);
      nw = (char *)malloc((size_t)160 * nnode + 256);
      if (!pamlh_newick_supports(p, n, node, sup, nw, 160 * nnode + 256)) printf("%s\n", nw);
      free(nw); free(node); free(delta); free(sup); free(l3); free(fa_of);
      pamlh_free(p);
      return 0;
   }
   if (fg_scan) {      /* the foreground scan at x (after --optimize: at the estimates); instead of the evaluation */
      static const double dflt[9] = {1, 1.5, 2, 3, 5, 8, 12, 20, 50};
      int nnode = 0, nb = 0, n_eval = 0, *node, *best, *fa_of, *lab0, *order, j, k;
      double base = 0, *sl, *sp0, *sp1, *delta, *xa, *lo, *hi;
      char *nw;
      if (gpus > 0) { fprintf(stderr, "error: --foreground-scan runs on one GPU\n"); return 1; }
      if (!fg_ngrid) { memcpy(fg_grid, dflt, sizeof(dflt)); fg_ngrid = 9; }
      pamlh_dims(p, NULL, NULL, NULL, &nnode, NULL, NULL, NULL, NULL, NULL, NULL);
      if (pamlh_foreground_scan(p, NULL, 0, NULL, &nb, NULL, NULL, NULL, NULL, NULL, NULL, NULL)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
      if (optimize && pamlh_optimize(p, x, &lnL, 500, 1e-10, 0, &n_eval) < 0) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
      node = (int *)malloc(nb * sizeof(int)); best = (int *)malloc(nb * sizeof(int)); order = (int *)malloc(nb * sizeof(int));
      fa_of = (int *)malloc(nnode * sizeof(int)); lab0 = (int *)malloc(nnode * sizeof(int));
      sl = (double *)malloc((size_t)nb * fg_ngrid * sizeof(double)); sp0 = (double *)malloc((size_t)nb * fg_ngrid * sizeof(double));
      sp1 = (double *)malloc((size_t)nb * fg_ngrid * sizeof(double)); delta = (double *)malloc(nb * sizeof(double));
      xa = (double *)malloc((np + 1) * sizeof(double)); lo = (double *)malloc((np + 1) * sizeof(double)); hi = (double *)malloc((np + 1) * sizeof(double));
      memcpy(lab0, pamlh_labels(p), nnode * sizeof(int));
      if (pamlh_foreground_scan(p, x, fg_ngrid, fg_grid, &nb, node, &base, sl, sp0, sp1, delta, best)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
      {
         const int *sp = pamlh_sons_ptr(p), *so = pamlh_sons(p);
         int v;
         for (v = 0; v < nnode; v++) fa_of[v] = -1;
         for (v = 0; v < nnode; v++)
            for (j = sp[v]; j < sp[v + 1]; j++) fa_of[so[j]] = v;
      }
      printf("Foreground scan (branch-site model A, one engine call, %d branches x %d values of w2): lnL without a foreground class = %.6f\n%10s %10s %10s %10s %16s %12s\n",
             nb, fg_ngrid, base, "branch", "w2", "p0", "p1", "lnL", "delta");
      for (i = 0; i < nb; i++) {
         const int g = best[i];
         printf("%4d..%-4d %10.4f %10.6f %10.6f %16.6f %12.6f\n", fa_of[node[i]] + 1, node[i] + 1, fg_grid[g], sp0[i * fg_ngrid + g], sp1[i * fg_ngrid + g], sl[i * fg_ngrid + g], delta[i]);
      }
      for (i = 0; i < nb; i++) order[i] = i;
      for (i = 0; i < nb; i++)      /* descending delta, ties in node order */
         for (j = i + 1; j < nb; j++)
            if (delta[order[j]] > delta[order[i]]) { k = order[i]; order[i] = order[j]; order[j] = k; }
      pamlh_bounds(p, lo, hi);
      nw = (char *)malloc((size_t)160 * nnode + 256);
      for (k = 0; k < top && k < nb && delta[order[k]] > 0; k++) {      /* the best branches maximised as the foreground, from the scan's point */
         const int b = order[k], g = best[b];
         double l1 = 0;
         if (pamlh_foreground_point(p, x, node[b], fg_grid[g], sp0[b * fg_ngrid + g], sp1[b * fg_ngrid + g], xa) || pamlh_set_foreground(p, node[b])) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
         for (j = 0; j < np; j++) xa[j] = xa[j] < lo[j] ? lo[j] : xa[j] > hi[j] ? hi[j] : xa[j];
         if (pamlh_optimize(p, xa, &l1, 500, 1e-10, 0, &n_eval) < 0) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
         printf("foreground %d..%d maximised from the scan's point (lnL %.6f): lnL = %.6f\nx:", fa_of[node[b]] + 1, node[b] + 1, sl[b * fg_ngrid + g], l1);
         for (j = 0; j < np; j++) printf(" %.6f", xa[j]);
         printf("\n");
         if (!pamlh_newick(p, nw, 160 * nnode + 256)) printf("%s\n", nw);
      }
      if (top > 0) {      /* the tree's own labels again */
         for (j = 0; j < nnode && lab0[j] != 1; j++) ;
         if (j < nnode && pamlh_set_foreground(p, j)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
      }
      free(nw); free(node); free(best); free(order); free(fa_of); free(lab0); free(sl); free(sp0); free(sp1); free(delta); free(xa); free(lo); free(hi);
      pamlh_free(p);
      return 0;
   }
   if (nni_scores || nni_search) {      /* the neighbours' table at x, or the hill climb from x; instead of the evaluation */
      int nnode = 0, n = 0, stats[3] = {0, 0, 0};
      char *nw;
      if (gpus > 0) { fprintf(stderr, "error: --nni-scores and --nni-search run on one GPU\n"); return 1; }
      pamlh_dims(p, NULL, NULL, NULL, &nnode, NULL, NULL, NULL, NULL, NULL, NULL);
      if (nni_scores) {
         int *sw;
         double *sc, l0 = 0;
         if (pamlh_nni_scores(p, NULL, &n, NULL, NULL, NULL)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
         sw = (int *)malloc((size_t)(3 * n + 3) * sizeof(int)); sc = (double *)malloc((n + 1) * sizeof(double));
         if (pamlh_nni_scores(p, x, &n, sw, &l0, sc)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
         printf("NNI neighbours at the present branch lengths (one engine call): lnL of the present tree = %.6f\n%6s%6s%6s %16s %14s\n", l0, "v", "s", "x", "lnL", "difference");
         for (i = 0; i < n; i++) printf("%6d%6d%6d %16.6f %14.6f\n", sw[3 * i] + 1, sw[3 * i + 1] + 1, sw[3 * i + 2] + 1, sc[i], sc[i] - l0);
         free(sw); free(sc);
      }
      if (nni_search) {
         if (pamlh_nni_search(p, x, &lnL, max_moves, 1, stats)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
         printf("NNI search: %d moves, %d screening calls, %d neighbours maximised\n", stats[0], stats[1], stats[2]);
         nw = (char *)malloc((size_t)160 * nnode + 256);
         if (!pamlh_newick(p, nw, 160 * nnode + 256)) printf("%s\n", nw);
         free(nw);
         printf("x:");
         for (i = 0; i < np; i++) printf(" %.6f", x[i]);
         printf("\nlnL  = %.4f\n", lnL);
      }
      pamlh_free(p);
      return 0;
   }
   if (spr_scores || spr_search) {      /* the SPR neighbours' table at x, or the hill climb from x; instead of the evaluation */
      int nnode = 0, n = 0, stats[3] = {0, 0, 0};
      char *nw;
      if (gpus > 0) { fprintf(stderr, "error: --spr-scores and --spr-search run on one GPU\n"); return 1; }
      pamlh_dims(p, NULL, NULL, NULL, &nnode, NULL, NULL, NULL, NULL, NULL, NULL);
      if (spr_scores) {
         int *mv;
         double *sc, l0 = 0;
         if (pamlh_spr_scores(p, NULL, radius, split, &n, NULL, NULL, NULL)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
         mv = (int *)malloc((size_t)(2 * n + 2) * sizeof(int)); sc = (double *)malloc((n + 1) * sizeof(double));
         if (pamlh_spr_scores(p, x, radius, split, &n, mv, &l0, sc)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
         printf("SPR neighbours at the present branch lengths (one engine call, split %g): lnL of the present tree = %.6f\n%6s%6s %16s %14s\n", split, l0, "s", "x", "lnL", "difference");
         for (i = 0; i < n; i++) printf("%6d%6d %16.6f %14.6f\n", mv[2 * i] + 1, mv[2 * i + 1] + 1, sc[i], sc[i] - l0);
         free(mv); free(sc);
      }
      if (spr_search) {
         if (pamlh_spr_search(p, x, &lnL, radius, top, max_moves, 1, stats)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
         printf("SPR search: %d moves, %d screening calls, %d neighbours maximised\n", stats[0], stats[1], stats[2]);
         nw = (char *)malloc((size_t)160 * nnode + 256);
         if (!pamlh_newick(p, nw, 160 * nnode + 256)) printf("%s\n", nw);
         free(nw);
         printf("x:");
         for (i = 0; i < np; i++) printf(" %.6f", x[i]);
         printf("\nlnL  = %.4f\n", lnL);
      }
      pamlh_free(p);
      return 0;
   }
   if (place) {      /* the queries on every branch at x, or at the estimates on the tree's sequences; instead of the evaluation */
      const int nq = pamlh_n_queries(p), *order = pamlh_branch_order(p), *sptr = pamlh_sons_ptr(p), *sons = pamlh_sons(p);
      int nnode = 0, nb, q, e, j, n_eval = 0, *father, *be;
      double l0 = 0, *sc, *lwr, *bp, *bl;
      char *nw;
      pamlh_dims(p, NULL, NULL, NULL, &nnode, NULL, NULL, NULL, NULL, NULL, NULL);
      nb = nnode - 1;
      if (optimize && np > 0) {
         if (pamlh_optimize(p, x, &lnL, 500, 1e-10, 0, &n_eval) < 0) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
         printf("estimates on the tree's sequences after %d likelihood evaluations: lnL = %.6f\nx:", n_eval, lnL);
         for (i = 0; i < np; i++) printf(" %.6f", x[i]);
         printf("\n");
      }
      father = (int *)malloc(nnode * sizeof(int));
      for (i = 0; i < nnode; i++) for (j = sptr[i]; j < sptr[i + 1]; j++) father[sons[j]] = i;
      sc = (double *)malloc((size_t)(nq > 0 ? nq : 1) * nb * n_pend * sizeof(double)); lwr = (double *)malloc((size_t)(nq > 0 ? nq : 1) * nb * sizeof(double));
      be = (int *)malloc((nq > 0 ? nq : 1) * sizeof(int)); bp = (double *)malloc((nq > 0 ? nq : 1) * sizeof(double)); bl = (double *)malloc((nq > 0 ? nq : 1) * sizeof(double));
      nw = (char *)malloc((size_t)160 * (nnode + 2) + 256);
      if (place_ml) {      /* the kept branches of every query maximised over the three lengths at the new node */
         int n_rows = 0, r, *rq = (int *)malloc((size_t)(nq > 0 ? nq : 1) * nb * sizeof(int)), *re = (int *)malloc((size_t)(nq > 0 ? nq : 1) * nb * sizeof(int));
         double *t3 = (double *)malloc((size_t)3 * (nq > 0 ? nq : 1) * nb * sizeof(double)), *ml = (double *)malloc((size_t)(nq > 0 ? nq : 1) * nb * sizeof(double));
         if (pamlh_placement_scores(p, x, n_pend, pend, split, &l0, sc) || pamlh_place_ml(p, x, keep, n_pend, pend, split, rq, re, t3, ml, lwr, &n_rows)) {
            fprintf(stderr, "error: %s\n", pamlh_error(p));
            return 1;
         }
         printf("maximum-likelihood placement of %d quer%s, %d of %d branches kept per query: lnL of the tree = %.6f\n", nq, nq == 1 ? "y" : "ies", n_rows / nq, nb, l0);
         for (q = 0, r = 0; q < nq; q++) {
            int best = r;
            printf("\nquery %d (%s)\n%10s %10s %10s %10s %16s %14s %9s\n", q + 1, pamlh_query_name(p, q), "branch", "t_up", "t_dn", "pendant", "lnL", "difference", "LWR");
            for (; r < n_rows && rq[r] == q; r++) if (ml[r] > ml[best]) best = r;
            for (e = r - n_rows / nq; e < r; e++) {
               char br[32];
               snprintf(br, sizeof(br), "%d..%d", father[order[re[e]]] + 1, order[re[e]] + 1);
               printf("%10s %10.6f %10.6f %10.6f %16.6f %14.6f %9.6f%s\n", br, t3[3 * e], t3[3 * e + 1], t3[3 * e + 2], ml[e], ml[e] - l0, lwr[e], e == best ? " *" : "");
            }
            if (pamlh_placement_newick3(p, q, re[best], t3[3 * best], t3[3 * best + 1], t3[3 * best + 2], nw, 160 * (nnode + 2) + 256)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
            printf("%s\n", nw);
         }
         free(rq); free(re); free(t3); free(ml); free(father); free(sc); free(lwr); free(be); free(bp); free(bl); free(nw);
         pamlh_free(p);
         return 0;
      }
      if (pamlh_placement_scores(p, x, n_pend, pend, split, &l0, sc) || pamlh_place(p, x, n_pend, pend, split, be, bp, bl, lwr)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
      printf("placement of %d quer%s on %d branches (one engine call): lnL of the tree = %.6f, split %.4f\n", nq, nq == 1 ? "y" : "ies", nb, l0, split);
      for (q = 0; q < nq; q++) {
         printf("\nquery %d (%s)\n%10s %10s %16s %14s %9s\n", q + 1, pamlh_query_name(p, q), "branch", "pendant", "lnL", "difference", "LWR");
         for (e = 0; e < nb; e++) {
            const double *row = sc + ((size_t)q * nb + e) * n_pend;
            char br[32];
            int mj = 0;
            for (j = 1; j < n_pend; j++) if (row[j] > row[mj]) mj = j;
            snprintf(br, sizeof(br), "%d..%d", father[order[e]] + 1, order[e] + 1);
            printf("%10s %10.6f %16.6f %14.6f %9.6f%s\n", br, pend[mj], row[mj], row[mj] - l0, lwr[(size_t)q * nb + e], e == be[q] ? " *" : "");
         }
         if (pamlh_placement_newick(p, q, be[q], split, bp[q], nw, 160 * (nnode + 2) + 256)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
         printf("%s\n", nw);
      }
      free(father); free(sc); free(lwr); free(be); free(bp); free(bl); free(nw);
      pamlh_free(p);
      return 0;
   }
   if (optimize) {
      /* method = 1 in the control file: minB / minbranches (one branch at a time on the branch-local derivatives) */
      const int method1 = pamlh_method(p) == 1;
      int n_eval = 0, rc;
      if (newton_full) {
         int st[3] = {0, 0, 0};
         if (pamlh_newton_full(p, x, 1e-8, 50, &lnL, 1, st)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
         printf("newton-full: lnL %.6f after %d sweeps (%d engine calls, %d rejected)\n", lnL, st[0], st[1], st[2]);
      }
      rc = newton    ? pamlh_optimize_newton(p, x, &lnL, 1e-6, 2, &n_eval)
                           : method1 ? pamlh_optimize_minb(p, x, &lnL, 1e-6, 1, &n_eval)
                                     : pamlh_optimize(p, x, &lnL, 500, 1e-10, 1, &n_eval);
      if (rc < 0) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
      printf("%s after %d likelihood evaluations\nx:", rc ? "iteration limit reached" : "converged", n_eval);
      for (i = 0; i < np; i++) printf(" %.6f", x[i]);
      printf("\n");
      for (i = ntime; i < np; i++) { char nm[64]; pamlh_param_name(p, i, nm, sizeof(nm)); printf("  %-24s %12.6f\n", nm, x[i]); }
      {
         int nnode = 0;
         char *nw;
         pamlh_dims(p, NULL, NULL, NULL, &nnode, NULL, NULL, NULL, NULL, NULL, NULL);
         nw = (char *)malloc((size_t)160 * nnode + 256);
         if (!pamlh_set_x(p, x, np) && !pamlh_newick(p, nw, 160 * nnode + 256)) printf("%s\n", nw);
         free(nw);
      }
      if (!gpus) {      /* (the scores' outer product is a sum over all site patterns: one GPU holds them all) */
         double *se = (double *)malloc((np + 1) * sizeof(double));
         if (!pamlh_standard_errors(p, x, 0, se, NULL)) {
            printf("SEs for parameters:\n ");
            for (i = 0; i < np; i++) printf(" %.6f", se[i]);
            printf("\n");
         }
         free(se);
      }
   }
   if (bv_out) {      /* at the vector evaluated or just estimated */
      if (gpus > 0) { fprintf(stderr, "error: --bv runs on one GPU\n"); return 1; }
      if (exact_hessian ? pamlh_write_bv_exact(p, x, bv_out) : pamlh_write_bv(p, x, bv_out)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
      printf("gradient and Hessian of the %d branch lengths -> %s\n", ntime, bv_out);
   }
   if (se_exact) {      /* at the vector evaluated or just estimated */
      double *se = (double *)malloc((np + 1) * sizeof(double));
      if (gpus > 0) { fprintf(stderr, "error: --se-exact runs on one GPU\n"); return 1; }
      if (pamlh_standard_errors_exact(p, x, se, NULL)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
      printf("SEs for parameters (observed information, exact branch block):\n ");
      for (i = 0; i < np; i++) printf(" %.6f", se[i]);
      printf("\n");
      free(se);
   }
   if (subst_counts) {      /* at the vector evaluated or just estimated */
      const int *order = pamlh_branch_order(p), *sptr = pamlh_sons_ptr(p), *sons = pamlh_sons(p);
      int n = 0, nnode = 0, nl = 0, one = 0, n_sites = 0, l, b, h, j, *father;
      char names[3][32];
      double *M, *cnt, *site = NULL;
      if (gpus > 0) { fprintf(stderr, "error: --subst-counts runs on one GPU\n"); return 1; }
      pamlh_dims(p, &n, NULL, NULL, &nnode, NULL, NULL, NULL, NULL, NULL, NULL);
      pamlh_pose(p, &n_sites);
      M = (double *)malloc((size_t)3 * n * n * sizeof(double));
      if (pamlh_count_labels(p, NULL, &nl, M, names) || pamlh_count_labels(p, "total", &one, M + (size_t)nl * n * n, names + nl)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
      nl += one;
      cnt = (double *)malloc((size_t)nl * (ntime + 1) * sizeof(double));
      if (per_site) site = (double *)malloc((size_t)nl * (ntime + 1) * (n_sites + 1) * sizeof(double));
      if (pamlh_subst_counts(p, x, nl, M, cnt, site)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
      father = (int *)malloc(nnode * sizeof(int));
      for (b = 0; b < nnode; b++) father[b] = -1;
      for (b = 0; b < nnode; b++) for (j = sptr[b]; j < sptr[b + 1]; j++) father[sons[j]] = b;
      printf("\nExpected numbers of substitutions for each branch (posterior means given the data, one engine call)\n\n%10s %10s", "branch", "t");
      for (l = 0; l < nl; l++) printf(" %15s", names[l]);
      printf("\n\n");
      for (b = 0; b < ntime; b++) {
         char br[32];
         snprintf(br, sizeof(br), "%d..%d", father[order[b]] + 1, order[b] + 1);
         printf("%10s %10.6f", br, x[b]);
         for (l = 0; l < nl; l++) printf(" %15.6f", cnt[(size_t)l * ntime + b]);
         printf("\n");
      }
      for (l = 0; per_site && l < nl; l++) {
         printf("\nExpected %s substitutions: site, then the branches in the order above\n", names[l]);
         for (h = 0; h < n_sites; h++) {
            printf("%6d", h + 1);
            for (b = 0; b < ntime; b++) printf(" %9.6f", site[((size_t)l * ntime + b) * n_sites + h]);
            printf("\n");
         }
      }
      free(M); free(cnt); free(site); free(father);
   }
   if (sim_out) {      /* the data sets of a parametric bootstrap instead of the evaluation */
      int ns = 0, n_pose = 0, r;
      const int nrep = replicates > 0 ? replicates : 1;
      unsigned char *zs;
      if (gpus > 0) { fprintf(stderr, "error: --simulate runs on one GPU\n"); return 1; }
      pamlh_dims(p, NULL, &ns, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
      pamlh_pose(p, &n_pose);
      if (sim_sites < 1) sim_sites = n_pose;
      zs = (unsigned char *)malloc((size_t)ns * sim_sites);
      for (r = 0; r < nrep; r++) {
         char path[4096];
         if (nrep == 1) snprintf(path, sizeof(path), "%s", sim_out); else snprintf(path, sizeof(path), "%s.%04d", sim_out, r);
         if (pamlh_simulate(p, x, sim_sites, sim_seed, (unsigned)r, zs, NULL) || pamlh_write_alignment(p, zs, sim_sites, path)) {
            fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1;
         }
         printf("simulated %d sequences x %ld sites (seed %llu, replicate %d) -> %s\n", ns, sim_sites, sim_seed, r, path);
      }
      free(zs);
      pamlh_free(p);
      return 0;
   }
   if (pamlh_set_x(p, x, np)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
   lnf = (double *)malloc(npatt * sizeof(double));
   if (pamlh_eval_gpu(p, &lnL, lnf)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
   printf("ntime & np: %d %d   npatt %d\nlnL  = %.6f\n", ntime, np, npatt, lnL);
   if (gpus > 0) {      /* sharded run: lnL (the total over the ranks) and the estimates are the output */
      int st = 0, bad = 0;
      printf("(site patterns sharded over %d GPUs, %d on rank 0; lnL is the all-reduced total)\n", gpus, npatt);
      fflush(stdout);
      free(lnf);
      pamlh_free(p);
      if (rank == 0) {      /* the result is out: from here on the ranks just end (on_sigchld reaps them too; ECHILD ends the loop) */
         ranks_done = 1;
         signal(SIGCHLD, SIG_DFL);
         while (wait(&st) > 0) bad |= !WIFEXITED(st) || WEXITSTATUS(st);
      }
      return bad ? 1 : 0;
   }
   {  /* codon models without site classes: the reference's "dN & dS for each branch" table (codeml.c:1361-1404) */
      int nn = 0, b;
      double *tab;
      pamlh_dims(p, NULL, NULL, NULL, &nn, NULL, NULL, NULL, NULL, NULL, NULL);
      tab = (double *)malloc((size_t)nn * 6 * sizeof(double));
      if (!strcmp(argv[1], "codeml") && !pamlh_dnds(p, x, tab)) {
         double dnt = 0, dst = 0;
         printf("\ndN & dS for each branch\n\n%7s%11s%8s%8s%8s%8s%8s\n\n", "branch", "t", "N", "S", "dN/dS", "dN", "dS");
         for (b = 0; b < nn - 1; b++) {
            const double *r = tab + b * 6;
            printf("%7d %10.3f %7.1f %7.1f %7.4f %7.4f %7.4f\n", b + 1, r[0], r[1], r[2], r[3], r[4], r[5]);
            dnt += r[4]; dst += r[5];
         }
         printf("\ntree length for dN: %12.4f\ntree length for dS: %12.4f\n", dnt, dst);
      }
      free(tab);
      if (pamlh_set_x(p, x, np)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
   }
   {  /* site-class models: the NEB table the reference prints (sites with Pr(last class) > 0.5 when its omega > 1) */
      int mode, K, n_sites, h, npos = pamlh_positive_classes(p);
      pamlh_model(p, &mode, &K, NULL, NULL);
      if (mode == 1 && K > 1 && npos && pamlh_class_omega(p)[K - 1] > 1) {
         double *post = (double *)malloc((size_t)K * npatt * sizeof(double)), *mw = (double *)malloc(npatt * sizeof(double));
         const int *pose = pamlh_pose(p, &n_sites);
         if (!pamlh_neb(p, post, mw)) {
            printf("\nNaive Empirical Bayes (NEB): sites with Pr(w>1) > 0.5\n   site   Pr(w>1)   post mean w\n");
            for (h = 0; h < n_sites; h++) {      /* branch-site models: classes 2a + 2b (foreground omega) */
               const double pr = post[(size_t)(K - 1) * npatt + pose[h]] + (npos == 2 ? post[(size_t)(K - 2) * npatt + pose[h]] : 0);
               if (pr > 0.5) printf("%7d   %7.3f   %9.3f\n", h + 1, pr, mw[pose[h]]);
            }
         }
         if (npos == 2) {  /* branch-site model A: BEB over (p0, p1, w0, w2), classes 2a + 2b */
            double *bp = (double *)malloc((size_t)4 * npatt * sizeof(double));
            if (!pamlh_beb_acd(p, x, bp)) {
               printf("\nBayes Empirical Bayes (BEB): positive sites for foreground lineages Prob(w>1) > 0.5\n   site   Pr(w>1)\n");
               for (h = 0; h < n_sites; h++) {
                  const double pr = bp[(size_t)2 * npatt + pose[h]] + bp[(size_t)3 * npatt + pose[h]];
                  if (pr > 0.5) printf("%7d   %7.3f%s\n", h + 1, pr, pr > 0.99 ? "**" : pr > 0.95 ? "*" : "");
               }
            }
            free(bp);
         }
         if (npos == 1) {  /* M2a / M8: the BEB table as well */
            double *pr = (double *)malloc(npatt * sizeof(double)), *sw = (double *)malloc(npatt * sizeof(double));
            if (!pamlh_beb(p, x, pr, mw, sw)) {
               printf("\nBayes Empirical Bayes (BEB): sites with Pr(w>1) > 0.5\n   site   Pr(w>1)   post mean +- SE for w\n");
               for (h = 0; h < n_sites; h++)
                  if (pr[pose[h]] > 0.5) printf("%7d   %7.3f   %9.3f +- %5.3f\n", h + 1, pr[pose[h]], mw[pose[h]], sw[pose[h]]);
            }
            free(pr); free(sw);
         }
         free(post); free(mw);
      }
   }
   if (ancestral) {   /* RateAncestor = 1: most probable state and its probability at every internal node, per site (rst's marginal table) */
      static const char *const alpha[3] = {"TCAG", "", "ARNDCQEGHILKMFPSTWYV"};
      int n, ns, nnode, seqtype_n, n_sites, h, node, k;
      const int *pose = pamlh_pose(p, &n_sites);
      double *post, *best_p;
      int *best;
      pamlh_dims(p, &n, &ns, NULL, &nnode, NULL, NULL, NULL, NULL, NULL, NULL);
      seqtype_n = n == 4 ? 0 : n == 20 ? 2 : 1;
      post = (double *)malloc((size_t)npatt * n * sizeof(double));
      best = (int *)malloc((size_t)(nnode - ns) * npatt * sizeof(int));
      best_p = (double *)malloc((size_t)(nnode - ns) * npatt * sizeof(double));
      for (node = ns; node < nnode; node++) {
         if (pamlh_node_posterior(p, node, post)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
         for (h = 0; h < npatt; h++) {
            int bi = 0;
            for (k = 1; k < n; k++) if (post[(size_t)h * n + k] > post[(size_t)h * n + bi]) bi = k;
            best[(size_t)(node - ns) * npatt + h] = bi; best_p[(size_t)(node - ns) * npatt + h] = post[(size_t)h * n + bi];
         }
      }
      printf("\nMarginal reconstruction of ancestral states: site, then for nodes %d..%d the most probable state (probability)\n", ns + 1, nnode);
      for (h = 0; h < n_sites; h++) {
         printf("%6d ", h + 1);
         for (node = ns; node < nnode; node++) {
            const int b = best[(size_t)(node - ns) * npatt + pose[h]];
            if (seqtype_n == 1) printf(" %2d(%.3f)", b, best_p[(size_t)(node - ns) * npatt + pose[h]]);      /* codons: index among the sense codons */
            else printf(" %c(%.3f)", alpha[seqtype_n][b], best_p[(size_t)(node - ns) * npatt + pose[h]]);
         }
         printf("\n");
      }
      free(post); free(best); free(best_p);
   }
   if (ancestral_all) {   /* the same marginal table from ONE engine call for all nodes, then (one rate class) the joint reconstruction */
      static const char *const alpha[3] = {"TCAG", "", "ARNDCQEGHILKMFPSTWYV"};
      int n, ns, nnode, seqtype_n, n_sites, h, node, ni;
      const int *pose = pamlh_pose(p, &n_sites);
      double *best_p;
      unsigned char *best;
      pamlh_dims(p, &n, &ns, NULL, &nnode, NULL, NULL, NULL, NULL, NULL, NULL);
      seqtype_n = n == 4 ? 0 : n == 20 ? 2 : 1;
      ni = nnode - ns;
      best = (unsigned char *)malloc((size_t)ni * npatt);
      best_p = (double *)malloc((size_t)ni * npatt * sizeof(double));
      if (pamlh_ancestral_marginal(p, best, best_p, NULL)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
      printf("\nMarginal reconstruction of ancestral states: site, then for nodes %d..%d the most probable state (probability)\n", ns + 1, nnode);
      for (h = 0; h < n_sites; h++) {
         printf("%6d ", h + 1);
         for (node = ns; node < nnode; node++) {
            const int b = best[(size_t)(node - ns) * npatt + pose[h]];
            if (seqtype_n == 1) printf(" %2d(%.3f)", b, best_p[(size_t)(node - ns) * npatt + pose[h]]);      /* codons: index among the sense codons */
            else printf(" %c(%.3f)", alpha[seqtype_n][b], best_p[(size_t)(node - ns) * npatt + pose[h]]);
         }
         printf("\n");
      }
      if (pamlh_n_classes(p) == 1) {
         if (pamlh_ancestral_joint(p, best, best_p)) { fprintf(stderr, "error: %s\n", pamlh_error(p)); return 1; }
         printf("\nJoint reconstruction of ancestral states: site, the states at nodes %d..%d, the probability of the assignment\n", ns + 1, nnode);
         for (h = 0; h < n_sites; h++) {
            printf("%6d  ", h + 1);
            for (node = ns; node < nnode; node++) {
               const int b = best[(size_t)(node - ns) * npatt + pose[h]];
               if (seqtype_n == 1) printf(" %2d", b);
               else printf("%c", alpha[seqtype_n][b]);
            }
            printf("  %.3f\n", exp(best_p[pose[h]] - lnf[pose[h]]));
         }
      }
      free(best); free(best_p);
   }
   pamlh_write_lnf(p, "lnf", lnf);
   free(lnf);
   pamlh_free(p);
   return 0;
}
