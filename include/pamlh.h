/* pamlh.h — host side of the MI355X likelihood engine, in C as the reference is.
 *
 * It reads the same inputs the reference programs read — the `.ctl` file (GetOptions codeml.c:1694 / baseml.c:954),
 * the sequence file (ReadSeq treesub.c:487: PHYLIP sequential / interleaved, `.` repeats, the `P` pattern format, options G / GC;
 * aligned FASTA and NEXUS, GetSeqFileType treesub.c:367),
 * the tree file (ReadTreeN treesub.c:3048) and `in.codeml` / `in.baseml` (readx treesub.c:4035) — compresses sites
 * into patterns in the reference's order (PatternWeight treesub.c:1386), encodes them (EncodeSeqs 1116,
 * SetMapAmbiguity 1218), and turns a parameter vector x[] into the engine's inputs the way SetParameters
 * (codeml.c:2757, baseml.c:1306) does: branch lengths, pi, eigen systems, site classes.  It then drives
 * libpaml_amd.so through include/paml_amd.h.  Scope (this round): codeml seqtype 1 (icode 0 and 1; CodonFreq 0-5 (incl. F1x4MG / F3x4MG); NSsites
 * 0-13 and 22 with model 0; with '#' labels in the tree the branch model (model 2, NSsites 0), the branch-site models A and B
 * (model 2, NSsites 2 / 3) and the clade models C and D (model 3, NSsites 2 / 3)) and seqtype 2 / 3 (aa models 0,1,2,3), baseml models JC69,K80,F81,F84,HKY85,T92,TN93,REV,UNREST; +Gamma, auto-discrete-gamma (rho), nhomo 1 (base frequencies as parameters); several genes
 * (option G / GC of the sequence file) with Mgene 0,1,2,3,4 for baseml, codeml M0 and aaml;
 * clock 0 and 1 (global clock: x holds the internal node ages); fix_blength 0, 2 (fixed) and 3 (proportional); cleandata 0/1; sequential and interleaved (I) PHYLIP, the P pattern format.  Anything else fails with a message
 * instead of guessing.
 */
#ifndef PAMLH_H
#define PAMLH_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pamlh pamlh;

/* program: "codeml" or "baseml".  Paths inside the ctl are resolved relative to the ctl file's directory. */
int pamlh_load(pamlh **out, const char *ctl_path, const char *program, char *err, int errcap);
/* the same with the tree_index-th (0-based) tree of the tree file — the reference evaluates the trees of the file one after the
 * other (Forestry codeml.c:635, baseml.c:451) — and the number of trees the file holds */
int pamlh_load_tree(pamlh **out, const char *ctl_path, const char *program, int tree_index, char *err, int errcap);
int pamlh_n_trees(const pamlh *p);
/* ... and with control-file options replaced or added: overrides = "key = value" lines separated by newlines or ';' (NULL: none).  A
 * control file that lists several site models ("NSsites = 0 1 2 7 8": the reference runs them in turn, the insmodel loop codeml.c:657-906) is one analysis
 * per model here: overrides = "NSsites = 2".  pamlh_ctl_option returns an option's text as the control file (or an override) gave it. */
int pamlh_load_with(pamlh **out, const char *ctl_path, const char *program, int tree_index, const char *overrides, char *err, int errcap);
const char *pamlh_ctl_option(const pamlh *p, const char *key);
/* "dN & dS for each branch" (DetailOutput codeml.c:1349-1404) under the codon models without site classes: out[n_branches][6] = t, N, S,
 * omega, dN, dS at the parameter vector x; n_branches = n_nodes - 1, in the order of the branch lengths in x (first appearance in the tree file) */
int pamlh_dnds(pamlh *p, const double *x, double *out);
/* Comparison of the trees of a tree file from the per-pattern log likelihoods of their analyses (rell treesub.c:5844-6009: the table
 * "tree li Dli +- SE pKH pSH pRELL" of a run with several trees).  lnf [n_trees][n_patt], w pattern counts, gene_off n_genes + 1 offsets
 * (NULL: one gene); n_rep = 0: the reference's number of bootstrap replicates; outputs have n_trees entries each (pKH, pSH = -1 for the best
 * tree, whose index goes to *best).  li, Dli, SE, pKH are deterministic; pSH and pRELL come from seeded resampling. */
int pamlh_tree_comparison(int n_trees, int n_patt, const double *w, const double *lnf, int n_genes, const int *gene_off, int n_rep,
                          unsigned long long seed, double *li, double *dli, double *se, double *pkh, double *psh, double *prell, int *best);
/* The table arithmetic alone, from a given replicate matrix rep[n_rep][n_trees] (rep[r][t] = log likelihood of tree t on resampled
 * alignment r): same tie rule (within 1e-5: the replicate is shared), same per-tree centring for S-H, pKH = pSH = -1 for the best tree. */
int pamlh_tree_comparison_from_replicates(int n_trees, int n_patt, const double *w, const double *lnf, int n_rep, const double *rep,
                                          double *li, double *dli, double *se, double *pkh, double *psh, double *prell, int *best);
/* pamlh_tree_comparison with the replicates drawn on the GPU (paml_amd_rell_replicates; a generator of its own, so pSH and pRELL differ
 * from the host path's within Monte-Carlo accuracy).  n_rep = 0: 10 000 replicates at EVERY alignment length — the reference and the host
 * path drop to 50 at 10^5 sites.  Returns 0 or the engine library's negative code (message: paml_amd_last_error(NULL)). */
int pamlh_tree_comparison_gpu(int n_trees, int n_patt, const double *w, const double *lnf, int n_genes, const int *gene_off, int n_rep,
                              unsigned long long seed, double *li, double *dli, double *se, double *pkh, double *psh, double *prell, int *best);
void pamlh_free(pamlh *p);
const char *pamlh_error(const pamlh *p);

/* sizes: n_states (com.ncode), n_tips (com.ns), n_patt (com.npatt), n_nodes (tree.nnode), root, n_codes, cleandata,
 * ls (sites or codons after cleaning), np (free parameters the reference would put in x[]), ntime (branch lengths in x) */
int pamlh_dims(const pamlh *p, int *n_states, int *n_tips, int *n_patt, int *n_nodes, int *root, int *n_codes,
               int *cleandata, int *ls, int *np, int *ntime);

/* data (valid until pamlh_free) */
const unsigned char *pamlh_tips(const pamlh *p);        /* [n_tips][n_patt] */
const double *pamlh_weights(const pamlh *p);            /* [n_patt] */
const int *pamlh_n_chara(const pamlh *p);               /* [n_codes] */
const unsigned char *pamlh_chara_map(const pamlh *p);   /* [n_codes][n_states] */
const int *pamlh_sons_ptr(const pamlh *p);              /* [n_nodes+1] */
const int *pamlh_sons(const pamlh *p);
const int *pamlh_labels(const pamlh *p);                /* [n_nodes] */
const unsigned char *pamlh_scale_nodes(const pamlh *p); /* [n_nodes], SetNodeScale treesub.c:7177 */
const int *pamlh_branch_order(const pamlh *p);          /* [ntime_all]: node below the i-th branch of tree.branches */

/* default x[]: branch lengths from the tree file, substitution parameters from the ctl (GetInitials) */
int pamlh_default_x(const pamlh *p, double *x, int cap);
/* in.codeml / in.baseml next to the ctl ("-1 x0 x1 ..."); returns the number of values read, 0 if absent */
int pamlh_read_inx(const pamlh *p, double *x, int cap);

/* SetParameters: x -> model state */
int pamlh_set_x(pamlh *p, const double *x, int np);
int pamlh_model(const pamlh *p, int *mode, int *K, int *n_eigen, int *n_labels);
const double *pamlh_branch(const pamlh *p);             /* [n_nodes] */
const double *pamlh_pi(const pamlh *p);                 /* [n_states] */
const double *pamlh_freqK(const pamlh *p);
const double *pamlh_rate(const pamlh *p);
const int *pamlh_eigen_of(const pamlh *p);              /* [K][n_labels] */
const double *pamlh_qfactor(const pamlh *p);
const double *pamlh_adg_matrix(const pamlh *p);         /* [K][K] auto-discrete-gamma transition matrix (rho != 0), else NULL */
/* option G (several genes): returns n_genes; gene_off[n_genes + 1] = first pattern of each gene (com.posG), gene_rate[n_genes]
 * = com.rgene after pamlh_set_x, n_pi = frequency vectors in pamlh_pi (1, or n_genes under Mgene 2 / 4), gene_eigen_of
 * [n_genes][K] = eigen system of (gene, class) (NULL with one gene).  Any output pointer may be NULL. */
/* Mgene = 1 (separate analyses): gene g of the data set as an independent analysis (own patterns, frequencies, parameters); the
 * caller frees it with pamlh_free. */
int pamlh_gene_subset(const pamlh *p, int g, pamlh **out);
int pamlh_mgene(const pamlh *p);                       /* the Mgene option in effect (0 with one gene) */
int pamlh_n_classes(const pamlh *p);                   /* site classes of the model as set up (1: none) */
int pamlh_malpha(const pamlh *p);      /* 1: a gamma shape per gene (Malpha); pamlh_rate() then returns [n_genes][K] */
int pamlh_genes(const pamlh *p, const int **gene_off, const double **gene_rate, int *n_pi, const int **gene_eigen_of);            /* [K][n_labels] time scale per (class, branch type); NULL = all 1 */
/* eigen system i: kind (paml_amd.h), and pointers (NULL when not applicable) */
int pamlh_eigen(const pamlh *p, int i, int *kind, int *nR, double *kappa, const double **U, const double **V,
                const double **Root, const double **Cijk);

/* Multi-GPU, one process per GPU: keep this rank's contiguous block of site patterns and join the ranks' RCCL communicator when the
 * engine is created (id128 = rank 0's paml_amd_comm_unique_id, handed over by any means); every evaluation then returns the
 * lnL of the WHOLE alignment on every rank, bit for bit the same for any number of ranks.  `pamlh_lnl --gpus N` is the driver. */
int pamlh_set_shard(pamlh *p, int rank, int world, const void *id128);

/* The paml_amd_engine behind this analysis (NULL before the first evaluation). */
void *pamlh_engine_handle(const pamlh *p);

/* One likelihood evaluation on the GPU through the engine ABI (creates the engine on first use).  lnf may be NULL. */
int pamlh_eval_gpu(pamlh *p, double *lnL, double *lnf);
/* lnL at n_batch parameter vectors xs[n_batch][np] in ONE launch (paml_amd_eval_batch): vectors that differ only in branch
 * lengths share one model set-up; vectors the model rejects get -1e300. */
int pamlh_eval_batch_gpu(pamlh *p, int n_batch, const double *xs, double *lnL);
/* Box constraints of x[] as SetxBound sets them (codeml.c:1880, baseml.c:1100). */
int pamlh_bounds(const pamlh *p, double *lo, double *hi);
/* Maximum-likelihood estimation (the job of ming2, tools.c:6595): BFGS in the box, every gradient (2 np central
 * differences) and every line search (12 trial steps) evaluated as one batch on the GPU.  x: start in, estimate out.
 * Returns 0 converged, 1 max_iter reached, < 0 error.  n_eval (may be NULL): likelihood evaluations spent. */
int pamlh_optimize(pamlh *p, double *x, double *lnL, int max_iter, double tol, int verbose, int *n_eval);
/* The gradient d(+lnL)/dx at x (np entries) and lnL.  The entries of x that are plain branch lengths — the leading ntime ones when
 * there is no clock and no proportional fix_blength = 3 — come from ONE engine call (paml_amd_gradient: the derivative of the lnL of
 * the tree as it is rooted, whatever models its branches carry), mapped by pamlh_branch_order; every other entry by the central
 * differences pamlh_optimize uses, in one batch.  All entries come by differences with rho != 0 (lfunAdG) and with a rate-matrix
 * (UNREST) model. */
int pamlh_gradient(pamlh *p, const double *x, double *lnL, double *g);
/* on != 0: pamlh_optimize takes the branch-length entries of its gradients from that call and batches only the remaining parameters;
 * the call counts as one evaluation in n_eval.  Off by default: pamlh_optimize then does exactly what it did without it. */
int pamlh_use_analytic_gradient(pamlh *p, int on);
/* on = 2: every entry of pamlh_optimize's gradients comes from pamlh_gradient_full (one engine call per gradient, counted as one
 * evaluation); where that call does not serve, what on = 1 does.
 * pamlh_rate_matrix: A[n][n], the matrix the engine exponentiates (P = exp(A tau)) for eigen set `set` of the present model state.
 * pamlh_gradient_full: d(+lnL)/dx at x (np entries) and lnL from ONE paml_amd_model_gradient call and a chain rule on the host: the
 * engine inputs the state would install at x +- h e_i (rate matrices, effective lengths, freqK, root frequencies; pamlh_set_x only, no
 * evaluation and no device decomposition per parameter) are differenced (a Richardson pair of central differences at 1e-3 (1 + |x_i|)
 * and half of it; h = 1e-6 (1 + |x_i|), one-sided where needed, next to the box) and contracted with the engine's
 * derivatives.  The state is left at x.  Returns 1, touching nothing, where pamlh_gradient differences the branch lengths (a clock,
 * fix_blength = 3, rho != 0, a rate-matrix (UNREST) model). */
int pamlh_rate_matrix(pamlh *p, int set, double *A);
int pamlh_gradient_full(pamlh *p, const double *x, double *lnL, double *g);
/* g[ntime] as pamlh_gradient's leading entries and H[ntime][ntime], H_ij = -sum_h w_h s_i(h) s_j(h) with the analytic per-pattern
 * scores s_i(h) = d log f_h / d t_i (HessianSKT2004's method 1, treesub.c:7241).  Refused where pamlh_gradient would difference the
 * branch lengths. */
int pamlh_branch_hessian(pamlh *p, const double *x, double *g, double *H);
/* The block the reference writes to rst2 for mcmctree's in.BV (baseml.c:581-596), at x: the number of sequences, the Newick tree with
 * branch lengths, the ntime lengths (%9.6f), the gradient (an entry with x > 0.0004 and |g| < 0.005 written as 0), the line "Hessian" and
 * the matrix (%10.4g), from pamlh_branch_hessian.  Refused unless the tree is unrooted (three sons at the root) and there is no clock. */
int pamlh_write_bv(pamlh *p, const double *x, const char *path);

/* Nearest-neighbour interchange (NNI) on the analysis's tree (pamlh_nni.c).  A swap is (v, s, x), 0-based nodes: v an internal node that
 * is not the root, s a son of v, x a son of the father of v other than v; the subtrees below s and x change places and each keeps the
 * branch above it, so the same parameter vector describes the rearranged tree.  All three are refused by name with a clock (the
 * reference's search refuses it too, treesub.c:4653), with rho models and for runmode = -2.
 * pamlh_nni_scores: the canonical list of the tree as it stands (paml_amd_nni_list: 2 (ns - 3) swaps on an unrooted binary tree, the
 *   reference's neighbours, treesub.c:4687) scored at x in ONE engine call (paml_amd_nni_scores): swaps[*n_swaps][3], lnL[*n_swaps] =
 *   the neighbours' lnL at the branch lengths and parameters of x, *lnL0 = the present tree's.  With swaps = lnL = NULL only *n_swaps
 *   is written (host only): the room for the list is the caller's.
 * pamlh_apply_nni: exchanges the two sons in place in the son lists, marks the scaling nodes as for a tree just read (SetNodeScale
 *   treesub.c:7177) and sends the tree to the engine again.  Node ids, labels and pamlh_branch_order stay, so the layout of x does not
 *   change; (v, x, s) afterwards undoes it.
 * pamlh_nni_search: the hill climb of the reference's runmode = 5 (Perturbation treesub.c:4642).  pamlh_optimize on the present tree;
 *   then per step one pamlh_nni_scores at the estimates, the neighbours in descending order of their screened lnL, each applied and
 *   maximised from the present x: the first whose maximised lnL is higher by more than 1e-4 (the reference prints the search's lnL
 *   with four decimals, treesub.c:4709) is kept, every other is undone.  It ends after a step in which every neighbour was maximised
 *   and none was better: the final tree is an NNI-local optimum, as the reference's — the screening only decides the order — or after
 *   max_moves moves (<= 0: no limit).  x: start in, estimates on the final tree out (the model state is left at them: pamlh_newick
 *   prints the tree found).  stats (NULL or 3 entries): moves, screening calls, neighbours maximised (the starting tree's own
 *   maximisation not counted).  verbose: every accepted move on stdout. */
int pamlh_nni_scores(pamlh *p, const double *x, int *n_swaps, int *swaps, double *lnL0, double *lnL);
int pamlh_apply_nni(pamlh *p, int v, int s, int x);
int pamlh_nni_search(pamlh *p, double *x, double *lnL, int max_moves, int verbose, int *stats);

/* Branch supports by the approximate likelihood-ratio test in its SH-like form (pamlh_support.c; aLRT: Anisimova & Gascuel 2006, the
 * non-parametric SH-like support: Guindon et al. 2010).  An edge is the branch above an internal node v with two sons whose father is a
 * non-root node with two sons or a root with three (paml_amd_edge_list); its three configurations are the present one and its two NNI
 * alternatives; the five branches around it are s1, s2, v, then c and f, or c1 and c2 (include/paml_amd.h).
 * pamlh_edge_list: edges[*n_edges][3][3] and five[*n_edges][5] of the tree as it stands; both NULL: the count only.
 * pamlh_edge_optimize: all 3 n_edges rows are maximised over their five lengths in lock step at the parameters of x, everything else
 *   held fixed, the present configuration treated like the other two; ONE paml_amd_edge_scores call per step gives every row's lnL, d1
 *   and d2 at its own lengths.  A cyclic, safeguarded Newton iteration: per sweep the five roles in turn; per role one call for the
 *   derivatives at the accepted lengths and at most 4 calls at trial lengths; a row takes -d1 / d2 where d2 < 0, otherwise doubles
 *   (d1 > 0) or halves (d1 < 0) the length; a step is clipped to [4e-6, 50], the bounds pamlh_optimize uses, and halved while the next
 *   call shows the row's lnL fell; no damping.  It ends after a sweep in which no row gained more than 1e-6 or after 30 sweeps; a row
 *   that gained no more than 1e-6 in a sweep is finished and stays in the calls with u = -1.  t5_out[n_edges][3][5] (in the order of
 *   five), l_out[n_edges][3]; stats (NULL or 3 entries): sweeps, engine calls, rows with a length at a bound.
 * pamlh_edge_lnf: lnL[n_edges][3] and lnf[n_edges][3][npatt] of every configuration at the lengths t5 and the parameters of x: one call.
 * pamlh_branch_supports: the list, the optimisation, one last call with the per-pattern values of all rows; delta = 2 (l0 - max(l1,
 *   l2)); the replicate sums from paml_amd_rell_replicates over the 3 n_edges rows (genes respected); the table arithmetic of
 *   pamlh_branch_supports_from_replicates.  edge_node[*n_edges] = v, l3[*n_edges][3]; all four NULL: the count only.
 * pamlh_branch_supports_from_replicates (host only): rep[n_rep][3 n_edges]; per row its mean over the replicates is subtracted (the
 *   centring of the S-H column of the tree comparison); per edge and replicate delta*_r = 2 (largest - second largest of the three
 *   centred sums); support = #{r : delta*_r < delta} / n_rep, and 0 where delta <= 0 (a better NNI neighbour exists).
 * pamlh_newick_supports: pamlh_newick with the supports as the labels of the internal nodes (buf needs 80 bytes per node + 128).
 * Refused by name: a clock, rho models, runmode = -2, fix_blength = 2 or 3 (the branch lengths are not parameters), a tree whose root
 * has two sons.  Not done here: parameters other than the five lengths, chi-square-based aLRT P values, edges next to polytomies. */
int pamlh_edge_list(pamlh *p, int *n_edges, int *edges, int *five);
int pamlh_edge_optimize(pamlh *p, const double *x, int n_edges, const int *edges, const int *five, double *t5_out, double *l_out, int *stats);
int pamlh_edge_lnf(pamlh *p, const double *x, int n_edges, const int *edges, const int *five, const double *t5, double *lnL, double *lnf);
int pamlh_branch_supports(pamlh *p, const double *x, int n_rep, unsigned long long seed, int *n_edges, int *edge_node, double *delta, double *support, double *l3);
int pamlh_branch_supports_from_replicates(int n_edges, int n_rep, const double *rep, const double *l3, double *delta, double *support);
int pamlh_newick_supports(const pamlh *p, int n_edges, const int *edge_node, const double *support, char *buf, int cap);

/* Subtree prune and regraft (SPR) on the analysis's tree (pamlh_spr.c).  A move is (s, x), 0-based nodes, with a split phi in [0, 1]
 * (the definition: paml_amd_spr_scores, include/paml_amd.h): the subtree below s leaves with its father f; c, the other son of f, takes
 * f's place on a branch of length t_c + t_f; f takes x's place with the sons (x, s), the branch above f has length (1 - phi) t_x and x's
 * label, the branch above x phi t_x.  Valid: s and its father are not the root, the father has exactly two sons, x is not the root, not
 * f, not c and not below s; pruning the side of a branch that holds the root is out of scope.  All three are refused by name with a
 * clock, with rho models and for runmode = -2, as the NNI calls.
 * pamlh_spr_scores: the canonical list of the tree as it stands within `radius` branches of the pruned place (paml_amd_spr_list; <= 0:
 *   no limit) scored at x in ONE engine call (paml_amd_spr_scores): moves[*n_moves][2], lnL[*n_moves], *lnL0 = the present tree's.  With
 *   moves = lnL = NULL only *n_moves is written (host only): the room for the list is the caller's.
 * pamlh_apply_spr: edits son lists, fathers and label[f] in place and rewrites in xvec the three branch lengths of the definition (at c,
 *   f and x); marks the scaling nodes as for a tree just read and sends the tree to the engine again.  Node ids and pamlh_branch_order
 *   stay, so the layout of x does not change.  Afterwards the move (s, c) brings the topology back (and with phi = t_c / (t_c + t_f) the
 *   three lengths).  Refused where the branch lengths are not parameters (fix_blength).
 * pamlh_spr_search: pamlh_optimize on the present tree; then per step one pamlh_spr_scores (radius, phi = 0.5) at the estimates, the
 *   candidates in descending order of their screened lnL, at most one per distinct unrooted topology and at most `top` of them (<= 0:
 *   all), each applied and maximised: the first whose maximised lnL is higher by more than 1e-4 is kept, every other is undone from a
 *   saved copy of the tree and of x.  It ends after a step in which none of the tried candidates was better, or after max_moves moves
 *   (<= 0: no limit).  x: start in, estimates on the final tree out.  stats (NULL or 3 entries): moves, screening calls, neighbours
 *   maximised.  verbose: every accepted move on stdout.  On an error inside a step the candidate is undone too: the analysis is left on
 *   the last tree the search kept, x holds its estimates, and *lnL and stats are written.  The search keeps no state outside the call. */
int pamlh_spr_scores(pamlh *p, const double *x, int radius, double phi, int *n_moves, int *moves, double *lnL0, double *lnL);
int pamlh_apply_spr(pamlh *p, int s, int x, double phi, double *xvec);
int pamlh_spr_search(pamlh *p, double *x, double *lnL, int radius, int top, int max_moves, int verbose, int *stats);

/* Query sequences placed on every branch of the analysis's tree (pamlh_place.c): the likelihood of the tree with one more tip hung on
 * branch e, for every query, every branch and every pendant length of a grid, from ONE engine call (paml_amd_placement_scores) — the
 * primitive under the reference's stepwise addition (StepwiseAddition treesub.c:4866 on AddSpecies treesub.c:4592, which sets and
 * evaluates one enlarged tree after the other), under the regraft half of an SPR move and under placing new sequences on a fitted tree.
 * pamlh_load_placement: pamlh_load_with, except that the tree may name only some of the sequence file's sequences, at least 3, by name
 *   or by 1-based number in file order.  The sequences absent from the tree are the QUERIES; the tree's sequences become the tips
 *   0 .. m - 1 in file order.  Site patterns are compressed over all sequences together, so patterns that differ only in a query stay
 *   apart, with their own weights.  Everything counted from the data (observed frequencies, F3x4, ...) is counted on the tree's sequences
 *   only: an x estimated without the queries means the same thing here.  With cleandata = 1 a site is dropped if ANY sequence has an
 *   ambiguity character there, the queries included.  pamlh_load / pamlh_load_with themselves are as they were.
 * pamlh_n_queries, pamlh_query_name, pamlh_query_codes ([n_queries][npatt] character codes, the tips' table).
 * pamlh_placement_scores: lnL[n_queries][nbranch][n_pend] of query q hung on the b-th branch of x's branch-length block
 *   (pamlh_branch_order), the new node at phi of the branch's length above its lower end, with pendant length pendant[j] (branch label 0),
 *   at the branch lengths and parameters of x; *lnL0 the tree's own lnL.
 * pamlh_place: per query the best (branch, pendant length) of the grid — best_edge[n_queries] (index into pamlh_branch_order),
 *   best_pendant, best_lnL — and lwr[n_queries][nbranch], the likelihood weight ratios exp(l_e - logsumexp_e' l_e') with l_e the largest
 *   lnL of branch e over the grid.  Any output may be NULL.
 * pamlh_placement_newick: the tree with query q hung on branch `edge`, with the lengths of the last x (written so that they read back
 *   to the same doubles); cap >= 160 (n_nodes + 2) + 256.
 * Refused by name: a clock (x holds node ages), rho models, runmode = -2, an analysis without queries, a pattern shard. */
int pamlh_load_placement(pamlh **out, const char *ctl_path, const char *program, int tree_index, const char *overrides, char *err, int errcap);
int pamlh_n_queries(const pamlh *p);
const char *pamlh_query_name(const pamlh *p, int i);
const unsigned char *pamlh_query_codes(const pamlh *p);
int pamlh_placement_scores(pamlh *p, const double *x, int n_pend, const double *pendant, double phi, double *lnL0, double *lnL);
int pamlh_place(pamlh *p, const double *x, int n_pend, const double *pendant, double phi, int *best_edge, double *best_pendant, double *best_lnL, double *lwr);
int pamlh_placement_newick(pamlh *p, int q, int edge, double phi, double pendant, char *buf, int cap);

/* Maximum-likelihood placement (pamlh_place.c): the grid above scores one split for all branches and a list of pendant lengths; here
 * the three branches that meet at the new node — the part above it (t_up), the part above the branch's lower node (t_dn), the query's
 * (t_pend) — are free, and a (query, branch) row is maximised over them, as EPA and pplacer do and as the reference's AddSpecies ends
 * once the enlarged tree is optimised.  Everything else (the other branch lengths, the model) is held at x.
 * pamlh_attach_scores: one engine call (paml_amd_attach_scores) at x's branch-length block: lnL[i], d1[i], d2[i] of query q[i] hung on
 *   the edge[i]-th branch of pamlh_branch_order at the lengths t3[i] = (t_up, t_dn, t_pend), the derivatives along the branch role[i]
 *   names (-1: none, both 0; 0: up; 1: dn; 2: pendant); *lnL0 the tree's own lnL.
 * pamlh_place_optimize: all rows are maximised over their three lengths in lock step, started at t3 (in: the start, clipped to the box
 *   of pamlh_bounds for a branch length, 4e-6 .. 50; out: the maximum) — the cyclic, safeguarded Newton iteration of pamlh_edge_optimize
 *   with the roles up, dn, pendant: per role one call at the accepted lengths and at most 4 at trial lengths (Newton's step where
 *   d2 < 0, otherwise the length doubled or halved along the gradient; a trial whose lnL fell is halved from the accepted length), ONE
 *   engine call per step for every unfinished row; a row is finished after a sweep that gained it no more than 1e-6; at most 30 sweeps.
 *   No row's lnL ever falls.  lnL[n_rows]: the maxima; stats[3] (or NULL) = sweeps, engine calls, rows that ended with a length at a bound.
 * pamlh_place_ml: pamlh_placement_scores on the grid first; per query the `keep` best branches of the grid (keep <= 0: all; best
 *   first), each started at ((1 - phi) t_v, phi t_v, its best grid pendant) and maximised by pamlh_place_optimize; lwr[i] = the
 *   likelihood weight ratio over the query's kept, maximised rows.  Outputs (room for n_queries x nbranch rows each, 3 per row in t3):
 *   rows_q, rows_edge (index into pamlh_branch_order), t3, lnL, lwr; *n_rows = n_queries x the branches kept, the queries in order.
 * pamlh_placement_newick3: pamlh_placement_newick with the three lengths written in (its phi form cannot express parts that do not
 *   add up to t_v).
 * Refused by name: what the grid calls refuse, fix_blength = 2 or 3 (the branch lengths are not parameters), and rate-matrix (UNREST)
 *   models (the engine's message: the derivative of their P(t) needs a matrix product of its own). */
int pamlh_attach_scores(pamlh *p, const double *x, int n_rows, const int *q, const int *edge, const int *role, const double *t3, double *lnL0, double *lnL, double *d1,
                        double *d2);
int pamlh_place_optimize(pamlh *p, const double *x, int n_rows, const int *q, const int *edge, double *t3, double *lnL, int *stats);
int pamlh_place_ml(pamlh *p, const double *x, int keep, int n_pend, const double *pendant, double phi, int *rows_q, int *rows_edge, double *t3, double *lnL,
                   double *lwr, int *n_rows);
int pamlh_placement_newick3(pamlh *p, int q, int edge, double t_up, double t_dn, double t_pend, char *buf, int cap);

/* method = 1 of the control file: minB / minbranches (treesub.c:7826, 8039) — the branch lengths are optimised one at a time
 * by Newton steps on the branch-local lnL, dlnL/dt, d2lnL/dt2 (paml_amd_eval_branch; the engine keeps the partials of both
 * sides of every edge resident, so a step along the tree costs the nodes on the path, not the tree), alternating with BFGS
 * on the other parameters.  pamlh_minbranches: one such pass over the branch lengths in x (tolerance e), the rest of x held.
 * pamlh_optimize_minb: the alternation until |delta lnL| < e0.  n_eval: full evaluations spent on the other parameters. */
int pamlh_method(const pamlh *p);      /* the control file's `method` */
int pamlh_minbranches(pamlh *p, double *x, double e, double *lnL, int verbose);
int pamlh_optimize_minb(pamlh *p, double *x, double *lnL, double e0, int verbose, int *n_eval);

/* ---- Newton steps on every branch length at once (pamlh_newton.c), from the engine call that returns lnL, the gradient and the curvature
 * along every branch (paml_amd_curvature): a sweep is ONE engine call, where a pamlh_minbranches sweep is at least 2 (n - 1).
 * pamlh_curvature: lnL at x and, over x's branch-length block (pamlh_branch_order, ntime entries), g = d lnL / d t and h = d2 lnL / d t2
 *   — the diagonal of the Hessian of the tree as it is rooted; one engine call.
 * pamlh_newton_branches: maximises over the branch block with the rest of x held.  Per sweep and branch the step -g / h where h < 0,
 *   otherwise a step of the gradient's sign of the size of the current length (0.01 for a shorter one), capped by a trust factor per
 *   branch and clipped to the box of pamlh_bounds; the next sweep's call is also the test of the step: if lnL fell the previous lengths
 *   are restored and every trust factor is halved (quartered where the gradient changed sign), if not they grow back.  Ends when an
 *   accepted sweep gained less than e with max |step| < sqrt(e), or after max_sweeps sweeps.  lnL never decreases from entry to exit; x
 *   returns the best lengths seen, *lnL their lnL, stats[3] (may be NULL) the sweeps, the engine calls and the rejected sweeps.
 *   verbose: a line per sweep on stderr.
 * pamlh_optimize_newton: the alternation of pamlh_optimize_minb with pamlh_newton_branches in the place of pamlh_minbranches; BFGS on
 *   the other parameters unchanged.  n_eval: the evaluations of the parameter steps plus one per engine call of the branch steps.
 * Refused by name, as pamlh_gradient declines them: a clock (x holds ages), fix_blength = 2 / 3, rho != 0, a rate-matrix (UNREST) model,
 * a pattern shard. */
int pamlh_curvature(pamlh *p, const double *x, double *lnL, double *g, double *h);
int pamlh_newton_branches(pamlh *p, double *x, double e, int max_sweeps, double *lnL, int verbose, int *stats);
int pamlh_optimize_newton(pamlh *p, double *x, double *lnL, double e0, int verbose, int *n_eval);

/* ---- The exact Hessian of lnL over the branch lengths on the host (pamlh_hessian.c), from the engine call that returns lnL, the gradient
 * and every second derivative d2 lnL / d t_i d t_j (paml_amd_hessian).  Everything here is opt-in; pamlh_branch_hessian, pamlh_write_bv,
 * pamlh_standard_errors, pamlh_newton_branches and the optimisers are as they were.
 * pamlh_branch_hessian_exact: lnL at x, g[ntime] and H[ntime][ntime] over x's branch-length block (pamlh_branch_order); one engine call.
 *   Where pamlh_branch_hessian returns minus the outer product of the scores (an estimate of the information), this is the Hessian itself.
 * pamlh_write_bv_exact: the block pamlh_write_bv writes for mcmctree's in.BV, with this Hessian.
 * pamlh_standard_errors_exact: the observed information over all free parameters — branch x branch from the call, branch x model
 *   parameter from central differences of the branch gradient (two gradient calls per model parameter), model x model from
 *   pamlh_standard_errors method 1's stencil restricted to the model parameters — inverted as a whole; the parameters method 1 leaves
 *   out at a bound are left out and get se = -1.  hess (may be NULL): the information matrix, np x np.
 * pamlh_newton_full: pamlh_newton_branches with the step from the whole block, (-H + lambda I) d = g by Cholesky on the branches that
 *   can move, lambda raised from 0 until the factorisation succeeds; the same trust factors, clipping, accept / reject rule, ending and
 *   stats.  One engine call per sweep; lnL never decreases.
 * Refused by name, as pamlh_curvature refuses them: a clock, fix_blength = 2 / 3, rho != 0, a rate-matrix (UNREST) model, a pattern shard. */
int pamlh_branch_hessian_exact(pamlh *p, const double *x, double *lnL, double *g, double *H);
int pamlh_write_bv_exact(pamlh *p, const double *x, const char *path);
int pamlh_standard_errors_exact(pamlh *p, const double *x, double *se, double *hess);
int pamlh_newton_full(pamlh *p, double *x, double e, int max_sweeps, double *lnL, int verbose, int *stats);

/* ---- Posterior expected numbers of labelled substitutions per branch and per site (pamlh_counts.c), from the engine call that returns
 * them for every branch and pattern at once (paml_amd_subst_counts): multiple hits and the uncertainty of the ancestral states are
 * integrated over, where the "changes along branches" of a reconstruction counts the differences between two reconstructed sequences.
 * A label is an n x n matrix of weights: off the diagonal of the jumps a -> b, on it of the time spent in a (in units of the branch length).
 * pamlh_count_labels: the labels that go with the analysis's data type.  kind NULL or "standard": codons "synonymous", "nonsynonymous"
 *   by the analysis's genetic code; nucleotides "transitions", "transversions"; amino acids "changes".  kind "total": every jump;
 *   kind "dwell": the identity, whose count is the branch length.  *n_lab: how many; M (may be NULL): room for [*n_lab][n][n], two
 *   at most; names (may be NULL): room for *n_lab names of 32 characters.
 * pamlh_subst_counts: counts[n_lab][ntime] at x over x's branch-length block (pamlh_branch_order), summed over the alignment's sites;
 *   site_counts (may be NULL): [n_lab][ntime][sites] per site of the alignment (pamlh_pose: the patterns' values expanded).  One engine
 *   call; the state is left at x.
 * Refused by name, as pamlh_curvature refuses them: a clock, fix_blength = 2 / 3, rho != 0, a rate-matrix (UNREST) model, a pattern shard. */
int pamlh_count_labels(pamlh *p, const char *kind, int *n_lab, double *M, char (*names)[32]);
int pamlh_subst_counts(pamlh *p, const double *x, int n_lab, const double *M, double *counts, double *site_counts);

/* ---- Every branch as the foreground of branch-site model A in turn (pamlh_scan.c; codeml model = 2, NSsites = 2, fix_omega = 0), from
 * ONE engine call (paml_amd_relabel_scores) instead of a tree file, a model set-up and a search per branch.  Model A gives a branch type
 * the time scale Qfactor_bg = 1 / mr(kappa, r w0 + 1 - r) or Qfactor_fg = 1 / mr(kappa, p0 w0 + p1 + (1 - p0 - p1) w2), r = p0 / (p0 + p1):
 * with the EFFECTIVE lengths tau_v = t_v Qfactor held fixed the four class likelihoods do not depend on the proportions, so re-mixing
 * them on the host is an exact point of model A (pamlh_foreground_point gives its parameter vector); the lengths, kappa and w0 are not
 * maximised again.
 * pamlh_mixture_max (host only, no engine): maximises sum_h w_h log(s r f0 + s (1 - r) f1 + (1 - s) r f2a + (1 - s)(1 - r) f2b) over
 *   (s, r) in [1e-6, 1 - 1e-6]^2 from (s0, r0): EM steps, then a safeguarded projected Newton iteration; lnL never decreases.  lnf4[4][n_patt]
 *   are logs (-inf allowed), rescaled per pattern.  *p0 = s r, *p1 = s (1 - r).
 * pamlh_foreground_scan: omega2[n_grid] ascending with omega2[0] = 1; lnL, p0, p1 are [*n_br][n_grid], delta and best [*n_br], node
 *   [*n_br] = every non-root node in node order.  From x it takes kappa, w0, the branch lengths and (p0, p1); the tree's own '#' labels
 *   and x's w2 are not used; tau_v = t_v Qfactor_bg(r_x) for EVERY branch.  delta = 2 (max_{g >= 1} lnL - lnL at g = 0), best that g;
 *   *lnL_base the mixture without a foreground class (s -> 1).  With node = lnL = NULL only *n_br is written.  The tree's labels and the
 *   engine's model are left as they were.
 * pamlh_foreground_point: the model-A parameter vector, in x's layout, of a row for the tree with `node` as the only foreground branch:
 *   t'_u = tau_u / Qfactor_bg(r') (u != node), t'_node = tau_node / Qfactor_fg(p0, p1, omega2), kappa and w0 from x, then p0, p1, omega2.
 *   Not clamped into pamlh_bounds.
 * pamlh_set_foreground: label 1 on the branch above `node` and 0 elsewhere, in place (as pamlh_apply_nni changes the tree in place);
 *   pamlh_newick then prints #1 there.
 * Refused by name: models other than branch-site A, fix_omega = 1, a clock, rho, several genes, a pattern shard. */
int pamlh_mixture_max(int n_patt, const double *w, const double *lnf4 /* [4][n_patt] logs */, double s0, double r0, double *p0, double *p1, double *lnL);
int pamlh_foreground_scan(pamlh *p, const double *x, int n_grid, const double *omega2, int *n_br, int *node, double *lnL_base, double *lnL, double *p0,
                          double *p1, double *delta, int *best);
int pamlh_foreground_point(pamlh *p, const double *x, int node, double omega2, double p0, double p1, double *xA);
int pamlh_set_foreground(pamlh *p, int node);

/* Standard errors of the estimates (getSE = 1).  method 0: HessianSKT2004 (treesub.c:7241), the outer product of per-pattern
 * scores that the reference's programs print; method 1: observed information from central second differences of lnL
 * (Hessian() tools.c:5984).  Either way all perturbed evaluations are one batch.  se[np] (-1: not available, e.g. a parameter
 * on its bound under method 1); hess: NULL or np x np, the information matrix that was inverted. */
int pamlh_standard_errors(pamlh *p, const double *x, int method, double *se, double *hess);

/* Naive empirical Bayes posterior probabilities of the site classes (lfunNSsites_rate codeml.c:5241) at the model state of
 * the last pamlh_set_x, from the device's fhK: post[K][n_patt]; mean_w[n_patt] (may be NULL) = posterior mean omega.
 * pamlh_pose maps a site (after cleaning) to its pattern; pamlh_class_omega gives the omega of every class. */
int pamlh_neb(pamlh *p, double *post, double *mean_w);
/* Bayes empirical Bayes for M2a / M8 at the estimates x (lfunNSsites_M2M8 codeml.c:6387): posterior probability of the
 * w > 1 class, posterior mean and sd of omega, per pattern [n_patt].  f(x_h | w) for the grid's omegas is one evaluation on
 * the device; the 10^4-point grid sums run on the host. */
/* Reporting: the name of parameter i of x[] ("t 6..7", "kappa", "p0", "w2 (foreground)", ...), and the tree in Newick form with
 * the branch lengths of the current model state (buf needs 64 bytes per node + 128). */
int pamlh_param_name(const pamlh *p, int i, char *buf, int cap);
int pamlh_newick(const pamlh *p, char *buf, int cap);

/* com.plfun's calling convention (codeml.c:125 / baseml.c:70): SetParameters(x) + one likelihood evaluation on the GPU,
 * returns -lnL (what ming2 minimises); +1e300 on error (see pamlh_error). */
double pamlh_plfun(pamlh *p, const double *x, int np);

/* mcmctree's exact-likelihood seam (usedata = 1; lnpD_locus mcmctree.c:1130-1166 -> com.plfun(NULL, -1)): lnL of the locus for
 * node ages age[n_nodes] and either the locus rate rgene (clock = 1) or per-branch rates rate[n_nodes] (clock = 2 / 3), at the
 * substitution parameters of the last pamlh_set_x.  model_changed = 0: only the branch lengths are sent. */
int pamlh_lnpd_locus(pamlh *p, const double *age, double rgene, const double *rate, int model_changed, double *lnL);

/* Marginal ancestral reconstruction (RateAncestor = 1; AncestralMarginal treesub.c:6288) at the current model state:
 * post[n_patt][n_states] = Pr(state at internal node `node` (0-based, >= n_tips) | pattern). */
int pamlh_node_posterior(pamlh *p, int node, double *post);
/* Joint ancestral reconstruction (Pupko et al. 2000; the reference's "(2) Joint reconstruction" in rst): the most probable
 * assignment of states to all internal nodes per pattern — states[n_patt][n_nodes - n_tips] in node order — and its probability. */
int pamlh_joint_reconstruction(pamlh *p, int *states, double *prob);
/* Both reconstructions at every internal node in one engine call each (paml_amd_ancestral_marginal / paml_amd_ancestral_joint), at
 * the current model state; ni = n_nodes - n_tips internal nodes in node order.  Marginal: best[ni][n_patt] the most probable state,
 * prob[ni][n_patt] its posterior, post[ni][n_patt][n_states] or NULL.  Joint (one rate class; refused otherwise): states[ni][n_patt] and
 * ln_best[n_patt] = log Pr(data, assignment) — exp(ln_best - ln f_h) is pamlh_joint_reconstruction's prob. */
int pamlh_ancestral_marginal(pamlh *p, unsigned char *best, double *prob, double *post);
int pamlh_ancestral_joint(pamlh *p, unsigned char *states, double *ln_best);
int pamlh_beb(pamlh *p, const double *x, double *pr_pos, double *mean_w, double *se_w);
/* BEB under branch-site model A and clade models C / D with two branch types (lfunNSsites_ACD codeml.c:6827):
 * post[nc][n_patt] = posterior of the site classes; nc = 4 for A (classes 0, 1, 2a, 2b: Pr(positive selection on the foreground)
 * = post[2] + post[3]), 3 for C and D. */
int pamlh_beb_acd(pamlh *p, const double *x, double *post);
const int *pamlh_pose(const pamlh *p, int *n_sites);
const double *pamlh_class_omega(const pamlh *p);
int pamlh_positive_classes(const pamlh *p);             /* trailing classes that allow omega > 1 (2 for branch-site: 2a + 2b) */

/* ---- runmode = -2 (codeml, seqtype = 1): maximum-likelihood t, kappa, omega and dN, dS for every pair of sequences (PairwiseCodon
 * codeml.c:4344-4604, lfun2dSdN 4219-4264).  pamlh_load* accepts such a control file without a tree file and, like the reference
 * (codeml.c:1849-1852), deletes every site with a gap or an ambiguity; NSsites, alpha, aaDist, hkyREV, CodonFreq > 3, several genes,
 * runmode = -3 and seqtype 2 / 3 are refused by name.  The pairs are numbered in the reference's order: (2,1), (3,1), (3,2), (4,1) ...
 * pamlh_pairwise: the searches of all pairs in lock step on the GPU — every round's gradient and line-search points of all unfinished
 *   pairs are one paml_amd_pairset_eval call; bounds t [1e-5, 50], kappa [0.4, 999], omega [0.001, 99]; fix_kappa / fix_omega honoured;
 *   deterministic starting values (pamlh_pairwise.c states the rule).  out[n_pairs][9] = t, kappa, omega, lnL, S, N, dN, dS (as
 *   eigenQcodon(2, ...) at codeml.c:4522: the code behind pamlh_dnds), likelihood evaluations used.  counters (NULL or 4 entries): elements
 *   evaluated, decompositions done, evaluate calls, elements done again on the host after PAML_AMD_ENOCONV.
 * pamlh_pairwise_freqs (host only): the codon frequencies of a pair from its count table fp[n][n] (row = the larger state) and its number
 *   of sites, by GetCodonFreqs2 (codeml.c:4169-4216).
 * pamlh_pairwise_write (host only): 2ML.t, 2ML.dN, 2ML.dS and the pair table of rst, in the reference's layout, into `dir`. */
int pamlh_is_pairwise(const pamlh *p);
int pamlh_pairwise_n(const pamlh *p);      /* ns (ns - 1) / 2 */
int pamlh_pairwise(pamlh *p, double *out, long *counters, int verbose);
int pamlh_pairwise_freqs(const pamlh *p, const double *fp, double ls, double *pi);
int pamlh_pairwise_write(pamlh *p, const double *out, const char *dir);
const char *pamlh_seq_name(const pamlh *p, int i);

/* Simulation under the analysis's model on the GPU (the job of evolver: Simulate evolver.c:818, Evolve 753; paml_amd_simulate).
 * pamlh_simulate: SetParameters(x) (x = NULL: the model state as it stands), the model to the engine as pamlh_eval_gpu sends it, then
 *   n_sites sites (0: the alignment's own length) drawn with the branch vector an evaluation would get: z[n_tips][n_sites] states
 *   0 .. n_states - 1, cls[n_sites] the sites' classes (may be NULL).  (seed, replicate) name the data set: the same bytes every time.
 *   Refused with a message: several genes, rho (rates correlated along the sequence are not independent per site), runmode = -2.
 * pamlh_write_alignment (host only): z as a sequential PHYLIP file that this library and the reference read — names from
 *   pamlh_seq_name, nucleotides in T, C, A, G order, amino acids in the reference's order, codons as the triplets of the analysis's
 *   genetic code (state k = the k-th sense codon). */
int pamlh_simulate(pamlh *p, const double *x, long n_sites, unsigned long long seed, unsigned replicate, unsigned char *z, unsigned char *cls);
int pamlh_write_alignment(const pamlh *p, const unsigned char *z, long n_sites, const char *path);

/* Write the reference's `lnf` file layout (print_lnf_site treesub.c:7598) for the last pamlh_eval_gpu. */
int pamlh_write_lnf(const pamlh *p, const char *path, const double *lnf);

#ifdef __cplusplus
}
#endif
#endif
