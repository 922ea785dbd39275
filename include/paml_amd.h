/* paml_amd.h — C ABI of the MI355X-native likelihood engine (libpaml_amd.so).
 *
 * This is the drop-in boundary for PAML's likelihood hot path.  The reference has no plugin/FFI
 * layer; its de-facto seams are plain C symbols + globals:
 *     double (*com.plfun)(double x[], int np)           codeml.c:125  / baseml.c:70
 *     int ConditionalPNode(int inode, int igene, double x[])   codeml.c:3526 / baseml.c:1517
 *     int GetPMatBranch(double Pt[], double x[], double t, int inode)   treesub.c:7503 / 7534
 *     int PMatUVRoot(double P[], double t, int n, double U[], double V[], double Root[])  tools.c:516
 * Each entry point below names the reference interface (file:line under /root/reference/src) whose
 * role it takes over.  All pointers are host pointers unless the name starts with d_.  Every call
 * returns 0 on success or a negative PAML_AMD_E* code (the engine never exits the process, unlike
 * zerror() tools.c:1204); paml_amd_last_error() gives the message.
 *
 * Threading: one engine = one GPU + one HIP stream; calls on one engine must be serialised by the
 * caller, different engines (also on different devices and host threads) are independent.
 * Multi-GPU = one process and one engine per GPU over a contiguous pattern shard; after
 * paml_amd_comm_init every evaluation entry point returns the TOTAL over all ranks (the one
 * exchange step, an RCCL all-reduce over xGMI, runs inside the call on the engine's stream) — as the
 * reference's one com.plfun call returns the lnL of the whole alignment (codeml.c:748).
 */
#ifndef PAML_AMD_H
#define PAML_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct paml_amd_engine paml_amd_engine;

enum {
   PAML_AMD_OK = 0,
   PAML_AMD_EINVAL = -1,    /* bad argument / call order */
   PAML_AMD_ENOMEM = -2,    /* device or host allocation failed */
   PAML_AMD_EHIP = -3,      /* HIP runtime error (no device, launch failure ...) */
   PAML_AMD_EUNSUPPORTED = -4,
   PAML_AMD_ENOCONV = -5    /* a device eigen-decomposition (paml_amd_set_eigen_qrev_batch) hit its sweep limit: reported by the next
                               evaluation; decompose on the host and pass U, V, Root (paml_amd_set_eigen_uvroot) */
};

/* create flags */
enum {
   PAML_AMD_KEEP_PARTIALS = 1,  /* keep every internal node's partials resident: needed by
                                   paml_amd_get_partials / dirty-node re-evaluation
                                   (com.conPSiteClass = 1 memory model, codeml.c:2343-2346) */
   PAML_AMD_JIT = 2,            /* compile a pruning kernel specialised for the tree (hiprtc, a few seconds per
                                   new topology) even for small data sets; large ones do so by default
                                   (env PAML_AMD_JIT=0/1 overrides) */
   PAML_AMD_SHARD = 4           /* this engine will hold one rank's SHARD of a larger alignment (paml_amd_comm_init with
                                   n_patt_global > n_patt): kernels whose summation order differs are then never chosen by
                                   the shard's own size, so that lnL keeps the same bits for every number of ranks.  (Only
                                   20-state data sets of at most 4096 patterns are affected: without the flag they take the
                                   latency path of small data; paml_amd_comm_init refuses such an engine as a shard.) */
};

/* eigen-system kinds = the branches of GetPMatBranch (treesub.c:7503-7592) */
enum { PAML_AMD_EIGEN_UVROOT = 0, PAML_AMD_EIGEN_CIJK = 1, PAML_AMD_EIGEN_K80 = 2, PAML_AMD_EIGEN_JC69LIKE = 3, PAML_AMD_EIGEN_QMAT = 4 };

/* likelihood reduction = which com.plfun the reference would have installed (codeml.c:2338-2340) */
enum { PAML_AMD_MODE_LFUN = 0 /* treesub.c:7764 */, PAML_AMD_MODE_LFUNDG = 1 /* treesub.c:7608 + fx_r 7696 */ };

/* Once per data set, after the sequence file is read (replaces the conP/fhK/nodeScaleF allocations
 * of GetInitials codeml.c:2330-2354 and PointconPnodes treesub.c:3518).  n_states = com.ncode (<= 64),
 * n_tips = com.ns, n_patt = com.npatt, max_classes >= com.ncatG, n_genes = com.ngene.
 * The engine is created on the calling thread's current HIP device. */
int paml_amd_create(paml_amd_engine **out, int n_states, int n_tips, int n_patt, int max_classes, int n_genes,
                    unsigned flags);
void paml_amd_destroy(paml_amd_engine *e);
const char *paml_amd_last_error(const paml_amd_engine *e);      /* e = NULL: the calling thread's last failed stand-alone entry */

/* ---- Pattern shards over several GPUs (site patterns are independent given the tree, P(t), pi and the class
 * table; the reference has no counterpart — its lfun loops over all of com.npatt on one core, treesub.c:7764-7800).
 *
 * paml_amd_shard_bounds (host only, no GPU): the contiguous block [*first, *first + *count) of n_patt_global patterns that
 *   rank `rank` of `world` owns.  Blocks are cut at multiples of the reduction chunk (a function of n_patt_global alone,
 *   >= 256 patterns), so the partial sums of every rank are entries of ONE global array.  More ranks than chunks
 *   (paml_amd_max_ranks) would leave ranks without patterns: PAML_AMD_EUNSUPPORTED, for every rank alike, so that the ranks of
 *   a job fail together before any of them enters a collective call.
 * paml_amd_comm_unique_id: rank 0 obtains the 128-byte RCCL id (ncclGetUniqueId) and hands it to the other ranks by any
 *   means (a pipe, a file, MPI, torch.distributed's store).
 * paml_amd_comm_init: collective over the ranks (ncclCommInitRank).  The engine was created for its shard's n_patt and holds
 *   patterns [first_pattern, first_pattern + n_patt) of n_patt_global.  From then on eval / eval_device / eval_batch /
 *   eval_dirty / eval_branch return totals over all ranks, identical bits on every rank; the lnL of eval* is moreover
 *   independent of `world` (the ranks' zero-padded partial-sum arrays are added — exact — and summed in one fixed order).
 *   lnf / fhK / partials / posteriors stay per-shard.  world = 1 with a non-NULL id makes a one-rank communicator (the
 *   collective path on a single GPU); world = 1 with id = NULL only sets the global chunking.
 *   eval_adg (the rate chain runs over the sites in order): pose[] holds GLOBAL pattern indices, the same on every rank; the
 *   shards' class likelihoods are gathered over the ranks and every rank runs the chain — the same bits as a single engine.
 *   beb_grid / beb_grid_classes: a grid point's log-likelihood is a sum over all patterns, so the shards' sums are all-reduced
 *   before the grid weights are formed; every rank passes the same grid and gets the posteriors of ITS patterns and the
 *   global ln_fx.  node_posterior and the host's NEB work per pattern and need no exchange.
 *   The exchange step (all-reduce of the partial sums + their fixed-order total) runs on a stream of the engine's own, ordered
 *   by events: consecutive paml_amd_eval_device calls prune evaluation i + 1 while evaluation i is being reduced.  Every other
 *   entry point, and paml_amd_flush, joins the engine's stream to the totals still on their way.
 * The RCCL library (librccl.so.1, or the one PAML_AMD_RCCL_LIB names) is bound at run time on first use; PAML_AMD_EUNSUPPORTED
 * when it is not installed. */
/* GPUs visible to this process, and the one the calling thread's next paml_amd_create uses (hipSetDevice): a host written in C
 * — one process per GPU, as `pamlh_lnl --gpus N` forks them — needs no HIP headers. */
int paml_amd_device_count(void);
int paml_amd_set_device(int device);
#define PAML_AMD_COMM_ID_BYTES 128
int paml_amd_shard_bounds(long n_patt_global, int world, int rank, long *first, long *count);
int paml_amd_max_ranks(long n_patt_global);      /* the number of reduction chunks = the largest world shard_bounds accepts */
int paml_amd_comm_unique_id(void *id128);
int paml_amd_comm_init(paml_amd_engine *e, int rank, int world, const void *id128, long n_patt_global, long first_pattern);
int paml_amd_comm_destroy(paml_amd_engine *e);
int paml_amd_comm_info(const paml_amd_engine *e, int *rank, int *world, long *n_patt_global, long *first_pattern, int *chunk);
/* Which collective library the engine's exchange step is bound to (no reference counterpart): the path of the shared object that
 * holds ncclAllReduce (dladdr), loading it first if no communicator has been made yet — PyTorch ships a librccl of its own, and a
 * process that has imported torch shares THAT copy (dlopen matches by soname).  Returns the length written (truncated to cap - 1),
 * PAML_AMD_EUNSUPPORTED when no library could be bound. */
int paml_amd_comm_library(char *path, int cap);
/* Diagnostics of the exchange step (no reference counterpart; what `bench.py --gpus N` prints so that a scaling run explains
 * itself).  enable != 0 switches timed events on for the evaluations that follow (also: PAML_AMD_COMM_STATS=1), 0 off.  With
 * non-NULL outputs it reports, over the last *n (<= 64) evaluations whose exchange step ran on the engine's collective stream
 * — the caller has flushed and synchronised the stream —
 *   exchange_us:  partial sums ready -> total formed (the all-reduce over the ranks + the fixed-order total), mean and maximum;
 *   lane_wait_us: how long an evaluation's pruning stream stood in front of the previous exchange of its slot (0 when the
 *                 exchange had finished before the stream got there), mean and maximum. */
int paml_amd_comm_stats(paml_amd_engine *e, int enable, int *n, double *exchange_us_mean, double *exchange_us_max,
                        double *lane_wait_us_mean, double *lane_wait_us_max);

/* Launch all work on this hipStream_t (default: the null stream). */
int paml_amd_set_stream(paml_amd_engine *e, void *hip_stream);

/* com.z (treesub.c:1116 EncodeSeqs), nChara/CharaMap (tools.c:20, treesub.c:1218), com.fpatt, com.posG.
 * z is row-major [n_tips][n_patt] one byte per character code; with cleandata != 0 codes are states
 * 0..n-1 and the map may be NULL; otherwise n_chara[code] states listed in chara_map[code*n_states + k], each state at most once
 * in a code's list (PAML_AMD_EINVAL otherwise).  Any table of up to 256 codes is accepted: codes need not put the single states
 * first, may repeat a state set, or be empty (and then not occur in z).
 * gene_off has n_genes+1 non-decreasing entries from 0 to n_patt (NULL = one gene covering all patterns; a pattern shard of a
 * multi-GPU run may hold nothing of a gene: equal neighbours).  Uploaded once. */
int paml_amd_set_tips(paml_amd_engine *e, const unsigned char *z, int cleandata, int n_codes, const int *n_chara,
                      const unsigned char *chara_map, const double *weights, const int *gene_off);

/* nodes[].sons / nson / label (codeml.c:143-147) as CSR, tree.root, com.nodeScale (treesub.c:7177; NULL = none).
 * Tips are nodes 0..n_tips-1.  The root may be a tip ("young ancestor", codeml.c:3535) and nodes may
 * have any number of sons.  Replaces the recursion of ConditionalPNode by a flattened post-order
 * program; send again after ReRootTree (treespace.c:236). */
int paml_amd_set_tree(paml_amd_engine *e, int n_nodes, int root, const int *sons_ptr, const int *sons,
                      const int *label, const unsigned char *scale_node);

/* com.pi (n_pi = 1) or com.piG per gene (n_pi = n_genes), row-major [n_pi][n_states].  Callable at any time, also with another n_pi
 * than before: every later call reads the new vector.  The branch-local state of paml_amd_eval_branch (resident partials, eigen-basis
 * coefficients and operand fragments, which hold pi) starts over; the resident partials of PAML_AMD_KEEP_PARTIALS, P(t) and the per-tree
 * kernels do not depend on pi and stay. */
int paml_amd_set_pi(paml_amd_engine *e, int n_pi, const double *pi);

/* The same decomposition done ON THE DEVICE, for a batch of reversible rate matrices at once — what eigenQREV (tools.c:5023-5110,
 * called by eigenQcodon codeml.c:3229 for every omega class of every trial point) does on one CPU core, 0.3-0.9 ms per 61 x 61
 * matrix.  Q[n_sets][n*n] row-major (only the lower triangle is read, like eigenQREV), pi[n_sets][n], scale[n_sets] (NULL = 1):
 * set set_ids[i] becomes Root = w / scale (descending), U = diag(1/sqrt pi) R, V = R^T diag(sqrt pi) with
 * diag(sqrt pi) Q diag(1/sqrt pi) = R diag(w) R^T; states with pi = 0 are left out (Root 0, unit rows / columns).  One workgroup
 * per matrix (cyclic Jacobi in LDS, FP64, ~0.5 ms cold): a gradient's or a line search's several hundred decompositions take about the time
 * of one, and U, V, Root never cross PCIe.  Asynchronous on the engine's stream.  paml_amd_get_eigen reads a set back (parity);
 * paml_amd_eigen_counters: matrices decomposed so far and the Jacobi sweeps each matrix of the last batch took (-1: the limit of 40
 * sweeps was reached without convergence — decompose that matrix on the host instead).  The decomposition is asynchronous, so a set
 * that did not converge is reported by the next synchronous evaluation (paml_amd_eval, _eval_batch, _eval_dirty, _eval_branch), which
 * returns PAML_AMD_ENOCONV instead of a likelihood formed from unconverged eigenvectors; the C host (pamlh_*.c) and the reference-side
 * binding (integration/codeml_plfun.patch) then decompose on the host and evaluate again. */
int paml_amd_set_eigen_qrev_batch(paml_amd_engine *e, int n_sets, const int *set_ids, const double *Q, const double *pi, const double *scale);
/* The same with the matrices handed over as the elements they can have: nnz positions (row[k] >= col[k]: the lower triangle and the
 * diagonal — what eigenQREV reads, tools.c:5048-5060 — each position once), shared by the batch, and vals[n_sets][nnz]; every other
 * element is zero.  A codon matrix has 263 elements below its diagonal (single-nucleotide changes between sense codons, universal
 * code) + 61 on it of 3 721: 2.6 KB instead of 30 KB per matrix cross from pageable host memory, which is what a batch call's host time
 * is (tools/eigen_call_cost.py).  Same decomposition; the stopping threshold's norm is summed in another order, so the last bits may
 * differ from the dense call's. */
int paml_amd_set_eigen_qrev_batch_sparse(paml_amd_engine *e, int n_sets, const int *set_ids, int nnz, const int *row, const int *col,
                                         const double *vals, const double *pi, const double *scale);
/* Warm start for the above (on = 1; 0 = off, the default; -1 = leave as is; *n_warm, if not NULL, receives the number of
 * decompositions that started warm so far): a decomposition starts its Jacobi sweeps from the eigenvectors of the NEAREST matrix any set
 * of the engine was last decomposed for (told by a signature of eight weighted row sums; round 6 — until then: the set's own previous
 * matrix) — the set's predecessor along a line search, the base point's sets for the perturbed points of a gradient: 2 sweeps after a
 * finite-difference step, 4 after a 5 % step, instead of 8-9 (0.52 ms per call cold, 0.19 ms after a finite-difference step, 0.31 ms
 * after a 5 % step: tools/eigen_probe.py).  The answer is a decomposition of the NEW matrix to the same threshold either way; its last
 * bits then depend on the matrices the engine held before, which is why the default is off.  Every 16th decomposition of a chain, and
 * any whose pi has other zero entries than every candidate's, starts cold. */
int paml_amd_set_eigen_warm_start(paml_amd_engine *e, int on, long *n_warm);
int paml_amd_get_eigen(paml_amd_engine *e, int set_id, double *U, double *V, double *Root);
int paml_amd_eigen_counters(paml_amd_engine *e, long *n_decomposed, int *sweeps_last_batch, int cap);

/* Eigen systems, mirroring U,V,Root / _UU,_VV,_Root[NBTYPE+2] (codeml.c:185, treesub.c:9250) and
 * Cijk,Root,nR (baseml.c:123-124).  set_id is dense from 0.  Small H2D copies, typically per evaluation. */
int paml_amd_set_eigen_uvroot(paml_amd_engine *e, int set_id, const double *U, const double *V, const double *Root);
int paml_amd_set_eigen_cijk(paml_amd_engine *e, int set_id, int nR, const double *Cijk, const double *Root);
int paml_amd_set_eigen_k80(paml_amd_engine *e, int set_id, double kappa);        /* PMatK80 tools.c:578 */
int paml_amd_set_eigen_jc69like(paml_amd_engine *e, int set_id);                 /* PMatJC69like codeml.c:3585 */
/* No eigen system at all: the rate matrix Q[n*n] itself (baseml UNREST / UNRESTu, QUNREST treesub.c:2543), from which
 * GetPMatBranch builds P(t) = e^{Qt} with matexp(Qt, n, 7 Taylor terms, 5 squarings) (treesub.c:7524-7526, tools.c:4879).
 * n_states <= 8.  The branch-local evaluation (eval_branch) is not available for this kind. */
int paml_amd_set_eigen_qmat(paml_amd_engine *e, int set_id, const double *Q);

/* Site classes: com.ncatG, com.freqK, per-class _rateSite (treesub.c:7669/7678), and for each
 * (gene, class, branch label) the eigen set (Set_UVR_BranchSite codeml.c:2663, SetPSiteClass
 * treesub.c:7663) and for each (class, label) the Qfactor applied to t (treesub.c:7549, 7587).
 * eigen_of is [n_genes][K][n_labels], qfactor is [K][n_labels] (NULL = all 1).  mode selects the
 * lfun (K must be 1) or the fx_r + lfundG reduction, including their different f<=0 floors. */
int paml_amd_set_classes(paml_amd_engine *e, int mode, int K, const double *freqK, const double *rate, int n_labels,
                         const int *eigen_of, const double *qfactor);

/* Malpha = 1 (a gamma shape per gene: lfundG calls SetPGene for every gene, which runs DiscreteGamma with that gene's alpha,
 * treesub.c:7627-7629, codeml.c:2441 / baseml.c:1460): class rates per gene, rate[n_genes][K], replacing the rate[K] of the
 * last set_classes (which also switches back).  With it, the `rate` argument of paml_amd_eval_batch is [n_batch][n_genes][K]. */
int paml_amd_set_gene_class_rates(paml_amd_engine *e, const double *rate);

/* One com.plfun call (codeml.c:748): batched P(t) for every branch x class x gene, fused pruning,
 * root / class-mixture / weighted-log reduction.  branch[n_nodes] = nodes[].branch, gene_rate =
 * com.rgene (NULL = 1).  Returns +lnL (the reference returns -lnL).  lnf[n_patt] (log f_h as
 * print_lnf_site treesub.c:7598 prints it) and fhK[K*n_patt] (com.fhK, class-major) are optional. */
int paml_amd_eval(paml_amd_engine *e, const double *branch, const double *gene_rate, double *lnL, double *lnf,
                  double *fhK);

/* Same evaluation without the final device->host copy or synchronisation: lnL (the total over the ranks when the engine has a
 * communicator) is left in d_lnL (a device pointer, e.g. a torch tensor).  Consecutive calls are pipelined: the next
 * evaluations' P(t) are built on a side stream, the pruning kernels of consecutive evaluations (large problems on the
 * matrix-core kernels) alternate between the engine's stream and a second stream of the engine's own so that one takes the CUs
 * as the other releases them, and the fixed-order total — with a communicator the exchange step in front of it — runs on a
 * third.  The values of a run are written in call order, but the last of them may still be on the engine's own streams:
 * paml_amd_flush makes the engine's stream wait for them.  Call it once after a run of eval_device calls, before synchronising
 * the stream or reading d_lnL on it (a device-wide synchronisation covers the engine's streams too); every other entry point
 * of the engine does it implicitly.  Give every evaluation of a run its own d_lnL slot if all values are wanted. */
int paml_amd_eval_device(paml_amd_engine *e, const double *branch, const double *gene_rate, double *d_lnL);
int paml_amd_flush(paml_amd_engine *e);
/* The device eigen-decompositions queued so far (paml_amd_set_eigen_qrev_batch): waits for the engine's stream and returns
 * PAML_AMD_ENOCONV if one of them reached its sweep limit — what every synchronous entry point (eval, eval_batch, eval_dirty, eval_branch,
 * eval_adg, beb_grid*, node_posterior) reports by itself; for callers of eval_device, which never synchronises.  paml_amd_flush reports
 * a failure that has already been recorded, without waiting. */
int paml_amd_eigen_status(paml_amd_engine *e);

/* Re-evaluate after a change that leaves the partials of the nodes with clean[node] != 0 valid
 * (com.oldconP, codeml.c:112, treespace.c:250): those subtrees are read back instead of recomputed.
 * Needs PAML_AMD_KEEP_PARTIALS and one earlier full evaluation with the same classes. */
int paml_amd_eval_dirty(paml_amd_engine *e, const double *branch, const double *gene_rate, const unsigned char *clean,
                        double *lnL);

/* lfunAdG (treesub.c:7447-7494), the auto-discrete-gamma model (rho != 0): fx_r runs on the device exactly as for lfundG;
 * the K-state rate chain with transition matrix MK[K*K] (AutodGamma tools.c:2630, the caller's) is then run over the ls
 * sites in their original order, pose[site] = pattern index (com.pose) — a sequential recurrence, done on the host from the
 * device's fhK.  Needs PAML_AMD_MODE_LFUNDG classes.  Returns +lnL. */
int paml_amd_eval_adg(paml_amd_engine *e, const double *branch, const double *gene_rate, const double *MK, const int *pose, int ls,
                      double *lnL);

/* The grid integral of Bayes empirical Bayes (lfunNSsites_M2M8 codeml.c:6482-6580; also the M8 / M2a tables of
 * get_pclassM_iw_M2M8, 6340) over the class likelihoods fhK of the LAST evaluation (lfundG mode, K <= 32 classes = all the
 * omega values the grid needs).  Grid point g is a mixture of n_cls classes: proportion pcl[g][c], class iw[g][c] (index into
 * the K classes); w_class[K] = omega of each class.  For every pattern: pr_last = posterior probability of the last class of
 * the mixtures, mean_w, sd_w = posterior mean and sd of omega; ln_fx (may be NULL) = log of the marginal likelihood over the
 * grid (up to the per-pattern scaling constants).  n_grid x n_patt x n_cls terms with a log each — the reference's second
 * hot loop at scale. */
int paml_amd_beb_grid(paml_amd_engine *e, int n_grid, int n_cls, const double *pcl, const int *iw, const double *w_class,
                      double *ln_fx, double *pr_last, double *mean_w, double *sd_w);

/* The same grid integral returning the posterior of EVERY mixture class — what lfunNSsites_ACD (codeml.c:6827-7010) computes
 * for branch-site model A (4 classes per grid point drawn from 121 evaluated (background, foreground) omega pairs, table 1 of
 * Yang, Wong & Nielsen 2005) and the clade models.  Any K (the class likelihoods are read from memory), n_cls <= 8.
 * post[n_cls][n_patt]; ln_fx as above. */
int paml_amd_beb_grid_classes(paml_amd_engine *e, int n_grid, int n_cls, const double *pcl, const int *iw, double *ln_fx, double *post);

/* n_batch evaluations in one launch: the finite-difference loops of the optimiser (gradientB tools.c:6561, the forward /
 * central differences of ming2 tools.c:6595 and of the Hessian, HessianSKT2004 treesub.c:7241) call com.plfun np (or 2np,
 * np^2) times on the same data with one parameter nudged; here those calls become the elements of one batch.  Element b
 * uses branch[b][n_nodes] and gene_rate[b][n_genes] (NULL = all 1) and, where a non-NULL table is given, its own
 * eigen_of[b][n_genes][K][n_labels], qfactor[b][K][n_labels], freqK[b][K], rate[b][K] — layouts of one element as in
 * paml_amd_set_classes; NULL = the tables set there, shared by all elements.  Eigen systems are referenced by set id, so
 * a nudged kappa / omega is a further paml_amd_set_eigen_* id.  lnL[n_batch] comes back (+lnL each), and, when lnf is
 * not NULL, the per-pattern log f_h of every element, lnf[n_batch][n_patt] — what HessianSKT2004 (treesub.c:7241) collects
 * in dfsites for its 2 np perturbed evaluations.  pi and the mode (lfun / lfundG) are those of the engine.  Not with
 * PAML_AMD_KEEP_PARTIALS. */
int paml_amd_eval_batch(paml_amd_engine *e, int n_batch, const double *branch, const double *gene_rate, const int *eigen_of,
                        const double *qfactor, const double *freqK, const double *rate, double *lnL, double *lnf);

/* Branch-local evaluation = lfuntdd / lfuntdd_SiteClass (treesub.c:8204, 8403; lfunt / lfunt_SiteClass 8127, 8298 are
 * the lnL-only case), the function minbranches (treesub.c:8039) iterates with Newton steps: for the branch above
 * node_b, and for each of the n_t (<= 64) trial lengths t[], the log-likelihood and its first two derivatives in t,
 * all other branch lengths taken from branch[].  Outputs are in lnL convention: lnL = -l, dlnL = -dl, ddlnL = -ddl
 * of the reference.  Like the reference (ReRootTree treespace.c:236 marks the nodes on the path, com.oldconP[a] = 0 at
 * line 250; updateconP treesub.c:7982 recomputes only those), the engine keeps the partials of BOTH sides of every edge
 * it has visited resident in HBM between calls: moving to a neighbouring branch recomputes the one or two nodes on the
 * path, a changed branch length only the partials that look across it.  The contraction reads the two resident partials;
 * for 21..64 states with (U, V, Root) eigen systems and one gene it works in the eigen basis (f(t) = sum_k e^{mu_k t} z_k w_k,
 * w = V A, z = U^T (pi o B): two matrix-core products per pattern for any number of trial lengths and derivatives, the
 * coefficients z_k w_k kept for further calls on the same branch), otherwise it builds P, dP, ddP for all trial lengths in one
 * batched kernel as lfuntdd does.  One host synchronisation per call.  Scaling nodes keep rescaling; their factors are stored
 * with the partials.
 * Any set_tips / set_tree / set_eigen_* / set_classes call drops the resident partials. */
int paml_amd_eval_branch(paml_amd_engine *e, int node_b, int n_t, const double *t, const double *branch,
                         const double *gene_rate, double *lnL, double *dlnL, double *ddlnL);
/* Work done by paml_amd_eval_branch so far: calls, and internal-node partials recomputed (a full tree costs n_nodes - n_tips). */
int paml_amd_branch_counters(const paml_amd_engine *e, long *n_calls, long *n_nodes_recomputed);
/* eval_branch calls so far that were served from the stored eigen-basis coefficients of the branch (21..64 states: a further
 * trial length on the branch just evaluated needs no matrix product; kernels_branch.h). */
long paml_amd_branch_coef_hits(const paml_amd_engine *e);
/* eval_branch calls so far in which most of the tree was dirty (every branch length moved: minB's round after ming2, treesub.c:7982) and
 * the forest of dirty subtrees ran on a per-tree kernel of its own instead of the interpreter (compiled in the background from the second
 * request of the same forest on; at once with PAML_AMD_JIT). */
long paml_amd_branch_refill_kernels(const paml_amd_engine *e);
/* With paml_amd_profile(e, 1): milliseconds (HIP events on the engine's stream) between the first and the last contraction kernel of
 * the last eval_branch call — the coefficient-forming kernel and / or the polynomial kernel(s); < 0 when the call took the
 * P / dP / ddP form or profiling was off. */
double paml_amd_branch_kernel_ms(paml_amd_engine *e);
/* Parity accessor: the per-block partial sums of the last eval_branch, [rows][cols = 3 n_t] at their global block positions
 * (after the all-reduce when a communicator is attached) — summed in a fixed order they give lnL, dlnL, ddlnL with the same bits
 * for every number of ranks.  out = NULL: the shape only. */
int paml_amd_get_branch_partials(paml_amd_engine *e, double *out, long cap, long *rows, int *cols);

/* Marginal ancestral reconstruction (AncestralMarginal treesub.c:6288, PostProbNode 6142): post[n_patt][n_states] =
 * posterior probabilities of the states at internal node `node` given the data, at the current classes / eigen systems and
 * the given branch lengths.  The reference re-roots the tree at the node and reuses conP (ReRootTree + updateconP); the
 * engine walks the tree rooted at the node in one fused pass.  Reversible models only. */
int paml_amd_node_posterior(paml_amd_engine *e, int node, const double *branch, const double *gene_rate, double *post);

/* Parity / post-processing accessors.
 * get_pmat: the matrix GetPMatBranch (treesub.c:7534) would have produced for the branch above
 *   `node`, row-major P[from*n + to], from the last evaluation.
 * get_partials: nodes[node].conP for class iclass, layout [n_patt][n_states] (PointconPnodes
 *   treesub.c:3518); needs PAML_AMD_KEEP_PARTIALS.
 * get_scale: com.nodeScaleF row of a scaling node, [n_patt] (treesub.c:7207-7227). */
int paml_amd_get_pmat(paml_amd_engine *e, int gene, int iclass, int node, double *P);
int paml_amd_get_partials(paml_amd_engine *e, int node, int iclass, double *conP);
int paml_amd_get_scale(paml_amd_engine *e, int node, int iclass, double *scale);
/* The partial sums sum_h w_h log f_h of the last evaluation, one per reduction chunk of the GLOBAL pattern range (zero for
 * chunks other ranks own when there is no communicator; the all-reduced array when there is one): the quantities of lfun's
 * accumulation loop (treesub.c:7796-7800) before the final total.  Returns the number of chunks. */
int paml_amd_get_partial_sums(paml_amd_engine *e, double *out, int cap);

/* Per-kernel timing with HIP events on the engine's stream (bench.py roofline leg).
 * profile(1) starts recording an event pair around every kernel launch; profile_read sums the
 * elapsed milliseconds per kernel family since the last read and resets the accumulators. */
int paml_amd_profile(paml_amd_engine *e, int enable);
int paml_amd_profile_read(paml_amd_engine *e, double *ms_pmat, double *ms_prune, double *ms_reduce, long *n_evals);

/* Counters mirroring NFunCall / NPMatUVRoot (tools.c:88, printed codeml.c:770). */
int paml_amd_counters(const paml_amd_engine *e, long *n_eval, long *n_pmat);

/* Cherry tables of the last evaluation.  On large codon data sets (60..64 states, at most 64 character codes, one gene and one
 * frequency vector, no PAML_AMD_KEEP_PARTIALS, single evaluations, at most 95 tips — trees whose tip codes fit two LDS blocks of the
 * per-tree kernel —; from PAML_AMD_CHERRY_MIN_PATT = 32768 patterns of this engine on, where per-tree kernels are on)
 * the per-tree kernel replaces the product P(t) . (tipA o tipB) of a cherry — an internal node with two tip sons — by a lookup in a
 * table of all n_codes^2 such products, built once per evaluation right behind P(t).  Same bits as without.  *n_tabulated: cherries
 * looked up (in program order, as many as PAML_AMD_CHERRY_CAP_MB = 192 MB of tables hold over all classes); *bytes: the tables' size.
 * Both 0 when the evaluation ran without.  PAML_AMD_CHERRY_TABLES=0 / 1 switches the tables off / on whatever the number of patterns. */
int paml_amd_cherry_tables(const paml_amd_engine *e, long *n_tabulated, long *bytes);
/* Subtree tables of the last evaluation (tables of repeated patterns above the cherries): the nodes tabulated (at most `cap` of them
 * into nodes[] / u[], sons before fathers, with their numbers of classes), the tables' bytes, the operand blocks the per-tree kernel is
 * left with per tile (-1: it ran without subtree tables), and how often the engine has computed the classes (once per tips + tree). */
int paml_amd_subtree_tables(const paml_amd_engine *e, long *n_tabulated, int *nodes, long *u, int cap, long *bytes, long *blocks_left, long *n_computed);
/* The pattern order of the walk with subtree tables (the patterns sorted by their classes at the walk's lookups; PAML_AMD_SUBTREE_ORDER=0
 * switches it off): whether the last evaluation ran with it, how often the engine has computed it (once per tips + tree + selection,
 * never per evaluation) and the host time of the last computation. */
int paml_amd_subtree_order(const paml_amd_engine *e, int *in_use, long *n_computed, double *host_seconds);
/* The gathering walk (a table form that is lookups and the root only runs on a kernel that fetches every distinct table row of a tile
 * once into LDS; PAML_AMD_GATHER_WALK=0, read at every evaluation, keeps the generated walk): whether the last evaluation ran on it, the
 * tiles and distinct rows (per class of the model) of its layout, the most rows of a tile (R), how often the engine has laid the tiles
 * out (once per tips + tree + selection, never per evaluation) and the host time of the last layout. */
int paml_amd_gather_walk(const paml_amd_engine *e, int *in_use, long *n_tiles, long *n_rows, int *R, long *n_computed, double *host_seconds);

/* Host-only introspection (no GPU needed): the flattened post-order program the engine would run for
 * a tree — 4 ints per op (code, a, b, c; paml_amd/csrc/program.h).  Returns the number of ops (or a
 * negative error); at most cap ops are written.  Used by the CPU test-suite to check the traversal. */
int paml_amd_debug_program(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons,
                           const unsigned char *scale_node, int keep_partials, const unsigned char *clean,
                           int *ops_out, int cap, int *max_stack);

/* Host-only: the bookkeeping of paml_amd_eval_branch (paml_amd/csrc/branch_plan.h) played for n_calls calls on a tree given as for
 * paml_amd_debug_program (one class, no gene rates): call i works on the branch of node_b[i] with the lengths branch[i][n_nodes], and
 * every call forms what it finds dirty.  Per call: ends_out[i] = (A, B), up_out[i][n_nodes] the orientation towards the branch,
 * clean_out[i][n_nodes] the internal nodes whose stored partial served as it was.  For the last call also the program of the dirty
 * subtrees below A, then B (the P / dP / ddP form's), 4 ints per op, at most cap ops.  Returns their number, or a negative error. */
int paml_amd_debug_branch_plan(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, const unsigned char *scale_node,
                               int n_calls, const int *node_b, const double *branch, int *ends_out, int *up_out, unsigned char *clean_out,
                               int *ops_out, int cap);

/* Host-only: the order in which set_tips keeps the n_codes (> 64) character codes of a table at 21..64 states — order_out[new code] =
 * the caller's code — given the table and the nz codes of z (the per-tree kernel's rows beyond 64 codes).  Returns n_codes, or a
 * negative error. */
int paml_amd_debug_code_order(int n_states, int n_codes, const int *n_chara, const unsigned char *chara_map, const unsigned char *z,
                              long nz, int *order_out);

/* Host-only: generate (and with compile != 0 also hiprtc-compile for gfx950, no GPU needed) the kernel
 * specialised for a tree (paml_amd/csrc/jit.h).  compile: bit 0 = compile; bits 8..15 = n_states (4, 5 or 20 select the
 * one-pattern-per-lane kernel, 64 + n the MFMA kernel trimmed to n states, anything else the 61-state MFMA kernel); bit 1 = the
 * fused 4 / 5-state kernel for K = bits 16..23 classes, bits 24..31 character codes and a reduction chunk of 256 x bits 2..7 patterns.  Returns the source length, or a negative error
 * with the compiler log in text_out. */
int paml_amd_debug_jit(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons,
                       const unsigned char *scale_node, char *text_out, int cap, int compile);

/* Host-only: the cherry-table form of the 61-state kernel for a tree (61 character codes, one class), at most max_tabs cherries
 * tabulated in program order: its source in text_out, the operand stream it is left with in stream_out ((is_tip, node) pairs,
 * *n_stream of them) and the tabulated cherries in tabs_out ((tip a, tip b, node) triples).  Returns the number of cherries
 * tabulated (0, with empty outputs, where the table form does not apply), or a negative error. */
int paml_amd_debug_jit_tables(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, const unsigned char *scale_node,
                              int max_tabs, char *text_out, int cap, int *stream_out, int stream_cap, int *n_stream, int *tabs_out,
                              int tabs_cap);

/* Host-only: the classes of the subtree tables for a tree and tip codes z[n_tips][n_patt] (< n_codes): u_out[n_nodes] = the number of
 * distinct columns of the tips below every internal node below the root (0 elsewhere); cls_out (optional) [n_nodes][n_patt] = each
 * pattern's class there — dense ranks in order of first occurrence, at a cherry ca * n_codes + cb. */
int paml_amd_debug_subtree_classes(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, const unsigned char *z, long n_patt,
                                   int n_codes, unsigned int *u_out, unsigned int *cls_out);

/* Host-only: the pattern order of the walk with subtree tables for n_keys class arrays keys[n_keys][n_patt] (entries < bound[k]):
 * order_out[position] = pattern, the patterns sorted by their classes, the keys taken smallest bound first (largest_first: the reverse;
 * as_given: in the order given), ties by pattern number. */
int paml_amd_debug_subtree_order(int n_keys, const unsigned int *keys, const unsigned int *bound, long n_patt, int largest_first, int as_given,
                                 unsigned int *order_out);

/* Host-only: the tiles of the gathering walk (paml_amd/csrc/gather_tiles.h) for n_keys (1 .. 4) row arrays keys[n_keys][n_patt] (entries
 * < bound[k]) along order[position] = pattern (null: the identity), at most R (n_keys .. 160) distinct rows per tile, with the weight
 * flags wflag[n_patt] (null: all 1): the blocks the kernel reads, one per tile, into blocks_out (at most cap_bytes; null: none).  Returns
 * the bytes of one block, or a negative error; *n_tiles, *n_rows: tiles and distinct rows in all. */
int paml_amd_debug_gather_tiles(int n_keys, const unsigned int *keys, const unsigned int *bound, const unsigned int *order, const unsigned char *wflag,
                                long n_patt, int R, unsigned char *blocks_out, long cap_bytes, long *n_tiles, long *n_rows);

/* Host-only: the nodes an engine of these sizes (one gene, K classes, the PAML_AMD_SUBTREE_* / PAML_AMD_CHERRY_* switches of the
 * environment) tabulates above the cherries for tip codes z[n_tips][n_patt], sons before fathers.  Returns their number. */
int paml_amd_debug_subtree_select(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, const unsigned char *scale_node, int n_states,
                                  int n_codes, int K, const unsigned char *z, long n_patt, int *sel_out, int cap);

/* Host-only: the 60..64-state per-tree kernel with subtree tables of the nodes sel[n_sel] (sons before fathers) beside the cherry tables
 * of an engine with K classes: its source in text_out — compiled for gfx950 when `compile`, the code object kept in `dir` when given —
 * and the operand blocks left per tile.  Returns the length of the source, 0 where the table form does not apply or a node of sel
 * cannot be tabulated, or a negative error (PAML_AMD_EHIP: the compiler's log is in text_out). */
int paml_amd_debug_jit_subtree(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, const unsigned char *scale_node, int n_states,
                               int n_codes, int K, const int *sel, int n_sel, int compile, const char *dir, char *text_out, int cap, int *blocks_left);

/* Bytes of device memory the library's own buffers (the engines', the pair sets', the scratch of calls in progress) hold at this moment,
 * over the whole process: what a call allocated for itself is gone when it returns, and everything of an engine when it is destroyed.
 * (The tests' check on both; not a measure of the device's free memory.) */
long long paml_amd_debug_device_bytes(void);

/* Host-only (hiprtc cross-compiles without a GPU): compile the per-tree kernel an engine of these sizes would select for this tree
 * and keep the code object in `dir` (the library's read-only lib/jit directory, or a user cache), so that the first evaluation on
 * a fresh machine does not start with seconds of compilation.  n_patt_global fixes the reduction chunk the 4 / 5-state kernel is
 * specialised on; K = site classes. */
int paml_amd_jit_prebuild(int n_states, int n_tips, int n_codes, int K, long n_patt_global, int n_nodes, int root, const int *sons_ptr,
                          const int *sons, const unsigned char *scale_node, const char *dir, char *log_out, int log_cap);

/* Name of the pruning kernel the engine selected ("mfma64", "valu4", "valu20", ...). */
const char *paml_amd_kernel_name(const paml_amd_engine *e);

/* PatternWeight (treesub.c:1386-1516) on the device, stand-alone (no engine): collapse the n_sites alignment columns of
 * chars[n_seq][n_sites * width] (raw characters; width = 1, or 3 for codons) into distinct site patterns in the reference's
 * order — sorted by the characters of sequence 0, then sequence 1, ... (unsigned byte order = the strcmp order of the
 * reference's char + 1 strings), within genes when gene[n_sites] (com.pose on input) is given.  Out: *n_patt; first_site
 * [n_patt] = the first site showing each pattern (p2s[]), weights[n_patt] = com.fpatt, pose[n_sites] = pattern of every site
 * (com.pose on output).  first_site and weights need room for n_sites entries.  A radix sort of the site indices over the
 * key bytes, then run detection and a scan — HBM / latency-bound byte work.  PAML_AMD_EHIP when no device is visible. */
int paml_amd_compress_patterns(int n_seq, int n_sites, int width, const unsigned char *chars, const int *gene, int *n_patt,
                               int *first_site, double *weights, int *pose);

/* The bootstrap replicates of the tree comparison (the resampling loop of rell(), treesub.c:5844-6009: RELL and Shimodaira-Hasegawa
 * columns of the table) on the device, stand-alone (no engine).  lnf[n_trees][n_patt] = per-pattern log likelihoods of the trees,
 * w[n_patt] = pattern counts (non-negative integers below 2^31, at most 2^31 - 1 sites in all), gene_off = n_genes + 1 pattern
 * offsets (NULL: one gene; a gene without sites is skipped).  Out: rep[n_rep][n_trees],
 *     rep[r][t] = sum over the ls draws of replicate r of lnf[t][pattern(draw)],
 * sites drawn with replacement inside each gene.  The likelihoods are re-weighted, not re-estimated, so 10 000 replicates of 10^6
 * sites are 10^10 gathers of an n_trees-vector: the reference drops to 50 replicates at 10^5 sites, this entry does not.
 * The draws are counter-based (a SplitMix64 finaliser of (seed, replicate, gene, draw); written out in csrc/kernels_rell.h) and
 * the summation order is fixed (chunks of 4096 draws; no floating-point atomics): replicate r has the same bits for every n_rep,
 * batch and call.  n_rep is walked in batches of what the workspace holds (256 MiB of chunk sums; the environment variable
 * PAML_AMD_RELL_ARENA_MB gives another size in MiB): never PAML_AMD_ENOMEM for n_rep, only for the inputs themselves.
 * PAML_AMD_EINVAL (message: paml_amd_last_error(NULL), per thread) for n_trees, n_patt or n_rep < 1, a weight that is negative, not
 * an integer or >= 2^31, no sites at all, a gene_off that does not run non-decreasing from 0 to n_patt; PAML_AMD_EHIP when no device
 * is visible. */
int paml_amd_rell_replicates(int n_trees, int n_patt, const double *w, const double *lnf, int n_genes, const int *gene_off, int n_rep,
                             unsigned long long seed, double *rep);
/* Constants of the replicate kernels (draws per chunk, trees per pass), the number of batches the calling thread's last
 * paml_amd_rell_replicates walked and the time of its replicate kernels by HIP events (ms, summed over the batches); any pointer may
 * be NULL. */
void paml_amd_rell_info(int *chunk, int *tree_block, int *last_batches, double *last_kernel_ms);

/* Alignments drawn under the engine's model on the device: the role of Evolve / Simulate (evolver.c:737-805, 818).  Needs set_tree,
 * set_pi, set_classes and the eigen sets they refer to; needs no tips and leaves tips alone.  For each of n_sites sites a class is
 * drawn from freqK, a root state from pi, and along every branch, in pre-order, the state at its lower end from the row of P(t) of the
 * site's class — the matrices an evaluation at (branch[n_nodes], gene_rate[1] or NULL = 1) would build, by the same kernels; afterwards
 * paml_amd_get_pmat returns them (branch-local state of eval_branch starts over).  Out: z[n_tips][n_sites] states 0 .. n-1; cls[n_sites]
 * the sites' classes and anc[n_nodes - n_tips][n_sites] the states at the internal nodes (either may be NULL).  A root that is a tip
 * gets its drawn state as its sequence.
 * The draws are counter-based (a SplitMix64 finaliser of (seed, replicate, global site index first_site + j, draw); the whole definition,
 * inverse CDFs included, is written out in csrc/kernels_simulate.h): site first_site + j has the same bytes in whatever call, batch or
 * company it is drawn, so callers shard a long alignment by first_site — an engine with a communicator simulates locally.  n_sites is
 * walked in batches of what the workspace of state bytes holds (256 MiB; the environment variable PAML_AMD_SIM_ARENA_MB gives another
 * size in MiB): never PAML_AMD_ENOMEM for n_sites.  Synchronous.
 * PAML_AMD_EINVAL for n_sites < 1, first_site < 0, a null z or branch, a model that is not set yet; PAML_AMD_EUNSUPPORTED for an engine
 * of several genes (a stated limit: one gene) or class rates per gene; PAML_AMD_ENOCONV when a device eigen-decomposition queued in
 * front of it reached its sweep limit. */
int paml_amd_simulate(paml_amd_engine *e, const double *branch, const double *gene_rate, long n_sites, long first_site,
                      unsigned long long seed, unsigned replicate,
                      unsigned char *z /* [n_tips][n_sites] states 0..n-1 */,
                      unsigned char *cls /* [n_sites] or NULL */, unsigned char *anc /* [n_nodes - n_tips][n_sites] or NULL */);
/* The number of batches the calling thread's last paml_amd_simulate walked and the time of its kernels (P(t), the cumulative tables,
 * the walk) by HIP events (ms, summed over the batches); either pointer may be NULL. */
void paml_amd_simulate_info(int *last_batches, double *last_kernel_ms);

/* ---- Ancestral reconstruction at every internal node in one call (AncestralSeqs treesub.c:7071; the definitions and the kernels are
 * written out in csrc/kernels_ancestral.h).  Both calls are synchronous, build the P(t) an evaluation at (branch[n_nodes],
 * gene_rate[n_genes] or NULL = 1) would build, by the same kernels, start eval_branch's resident state over, and leave a following
 * paml_amd_eval its bits.  n_patt is walked gene by gene in batches of what a workspace holds (256 MiB; the environment variable
 * PAML_AMD_ANC_ARENA_MB gives another size in MiB): never PAML_AMD_ENOMEM because of n_patt or n_query, and a pattern's result has the
 * same bits whatever batch it falls in.  An engine with a communicator works on its shard's own patterns; nothing is exchanged.
 * PAML_AMD_EINVAL (with a message) for a null branch or output (post alone may be NULL), n_query < 1 with non-NULL nodes, a queried
 * node that is a tip, out of range or listed twice, a model or tips not set; PAML_AMD_ENOCONV as the other synchronous entries.
 *
 * AncestralMarginal / PostProbNode (treesub.c:6288, 6142) for many nodes at once: one down pass, one outer pass, then every queried
 * node's posterior — what paml_amd_node_posterior returns for the node, without a pass per node.  K classes, several genes, branch
 * labels, ambiguity codes, polytomies, scaling nodes, a root that is a tip.  Reversible models only: PAML_AMD_EUNSUPPORTED for a
 * rate-matrix (UNREST) set, as paml_amd_node_posterior.  best = the lowest state among the maxima of the node's posterior, best_prob
 * the bits of post[best].  Afterwards paml_amd_get_pmat refuses until the next evaluation, as after paml_amd_node_posterior. */
int paml_amd_ancestral_marginal(paml_amd_engine *e, const double *branch, const double *gene_rate,
                                int n_query, const int *nodes /* internal nodes; NULL = all, in node order */,
                                unsigned char *best   /* [n_query][n_patt] most probable state */,
                                double *best_prob     /* [n_query][n_patt] its posterior */,
                                double *post          /* [n_query][n_patt][n_states], or NULL */);

/* AncestralJointPPSG2000 (treesub.c:6964; Pupko et al. 2000), best assignment only, in logarithms (the reference's -log P,
 * treesub.c:7043-7046: a tree of a few hundred nodes underflows the product).  One class (PAML_AMD_EUNSUPPORTED for K != 1), any number
 * of genes.  Sums over sons run in the order of the tree's son lists and the lowest state wins among equal maxima.  Afterwards
 * paml_amd_get_pmat returns the matrices the call used. */
int paml_amd_ancestral_joint(paml_amd_engine *e, const double *branch, const double *gene_rate,
                             unsigned char *states /* [n_nodes - n_tips][n_patt], internal nodes in node order */,
                             double *ln_best       /* [n_patt] log joint probability of data and assignment */);

/* The number of batches the calling thread's last ancestral call walked and the time of its kernels by HIP events (ms, summed over the
 * batches); either pointer may be NULL. */
void paml_amd_ancestral_info(int *last_batches, double *last_kernel_ms);

/* ---- The derivative of lnL with respect to every branch length, and the per-pattern scores, in one call (what gradientB and
 * HessianSKT2004, treesub.c:7241, take 2 np evaluations for; the definition and the kernels are written out in csrc/kernels_gradient.h).
 * grad[v] is the derivative with respect to branch[v] of exactly the number paml_amd_eval returns at (branch[n_nodes],
 * gene_rate[n_genes] or NULL = 1), for any rooting and any mix of eigen systems on the branches — the tree is not re-rooted and no
 * reversibility is assumed, unlike paml_amd_eval_branch.  grad[root] = 0.  scores[v][h] = d log f_h / d branch[v] (the root's row and the
 * patterns of weight 0: 0), lnf[h] = log f_h, *lnL = sum_h w_h lnf[h] (equal to paml_amd_eval's to rounding, not to the bit).
 * One down pass, one outer pass that also forms the derivative at every branch; K classes, several genes, branch labels, ambiguity
 * codes, polytomies, scaling nodes, a root that is a tip; UVROOT, CIJK, K80 and JC69LIKE sets, at most 64 states.  Synchronous; builds
 * the P(t) an evaluation would build, by the same kernels, starts eval_branch's resident state over, leaves a following paml_amd_eval
 * its bits, and paml_amd_get_pmat returns the matrices the call used.  n_patt is walked gene by gene in batches of what a workspace
 * holds (256 MiB; the environment variable PAML_AMD_GRAD_ARENA_MB gives another size in MiB): never PAML_AMD_ENOMEM because of n_patt,
 * and every result has the same bits whatever the batches and on every call (fixed-order sums, no atomics).
 * PAML_AMD_EINVAL (with a message) for a null branch, lnL or grad, a model or tips not set; PAML_AMD_EUNSUPPORTED for a rate-matrix
 * (UNREST) set (its dP needs a matrix product of its own), tips that are not the nodes 0 .. n_tips - 1, more than 64 states, an engine
 * whose communicator has more than one rank; PAML_AMD_ENOCONV as the other synchronous entries. */
int paml_amd_gradient(paml_amd_engine *e, const double *branch, const double *gene_rate, double *lnL,
                      double *grad   /* [n_nodes] */,
                      double *lnf    /* [n_patt], or NULL */,
                      double *scores /* [n_nodes][n_patt], or NULL */);
/* The number of batches the calling thread's last paml_amd_gradient walked and the time of its kernels by HIP events (ms, summed over
 * the batches); either pointer may be NULL. */
void paml_amd_gradient_info(int *last_batches, double *last_kernel_ms);

/* ---- lnL, its derivative and its SECOND derivative along every branch length in one call: what a Newton step on all branches at once
 * needs (the definition and the kernels are written out in csrc/kernels_curvature.h).  curv[v] = d^2 lnL / d branch[v]^2 of exactly the
 * number paml_amd_eval returns, for any rooting and any mix of eigen systems — the diagonal of the Hessian over the branch lengths; the
 * cross derivatives are not formed.  curv[root] = 0, a pattern of weight 0 contributes nothing.  *lnL, grad[] and lnf[] have the bytes
 * paml_amd_gradient returns on the same engine and inputs: the same statements run, plus one product and one dot product per non-root
 * node.  Takes what paml_amd_gradient takes and leaves the engine as it does (paml_amd_get_pmat afterwards returns the matrices the
 * call used); the workspace is 256 MiB or PAML_AMD_CURV_ARENA_MB (read at every call), and every result has the same bytes whatever
 * the batches and on every call.  PAML_AMD_EINVAL for a null branch, lnL, grad or curv, a model or tips not set; PAML_AMD_EUNSUPPORTED
 * for a rate-matrix (UNREST) set, more than 64 states, an engine whose communicator has more than one rank. */
int paml_amd_curvature(paml_amd_engine *e, const double *branch, const double *gene_rate, double *lnL,
                       double *grad /* [n_nodes] */,
                       double *curv /* [n_nodes] */,
                       double *lnf  /* [n_patt], or NULL */);
/* The number of batches the calling thread's last paml_amd_curvature walked and the time of its kernels by HIP events (ms). */
void paml_amd_curvature_info(int *last_batches, double *last_kernel_ms);

/* ---- lnL, its gradient and its HESSIAN over all branch lengths in one call (the definition and the kernels are written out in
 * csrc/kernels_hessian.h, the lists of steps in csrc/hessian_plan.h).  hess[u][v] = d^2 lnL / d branch[u] d branch[v] of exactly the
 * number paml_amd_eval returns, for any rooting and any mix of eigen systems.  Per source branch u, D_u = dP_u L_u is carried up the path
 * to the root (L'_a, giving the pairs with u's ancestors as H_a . dP_a L'_a) and outwards through modified outer messages (H'_w, giving
 * the unrelated pairs as H'_w . dP_w L_w); with m_uvk these sums,  hess[u][v] = sum_h w_h (sum_k freqK_k m_uvk / f_h - s_u(h) s_v(h)).
 * Every unordered pair is computed once (the lower node of an ancestor pair, else the smaller node number, is the source) and mirrored,
 * so hess is exactly symmetric; the diagonal has the bytes of paml_amd_curvature's curv, *lnL, grad[] and lnf[] those of
 * paml_amd_gradient; the root's row and column are 0; a pattern of weight 0 contributes nothing.
 * nodes = NULL, n_list = 0: every node, hess is [n_nodes][n_nodes].  Otherwise hess is [n_list][n_list] in the order of the list, and
 * an entry has the same bytes whatever else is listed.  Takes what paml_amd_curvature takes and leaves the engine as it does; the
 * workspace is 256 MiB or PAML_AMD_HESS_ARENA_MB (read at every call), and every result has the same bytes whatever the batches and
 * the groups of sources, and on every call.  PAML_AMD_EINVAL for a null branch, lnL, grad or hess, a model or tips not set, an entry of
 * nodes that is out of range, the root or repeated; PAML_AMD_EUNSUPPORTED for a rate-matrix (UNREST) set, more than 64 states, an
 * engine whose communicator has more than one rank.  Every message starts with "hessian:". */
int paml_amd_hessian(paml_amd_engine *e, const double *branch, const double *gene_rate,
                     const int *nodes, int n_list,
                     double *lnL,
                     double *grad /* [n_nodes] */,
                     double *hess /* [n_nodes][n_nodes], or [n_list][n_list] */,
                     double *lnf  /* [n_patt], or NULL */);
/* The number of batches the calling thread's last paml_amd_hessian walked and the time of its kernels by HIP events (ms). */
void paml_amd_hessian_info(int *last_batches, double *last_kernel_ms);

/* ---- The derivative of lnL with respect to every INPUT of the engine in one call: what a chain rule on the host needs to give
 * d lnL / d (any model parameter) without an evaluation or a decomposition per parameter (the definition and the kernels are written out
 * in csrc/kernels_modelgrad.h).  lnL is the number paml_amd_gradient returns at (branch, gene_rate), a function of
 *   tau_gkv = branch[v] x gene rate x class rate x Qfactor (UVROOT sets; 1 otherwise), the effective length in P_v = exp(A tau);
 *   A of every eigen set: U diag(Root) V as paml_amd_set_eigen_uvroot or the qrev_batch calls left them (after their scale);
 *     sum_r Root_r Cijk[.][.][r] of a CIJK set; the closed forms of K80 and JC69LIKE (the matrices whose exponential those sets take);
 *   freqK, and the root frequency vectors (paml_amd_set_pi).
 * g_eff[g][k][v] = d lnL / d tau_gkv (the root's entries 0): sum_{g,k} g_eff[g][k][v] d tau_gkv / d branch[v] is paml_amd_gradient's
 * grad[v].  g_freqK[k] = sum_h w_h f_hk / f_h.  g_pi[i][x] = d lnL / d pi_i[x] of the root's vector as it enters the root sum only
 * (a root that is a tip: zero outside the tip's state set).  g_A[set][a][b] = d lnL / d A_ab with every element of A taken as
 * independent, summed over the (gene, class, branch) that use the set.  W[g][k][v][y][x] = d lnL / d P_v(y, x) of that (gene, class):
 * the weighted outer products the other outputs are pulled back from, for parity checks.  Any of the five may be NULL.
 * Takes what paml_amd_gradient takes and leaves the engine as it does; the workspace is 256 MiB or PAML_AMD_MODELGRAD_ARENA_MB.  Every
 * result has the same bits whatever the batches and on every call: W is summed over segments of paml_amd_model_gradient_segment()
 * patterns counted from each gene's first pattern, a segment cut by a batch border is carried on in the same accumulator, and finished
 * segments are added in segment order (no atomics).  PAML_AMD_EINVAL for a null branch or lnL, a model or tips not set;
 * PAML_AMD_EUNSUPPORTED for a rate-matrix (UNREST) set, more than 64 states, an engine whose communicator has more than one rank.
 * (The auto-discrete-gamma correlation rho is not an engine input: paml_amd_eval_adg has no counterpart here.) */
int paml_amd_model_gradient(paml_amd_engine *e, const double *branch, const double *gene_rate, double *lnL,
                            double *g_eff   /* [n_genes][K][n_nodes], or NULL */,
                            double *g_freqK /* [K], or NULL */,
                            double *g_pi    /* [n_pi][n], or NULL */,
                            double *g_A     /* [n_eigen][n][n], or NULL */,
                            double *W       /* [n_genes][K][n_nodes][n][n], or NULL */);
/* The number of batches the calling thread's last paml_amd_model_gradient walked and the time of its kernels by HIP events (ms). */
void paml_amd_model_gradient_info(int *last_batches, double *last_kernel_ms);
/* Patterns per summation segment of W; the sizes of g_pi and g_A: the engine's root frequency vectors and eigen sets. */
int paml_amd_model_gradient_segment(void);
int paml_amd_model_gradient_sizes(paml_amd_engine *e, int *n_pi, int *n_eigen);

/* ---- Posterior expected numbers of labelled substitutions and expected dwell times, per branch and per pattern, in one call (the
 * definition and the kernels are written out in csrc/kernels_counts.h).  A label l is an n x n matrix of real weights M_l: off the
 * diagonal M_l[a][b] weights every jump a -> b, on it M_l[a][a] rewards the time spent in a, in units of branch[v].  With A and tau of
 * the branch above v as in paml_amd_model_gradient, B_l = A o M_l off the diagonal and (B_l)_aa = M_l[a][a] branch[v] / tau,
 *   n_lv(h) = E[ labelled jumps + rewards on the branch above v | pattern h ]
 *           = sum_k rho_k H_v^T (int_0^tau e^{Au} B_l e^{A(tau-u)} du) L_v / sum_k rho_k f_vk      (the classes by their posterior)
 * counts[l][i] = sum_h w_h n_lv(h), site_counts[l][i][h] = n_lv(h) (0 where w_h = 0), v = nodes[i].  nodes == NULL: every node in node
 * order, n_query is not read, the arrays have n_nodes columns and the root's are 0.  The identity as a label returns branch[v] at every
 * pattern; the all-ones off-diagonal label the expected number of substitutions.  Nothing is re-rooted and no reversibility is assumed.
 * *lnL has the bytes paml_amd_model_gradient returns on the same engine and inputs, whose passes these are; lnf[] is those passes' ln f_h.
 * Takes what paml_amd_gradient takes and leaves the engine as it does; the workspace is 256 MiB or PAML_AMD_COUNTS_ARENA_MB (read at
 * every call).  Every result has the same bytes whatever the batches, for any sub-list or order of the labels and of the nodes, and on
 * every call (no atomics).  PAML_AMD_EINVAL for a null branch, labels, lnL or counts, a model or tips not set, n_lab outside
 * 1 .. 16, a label entry that is not finite, a queried node that is the root, out of range or listed
 * twice; PAML_AMD_EUNSUPPORTED for a rate-matrix (UNREST) set, more than 64 states, an engine whose communicator has more than one rank. */
int paml_amd_subst_counts(paml_amd_engine *e, const double *branch, const double *gene_rate,
                          int n_lab, const double *labels /* [n_lab][n][n] */,
                          int n_query, const int *nodes   /* non-root nodes; NULL = all, node order */,
                          double *lnL, double *counts     /* [n_lab][n_query] */,
                          double *site_counts             /* [n_lab][n_query][n_patt], or NULL */,
                          double *lnf                     /* [n_patt], or NULL */);
/* The number of batches the calling thread's last paml_amd_subst_counts walked and the time of its kernels by HIP events (ms). */
void paml_amd_subst_counts_info(int *last_batches, double *last_kernel_ms);

/* ---- The lnL of every nearest-neighbour-interchange (NNI) neighbour of the tree at the present branch lengths, in one call (the trees
 * the reference's search, Perturbation treesub.c:4642 on NeighborNNI treespace.c:283, takes one after the other; the definition and the
 * kernels are written out in csrc/kernels_nni.h).  A swap is (v, s, x): v an internal node that is not the root, s a son of v, x a son
 * of the father of v other than v.  The subtrees below s and x change places; each keeps the branch above it, and with the branch its
 * length and its label.  lnL[i] and lnf[i][h] are what paml_amd_eval would return for that tree as rooted at (branch[n_nodes],
 * gene_rate[n_genes] or NULL = 1) — equal to rounding, not to the bit, and without regard to where the rearranged tree's scaling marks
 * would sit (the present tree's partials are reused; only the log factors differ).  *lnL0 is the present tree's lnL, taken as
 * paml_amd_gradient takes it.  One down pass, one outer pass (the gradient's without the derivative), then per swap the products of the
 * two nodes around the edge: no tree is set and no kernel is built per neighbour.  Everything paml_amd_gradient takes — K classes,
 * several genes, branch labels, ambiguity codes, polytomies, scaling nodes, a root that is a tip, at most 64 states — and rate-matrix
 * (UNREST) sets too: only P(t) is used.  Synchronous; builds the P(t) an evaluation would build, by the same kernels, starts
 * eval_branch's resident state over, leaves a following paml_amd_eval its bits, and paml_amd_get_pmat returns the matrices the call
 * used.  n_patt is walked gene by gene in batches of what a workspace holds (256 MiB; the environment variable PAML_AMD_NNI_ARENA_MB,
 * read at every call, gives another size in MiB), and the swaps in groups where one tile of patterns with all of them does not fit:
 * every output has the same bits for any workspace size, for any place of a swap in the list and on every call (fixed-order sums, no
 * atomics).  PAML_AMD_EINVAL (with a message starting "nni_scores") for a null branch, swaps, lnL0 or lnL, n_swaps < 1, a v that is a
 * tip, the root or out of range, an s that is not a son of v, an x that is not a son of the father of v or is v, a model or tips not
 * set; PAML_AMD_EUNSUPPORTED for tips that are not the nodes 0 .. n_tips - 1, more than 64 states, an engine whose communicator has
 * more than one rank; PAML_AMD_ENOCONV as the other synchronous entries. */
int paml_amd_nni_scores(paml_amd_engine *e, const double *branch, const double *gene_rate,
                        int n_swaps, const int *swaps /* [n_swaps][3] = v, s, x */,
                        double *lnL0, double *lnL /* [n_swaps] */, double *lnf /* [n_swaps][n_patt], or NULL */);
/* The number of pattern batches the calling thread's last paml_amd_nni_scores walked and the time of its kernels by HIP events (ms,
 * summed); either pointer may be NULL. */
void paml_amd_nni_info(int *last_batches, double *last_kernel_ms);
/* The canonical list of swaps of a tree given as paml_amd_set_tree takes it, host only (no engine, no device): every (s, x) of every
 * internal v that is not the root, in node order, s over the sons of v and x over its father's other sons in son-list order.  A v with
 * two sons under a root with exactly three sons lists its first son only — the other son's swaps are the same unrooted trees — so an
 * unrooted binary tree of ns tips gets the reference's 2 (ns - 3) neighbours (treesub.c:4687).  Returns the list's length (with swaps =
 * NULL the length only), or PAML_AMD_EINVAL for a bad tree or a list longer than cap. */
int paml_amd_nni_list(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, int *swaps /* [cap][3], or NULL */, int cap);

/* ---- Edge scores: the lnL of a configuration of an internal edge at trial lengths of the five branches around it, with the first and
 * second derivative along one of them, for all rows in ONE call: the device primitive under the approximate likelihood-ratio test of a
 * branch (aLRT, Anisimova & Gascuel 2006; its SH-like form, Guindon et al. 2010), which maximises the present resolution of an edge and
 * its two NNI alternatives over the five branches around it with everything else held fixed.  A row is (v, s, x, u): (v, s, x) is the
 * swap of paml_amd_nni_scores, or s = x = -1 for the present configuration of the edge above v.  A branch is named by the node below it
 * and keeps its length and label through the swap.  ovr_node names up to five branches (-1: unused) whose lengths are taken from ovr_t
 * instead of branch: v, the father f of v if f is not the root, any son of v, any son of f other than v.  u is -1 or one of the row's
 * override nodes: d1[i] is the derivative of lnL[i] with respect to the length of the branch above u at the given lengths and d2[i] the
 * second derivative; for u = -1 both are 0 and no derivative matrices are built.  lnL[i] and lnf[i][h] are what paml_amd_eval would
 * return for the rearranged tree with the override lengths written into branch, to rounding (the definition is written out in
 * csrc/kernels_edge.h; no reversibility is assumed and nothing is re-rooted); *lnL0 is the present tree's lnL at `branch`, taken as
 * paml_amd_nni_scores takes it.  No tree is set and no kernel is built per row.  K classes, several genes, branch labels, ambiguity
 * codes, polytomies elsewhere, scaling nodes, a root that is a tip, at most 64 states.  Synchronous; leaves a following paml_amd_eval,
 * paml_amd_gradient, paml_amd_nni_scores, paml_amd_placement_scores and paml_amd_spr_scores their results, and paml_amd_get_pmat
 * afterwards returns the tree's own matrices at `branch`.  n_patt is walked gene by gene in batches of what a workspace holds (256 MiB;
 * the environment variable PAML_AMD_EDGE_ARENA_MB, read at every call, gives another size in MiB), and the rows in groups where one tile
 * of patterns with all of them does not fit: every output has the same bits for any workspace size, for any sub-list or order of the
 * rows and on every call (fixed-order sums, no atomics).  PAML_AMD_EINVAL (with a message starting "edge_scores" that names the row)
 * for a null argument other than gene_rate and lnf, n_rows < 1, a bad v, s or x as paml_amd_nni_scores, an override node outside the
 * edge's neighbourhood or listed twice, f listed when it is the root, a u that is not among the row's override nodes, a model or tips
 * not set; PAML_AMD_EUNSUPPORTED for rate-matrix (UNREST) sets (as paml_amd_gradient), tips that are not the nodes 0 .. n_tips - 1, more
 * than 64 states, an engine whose communicator has more than one rank; PAML_AMD_ENOCONV as the other synchronous entries. */
int paml_amd_edge_scores(paml_amd_engine *e, const double *branch, const double *gene_rate,
                         int n_rows, const int *rows /* [n_rows][4] = v, s, x, u */,
                         const int *ovr_node /* [n_rows][5], -1 = unused */, const double *ovr_t /* [n_rows][5] */,
                         double *lnL0, double *lnL, double *d1, double *d2 /* [n_rows] each */, double *lnf /* [n_rows][n_patt], or NULL */);
/* The number of pattern batches the calling thread's last paml_amd_edge_scores walked and the time of its kernels by HIP events (ms,
 * summed); either pointer may be NULL. */
void paml_amd_edge_info(int *last_batches, double *last_kernel_ms);
/* The edges of a tree (given as paml_amd_set_tree takes it) that have three configurations, host only: every internal v that is not the
 * root, has exactly two sons (s1, s2) and whose father f is either a non-root node with two sons (v, c) or a root with exactly three
 * sons (v, c1, c2), in node order.  Per edge: the present configuration (v, -1, -1) and the two swaps paml_amd_nni_list gives for that
 * v — (s1, c), (s2, c), or (s1, c1), (s1, c2) under the root — and the five branches around it: s1, s2, v, then c and f, or c1 and c2.
 * Edges next to a polytomy or under a root with two sons are not listed.  Returns the count (with edges = five = NULL the count only),
 * or PAML_AMD_EINVAL for a bad tree or a list longer than cap. */
int paml_amd_edge_list(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons,
                       int *edges /* [cap][3][3] = per edge three (v, s, x), or NULL */, int *five /* [cap][5], or NULL */, int cap);

/* ---- Relabel scores: the lnL of the tree with the label of ONE branch changed, for all (branch, label) rows in ONE call: the device
 * primitive under a scan of every branch as the foreground of a branch-site or branch model.  Row (v, l) is the present tree — with
 * the labels of base_label where it is given, otherwise the tree's own — with the label of the branch above v set to l; v is any node
 * other than the root, tips included.  lnL[i] and lnf[i][h] are what paml_amd_eval would return for that tree at `branch`, to rounding
 * (the definition is written out in csrc/kernels_relabel.h); *lnL0 is the present tree's lnL, taken as paml_amd_nni_scores takes it.
 * lnfk[i][k][h] is the log of the likelihood of pattern h given class k, WITHOUT freqK (-inf where it is not positive), and lnfk0[k][h]
 * the same of the present tree: what a host needs to re-mix the class proportions without another call.  A class whose eigen set and
 * Qfactor are the same under l as under the branch's present label (for the pattern's gene) is not computed: its lnfk row has the bits
 * of lnfk0[k]; a row in which no class changes has the bits of the present tree's lnf, and lnL[i] those of *lnL0.  No tree is set and no
 * kernel is built per row.  K classes, several genes, ambiguity codes, polytomies, scaling nodes, a root that is a tip, at most 64
 * states.  Synchronous; leaves a following paml_amd_eval, paml_amd_gradient, paml_amd_nni_scores, paml_amd_placement_scores,
 * paml_amd_spr_scores and paml_amd_edge_scores their results, and paml_amd_get_pmat afterwards returns the tree's own matrices at
 * `branch`.  n_patt is walked gene by gene in batches of what a workspace holds (256 MiB; the environment variable
 * PAML_AMD_RELABEL_ARENA_MB, read at every call, gives another size in MiB), and the rows in groups where one tile of patterns with all
 * of them does not fit: every output has the same bits for any workspace size, for any sub-list or order of the rows and on every call
 * (fixed-order sums, no atomics).  PAML_AMD_EINVAL (with a message starting "relabel_scores" that names the row) for a null branch,
 * rows, lnL0 or lnL, n_rows < 1, a v that is the root or out of range, a label outside [0, n_labels) in a row or in base_label, lnfk
 * without lnfk0 or the reverse, a model or tips not set; PAML_AMD_EUNSUPPORTED for rate-matrix (UNREST) sets (as paml_amd_edge_scores),
 * tips that are not the nodes 0 .. n_tips - 1, more than 64 states, an engine whose communicator has more than one rank;
 * PAML_AMD_ENOCONV as the other synchronous entries. */
int paml_amd_relabel_scores(paml_amd_engine *e, const double *branch, const double *gene_rate,
                            const int *base_label /* [n_nodes], or NULL = the tree's labels */,
                            int n_rows, const int *rows /* [n_rows][2] = v, label */,
                            double *lnL0, double *lnL /* [n_rows] */, double *lnf /* [n_rows][n_patt], or NULL */,
                            double *lnfk0 /* [K][n_patt], or NULL */, double *lnfk /* [n_rows][K][n_patt], or NULL */);
/* The number of pattern batches the calling thread's last paml_amd_relabel_scores walked and the time of its kernels by HIP events (ms,
 * summed); either pointer may be NULL. */
void paml_amd_relabel_info(int *last_batches, double *last_kernel_ms);

/* ---- Placement: the lnL of the tree with one more tip hung on a branch, for every query, every branch and every pendant length in ONE
 * call.  The reference's stepwise addition (StepwiseAddition treesub.c:4866 on AddSpecies treesub.c:4592) sets and evaluates one enlarged
 * tree after the other; the same primitive lies under the regraft half of an SPR move and under placing new sequences on a fitted tree.
 * An edge is a node v != root (the branch above v, length t_v, label lambda_v).  Placing query q on edge v with split phi in [0, 1] and
 * pendant length tau makes a new internal node u between v's father and v: the branch above u has length (1 - phi) t_v, the branch above
 * v has length phi t_v (both labelled lambda_v), and u's second son is the query tip on a branch of length tau labelled pendant_label.
 * lnL[q][e][j] is what paml_amd_eval returns for that tree as rooted, to rounding (the definition: kernels_place.h); lnL0 is the present
 * tree's.  qz holds the queries' character codes per pattern, numbered as the table given to paml_amd_set_tips.  edges = NULL means every
 * non-root node in node order (n_edges must then be n_nodes - 1).  Nothing is re-rooted and no reversibility is assumed; every P(t) comes
 * from the evaluation's own builder, so every kind of set, class rates, gene rates and Qfactors are served.  Afterwards the engine holds
 * P(t) of the tree at `branch`, as after paml_amd_nni_scores.  n_patt is walked gene by gene in batches of what a workspace holds (256
 * MiB; the environment variable PAML_AMD_PLACE_ARENA_MB, read at every call, gives another size in MiB), and the edges in groups where one
 * tile of patterns with all rows does not fit: every output has the same bits for any workspace size, for any sub-list or order of
 * queries, edges and pendants and on every call (fixed-order sums, no atomics).  PAML_AMD_EINVAL (with a message starting
 * "placement_scores") for a null branch, qz, pendant, lnL0 or lnL, n_q, n_edges or n_pend < 1, a code in qz that is >= n_codes or has an
 * empty state set, an edge that is the root or out of range, phi outside [0, 1], a negative or non-finite pendant, a pendant_label
 * outside the class tables' labels, a model or tips not set; PAML_AMD_EUNSUPPORTED for tips that are not the nodes 0 .. n_tips - 1, more
 * than 64 states, an engine whose communicator has more than one rank; PAML_AMD_ENOCONV as the other synchronous entries. */
int paml_amd_placement_scores(paml_amd_engine *e, const double *branch, const double *gene_rate,
                              int n_q, const unsigned char *qz /* [n_q][n_patt] */,
                              int n_edges, const int *edges /* [n_edges] nodes v != root, or NULL */,
                              int n_pend, const double *pendant /* [n_pend] */, double phi, int pendant_label,
                              double *lnL0, double *lnL /* [n_q][n_edges][n_pend] */, double *lnf /* [n_q][n_edges][n_pend][n_patt], or NULL */);
/* The number of pattern batches the calling thread's last paml_amd_placement_scores walked and the time of its kernels by HIP events
 * (ms, summed); either pointer may be NULL. */
void paml_amd_placement_info(int *last_batches, double *last_kernel_ms);

/* ---- Attachment at free lengths: the lnL of the tree with a query tip hung on a branch at the row's own lengths of the three branches
 * that meet at the new node, with the first and second derivative along one of them, for many rows in ONE call: what a maximum-likelihood
 * placement (the maximum over the proximal, the distal and the pendant length) is iterated on, where paml_amd_placement_scores gives a
 * grid.  Row (q, v, role) with t3 = (t_up, t_dn, t_pend): v any node but the root, tips included; the new node u sits between v's father
 * and v; the branch above u has length t_up and the branch above v has length t_dn (both labelled as v's branch; t_up + t_dn need not be
 * branch[v]); query q hangs below u on a branch of length t_pend labelled pendant_label.  lnL[i] is what paml_amd_eval returns for that
 * tree as rooted, to rounding (the definition: kernels_attach.h); d1[i], d2[i] are its first and second derivative along the branch named
 * by role (0: up, 1: dn, 2: pendant) at those lengths, both 0 for role -1; lnL0 is the present tree's, taken as paml_amd_nni_scores takes
 * it.  qz holds the queries' character codes per pattern, numbered as the table given to paml_amd_set_tips; only the queries that a row
 * names are read.  Nothing is re-rooted and no reversibility is assumed; class rates, gene rates, Qfactors, branch labels, ambiguity
 * codes, polytomies, scaling nodes and a root that is a tip are served, up to 64 states.  Synchronous; leaves a following paml_amd_eval,
 * paml_amd_gradient, paml_amd_nni_scores, paml_amd_placement_scores, paml_amd_spr_scores, paml_amd_edge_scores and
 * paml_amd_relabel_scores their results and paml_amd_get_pmat the matrices of the tree at `branch`.  n_patt is walked gene by gene in
 * batches of what a workspace holds (256 MiB; the environment variable PAML_AMD_ATTACH_ARENA_MB, read at every call, gives another size
 * in MiB), and the rows in groups where one tile of patterns with all rows does not fit: every output has the same bits for any workspace
 * size, for any sub-list or order of the rows and of the queries and on every call (fixed-order sums, no atomics).  Beside the workspace
 * a row takes five matrices per (gene, class), and on the matrix cores four column tables.  PAML_AMD_EINVAL (with a message starting
 * "attach_scores" that names the row) for a null argument other than gene_rate and lnf, n_q or n_rows < 1, a q out of range, a v that is
 * the root or out of range, a role outside -1 .. 2, a negative or non-finite length, a code of a named query that is >= n_codes or has
 * an empty state set, a pendant_label outside the class tables' labels, a model or tips not set; PAML_AMD_EUNSUPPORTED for rate-matrix
 * (UNREST) sets (as paml_amd_edge_scores), tips that are not the nodes 0 .. n_tips - 1, more than 64 states, an engine whose communicator
 * has more than one rank; PAML_AMD_ENOCONV as the other synchronous entries. */
int paml_amd_attach_scores(paml_amd_engine *e, const double *branch, const double *gene_rate,
                           int n_q, const unsigned char *qz /* [n_q][n_patt] */,
                           int n_rows, const int *rows /* [n_rows][3] = q, v, role */,
                           const double *t3 /* [n_rows][3] = t_up, t_dn, t_pend */, int pendant_label,
                           double *lnL0, double *lnL, double *d1, double *d2 /* [n_rows] each */,
                           double *lnf /* [n_rows][n_patt], or NULL */);
/* The number of pattern batches the calling thread's last paml_amd_attach_scores walked and the time of its kernels by HIP events (ms,
 * summed); either pointer may be NULL. */
void paml_amd_attach_info(int *last_batches, double *last_kernel_ms);

/* ---- Subtree prune and regraft: the lnL of every requested SPR neighbour of the tree at the present branch lengths in ONE call.  A move
 * is (s, x) with a split phi in [0, 1]: f = father(s), g = father(f), c = the other son of f.  The subtree below s leaves with f; c takes
 * f's place under g on a branch of length t_c + t_f with c's label; f takes x's place under x's father with the sons (x, s), the branch
 * above f has length (1 - phi) t_x and x's label, the branch above x phi t_x.  Node ids, n_nodes and the root stay and the tree's length is
 * unchanged.  A move is valid when s is not the root, f is not the root and has exactly two sons, x is not the root, not f, not c (the same
 * topology) and not in the subtree below s.  Out of scope: pruning the side of a branch that holds the root (it would reverse branches),
 * and a prune whose father is the root or a polytomy.  lnL[i] and lnf[i][h] are what paml_amd_eval returns for the rearranged tree as
 * rooted, to rounding, without regard to where that tree's own scaling marks would sit (the definition: kernels_spr.h); *lnL0 is the
 * present tree's lnL, taken as paml_amd_gradient takes it.  One down pass and one outer pass, then per pruned s the products up the path
 * from g to the root, the outward chain over the nodes that lead to its targets, and two products and one dot product per target: no tree
 * is set and no kernel is built per neighbour.  Everything paml_amd_nni_scores takes is served — K classes, several genes, branch labels,
 * ambiguity codes, polytomies elsewhere in the tree, scaling nodes, a root that is a tip, at most 64 states, rate-matrix (UNREST) sets —
 * and the side effects are the same: the engine holds P(t) of the tree at `branch` afterwards, eval_branch's resident state starts over,
 * a following paml_amd_eval keeps its bits.  n_patt is walked gene by gene in batches of what a workspace holds (256 MiB; the environment
 * variable PAML_AMD_SPR_ARENA_MB, read at every call, gives another size in MiB).  The moves are walked in groups of whole s in two
 * cases: where one tile of patterns with the rows of all moves does not fit, and where those rows would leave a batch less than half
 * the patterns that the partials alone allow (a list of many moves would otherwise cut the batches short).  Every output has the same
 * bits for any workspace size, for any sub-list or order of the moves and on every call (fixed-order sums, no atomics).
 * PAML_AMD_EINVAL (with a message starting "spr_scores", naming "move i" for a bad move)
 * for a null branch, moves, lnL0 or lnL, n_moves < 1, phi outside [0, 1] or not finite, a move that is not valid or names a node out of
 * range, a model or tips not set; PAML_AMD_EUNSUPPORTED for tips that are not the nodes 0 .. n_tips - 1, more than 64 states, an engine
 * whose communicator has more than one rank; PAML_AMD_ENOCONV as the other synchronous entries. */
int paml_amd_spr_scores(paml_amd_engine *e, const double *branch, const double *gene_rate,
                        int n_moves, const int *moves /* [n_moves][2] = s, x */, double phi,
                        double *lnL0, double *lnL /* [n_moves] */, double *lnf /* [n_moves][n_patt], or NULL */);
/* The number of pattern batches the calling thread's last paml_amd_spr_scores walked and the time of its kernels by HIP events (ms,
 * summed); either pointer may be NULL. */
void paml_amd_spr_info(int *last_batches, double *last_kernel_ms);
/* The canonical list of moves of a tree given as paml_amd_set_tree takes it, host only (no engine, no device): every valid (s, x) with
 * d(s, x) <= radius (radius <= 0: no limit), s in node order and x in node order within s.  d is the number of branches, in the tree
 * without s and f, on the shortest chain of branches from the merged branch above c to the branch above x, x's counted and c's not:
 * adjacent branches have d = 1, and the trees of the radius-1 list are the NNI neighbours.  Returns the list's length (with moves = NULL
 * the length only), or PAML_AMD_EINVAL for a bad tree or a list longer than cap. */
int paml_amd_spr_list(int n_tips, int n_nodes, int root, const int *sons_ptr, const int *sons, int radius, int *moves /* [cap][2], or NULL */, int cap);

/* ---- Pairwise maximum-likelihood comparisons (codeml runmode = -2; PairwiseCodon codeml.c:4344-4604, Goldman & Yang 1994).
 * The reference takes the ns (ns - 1) / 2 pairs one after the other, each a search over (t, kappa, omega) whose every function call
 * (lfun2dSdN codeml.c:4219-4264) decomposes a rate matrix on one core.  Here a PAIR SET lives on an engine whose tips are clean data
 * (set_tips with cleandata != 0; no tree is needed), and the unit of work is a batch of ELEMENTS (pair, t, kappa, omega): all pairs'
 * gradient and line-search points of a round of the host's searches in one call.
 *
 * pairset_create: pairs p = (seq_a[p], seq_b[p]), 0-based tips.  Counts the pairs' tables fp[max(za, zb)][min(za, zb)] += w_h
 *   (codeml.c:4407-4413) on the device and keeps them resident; sizes the arena of eigen systems once (a quarter of the free device
 *   memory, at most 1 GiB; the environment variable PAML_AMD_PAIR_ARENA_MB gives another size in MiB).  PAML_AMD_EINVAL for unclean
 *   tips, a pair of a sequence with itself, indices out of range.  Destroy the pair set before its engine.
 * pairset_get_counts: fp[n_pairs][n * n] (row = the larger state) and ls_pair[n_pairs] = the pairs' numbers of sites (either may be
 *   NULL) — what the host needs once for the pairs' codon frequencies (codeml.c:4448-4453), and the parity accessor.
 * pairset_set_pi: pi[n_pairs][n], the codon frequencies of every pair (GetCodonFreqs2 codeml.c:4169-4216 is the host's).
 * pairset_set_pattern: the elements a rate matrix can have — nnz positions (row[k] >= col[k], each once, the n diagonal positions among
 *   them: the layout of paml_amd_set_eigen_qrev_batch_sparse) and for each flags[k]: bit 0 = a transition (the rate carries kappa),
 *   bit 1 = nonsynonymous (omega).  Q_ij = flags' factors x pi_j, scaled to one substitution per codon (eigenQcodon codeml.c:3229-3316).
 * pairset_eval: lnL[i] = +sum_{j >= k} fp[j][k] log(pi_j P_jk(t_i)) of element i (lfun2dSdN returns -lnL), f <= 0 floored at 1e-70 as
 *   there (codeml.c:4256-4260).  Only (pair, t, kappa, omega) crosses PCIe; the rate matrices are built, decomposed (the Jacobi of
 *   paml_amd_set_eigen_qrev_batch, on the pair set's own arena — not the engine's table of eigen sets) and used on the device.  Elements
 *   of one call with identical (pair, kappa, omega) share one decomposition.  A call of any size is walked in chunks of what the arena
 *   holds: never PAML_AMD_ENOMEM for n_elem.  An element's lnL has the same bits in whatever call, chunk or company it is evaluated.
 *   Synchronous.  PAML_AMD_ENOCONV when a decomposition reached its sweep limit: every other element's lnL is valid, and
 *   pairset_failed lists the indices (into the last call's elements; returns their number, writes at most cap) for the host to redo.
 * pairset_counters: elements evaluated, decompositions done, chunks walked so far; the arena's capacity in eigen systems. */
typedef struct paml_amd_pairset paml_amd_pairset;
int paml_amd_pairset_create(paml_amd_engine *e, paml_amd_pairset **out, int n_pairs, const int *seq_a, const int *seq_b);
void paml_amd_pairset_destroy(paml_amd_pairset *ps);
int paml_amd_pairset_get_counts(paml_amd_pairset *ps, double *fp, double *ls_pair);
int paml_amd_pairset_set_pi(paml_amd_pairset *ps, const double *pi);
int paml_amd_pairset_set_pattern(paml_amd_pairset *ps, int nnz, const int *row, const int *col, const unsigned char *flags);
int paml_amd_pairset_eval(paml_amd_pairset *ps, long n_elem, const int *pair, const double *t, const double *kappa, const double *omega,
                          double *lnL);
int paml_amd_pairset_failed(const paml_amd_pairset *ps, long *idx, long cap);
int paml_amd_pairset_counters(const paml_amd_pairset *ps, long *n_elem, long *n_decomp, long *n_chunks, long *arena_slots);

#ifdef __cplusplus
}
#endif
#endif
