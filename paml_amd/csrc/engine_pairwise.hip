// engine_pairwise.hip — pair sets: the pairwise maximum-likelihood comparison of codeml's runmode = -2 (PairwiseCodon codeml.c:4344-4604,
// lfun2dSdN 4219-4264) as batches of (pair, t, kappa, omega) elements on the tips an engine already holds.
// Built for gfx950 only (one of the translation units of libpaml_amd.so, see engine_state.h).
#include "engine_state.h"
#include "eigen_kernels.h"      // EigenQrevArgs (the kernel itself is instantiated and launched in engine_core.hip)
#include "kernels_pairwise.h"

#include <unordered_map>

namespace paml_amd {
int launch_eigen_qrev(paml_amd_engine *e, EigenQrevArgs a, int n_sets);
}

struct paml_amd_pairset {
   paml_amd_engine *e = nullptr;
   int n = 0, n_pairs = 0, nnz = 0;
   bool have_pi = false;
   DevBuf<int> d_seq, d_rc, d_sweeps;
   DevBuf<unsigned char> d_flags;
   DevBuf<double> d_fp, d_ls, d_pi;
   // the arena, sized once: `slots` eigen systems (U, V, Root), and what a chunk's decompositions and elements need beside them
   long slots = 0, elem_cap = 0;
   DevBuf<double> d_uvr, d_vals, d_pi_slot, d_scale, d_lnl;
   DevBuf<double *> d_ptr;
   DevBuf<PairDecomp> d_dec;
   DevBuf<PairElem> d_elem;
   // pinned staging of a chunk
   PairDecomp *h_dec = nullptr;
   PairElem *h_elem = nullptr;
   double *h_lnl = nullptr;
   int *h_sweeps = nullptr;
   std::vector<long> failed;      // elements of the last evaluate call whose decomposition hit the sweep limit
   long n_elem_done = 0, n_decomp_done = 0, n_chunks_done = 0;

   ~paml_amd_pairset()
   {
      if (h_dec) (void)hipHostFree(h_dec);
      if (h_elem) (void)hipHostFree(h_elem);
      if (h_lnl) (void)hipHostFree(h_lnl);
      if (h_sweeps) (void)hipHostFree(h_sweeps);
   }
};

extern "C" {

int paml_amd_pairset_create(paml_amd_engine *e, paml_amd_pairset **out, int n_pairs, const int *seq_a, const int *seq_b)
{
   enter(e);
   if (out) *out = nullptr;
   if (!e || !out || n_pairs < 1 || !seq_a || !seq_b) return fail(e, PAML_AMD_EINVAL, "pairset_create: bad arguments");
   if (!e->d_z.p || !e->d_weights.p) return fail(e, PAML_AMD_EINVAL, "pairset_create: the engine has no tips yet (paml_amd_set_tips)");
   if (!e->cleandata) return fail(e, PAML_AMD_EINVAL, "pairset_create: the tips must be clean data (set_tips with cleandata != 0): pairwise comparisons count states, not ambiguity codes");
   for (int p = 0; p < n_pairs; p++) {
      if (seq_a[p] < 0 || seq_a[p] >= e->n_tips || seq_b[p] < 0 || seq_b[p] >= e->n_tips)
         return fail(e, PAML_AMD_EINVAL, "pairset_create: pair " + std::to_string(p) + " names a sequence outside 0 .. n_tips - 1");
      if (seq_a[p] == seq_b[p]) return fail(e, PAML_AMD_EINVAL, "pairset_create: pair " + std::to_string(p) + " compares a sequence with itself");
   }
   std::unique_ptr<paml_amd_pairset> ps(new (std::nothrow) paml_amd_pairset());
   if (!ps) return fail(e, PAML_AMD_ENOMEM, "pairset_create: host allocation failed");
   ps->e = e; ps->n = e->n; ps->n_pairs = n_pairs;
   const size_t n = e->n, nn = n * n;
   std::vector<int> seq((size_t)2 * n_pairs);
   memcpy(seq.data(), seq_a, (size_t)n_pairs * sizeof(int));
   memcpy(seq.data() + n_pairs, seq_b, (size_t)n_pairs * sizeof(int));
   HIPCHK(upload(ps->d_seq, seq.data(), seq.size(), e->stream));
   HIPCHK(ps->d_fp.ensure((size_t)n_pairs * nn));
   HIPCHK(ps->d_ls.ensure(n_pairs));
   HIPCHK(ps->d_pi.ensure((size_t)n_pairs * n));
   PairCountArgs ca{};
   ca.n = (int)n; ca.n_patt = e->n_patt; ca.n_pairs = n_pairs; ca.z = e->d_z.p; ca.w = e->d_weights.p;
   ca.seq_a = ps->d_seq.p; ca.seq_b = ps->d_seq.p + n_pairs; ca.fp = ps->d_fp.p; ca.ls = ps->d_ls.p;
   hipLaunchKernelGGL(pair_count_kernel, dim3(n_pairs), dim3(256), 0, e->stream, ca);
   HIPCHK(hipGetLastError());
   // The arena: an element's U, V, Root is (2 n^2 + n) doubles (60 KB at 61 states), so all points of all pairs of a large alignment do
   // not fit at once (18 336 pairs x 4 points: 4.4 GB); an evaluation walks its elements in chunks of at most `slots` decompositions.
   // A quarter of the free memory, at most 1 GiB; PAML_AMD_PAIR_ARENA_MB sets another size (the tests shrink it to force several chunks).
   size_t free_b = 0, total_b = 0;
   HIPCHK(hipMemGetInfo(&free_b, &total_b));
   size_t arena = std::min<size_t>(free_b / 4, (size_t)1 << 30);
   if (const char *mb = getenv("PAML_AMD_PAIR_ARENA_MB")) arena = (size_t)std::max(1L, atol(mb)) << 20;
   const size_t slot_bytes = (2 * nn + n) * sizeof(double);
   ps->slots = (long)std::max<size_t>(1, std::min<size_t>(arena / slot_bytes, 1 << 20));
   while (ps->slots > 1 && ps->d_uvr.ensure((size_t)ps->slots * (2 * nn + n)) != hipSuccess) {      // (less memory than hipMemGetInfo promised: halve)
      (void)hipGetLastError();
      ps->slots /= 2;
   }
   HIPCHK(ps->d_uvr.ensure((size_t)ps->slots * (2 * nn + n)));
   ps->elem_cap = std::max<long>(4 * ps->slots, 1024);
   const long S = ps->slots;
   HIPCHK(ps->d_pi_slot.ensure((size_t)S * n));
   HIPCHK(ps->d_scale.ensure(S));
   HIPCHK(ps->d_sweeps.ensure(S));
   HIPCHK(ps->d_dec.ensure(S));
   HIPCHK(ps->d_elem.ensure(ps->elem_cap));
   HIPCHK(ps->d_lnl.ensure(ps->elem_cap));
   std::vector<double *> ptr((size_t)3 * S);
   for (long s = 0; s < S; s++) {
      ptr[s] = ps->d_uvr.p + (size_t)s * nn;
      ptr[S + s] = ps->d_uvr.p + (size_t)S * nn + (size_t)s * nn;
      ptr[2 * S + s] = ps->d_uvr.p + (size_t)2 * S * nn + (size_t)s * n;
   }
   HIPCHK(upload(ps->d_ptr, ptr.data(), ptr.size(), e->stream));
   HIPCHK(hipHostMalloc((void **)&ps->h_dec, (size_t)S * sizeof(PairDecomp), hipHostMallocDefault));
   HIPCHK(hipHostMalloc((void **)&ps->h_elem, (size_t)ps->elem_cap * sizeof(PairElem), hipHostMallocDefault));
   HIPCHK(hipHostMalloc((void **)&ps->h_lnl, (size_t)ps->elem_cap * sizeof(double), hipHostMallocDefault));
   HIPCHK(hipHostMalloc((void **)&ps->h_sweeps, (size_t)S * sizeof(int), hipHostMallocDefault));
   HIPCHK(hipStreamSynchronize(e->stream));
   *out = ps.release();
   return 0;
}

void paml_amd_pairset_destroy(paml_amd_pairset *ps)
{
   if (!ps) return;
   if (ps->e) (void)hipStreamSynchronize(ps->e->stream);
   delete ps;
}

int paml_amd_pairset_get_counts(paml_amd_pairset *ps, double *fp, double *ls_pair)
{
   if (!ps) return PAML_AMD_EINVAL;
   paml_amd_engine *e = ps->e;
   enter(e);
   const size_t nn = (size_t)ps->n * ps->n;
   if (fp) HIPCHK(hipMemcpyAsync(fp, ps->d_fp.p, (size_t)ps->n_pairs * nn * sizeof(double), hipMemcpyDeviceToHost, e->stream));
   if (ls_pair) HIPCHK(hipMemcpyAsync(ls_pair, ps->d_ls.p, (size_t)ps->n_pairs * sizeof(double), hipMemcpyDeviceToHost, e->stream));
   HIPCHK(hipStreamSynchronize(e->stream));
   return 0;
}

int paml_amd_pairset_set_pi(paml_amd_pairset *ps, const double *pi)
{
   if (!ps) return PAML_AMD_EINVAL;
   paml_amd_engine *e = ps->e;
   enter(e);
   if (!pi) return fail(e, PAML_AMD_EINVAL, "pairset_set_pi: null argument");
   for (size_t i = 0; i < (size_t)ps->n_pairs * ps->n; i++)
      if (!(pi[i] >= 0) || !std::isfinite(pi[i])) return fail(e, PAML_AMD_EINVAL, "pairset_set_pi: a frequency is negative or not a number");
   HIPCHK(hipMemcpyAsync(ps->d_pi.p, pi, (size_t)ps->n_pairs * ps->n * sizeof(double), hipMemcpyHostToDevice, e->stream));
   HIPCHK(hipStreamSynchronize(e->stream));
   ps->have_pi = true;
   return 0;
}

int paml_amd_pairset_set_pattern(paml_amd_pairset *ps, int nnz, const int *row, const int *col, const unsigned char *flags)
{
   if (!ps) return PAML_AMD_EINVAL;
   paml_amd_engine *e = ps->e;
   enter(e);
   const int n = ps->n;
   if (nnz < 1 || nnz > 1024 || !row || !col || !flags) return fail(e, PAML_AMD_EINVAL, "pairset_set_pattern: bad arguments (1 .. 1024 positions)");
   std::vector<char> seen((size_t)n * n, 0);
   std::vector<int> rc((size_t)2 * nnz);
   for (int k = 0; k < nnz; k++) {
      if (row[k] < col[k] || col[k] < 0 || row[k] >= n) return fail(e, PAML_AMD_EINVAL, "pairset_set_pattern: a position outside the lower triangle");
      if (seen[(size_t)row[k] * n + col[k]]++) return fail(e, PAML_AMD_EINVAL, "pairset_set_pattern: a position appears twice");
      rc[2 * k] = row[k]; rc[2 * k + 1] = col[k];
   }
   for (int i = 0; i < n; i++)
      if (!seen[(size_t)i * n + i]) return fail(e, PAML_AMD_EINVAL, "pairset_set_pattern: the diagonal's positions must be listed");
   HIPCHK(hipStreamSynchronize(e->stream));
   HIPCHK(upload(ps->d_rc, rc.data(), rc.size(), e->stream));
   HIPCHK(upload(ps->d_flags, flags, (size_t)nnz, e->stream));
   HIPCHK(ps->d_vals.ensure((size_t)ps->slots * nnz));
   HIPCHK(hipStreamSynchronize(e->stream));
   ps->nnz = nnz;
   return 0;
}

// One chunk: n_dec decompositions and n_el elements that use them, staged in the pinned buffers.
static int pairset_chunk(paml_amd_pairset *ps, long n_dec, long n_el)
{
   paml_amd_engine *e = ps->e;
   const size_t n = ps->n, nn = n * n;
   const long S = ps->slots;
   HIPCHK(hipMemcpyAsync(ps->d_dec.p, ps->h_dec, (size_t)n_dec * sizeof(PairDecomp), hipMemcpyHostToDevice, e->stream));
   HIPCHK(hipMemcpyAsync(ps->d_elem.p, ps->h_elem, (size_t)n_el * sizeof(PairElem), hipMemcpyHostToDevice, e->stream));
   PairQArgs qa{};
   qa.n = (int)n; qa.nnz = ps->nnz; qa.rc = ps->d_rc.p; qa.flags = ps->d_flags.p; qa.pi = ps->d_pi.p; qa.dec = ps->d_dec.p;
   qa.vals = ps->d_vals.p; qa.pi_slot = ps->d_pi_slot.p; qa.scale = ps->d_scale.p;
   hipLaunchKernelGGL(pair_q_kernel, dim3((unsigned)n_dec), dim3(256), 0, e->stream, qa);
   EigenQrevArgs ea{};
   ea.n = (int)n; ea.Q = ps->d_vals.p; ea.nnz = ps->nnz; ea.rc = ps->d_rc.p; ea.pi = ps->d_pi_slot.p; ea.scale = ps->d_scale.p;
   ea.U = ps->d_ptr.p; ea.V = ps->d_ptr.p + S; ea.Root = ps->d_ptr.p + 2 * S; ea.sweeps = ps->d_sweeps.p;
   ea.fail = nullptr;      // (the sweep counts are read back below: the engine's own eigen sets are not concerned)
   if (int rc = launch_eigen_qrev(e, ea, (int)n_dec)) return rc;
   PairLnlArgs la{};
   la.n = (int)n; la.elem = ps->d_elem.p; la.U = ps->d_uvr.p; la.V = ps->d_uvr.p + (size_t)S * nn; la.Root = ps->d_uvr.p + (size_t)2 * S * nn;
   la.pi = ps->d_pi.p; la.fp = ps->d_fp.p; la.lnL = ps->d_lnl.p;
   hipLaunchKernelGGL(pair_lnl_kernel, dim3((unsigned)n_el), dim3(256), 0, e->stream, la);
   HIPCHK(hipGetLastError());
   HIPCHK(hipMemcpyAsync(ps->h_lnl, ps->d_lnl.p, (size_t)n_el * sizeof(double), hipMemcpyDeviceToHost, e->stream));
   HIPCHK(hipMemcpyAsync(ps->h_sweeps, ps->d_sweeps.p, (size_t)n_dec * sizeof(int), hipMemcpyDeviceToHost, e->stream));
   HIPCHK(hipStreamSynchronize(e->stream));
   return 0;
}

int paml_amd_pairset_eval(paml_amd_pairset *ps, long n_elem, const int *pair, const double *t, const double *kappa, const double *omega, double *lnL)
{
   if (!ps) return PAML_AMD_EINVAL;
   paml_amd_engine *e = ps->e;
   enter(e);
   if (n_elem < 1 || !pair || !t || !kappa || !omega || !lnL) return fail(e, PAML_AMD_EINVAL, "pairset_eval: bad arguments");
   if (!ps->have_pi) return fail(e, PAML_AMD_EINVAL, "pairset_eval: the pairs' codon frequencies have not been set (paml_amd_pairset_set_pi)");
   if (!ps->nnz) return fail(e, PAML_AMD_EINVAL, "pairset_eval: the rate matrix's pattern has not been set (paml_amd_pairset_set_pattern)");
   for (long i = 0; i < n_elem; i++) {
      if (pair[i] < 0 || pair[i] >= ps->n_pairs) return fail(e, PAML_AMD_EINVAL, "pairset_eval: element " + std::to_string(i) + " names a pair outside the set");
      if (!(t[i] >= 0) || !(kappa[i] > 0) || !(omega[i] > 0) || !std::isfinite(t[i]) || !std::isfinite(kappa[i]) || !std::isfinite(omega[i]))
         return fail(e, PAML_AMD_EINVAL, "pairset_eval: element " + std::to_string(i) + " needs t >= 0, kappa > 0, omega > 0");
   }
   ps->failed.clear();
   struct Key {
      int pair; double k, w;
      bool operator==(const Key &o) const { return pair == o.pair && k == o.k && w == o.w; }
   };
   struct KeyHash {
      size_t operator()(const Key &x) const
      {
         unsigned long long a, b;
         memcpy(&a, &x.k, 8); memcpy(&b, &x.w, 8);
         return (size_t)(a * 0x9E3779B97F4A7C15ull ^ (b + 0x7F4A7C15ull) * 0xC2B2AE3D27D4EB4Full ^ (unsigned long long)x.pair * 0x165667B19E3779F9ull);
      }
   };
   std::unordered_map<Key, int, KeyHash> slot_of;
   long i0 = 0;
   while (i0 < n_elem) {
      // elements i0 .. i1 - 1: as many as the arena has eigen systems for; identical (pair, kappa, omega) share one (the t-nudged point of a
      // gradient, the points of a line search along t)
      slot_of.clear();
      long n_dec = 0, i1 = i0;
      for (; i1 < n_elem && i1 - i0 < ps->elem_cap; i1++) {
         const Key key{pair[i1], kappa[i1], omega[i1]};
         auto it = slot_of.find(key);
         int s;
         if (it != slot_of.end()) s = it->second;
         else {
            if (n_dec == ps->slots) break;
            s = (int)n_dec++;
            slot_of.emplace(key, s);
            ps->h_dec[s] = PairDecomp{pair[i1], 0, kappa[i1], omega[i1]};
         }
         ps->h_elem[i1 - i0] = PairElem{s, pair[i1], t[i1]};
      }
      if (int rc = pairset_chunk(ps, n_dec, i1 - i0)) return rc;
      for (long i = i0; i < i1; i++) {
         lnL[i] = ps->h_lnl[i - i0];
         if (ps->h_sweeps[ps->h_elem[i - i0].slot] < 0) ps->failed.push_back(i);
      }
      ps->n_elem_done += i1 - i0;
      ps->n_decomp_done += n_dec;
      ps->n_chunks_done++;
      i0 = i1;
   }
   if (!ps->failed.empty())
      return fail(e, PAML_AMD_ENOCONV, "pairset_eval: the eigen-decomposition of " + std::to_string(ps->failed.size()) +
                                          " element(s) reached its sweep limit without converging (paml_amd_pairset_failed lists them; their lnL is not valid)");
   return 0;
}

int paml_amd_pairset_failed(const paml_amd_pairset *ps, long *idx, long cap)
{
   if (!ps) return PAML_AMD_EINVAL;
   for (long i = 0; i < (long)ps->failed.size() && i < cap && idx; i++) idx[i] = ps->failed[i];
   return (int)std::min<size_t>(ps->failed.size(), 0x7fffffff);
}

int paml_amd_pairset_counters(const paml_amd_pairset *ps, long *n_elem, long *n_decomp, long *n_chunks, long *arena_slots)
{
   if (!ps) return PAML_AMD_EINVAL;
   if (n_elem) *n_elem = ps->n_elem_done;
   if (n_decomp) *n_decomp = ps->n_decomp_done;
   if (n_chunks) *n_chunks = ps->n_chunks_done;
   if (arena_slots) *arena_slots = ps->slots;
   return 0;
}

}  // extern "C"
