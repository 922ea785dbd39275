/* pamlh_simulate.c — alignments drawn under the analysis's model (the job of evolver: Simulate evolver.c:818, Evolve 753) on the GPU,
 * and the writer that turns drawn states back into a sequence file this library and the reference both read.
 *   pamlh_simulate: SetParameters(x), the model state to the engine exactly as pamlh_eval_gpu sends it — so clocks, TipDate, branch,
 *     branch-site and clade labels, nhomo and UNREST come for free — then paml_amd_simulate with the branch vector an evaluation
 *     would get.  Refused by name: several genes, rho (rates correlated along the sequence are not independent per site), runmode = -2.
 *   pamlh_write_alignment (host only): sequential PHYLIP; nucleotides in T, C, A, G order, amino acids in the reference's order, codons
 *     as the triplets of the analysis's genetic code (state k = the k-th sense codon). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pamlh_internal.h"

int pamlh_simulate(pamlh *p, const double *x, long n_sites, unsigned long long seed, unsigned replicate, unsigned char *z, unsigned char *cls)
{
   int i, rc;
   if (!p || !z) return -1;
   if (p->pairwise) return pamlh_fail(p, "simulate: runmode = -2 has no tree to simulate on");
   if (p->ngene > 1) return pamlh_fail(p, "simulate: ngene = %d > 1: one gene only", p->ngene);
   if (p->rho0 != 0 || !p->fix_rho) return pamlh_fail(p, "simulate: rho: rates correlated along the sequence are not independent per site");
   if (n_sites < 0) return pamlh_fail(p, "simulate: n_sites = %ld < 0", n_sites);
   if (n_sites == 0) n_sites = p->n_pose > 0 ? p->n_pose : p->ls;
   if (x && (rc = pamlh_set_x(p, x, p->np))) return rc;
   if (p->adg) return pamlh_fail(p, "simulate: rho: rates correlated along the sequence are not independent per site");
   if ((rc = pamlh_engine_model(p))) return rc;
   rc = paml_amd_simulate(p->eng, p->branch, NULL, n_sites, 0, seed, replicate, z, cls, NULL);
   if (rc == PAML_AMD_ENOCONV && pamlh_force_host_eigen()) {      /* as pamlh_eval_gpu: host decomposition, once more */
      for (i = 0; i < p->n_eigen; i++) pamlh_eig_host(&p->eig[i], p->n);
      return pamlh_simulate(p, NULL, n_sites, seed, replicate, z, cls);
   }
   if (rc) return pamlh_fail(p, "%s", paml_amd_last_error(p->eng));
   return 0;
}

int pamlh_write_alignment(const pamlh *p, const unsigned char *z, long n_sites, const char *path)
{
   static const char NUC[] = "TCAG", AA[] = "ARNDCQEGHILKMFPSTWYV";
   char sense[64][4];
   const int width = p && p->seqtype == 1 ? 3 : 1, per_line = 60;
   int i, k, ns = 0;
   long h;
   FILE *f;
   if (!p || !z || !path || n_sites < 1) return -1;
   if (p->translate) return pamlh_fail((pamlh *)p, "write_alignment: seqtype = 3 reads codons and analyses amino acids; the states drawn are amino acids");
   if (p->seqtype == 1) {
      for (k = 0; k < 64; k++)
         if (p->code[k] != '*') { sense[ns][0] = NUC[k >> 4]; sense[ns][1] = NUC[(k >> 2) & 3]; sense[ns][2] = NUC[k & 3]; sense[ns][3] = 0; ns++; }
      if (ns != p->n) return pamlh_fail((pamlh *)p, "write_alignment: the genetic code has %d sense codons, the model %d states", ns, p->n);
   }
   else if (p->n != (p->seqtype == 2 ? 20 : 4)) return pamlh_fail((pamlh *)p, "write_alignment: %d states?", p->n);
   for (i = 0; i < p->ns; i++)
      for (h = 0; h < n_sites; h++)
         if (z[(size_t)i * n_sites + h] >= p->n) return pamlh_fail((pamlh *)p, "write_alignment: state %d of sequence %d at site %ld", z[(size_t)i * n_sites + h], i + 1, h + 1);
   if (!(f = fopen(path, "w"))) return pamlh_fail((pamlh *)p, "write_alignment: cannot write %s", path);
   fprintf(f, " %d %ld\n", p->ns, n_sites * width);
   for (i = 0; i < p->ns; i++) {
      const unsigned char *zi = z + (size_t)i * n_sites;
      fprintf(f, "%s  \n", p->names[i]);      /* (a name ends at two blanks) */
      for (h = 0; h < n_sites; h++) {
         if (p->seqtype == 1) fputs(sense[zi[h]], f);
         else fputc(p->seqtype == 2 ? AA[zi[h]] : NUC[zi[h]], f);
         if ((h + 1) % (per_line / width) == 0 || h + 1 == n_sites) fputc('\n', f);
      }
   }
   if (fclose(f)) return pamlh_fail((pamlh *)p, "write_alignment: writing %s failed", path);
   return 0;
}
