/* host_oracle_quant_main.c -- TEST INFRASTRUCTURE.  The oracle backend of host_oracle_main.c with ONE more optional member,
 * `posterior` (the rows from the oracle's tables, the reference's expression f * b * s), and no `post_quantile`: the branch of the
 * PSMC_TMRCA_BAND writer (psmc_amd/host/run.c band_segment) that counts over a backend's posterior rows.  It must write the bytes
 * of the branch that reads the tables.  Built by tests/test_host_cli_band.py; never shipped. */
#define main host_oracle_main_not_used
#include "host_oracle_main.c"
#undef main

static int oq_posterior(void *self, int seg, double *post, double *recomb)
{
	orc_be *o = (orc_be *)self;
	const int n = o->n, L = o->L[seg];
	double *f = (double *)malloc(sizeof(double) * (size_t)L * n), *b = (double *)malloc(sizeof(double) * (size_t)L * n);
	double *s = (double *)malloc(sizeof(double) * (size_t)L);
	ob_tables(self, seg, f, b, s);
	for (int u = 0; u < L; ++u) {
		if (post)
			for (int k = 0; k < n; ++k) post[(size_t)u * n + k] = f[(size_t)u * n + k] * b[(size_t)u * n + k] * s[u]; /* khmm.c:285-292 */
		if (recomb) { /* aux.c:189-193 */
			double p = 0.0;
			if (u < L - 1) {
				const double *eu1 = o->e + (size_t)o->sym[seg][u + 1] * n;
				for (int l = 0; l < n; ++l) p += f[(size_t)u * n + l] * o->a[(size_t)l * n + l] * b[(size_t)(u + 1) * n + l] * eu1[l];
				p = 1.0 - p;
			}
			recomb[u] = p;
		}
	}
	free(f); free(b); free(s);
	return 0;
}

int main(int argc, char **argv)
{
	psmc_options o;
	psmc_options_default(&o);
	if (psmc_options_parse(&o, argc, argv)) return 1;
	psmc_pattern pat;
	char str[256] = "4+5*3+4";
	if (o.pattern_text) snprintf(str, sizeof str, "%s", o.pattern_text);
	if (psmc_pattern_parse(str, &pat)) return 1;
	orc_be ob; memset(&ob, 0, sizeof ob);
	ob.n = pat.n_states;
	ob.a = (double *)malloc(sizeof(double) * ob.n * ob.n); ob.e = (double *)malloc(sizeof(double) * 3 * ob.n); ob.a0 = (double *)malloc(sizeof(double) * ob.n);
	psmc_estep_backend be;
	memset(&be, 0, sizeof be);
	be.self = &ob; be.load = ob_load; be.estep = ob_estep; be.tables = ob_tables; be.error = ob_error; be.destroy = ob_destroy;
	be.posterior = oq_posterior; /* and no post_quantile */
	const int status = psmc_run(&o, &be);
	be.destroy(be.self);
	psmc_pattern_free(&pat);
	psmc_options_free(&o);
	return status;
}
