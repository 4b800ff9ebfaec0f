/* main.c -- the `psmc` executable: lh3/psmc's command line (main.c:6-34) with
 * the E-step bound to libpsmc_hip.so.  There is no CPU E-step in this binary:
 * without a visible AMD GPU it exits with an error.
 *   PSMC_HIP_MODE=exact (default: .psmc byte-identical to the reference) | fast
 *   PSMC_HIP_DECODE=fast             with PSMC_HIP_MODE=fast and -d/-D/-c/-s: stay in fast mode and decode from the fast
 *                                    tables (without it such a run is an exact run throughout)
 *   PSMC_HIP_WIDE=fast               with PSMC_HIP_MODE=fast and 129..256 states: factored fast E-steps on the wide fast path
 *                                    (option "wide_fast"); without it such a run is an exact run throughout, and so it is with
 *                                    -d/-D/-c/-s unless PSMC_HIP_DECODE=fast is set too: the EM rounds then stay on the wide fast
 *                                    path and the decoding reads its tables (option "wide_decode")
 *   PSMC_HIP_WIDE=fast-all           the same, and at 257..1024 states the factored fast E-steps of the multi-wave wide fast path
 *                                    ("wide_fast" = 2); a decoding run beyond 256 states stays on the exact kernels throughout
 *                                    unless PSMC_HIP_DECODE=fast-all is set too
 *   PSMC_HIP_DECODE=fast-all         what PSMC_HIP_DECODE=fast means, and with PSMC_HIP_WIDE=fast-all, 257..1024 states and
 *                                    -d/-D/-c/-s the EM rounds stay on the multi-wave wide fast path and the decoding reads its
 *                                    tables ("wide_fast" = 2 + "wide_decode")
 *   PSMC_HIP_WIDE_COUNTS=1           with PSMC_HIP_WIDE covering the run's size and a run that asks for full counts (PSMC_FACTORED=0 or
 *                                    PSMC_FAST_MSTEP=0): the full-count E-steps run on the wide fast path too (options "wide_fast" +
 *                                    "wide_counts"); without it they use the exact kernels.  With
 *                                    PSMC_HIP_OPTIONS=wide_ckpt=1,wide_counts_ckpt=1 these E-steps keep X at every 8th bin only and
 *                                    the counts pass recomputes the rest ("wide_counts_ckpt"): the same output bytes
 *   PSMC_HIP_DEVICE=<index>          one GPU
 *   PSMC_HIP_DEVICES=<i>,<j>,...     the segments of every E-step sharded over these GPUs (psmc_hip_group_*: LPT
 *                                    partition, one RCCL all-reduce of the statistics per EM iteration in fast mode,
 *                                    ordered per-segment sum in exact mode -- the output does not depend on the list) */
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "psmc_host.h"
#include "psmc_hip.h"
#include "hipbe.h"

typedef struct { const char *path; psmc_input *in; int rc; } prefetch_job;
static void *prefetch_input(void *arg) { prefetch_job *j = (prefetch_job *)arg; j->rc = psmc_input_read(j->path, j->in); return 0; }

static int mode_is_fast(void) { const char *s = getenv("PSMC_HIP_MODE"); return s && strcmp(s, "fast") == 0; }

int main(int argc, char *argv[])
{
	psmc_options o;
	psmc_options_default(&o);
	if (psmc_options_parse(&o, argc, argv)) { psmc_options_free(&o); return 1; }
	/* number of states is known only after the pattern (or -i file) is read: peek at it */
	psmc_pattern pat;
	int n_states = 0;
	if (o.param_file) {
		FILE *fp = fopen(o.param_file, "r"); char str[256];
		if (fp && fscanf(fp, "%255s", str) == 1 && psmc_pattern_parse(str, &pat) == 0) { n_states = pat.n_states; psmc_pattern_free(&pat); }
		if (fp) fclose(fp);
	} else if (psmc_pattern_parse(o.pattern_text ? o.pattern_text : "4+5*3+4", &pat) == 0) { n_states = pat.n_states; psmc_pattern_free(&pat); }
	if (n_states < 1) { fprintf(stderr, "psmc: malformed pattern\n"); return 1; }
	if (n_states > PSMC_HIP_MAX_STATES) { /* the reference has no limit at all (khmm.c:10-23 allocates for any n); the wide exact kernels keep one thread per state in a work-group */
		fprintf(stderr, "psmc: the pattern gives %d hidden states; this MI355X build supports at most %d. "
		        "Use a coarser pattern, or the reference binary for this run.\n", n_states, PSMC_HIP_MAX_STATES);
		psmc_options_free(&o);
		return 2;
	}
	/* PSMC_HIP_WIDE=fast: the factored E-step of 129..256 states on the fast kernels (with decoding: only when PSMC_HIP_DECODE=fast
	 * lets the decoding read that path's tables; otherwise it needs the exact ones) */
	const char *wide_s = getenv("PSMC_HIP_WIDE"), *dec_s = getenv("PSMC_HIP_DECODE");
	const int decoding = o.decode || o.print_prob || o.cnt_file;
	const int wide_level = !wide_s ? 0 : (strcmp(wide_s, "fast-all") == 0 ? 2 : (strcmp(wide_s, "fast") == 0 ? 1 : 0));
	const int dec_level = !dec_s ? 0 : (strcmp(dec_s, "fast-all") == 0 ? 2 : (strcmp(dec_s, "fast") == 0 ? 1 : 0));
	const int plan = psmc_mode_plan(mode_is_fast(), wide_level, dec_level, n_states, decoding);
	const int wide_fast = (plan & PSMC_PLAN_WIDE) != 0;
	const char *mode_s = getenv("PSMC_HIP_MODE"), *dev_s = getenv("PSMC_HIP_DEVICE");
	int mode = (mode_s && strcmp(mode_s, "fast") == 0) ? PSMC_HIP_MODE_FAST : PSMC_HIP_MODE_EXACT;
	if (decoding && mode == PSMC_HIP_MODE_FAST) {
		if (plan & PSMC_PLAN_WIDE_DECODE) /* (said below, once it is known that the factored E-step runs) */
			;
		else if (plan & PSMC_PLAN_FAST) /* opt-in: decode from the fast E-step's tables (include/psmc_hip.h: tolerances) */
			fprintf(stderr, "psmc: PSMC_HIP_DECODE=%s: fast E-steps throughout; the decoding reads the fast forward/backward tables\n", dec_s);
		else {
			fprintf(stderr, "psmc: decoding needs the exact forward/backward tables; using PSMC_HIP_MODE=exact\n");
			mode = PSMC_HIP_MODE_EXACT;
		}
	}
	{ /* the O(N) objective goes with the fast E-step unless asked otherwise */
		const char *fm = getenv("PSMC_FAST_MSTEP");
		o.fast_mstep = fm ? atoi(fm) != 0 : (mode == PSMC_HIP_MODE_FAST);
	}
	/* the factored E-step goes with the O(N) objective: fast mode (PSMC_FACTORED=0 keeps the full counts) */
	const char *fs = getenv("PSMC_FACTORED"), *devs = getenv("PSMC_HIP_DEVICES");
	const int use_factored = o.fast_mstep && mode == PSMC_HIP_MODE_FAST && (n_states <= 128 || wide_fast) && !(fs && atoi(fs) == 0);
	/* (PSMC_FACTORED=0 or PSMC_FAST_MSTEP=0 ask for full counts, which beyond 128 states only the exact kernels compute) */
	/* PSMC_HIP_WIDE_COUNTS=1: a run of a size PSMC_HIP_WIDE covers that asks for full counts gets them from the wide fast path as well */
	const char *wc_s = getenv("PSMC_HIP_WIDE_COUNTS");
	char note[256] = "";
	const int wide_counts = wide_fast && !use_factored && mode == PSMC_HIP_MODE_FAST && wc_s && atoi(wc_s) == 1;
	if (wide_fast && use_factored && (plan & PSMC_PLAN_WIDE_DECODE))
		fprintf(stderr, "psmc: %d hidden states: PSMC_HIP_WIDE=%s PSMC_HIP_DECODE=%s: factored E-steps on the wide fast kernels; the decoding reads the wide fast tables\n", n_states, wide_s, dec_s);
	else if (wide_fast && use_factored)
		fprintf(stderr, "psmc: %d hidden states: PSMC_HIP_WIDE=%s: factored E-steps on the wide fast kernels (full counts and decoding stay exact)\n", n_states, wide_s);
	else if (wide_counts) /* said once the first E-step has run: with what it kept (psmc_hipbe_note_counts) */
		snprintf(note, sizeof note, "psmc: %d hidden states: PSMC_HIP_WIDE=%s PSMC_HIP_WIDE_COUNTS=1: full-count E-steps on the wide fast kernels", n_states, wide_s);
	else if (n_states > 128 && mode_is_fast())
		fprintf(stderr, "psmc: %d hidden states: the fast kernels stop at 128, every E-step of this run uses the exact ones\n", n_states);
	/* The input is read on a thread of its own while the device comes up: 0.35 s for a 30 M-bin genome beside 0.4 s of HIP start-up, of a
	 * program that takes 1.0 s in all in fast mode (profiles/r06_fast_after_exact.txt).  psmc_run_begin takes the result over. */
	pthread_t rd_tid;
	prefetch_job pj = {o.in_file, (psmc_input *)calloc(1, sizeof(psmc_input)), 0};
	/* (not from stdin: a device that does not come up must say so at once, not after the pipe has closed) */
	const int rd_started = pj.in && o.in_file && strcmp(o.in_file, "-") != 0 && pthread_create(&rd_tid, 0, prefetch_input, &pj) == 0;
	psmc_estep_backend be;
	int rc = psmc_hipbe_create(&be, n_states, mode, use_factored, devs, dev_s ? atoi(dev_s) : 0);
	if (rc == 0 && wide_fast && (use_factored || wide_counts)) rc = psmc_hipbe_set_option(&be, "wide_fast", wide_level);
	if (rc == 0 && wide_counts) rc = psmc_hipbe_set_option(&be, "wide_counts", 1);
	if (rd_started) { pthread_join(rd_tid, 0); o.prefetched = pj.in; o.prefetch_rc = pj.rc; }
	else free(pj.in);
	if (note[0] && rc) fprintf(stderr, "%s\n", note);
	else if (note[0]) psmc_hipbe_note_counts(&be, note);
	if (rc) {
		fprintf(stderr, "psmc: cannot start the MI355X E-step (%s); this build has no CPU path\n", psmc_hip_strerror(rc));
		psmc_options_free(&o);
		return 2;
	}
	int status = psmc_run(&o, &be);
	be.destroy(be.self);
	psmc_options_free(&o);
	return status;
}
