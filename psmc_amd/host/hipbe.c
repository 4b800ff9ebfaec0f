/* hipbe.c -- psmc_estep_backend over libpsmc_hip.so: one context, or a group of devices (hipbe.h). */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hipbe.h"

typedef struct {
	psmc_hip_ctx *ctx; psmc_hip_group *grp; int n_seg, n_states; double *chk; char msg[256];
	/* what a fast-mode run needs to repeat ONE E-step in exact mode when its tile boundaries do not converge (PSMC_HIP_ECONVERGE):
	 * how it was created, the segments (borrowed from the caller's psmc_input, alive for the whole run), and the exact twin once made */
	int mode, device; char *devs;
	const uint8_t **sym; int32_t *L;
	psmc_hip_ctx *x_ctx; psmc_hip_group *x_grp; int n_fallbacks;
	/* decoding (prepare_decode): the parameters of the last E-step, and whether the exact twin holds its tables */
	int decoding, on_twin; double *pa, *pe, *pa0;
	/* the wide fast path is on ("wide_fast" went through psmc_hipbe_set_option) / its tables are what the decoding reads ("wide_decode") */
	int wide, wide_decode;
	/* the note about the full-count E-steps on the wide fast path, until the first E-step has run (psmc_hipbe_note_counts) */
	char *note;
	/* what hb_error answers after a failed hb_viterbi on a group: the shard context's message (in msg); cleared by the next call */
	const char *verr;
} hip_be;

/* the per-segment readers go to the context that holds the segment's tables: the exact twin's after a fallback */
static int route(hip_be *h, int seg, psmc_hip_ctx **c, int *local)
{
	if (h->on_twin) {
		if (!h->x_grp) { *c = h->x_ctx; *local = seg; return 0; }
		return psmc_hip_group_route(h->x_grp, seg, c, local);
	}
	if (!h->grp) { *c = h->ctx; *local = seg; return 0; }
	return psmc_hip_group_route(h->grp, seg, c, local);
}

static const char *hb_error(void *self)
{
	hip_be *h = (hip_be *)self;
	if (h->verr) return h->verr;
	if (h->on_twin) return h->x_grp ? psmc_hip_group_last_error(h->x_grp) : psmc_hip_last_error(h->x_ctx);
	return h->grp ? psmc_hip_group_last_error(h->grp) : psmc_hip_last_error(h->ctx);
}

static int hb_load(void *self, int n_seg, const uint8_t *const *sym, const int32_t *L)
{
	hip_be *h = (hip_be *)self;
	h->n_seg = n_seg;
	h->chk = (double *)realloc(h->chk, sizeof(double) * (size_t)n_seg);
	h->sym = (const uint8_t **)realloc((void *)h->sym, sizeof(void *) * (size_t)n_seg);
	h->L = (int32_t *)realloc(h->L, sizeof(int32_t) * (size_t)n_seg);
	for (int i = 0; i < n_seg; ++i) { h->sym[i] = sym[i]; h->L[i] = L[i]; }
	if (h->x_ctx) { psmc_hip_destroy(h->x_ctx); h->x_ctx = 0; }
	if (h->x_grp) { psmc_hip_group_destroy(h->x_grp); h->x_grp = 0; }
	return h->grp ? psmc_hip_group_load_segments(h->grp, n_seg, sym, L) : psmc_hip_load_segments(h->ctx, n_seg, sym, L);
}
/* PSMC_HIP_ECONVERGE from a fast E-step (the verify / repair rounds of the speculative tiles ran out: an input whose chain forgets
 * more slowly than anything the plan allows for) used to end the run.  The statistics are a well-defined quantity all the same:
 * this ONE E-step is repeated by the exact kernels -- a twin context / group in exact mode over the same segments, made on first
 * need -- with a note on stderr; the run goes on in fast mode.  (khmm.c:145-324 has no such failure mode.) */
static int exact_once(hip_be *h, const double *a, const double *e, const double *a0, double *A, double *E, double *LL, int quiet)
{
	int rc = 0;
	if (!quiet) /* (quiet: the caller has said why) */
		fprintf(stderr, "psmc: fast E-step did not converge (%s); repeating this E-step with the exact kernels\n",
		        h->grp ? psmc_hip_group_last_error(h->grp) : psmc_hip_last_error(h->ctx));
	if (!h->x_ctx && !h->x_grp) {
		h->on_twin = 0; /* (a twin that cannot be made holds no tables) */
		if (h->grp) {
			int list[64], n_list = 0;
			char *dup = strdup(h->devs ? h->devs : "0");
			for (char *t = strtok(dup, ","); t && n_list < 64; t = strtok(0, ",")) list[n_list++] = atoi(t);
			free(dup);
			rc = psmc_hip_group_create(&h->x_grp, h->n_states, n_list, list, PSMC_HIP_MODE_EXACT);
			if (rc == 0) rc = psmc_hip_group_load_segments(h->x_grp, h->n_seg, h->sym, h->L);
		} else {
			rc = psmc_hip_create(&h->x_ctx, h->n_states, h->device, PSMC_HIP_MODE_EXACT);
			if (rc == 0) rc = psmc_hip_load_segments(h->x_ctx, h->n_seg, h->sym, h->L);
		}
		if (rc) { fprintf(stderr, "psmc: cannot set up the exact E-step (%s)\n", psmc_hip_strerror(rc)); return rc; }
	}
	++h->n_fallbacks;
	rc = h->x_grp ? psmc_hip_group_estep(h->x_grp, a, e, a0, A, E, 0, LL, h->chk) : psmc_hip_estep(h->x_ctx, a, e, a0, A, E, 0, LL, h->chk);
	h->on_twin = rc == 0; /* the decoding that follows reads the twin's tables */
	return rc;
}

/* after the first E-step: the held-back note, and what that E-step kept when it was a counts E-step of the wide fast path */
static void say_note(hip_be *h, int counts_ok)
{
	if (!h->note) return;
	psmc_hip_ctx *c = h->ctx; int l; int64_t ti[4] = {0, 0, 0, 0};
	const int ck = counts_ok && (!h->grp || psmc_hip_group_route(h->grp, 0, &c, &l) == 0) && psmc_hip_wide_table_info(c, ti) == 0 && ti[2] == 8;
	fprintf(stderr, "%s%s\n", h->note, ck ? ", X at every 8th bin" : "");
	free(h->note); h->note = 0;
}

static void tri_sums(int n, const double *A, double *sums)
{
	memset(sums, 0, sizeof(double) * 5 * (size_t)n);
	for (int k = 0; k < n; ++k)
		for (int l = 0; l < n; ++l) {
			const double v = A[(size_t)k * n + l];
			if (l < k) { sums[k] += v; sums[3 * n + l] += v; } else if (l > k) { sums[n + k] += v; sums[4 * n + l] += v; } else sums[2 * n + k] = v;
		}
}

static int hb_estep(void *self, const double *a, const double *e, const double *a0, double *A, double *E, double *LL,
                    double *chk)
{
	hip_be *h = (hip_be *)self;
	if (h->decoding) { /* kept for the exact twin, should the fast tables turn out not to be decodable (hb_decoded) */
		const size_t n = (size_t)h->n_states;
		if (!h->pa) { h->pa = (double *)malloc(sizeof(double) * n * n); h->pe = (double *)malloc(sizeof(double) * 2 * n); h->pa0 = (double *)malloc(sizeof(double) * n); }
		if (!h->pa || !h->pe || !h->pa0) return PSMC_HIP_ENOMEM;
		memcpy(h->pa, a, sizeof(double) * n * n); memcpy(h->pe, e, sizeof(double) * 2 * n); memcpy(h->pa0, a0, sizeof(double) * n);
	}
	h->on_twin = 0; h->verr = 0;
	int rc;
	if (h->decoding && h->wide_decode) {
		/* the decoding E-step of the wide fast path: psmc_hip_estep would run the exact full-counts kernels beyond 128 states, and the
		 * decoding reads what the last single E-step left -- so the FACTORED wide E-step runs; decode_all reads neither A nor E */
		const size_t n = (size_t)h->n_states;
		double *sums = (double *)malloc(sizeof(double) * 5 * n);
		if (!sums) return PSMC_HIP_ENOMEM;
		memset(A, 0, sizeof(double) * n * n);
		rc = h->grp ? psmc_hip_group_estep_factored(h->grp, a, e, a0, sums, E, LL) : psmc_hip_estep_factored(h->ctx, a, e, a0, sums, E, LL);
		free(sums);
		say_note(h, 0);
		for (int i = 0; i < h->n_seg; ++i) h->chk[i] = 1.0; /* (fast mode has no underflow self-check) */
		if (rc == PSMC_HIP_ENOTSUP) { /* "structured" = 0, a matrix without the PSMC form (-C): nothing of the wide path to decode */
			fprintf(stderr, "psmc: the wide fast E-step cannot run (%s); repeating the decoding E-step with the exact kernels\n", hb_error(h));
			rc = exact_once(h, a, e, a0, A, E, LL, 1);
		} else if (rc == 0) { /* what that E-step kept ("wide_ckpt" + "wide_decode_ckpt" through PSMC_HIP_OPTIONS: checkpoints) */
			psmc_hip_ctx *c = h->ctx; int l; int64_t ti[4] = {0, 0, 0, 0};
			if ((!h->grp || psmc_hip_group_route(h->grp, 0, &c, &l) == 0) && psmc_hip_wide_table_info(c, ti) == 0 && ti[2] == 8)
				fprintf(stderr, "psmc: the decoding reads the wide fast tables (checkpoints: X at every 8th bin)\n");
		}
	} else {
		rc = h->grp ? psmc_hip_group_estep(h->grp, a, e, a0, A, E, 0, LL, h->chk) : psmc_hip_estep(h->ctx, a, e, a0, A, E, 0, LL, h->chk);
		say_note(h, rc == 0);
	}
	if (rc == PSMC_HIP_ECONVERGE && h->mode == PSMC_HIP_MODE_FAST) rc = exact_once(h, a, e, a0, A, E, LL, 0);
	if (rc) return rc;
	for (int i = 0; i < h->n_seg; ++i) { /* the diagnostic of khmm.c:239-240 */
		if (h->chk[i] > 1.0 + 1e-6 || h->chk[i] < 1.0 - 1e-6) fprintf(stderr, "++ Underflow may have happened (%lg).\n", h->chk[i]);
		if (chk) chk[i] = h->chk[i];
	}
	return 0;
}
static int hb_estep_factored(void *self, const double *a, const double *e, const double *a0, double *sums, double *E, double *LL)
{
	hip_be *h = (hip_be *)self;
	h->on_twin = 0;
	int rc = h->grp ? psmc_hip_group_estep_factored(h->grp, a, e, a0, sums, E, LL) : psmc_hip_estep_factored(h->ctx, a, e, a0, sums, E, LL);
	if (rc != PSMC_HIP_ENOTSUP && rc != PSMC_HIP_ECONVERGE) return rc;
	/* a matrix without the two rank-1 triangles (e.g. -C): full counts, triangular sums on the host; tile boundaries that
	 * did not converge: the exact kernels once (exact_once), sums of their A */
	const int n = h->n_states;
	double *A = (double *)calloc((size_t)n * n, sizeof(double));
	if (rc == PSMC_HIP_ECONVERGE) rc = exact_once(h, a, e, a0, A, E, LL, 0);
	else rc = hb_estep(self, a, e, a0, A, E, LL, 0);
	if (rc == 0) tri_sums(n, A, sums);
	free(A);
	return rc;
}
static int hb_tables(void *self, int seg, double *f, double *b, double *s)
{
	psmc_hip_ctx *c; int l; int rc = route((hip_be *)self, seg, &c, &l);
	return rc ? rc : psmc_hip_get_tables(c, l, f, b, s);
}
/* PSMC_HIP_DECODE=fast: the decoding E-step keeps the backward table (the fused and factored back halves never store it); on the
 * wide fast path (129..256 states, or 257..1024 with PSMC_HIP_WIDE=fast-all PSMC_HIP_DECODE=fast-all) it is a factored wide E-step (hb_estep) and the decoding reads its tables ("wide_decode") */
static int hb_prepare_decode(void *self)
{
	hip_be *h = (hip_be *)self;
	if (h->mode != PSMC_HIP_MODE_FAST) return 0;
	h->decoding = 1;
	if (h->wide) {
		const int rc = h->grp ? psmc_hip_group_set_option(h->grp, "wide_decode", 1) : psmc_hip_set_option(h->ctx, "wide_decode", 1);
		if (rc) return rc;
		h->wide_decode = 1;
	}
	int rc = h->grp ? psmc_hip_group_set_option(h->grp, "fuse", 0) : psmc_hip_set_option(h->ctx, "fuse", 0);
	if (rc == 0) rc = h->grp ? psmc_hip_group_set_option(h->grp, "fuse128", 0) : psmc_hip_set_option(h->ctx, "fuse128", 0);
	return rc;
}
/* a decoding call on the fast tables that answers PSMC_HIP_ENOTSUP (a plan whose forward table the kernels cannot read, e.g.
 * "merge" through PSMC_HIP_OPTIONS): the exact twin repeats the E-step with the same parameters and the call goes there */
static int hb_decoded(hip_be *h, int rc)
{
	if (rc != PSMC_HIP_ENOTSUP || h->on_twin || !h->decoding || !h->pa) return rc;
	const size_t n = (size_t)h->n_states;
	double *A = (double *)malloc(sizeof(double) * n * n), *E = (double *)malloc(sizeof(double) * 2 * n), LL;
	if (!A || !E) { free(A); free(E); return PSMC_HIP_ENOMEM; }
	fprintf(stderr, "psmc: the fast tables cannot be decoded (%s); repeating the decoding E-step with the exact kernels\n", hb_error(h));
	rc = exact_once(h, h->pa, h->pe, h->pa0, A, E, &LL, 1);
	free(A); free(E);
	return rc ? rc : -1000; /* -1000: call again, on the twin */
}
#define HB_DECODE_CALL(call) \
	hip_be *h = (hip_be *)self; \
	for (;;) { \
		psmc_hip_ctx *c; int l; int rc = route(h, seg, &c, &l); \
		if (rc == 0) rc = (call); \
		if ((rc = hb_decoded(h, rc)) != -1000) return rc; \
	}
static int hb_decode(void *self, int seg, int32_t *path, double *maxp) { HB_DECODE_CALL(psmc_hip_decode(c, l, path, maxp)) }
static int hb_posterior(void *self, int seg, double *post, double *recomb) { HB_DECODE_CALL(psmc_hip_posterior(c, l, post, recomb)) }
static int hb_post_counts(void *self, int seg, const int32_t *cnt1, int32_t l1, int32_t n_cnt, double *cnt) { HB_DECODE_CALL(psmc_hip_post_counts(c, l, cnt1, l1, n_cnt, cnt)) }
static int hb_scales(void *self, int seg, double *s) { HB_DECODE_CALL(psmc_hip_scales(c, l, s)) }
static int hb_post_mean(void *self, int seg, const double *w, int32_t n_w, double *mean) { HB_DECODE_CALL(psmc_hip_post_mean(c, l, w, n_w, mean)) }
static int hb_post_quantile(void *self, int seg, const double *q, int32_t n_q, int32_t *state) { HB_DECODE_CALL(psmc_hip_post_quantile(c, l, q, n_q, state)) }
#undef HB_DECODE_CALL
/* The Viterbi path of all segments in input order.  One context: psmc_hip_viterbi as it is.  A group: one call per shard context
 * (psmc_hip_group_route names every segment's context and its index there), the shard's results scattered to input order.  The call
 * reads observations only, so it goes to the run's own contexts whatever the exact twin holds. */
static int hb_viterbi(void *self, const double *a, const double *e, const double *a0, int32_t *path, double *score)
{
	hip_be *h = (hip_be *)self;
	h->verr = 0;
	if (!h->grp) return psmc_hip_viterbi(h->ctx, a, e, a0, path, score);
	const int n = h->n_seg;
	psmc_hip_ctx **cx = (psmc_hip_ctx **)malloc(sizeof(void *) * (size_t)n);
	int *loc = (int *)malloc(sizeof(int) * (size_t)n), *glob = (int *)malloc(sizeof(int) * (size_t)n);
	int64_t *off = (int64_t *)malloc(sizeof(int64_t) * ((size_t)n + 1));
	int32_t *sp = 0; double *ss = 0;
	int rc = cx && loc && glob && off ? 0 : PSMC_HIP_ENOMEM;
	if (rc == 0) off[0] = 0;
	for (int i = 0; rc == 0 && i < n; ++i) {
		off[i + 1] = off[i] + h->L[i];
		rc = psmc_hip_group_route(h->grp, i, &cx[i], &loc[i]);
	}
	for (int i = 0; rc == 0 && i < n; ++i) {
		int seen = 0, m = 0;
		int64_t bins = 0;
		for (int j = 0; j < i && !seen; ++j) seen = cx[j] == cx[i];
		if (seen) continue;
		for (int j = i; j < n; ++j) /* the shard's segments by their index there: 0 .. m-1 */
			if (cx[j] == cx[i]) { ++m; bins += h->L[j]; }
		for (int j = i; j < n; ++j)
			if (cx[j] == cx[i]) { if (loc[j] < 0 || loc[j] >= m) rc = PSMC_HIP_EINVAL; else glob[loc[j]] = j; }
		if (rc) break;
		sp = (int32_t *)realloc(sp, sizeof(int32_t) * (size_t)bins); ss = (double *)realloc(ss, sizeof(double) * (size_t)m);
		if (!sp || !ss) { rc = PSMC_HIP_ENOMEM; break; }
		rc = psmc_hip_viterbi(cx[i], a, e, a0, path ? sp : 0, score ? ss : 0);
		if (rc) { snprintf(h->msg, sizeof h->msg, "%s (a shard's index; its first segment is segment %d of the input)", psmc_hip_last_error(cx[i]), glob[0]); h->verr = h->msg; break; }
		int64_t so = 0;
		for (int l = 0; l < m; so += h->L[glob[l]], ++l) {
			if (path) memcpy(path + off[glob[l]], sp + so, sizeof(int32_t) * (size_t)h->L[glob[l]]);
			if (score) score[glob[l]] = ss[l];
		}
	}
	free(cx); free(loc); free(glob); free(off); free(sp); free(ss);
	return rc;
}
/* State paths drawn from the posterior, all segments in input order.  One context: psmc_hip_sample_paths as it is.  A group: one call
 * per shard context with the shard's segments' INPUT indices (or the caller's ids of them) as stream ids -- the samples do not depend
 * on how the input is dealt out -- scattered to input order as hb_viterbi does. */
static int hb_sample_paths(void *self, const double *a, const double *e, const double *a0, uint64_t seed, int32_t n_samp, const uint64_t *stream,
                           int32_t *path)
{
	hip_be *h = (hip_be *)self;
	h->verr = 0;
	if (!h->grp) return psmc_hip_sample_paths(h->ctx, a, e, a0, seed, n_samp, stream, path);
	if (n_samp < 1 || !path) return PSMC_HIP_EINVAL;
	const int n = h->n_seg;
	psmc_hip_ctx **cx = (psmc_hip_ctx **)malloc(sizeof(void *) * (size_t)n);
	int *loc = (int *)malloc(sizeof(int) * (size_t)n), *glob = (int *)malloc(sizeof(int) * (size_t)n);
	int64_t *off = (int64_t *)malloc(sizeof(int64_t) * ((size_t)n + 1));
	uint64_t *sid = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)n);
	int32_t *sp = 0;
	int rc = cx && loc && glob && off && sid ? 0 : PSMC_HIP_ENOMEM;
	if (rc == 0) off[0] = 0;
	for (int i = 0; rc == 0 && i < n; ++i) {
		off[i + 1] = off[i] + h->L[i];
		rc = psmc_hip_group_route(h->grp, i, &cx[i], &loc[i]);
	}
	for (int i = 0; rc == 0 && i < n; ++i) {
		int seen = 0, m = 0;
		int64_t bins = 0;
		for (int j = 0; j < i && !seen; ++j) seen = cx[j] == cx[i];
		if (seen) continue;
		for (int j = i; j < n; ++j) /* the shard's segments by their index there: 0 .. m-1 */
			if (cx[j] == cx[i]) { ++m; bins += h->L[j]; }
		for (int j = i; j < n; ++j)
			if (cx[j] == cx[i]) { if (loc[j] < 0 || loc[j] >= m) rc = PSMC_HIP_EINVAL; else glob[loc[j]] = j; }
		if (rc) break;
		for (int l = 0; l < m; ++l) sid[l] = stream ? stream[glob[l]] : (uint64_t)glob[l];
		sp = (int32_t *)realloc(sp, sizeof(int32_t) * (size_t)bins * (size_t)n_samp);
		if (!sp) { rc = PSMC_HIP_ENOMEM; break; }
		rc = psmc_hip_sample_paths(cx[i], a, e, a0, seed, n_samp, sid, sp);
		if (rc) { snprintf(h->msg, sizeof h->msg, "%s (a shard; its first segment is segment %d of the input)", psmc_hip_last_error(cx[i]), glob[0]); h->verr = h->msg; break; }
		for (int32_t j = 0; j < n_samp; ++j) {
			int64_t so = 0;
			for (int l = 0; l < m; so += h->L[glob[l]], ++l)
				memcpy(path + (size_t)j * off[n] + off[glob[l]], sp + (size_t)j * bins + so, sizeof(int32_t) * (size_t)h->L[glob[l]]);
		}
	}
	free(cx); free(loc); free(glob); free(off); free(sid); free(sp);
	return rc;
}
static void hb_destroy(void *self)
{
	hip_be *h = (hip_be *)self;
	say_note(h, 0); /* (no E-step ran) */
	if (h->x_ctx) psmc_hip_destroy(h->x_ctx);
	if (h->x_grp) psmc_hip_group_destroy(h->x_grp);
	if (h->grp) psmc_hip_group_destroy(h->grp); else psmc_hip_destroy(h->ctx);
	free(h->chk); free((void *)h->sym); free(h->L); free(h->devs); free(h->pa); free(h->pe); free(h->pa0); free(h);
}


int psmc_hipbe_create(psmc_estep_backend *be, int n_states, int mode, int use_factored, const char *devs, int device)
{
	hip_be *h = (hip_be *)calloc(1, sizeof(hip_be));
	int rc;
	memset(be, 0, sizeof *be);
	if (!h) return PSMC_HIP_ENOMEM;
	h->n_states = n_states; h->mode = mode;
	h->device = devs && *devs && !strchr(devs, ',') ? atoi(devs) : device;
	h->devs = devs ? strdup(devs) : 0;
	if (devs && strchr(devs, ',')) { /* several devices: shard every E-step */
		int list[64], n_list = 0;
		char *dup = strdup(devs);
		for (char *t = strtok(dup, ","); t && n_list < 64; t = strtok(0, ",")) list[n_list++] = atoi(t);
		free(dup);
		rc = psmc_hip_group_create(&h->grp, n_states, n_list, list, mode);
		const char *rc_s = getenv("PSMC_HIP_RCCL");
		if (rc == 0 && rc_s) rc = psmc_hip_group_set_option(h->grp, "rccl", atof(rc_s));
		if (rc == 0) {
			/* first contact with the devices, before a segment is loaded: every listed device answers, the exchange the
			 * E-steps will use comes up and adds correctly in stream order -- a failure names its step here, not in the first E-step */
			int sc[4] = {0, 0, 0, 0};
			static const char *path[] = {"single shard", "RCCL all-reduce", "host sum of the shards' vectors", "exact mode: ordered per-segment sum, nothing to exchange"};
			rc = psmc_hip_group_selfcheck(h->grp, sc);
			if (rc) fprintf(stderr, "psmc: devices %s: self-check failed: %s\n", devs, psmc_hip_group_last_error(h->grp));
			else {
				if (sc[3]) fprintf(stderr, "psmc: devices %s: RCCL wanted but not usable (%s); the host adds the shards' vectors\n", devs, psmc_hip_group_last_error(h->grp));
				if (getenv("PSMC_TIMING")) fprintf(stderr, "[timing] devices %s: self-check ok, %d shards, exchange: %s%s\n", devs, sc[0], path[sc[1] >= 0 && sc[1] <= 3 ? sc[1] : 0], sc[2] ? " (communicator up)" : "");
			}
		}
	} else rc = psmc_hip_create(&h->ctx, n_states, devs && *devs ? atoi(devs) : device, mode);
	if (rc) { if (h->grp) psmc_hip_group_destroy(h->grp); free(h->devs); free(h); return rc; }
	be->self = h; be->load = hb_load; be->estep = hb_estep; be->tables = hb_tables; be->decode = hb_decode;
	be->estep_factored = use_factored ? hb_estep_factored : 0; be->error = hb_error; be->destroy = hb_destroy;
	be->posterior = hb_posterior; be->post_counts = hb_post_counts; be->prepare_decode = hb_prepare_decode; be->scales = hb_scales;
	be->post_mean = hb_post_mean; be->post_quantile = hb_post_quantile; be->viterbi = hb_viterbi; be->sample_paths = hb_sample_paths;
	return 0;
}

int psmc_hipbe_set_option(psmc_estep_backend *be, const char *key, double value)
{
	hip_be *h = (hip_be *)be->self;
	if (strcmp(key, "wide_fast") == 0) h->wide = value != 0;
	return h->grp ? psmc_hip_group_set_option(h->grp, key, value) : psmc_hip_set_option(h->ctx, key, value);
}

void psmc_hipbe_note_counts(psmc_estep_backend *be, const char *line)
{
	hip_be *h = (hip_be *)be->self;
	free(h->note);
	h->note = strdup(line);
}

psmc_hip_ctx *psmc_hipbe_ctx(psmc_estep_backend *be) { return be && be->self ? ((hip_be *)be->self)->ctx : 0; }
