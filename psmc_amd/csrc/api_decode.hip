// api_decode.hip -- the decoding entry points psmc_hip_decode / _posterior / _post_counts / _scales / _post_mean / _post_quantile: one
// segment of the last single E-step, from whichever tables that E-step left (decode_source):
//   DEC_EXACT  f, b and s of the exact kernels (estep_exact.hip, estep_wide.hip beyond 128 states; _post_mean: estep_post_mean.hip;
//              _post_quantile: estep_post_quantile.hip)
//   DEC_FAST   X and bt of a fast E-step with the unfused back half, up to 128 states (estep_post_fast.hip)
//   DEC_WIDE   X, 1/d, entry and bentry of a wide fast E-step with "wide_decode": 129..256 states (estep_wide_post.hip), and
//              257..1024 states with "wide_fast" = 2 (the same file; the tables are 512, 768 or 1024 states wide).  After a
//              checkpointed E-step ("wide_ckpt") with "wide_decode_ckpt" = 1: its checkpoints and the tiles' last rows instead of X
//              (the CKPT kernels of the same files; nothing of the table's size is allocated)
// Every entry point is written once: argument check, decode_source, device scratch of its own (freed before it returns), uploads, a
// switch on the source that holds nothing but the launch, downloads, one synchronise, one error mapping.
#include "psmc_hip_ctx.h"
#include "wide_fast.h"

// Which tables the decoding entry points of context c read, and for the fast ones the segment's tiles in the plan of the E-step
// that wrote them: first_tile, and n_tiles of them.  Returns DEC_EXACT (exact mode; the exact fallback of a fast E-step; beyond
// 128 states unless "wide_fast" + "wide_decode" are on -- beyond 256 states "wide_fast" = 2 -- and the last single E-step was a
// wide fast one), DEC_FAST, DEC_WIDE, or a PSMC_HIP_E* code (message set).  Reads nothing but the context.
static int decode_source(psmc_hip_ctx *c, int seg, const char *who, int *first_tile, int *n_tiles)
{
	if (c->mode == PSMC_HIP_MODE_EXACT) return DEC_EXACT;
	const bool wide = c->ns > 128;
	char msg[256];
	if (wide) {
		if (!c->wide_fast || !c->wide_decode || (c->n > 256 && c->wide_fast < 2) || c->wd_kind == WD_NONE || c->wd_serial != c->tab_serial) return DEC_EXACT;
		if (c->wd_kind != WD_OK) {
			snprintf(msg, sizeof msg, "%s: the last wide fast E-step returned an error (no converged tile boundaries to decode from)", who);
			return fail(c, PSMC_HIP_ESTATE, msg);
		}
		// a checkpointed E-step ("wide_ckpt"): the CKPT decoding kernels read its checkpoints when "wide_decode_ckpt" is on NOW;
		// without it the decoding kernels read full X rows, which that E-step did not keep
		if (c->wf_last_iv != 1 && !(c->wf_last_iv == 8 && c->wide_decode_ckpt)) {
			snprintf(msg, sizeof msg, "%s: the last wide E-step kept checkpoints only (\"wide_ckpt\": X at every 8th bin); run an E-step with \"wide_decode\" = 1 first, or set \"wide_decode_ckpt\" = 1", who);
			return fail(c, PSMC_HIP_ESTATE, msg);
		}
		if (c->wd_sel != c->sel_serial) {
			snprintf(msg, sizeof msg, "%s: the selection changed since the last E-step", who);
			return fail(c, PSMC_HIP_ESTATE, msg);
		}
	} else {
		if (!c->d_f || c->tables_batch || c->dec_kind == DEC_NONE || c->dec_serial != c->tab_serial) {
			snprintf(msg, sizeof msg, "%s: no single E-step yet", who);
			return fail(c, PSMC_HIP_ESTATE, msg);
		}
		if (c->dec_kind == DEC_EXACT) return DEC_EXACT;
		if (c->dec_kind == DEC_MERGED) {
			snprintf(msg, sizeof msg, "%s: not after an E-step with the forward fix pass (merge=1: its forward table carries per-tile factors)", who);
			return fail(c, PSMC_HIP_ENOTSUP, msg);
		}
		if (c->dec_kind != DEC_FAST || !c->have_b) {
			snprintf(msg, sizeof msg, "%s: the last fast E-step kept no backward table (fused or factored back half); run it with fuse=0 (<= 64 states) / fuse128=0 (65..128)", who);
			return fail(c, PSMC_HIP_ESTATE, msg);
		}
	}
	// the segment's tiles are consecutive in either plan (a segment selected several times is in it once, with its multiplicity)
	const int nc = (int)(wide ? c->wf_chunks.size() : c->chunks.size());
	auto of_seg = [&](int t) { return wide ? c->wf_chunks[t].off == c->off[seg] : c->chunk_seg[t] == seg; };
	for (int t = 0; t < nc; ++t)
		if (of_seg(t)) {
			int e = t;
			while (e < nc && of_seg(e)) ++e;
			*first_tile = t; *n_tiles = e - t;
			return wide ? DEC_WIDE : DEC_FAST;
		}
	snprintf(msg, sizeof msg, "%s: segment %d was not in the selection of the last E-step", who, seg);
	return fail(c, PSMC_HIP_ESTATE, msg);
}

// the parameter block's pieces the fast decoding kernels read (fill_params / fill_common)
static const double *par_e(const psmc_hip_ctx *c) { return c->ns == 128 ? c->d_par + 32768 : c->d_par + 4 * 4096; }
static const double *par_a0(const psmc_hip_ctx *c) { return par_e(c) + 3 * c->ns; }
static const double *par_re(const psmc_hip_ctx *c) { return c->ns == 128 ? c->d_par + psmc_hip_ctx::RE128_OFF : c->d_par + 4 * 4096 + 192 + 64; }

// what every wide decoding launch reads: X, 1/d, entry, bentry, the parameter block and the plan of the last wide fast E-step
static void wide_post_common(const psmc_hip_ctx *c, WidePost &w, int what, int t0, int nt)
{
	memset(&w, 0, sizeof(w));
	w.stream = c->stream; w.what = what; w.ns = wf_width(c); w.waves = wf_waves(c); w.n_states = c->n; w.t0 = t0; w.n_tiles = nt;
	w.par = c->d_wf_par; w.obs = c->d_obs; w.chunks = c->d_wf_chunks;
	w.X = c->d_wf_X; w.inv = c->d_wf_inv; w.entry = c->d_wf_entry; w.bentry = c->d_wf_bentry;
	w.ckpt = c->wf_last_iv; w.xhi = c->wf_last_iv == 8 ? c->d_wf_xhi : nullptr; // (8: decode_source let it through, "wide_decode_ckpt")
}

extern "C" int psmc_hip_decode(psmc_hip_ctx *c, int seg, int32_t *path, double *maxp)
{
	if (!c || seg < 0 || seg >= c->n_seg || !path) return fail(c, PSMC_HIP_EINVAL, "decode: bad argument");
	int t0 = 0, nt = 0;
	const int src = decode_source(c, seg, "decode", &t0, &nt);
	if (src < 0) return src;
	if (src == DEC_EXACT && (!c->d_f || !c->have_b || c->tables_batch)) return fail(c, PSMC_HIP_ESTATE, "decode: no single E-step yet");
	HIPCHK(c, hipSetDevice(c->device));
	const int L = c->L[seg];
	Scratch sc;
	int32_t *dp = sc.get<int32_t>((size_t)L);
	double *dm = sc.get<double>((size_t)L);
	if (!sc.ok) return fail(c, PSMC_HIP_ENOMEM, "hipMalloc");
	int rc;
	switch (src) {
	case DEC_WIDE: {
		WidePost w;
		wide_post_common(c, w, WP_PATH, t0, nt);
		w.path = dp; w.maxp = dm;
		rc = launch_wide_post(w);
		break;
	}
	case DEC_FAST:
		rc = launch_post_fast(c->stream, c->d_f, c->d_b, c->d_sb, par_re(c), c->d_par, c->d_obs, c->off[seg], L, c->n, c->ns, nullptr, nullptr, dp, dm);
		break;
	default:
		rc = c->ns > 128 ? launch_post_decode_wide(c->stream, c->d_f, c->d_b, c->d_s, c->off[seg], L, c->n, c->ns, dp, dm)
		                 : launch_post_decode(c->stream, c->d_f, c->d_b, c->d_s, c->off[seg], L, c->n, c->ns, dp, dm);
	}
	hipError_t e1 = hipMemcpyAsync(path, dp, sizeof(int32_t) * (size_t)L, hipMemcpyDeviceToHost, c->stream);
	hipError_t e2 = maxp ? hipMemcpyAsync(maxp, dm, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
	hipError_t e3 = hipStreamSynchronize(c->stream);
	if (rc || e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess)
		return fail(c, PSMC_HIP_EDEVICE, src == DEC_WIDE ? "decode (wide fast tables)" : "decode");
	return PSMC_HIP_OK;
}

extern "C" int psmc_hip_posterior(psmc_hip_ctx *c, int seg, double *post, double *recomb)
{
	if (!c || seg < 0 || seg >= c->n_seg || (!post && !recomb)) return fail(c, PSMC_HIP_EINVAL, "posterior: bad argument");
	int t0 = 0, nt = 0;
	const int src = decode_source(c, seg, "posterior", &t0, &nt);
	if (src < 0) return src;
	if (src == DEC_EXACT && (!c->d_f || !c->have_b || c->tables_batch)) return fail(c, PSMC_HIP_ESTATE, "posterior: no single E-step yet");
	HIPCHK(c, hipSetDevice(c->device));
	const int L = c->L[seg], n = c->n;
	Scratch sc;
	double *dp = post ? sc.get<double>((size_t)L * n) : nullptr;
	double *dr = recomb ? sc.get<double>((size_t)L) : nullptr;
	if (!sc.ok) return fail(c, PSMC_HIP_ENOMEM, "hipMalloc");
	int rc;
	switch (src) {
	case DEC_WIDE: {
		WidePost w;
		wide_post_common(c, w, post ? (recomb ? WP_POST_REC : WP_POST) : WP_REC, t0, nt);
		w.post = dp; w.recomb = dr;
		rc = launch_wide_post(w);
		break;
	}
	case DEC_FAST:
		rc = launch_post_fast(c->stream, c->d_f, c->d_b, c->d_sb, par_re(c), c->d_par, c->d_obs, c->off[seg], L, n, c->ns, dp, dr, nullptr, nullptr);
		break;
	default: { // the emission rows of the exact parameter block: after a | aT beyond 128 states (estep_wide.hip), else as par_e
		const double *d_e = c->ns > 128 ? c->d_par + 2 * (size_t)c->ns * c->ns : par_e(c);
		rc = c->ns > 128 ? launch_post_full_wide(c->stream, c->d_par, d_e, c->d_obs, c->d_f, c->d_b, c->d_s, c->off[seg], L, n, c->ns, dp, dr)
		                 : launch_post_full(c->stream, c->d_par, d_e, c->d_obs, c->d_f, c->d_b, c->d_s, c->off[seg], L, n, c->ns, dp, dr);
	}
	}
	hipError_t e1 = post ? hipMemcpyAsync(post, dp, sizeof(double) * (size_t)L * n, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
	hipError_t e2 = recomb ? hipMemcpyAsync(recomb, dr, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
	hipError_t e3 = hipStreamSynchronize(c->stream);
	if (rc || e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess)
		return fail(c, PSMC_HIP_EDEVICE, src == DEC_WIDE ? "posterior (wide fast tables)" : "posterior");
	return PSMC_HIP_OK;
}

extern "C" int psmc_hip_post_counts(psmc_hip_ctx *c, int seg, const int32_t *cnt1, int32_t l, int32_t n_cnt, double *cnt)
{
	if (!c || seg < 0 || seg >= c->n_seg || !cnt || l < 0 || n_cnt < 1 || (l > 0 && !cnt1)) return fail(c, PSMC_HIP_EINVAL, "post_counts: bad argument");
	int t0 = 0, nt = 0;
	const int src = decode_source(c, seg, "post_counts", &t0, &nt);
	if (src < 0) return src;
	if (src == DEC_EXACT && (!c->d_f || !c->have_b || c->tables_batch)) return fail(c, PSMC_HIP_ESTATE, "post_counts: no single E-step yet");
	HIPCHK(c, hipSetDevice(c->device));
	const int L = c->L[seg], n = c->n, min_l = L < l ? L : l;
	if (min_l == 0) return PSMC_HIP_OK;
	// per-block (fast) or per-tile (wide) partial counts, n_cnt x the tables' padded width doubles each; the exact kernels need none
	const size_t n_part = src == DEC_FAST ? (size_t)post_counts_fast_blocks(min_l) * n_cnt * c->ns : (size_t)nt * n_cnt * wf_width(c);
	Scratch sc;
	int32_t *d1 = sc.get<int32_t>((size_t)min_l * n_cnt);
	double *dc = sc.get<double>((size_t)n * n_cnt);
	double *dpart = src == DEC_EXACT ? nullptr : sc.get<double>(n_part);
	if (!sc.ok) return fail(c, PSMC_HIP_ENOMEM, "hipMalloc");
	hipError_t e0 = hipMemcpyAsync(d1, cnt1, sizeof(int32_t) * (size_t)min_l * n_cnt, hipMemcpyHostToDevice, c->stream);
	hipError_t e1 = hipMemcpyAsync(dc, cnt, sizeof(double) * (size_t)n * n_cnt, hipMemcpyHostToDevice, c->stream);
	int rc;
	switch (src) {
	case DEC_WIDE: {
		WidePost w;
		wide_post_common(c, w, WP_COUNTS, t0, nt);
		w.cnt1 = d1; w.n_cnt = n_cnt; w.min_l = min_l; w.part = dpart; w.cnt = dc;
		rc = launch_wide_post(w);
		break;
	}
	case DEC_FAST:
		rc = launch_post_counts_fast(c->stream, c->d_f, c->d_b, par_re(c), c->d_obs, c->off[seg], L, min_l, d1, n_cnt, n, c->ns, dpart, dc);
		break;
	default:
		rc = c->ns > 128 ? launch_post_counts_wide(c->stream, c->d_f, c->d_b, c->d_s, c->off[seg], min_l, d1, n_cnt, n, c->ns, dc)
		                 : launch_post_counts(c->stream, c->d_f, c->d_b, c->d_s, c->off[seg], min_l, d1, n_cnt, n, c->ns, dc);
	}
	hipError_t e2 = hipMemcpyAsync(cnt, dc, sizeof(double) * (size_t)n * n_cnt, hipMemcpyDeviceToHost, c->stream);
	hipError_t e3 = hipStreamSynchronize(c->stream);
	if (rc || e0 != hipSuccess || e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess)
		return fail(c, PSMC_HIP_EDEVICE, src == DEC_WIDE ? "post_counts (wide fast tables)" : "post_counts");
	return PSMC_HIP_OK;
}

static_assert(MEAN_COLS == PSMC_HIP_MAX_MEAN_COLS, "the kernels' column count is the header's");

extern "C" int psmc_hip_post_mean(psmc_hip_ctx *c, int seg, const double *w, int32_t n_w, double *mean)
{
	if (!c || seg < 0 || seg >= c->n_seg || !w || !mean || n_w < 1 || n_w > PSMC_HIP_MAX_MEAN_COLS) return fail(c, PSMC_HIP_EINVAL, "post_mean: bad argument");
	int t0 = 0, nt = 0;
	const int src = decode_source(c, seg, "post_mean", &t0, &nt);
	if (src < 0) return src;
	if (src == DEC_EXACT && (!c->d_f || !c->have_b || c->tables_batch)) return fail(c, PSMC_HIP_ESTATE, "post_mean: no single E-step yet");
	HIPCHK(c, hipSetDevice(c->device));
	const int L = c->L[seg], n = c->n;
	// the weights at the tables' padded width, zeros beyond the n states
	const int ws = src == DEC_WIDE ? wf_width(c) : c->ns;
	std::vector<double> hw((size_t)n_w * ws, 0.0);
	for (int j = 0; j < n_w; ++j) memcpy(hw.data() + (size_t)j * ws, w + (size_t)j * n, sizeof(double) * (size_t)n);
	Scratch sc;
	double *dw = sc.get<double>(hw.size());
	double *dm = sc.get<double>((size_t)L * n_w);
	if (!sc.ok) return fail(c, PSMC_HIP_ENOMEM, "hipMalloc");
	hipError_t e0 = hipMemcpyAsync(dw, hw.data(), sizeof(double) * hw.size(), hipMemcpyHostToDevice, c->stream);
	int rc;
	switch (src) {
	case DEC_WIDE: {
		WidePost wp;
		wide_post_common(c, wp, WP_MEAN, t0, nt);
		wp.wts = dw; wp.n_w = n_w; wp.mean = dm;
		rc = launch_wide_post(wp);
		break;
	}
	case DEC_FAST:
		rc = launch_post_mean_fast(c->stream, c->d_f, c->d_b, par_re(c), c->d_obs, c->off[seg], L, c->ns, dw, n_w, dm);
		break;
	default:
		rc = launch_post_mean_exact(c->stream, c->d_f, c->d_b, c->d_s, c->off[seg], L, n, c->ns, dw, n_w, dm);
	}
	hipError_t e1 = hipMemcpyAsync(mean, dm, sizeof(double) * (size_t)L * n_w, hipMemcpyDeviceToHost, c->stream);
	hipError_t e2 = hipStreamSynchronize(c->stream); // (hw lives until here: the upload has been consumed)
	if (rc || e0 != hipSuccess || e1 != hipSuccess || e2 != hipSuccess)
		return fail(c, PSMC_HIP_EDEVICE, src == DEC_WIDE ? "post_mean (wide fast tables)" : "post_mean");
	return PSMC_HIP_OK;
}

static_assert(QUANT_COLS == PSMC_HIP_MAX_QUANT_COLS, "the kernels' column count is the header's");

extern "C" int psmc_hip_post_quantile(psmc_hip_ctx *c, int seg, const double *q, int32_t n_q, int32_t *state)
{
	if (!c || seg < 0 || seg >= c->n_seg || !q || !state || n_q < 1 || n_q > PSMC_HIP_MAX_QUANT_COLS) return fail(c, PSMC_HIP_EINVAL, "post_quantile: bad argument");
	QuantQ qq = {};
	for (int j = 0; j < n_q; ++j) {
		if (!(q[j] >= 0.0 && q[j] <= 1.0)) return fail(c, PSMC_HIP_EINVAL, "post_quantile: every q must lie in [0, 1]"); // (a NaN fails both)
		qq.q[j] = q[j];
	}
	int t0 = 0, nt = 0;
	const int src = decode_source(c, seg, "post_quantile", &t0, &nt);
	if (src < 0) return src;
	if (src == DEC_EXACT && (!c->d_f || !c->have_b || c->tables_batch)) return fail(c, PSMC_HIP_ESTATE, "post_quantile: no single E-step yet");
	HIPCHK(c, hipSetDevice(c->device));
	const int L = c->L[seg], n = c->n;
	Scratch sc;
	int32_t *dq = sc.get<int32_t>((size_t)L * n_q);
	if (!sc.ok) return fail(c, PSMC_HIP_ENOMEM, "hipMalloc");
	int rc; // (nothing to upload: the thresholds travel with the launch)
	switch (src) {
	case DEC_WIDE: {
		WidePost wp;
		wide_post_common(c, wp, WP_QUANT, t0, nt);
		wp.q = qq; wp.n_q = n_q; wp.qstate = dq;
		rc = launch_wide_post(wp);
		break;
	}
	case DEC_FAST:
		rc = launch_post_quantile_fast(c->stream, c->d_f, c->d_b, par_re(c), c->d_obs, c->off[seg], L, n, c->ns, qq, n_q, dq);
		break;
	default:
		rc = launch_post_quantile_exact(c->stream, c->d_f, c->d_b, c->d_s, c->off[seg], L, n, c->ns, qq, n_q, dq);
	}
	hipError_t e1 = hipMemcpyAsync(state, dq, sizeof(int32_t) * (size_t)L * n_q, hipMemcpyDeviceToHost, c->stream);
	hipError_t e2 = hipStreamSynchronize(c->stream);
	if (rc || e1 != hipSuccess || e2 != hipSuccess)
		return fail(c, PSMC_HIP_EDEVICE, src == DEC_WIDE ? "post_quantile (wide fast tables)" : "post_quantile");
	return PSMC_HIP_OK;
}

extern "C" int psmc_hip_scales(psmc_hip_ctx *c, int seg, double *s)
{
	if (!c || seg < 0 || seg >= c->n_seg || !s) return fail(c, PSMC_HIP_EINVAL, "scales: bad argument");
	int t0 = 0, nt = 0;
	const int src = decode_source(c, seg, "scales", &t0, &nt);
	if (src < 0) return src;
	if (src != DEC_WIDE && (!c->d_f || c->tables_batch)) return fail(c, PSMC_HIP_ESTATE, "scales: no single E-step yet");
	HIPCHK(c, hipSetDevice(c->device));
	const int L = c->L[seg];
	if (src == DEC_EXACT) { // the exact tables hold s itself (the same doubles psmc_hip_get_tables returns): no kernel, no scratch
		HIPCHK(c, hipMemcpy(s, c->d_s + c->off[seg], sizeof(double) * (size_t)L, hipMemcpyDeviceToHost));
		return PSMC_HIP_OK;
	}
	Scratch sc;
	double *ds = sc.get<double>((size_t)L);
	if (!sc.ok) return fail(c, PSMC_HIP_ENOMEM, "hipMalloc");
	int rc;
	switch (src) {
	case DEC_WIDE: {
		WidePost w;
		wide_post_common(c, w, WP_SCALES, t0, nt);
		w.s = ds;
		rc = launch_wide_post(w);
		break;
	}
	default:
		rc = launch_scales_fast(c->stream, c->d_f, c->d_s, c->d_entry, par_a0(c), par_e(c), c->d_obs, c->off[seg], L, c->chunk_used, t0, c->ns, ds);
	}
	hipError_t e1 = hipMemcpyAsync(s, ds, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost, c->stream);
	hipError_t e2 = hipStreamSynchronize(c->stream);
	if (rc || e1 != hipSuccess || e2 != hipSuccess)
		return fail(c, PSMC_HIP_EDEVICE, src == DEC_WIDE ? "scales (wide fast tables)" : "scales");
	return PSMC_HIP_OK;
}
