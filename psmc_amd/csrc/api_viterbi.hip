// api_viterbi.hip -- psmc_hip_viterbi: the jointly most probable state path of every loaded segment (khmm.c:83-141) on the kernels of
// estep_viterbi.hip.  It reads the context's observations and nothing else of it: no table, plan, selection or learned state is
// touched, in either mode, and the device memory of the call is released before it returns.
#include "psmc_hip_ctx.h"

// What psmc_hip_viterbi and psmc_hip_sample_paths (api_sample.hip) plan on the host: the segments longest first, rows and path entries
// in load order, and -- when a path is wanted -- the tiles of the backtrace.  `who` names the caller in the one refusal.
int path_plan(psmc_hip_ctx *c, const char *who, bool want_path, PathPlan &pl)
{
	const int n_seg = c->n_seg, T = c->vit_tile;
	std::vector<int64_t> row_off(n_seg);
	pl.bins = 0;
	for (int i = 0; i < n_seg; ++i) { row_off[i] = pl.bins; pl.bins += c->L[i]; }
	pl.segs.resize(n_seg);
	for (int i = 0; i < n_seg; ++i) pl.segs[i] = VitSeg{c->off[i], row_off[i], c->L[i], i};
	std::stable_sort(pl.segs.begin(), pl.segs.end(), [](const VitSeg &x, const VitSeg &y) { return x.L > y.L; });
	pl.tiles.clear();
	pl.seg_tile.assign((size_t)2 * n_seg, 0);
	if (!want_path) return 0;
	int64_t n_tiles = 0;
	for (int i = 0; i < n_seg; ++i) n_tiles += (c->L[i] + T - 1) / T;
	if (n_tiles > 0x7fffffff) {
		char msg[128];
		snprintf(msg, sizeof msg, "%s: more than 2^31 backtrace tiles (\"vit_tile\" is too small for this input)", who);
		return fail(c, PSMC_HIP_EINVAL, msg);
	}
	pl.tiles.reserve((size_t)n_tiles);
	for (int i = 0; i < n_seg; ++i) {
		pl.seg_tile[i] = (int32_t)pl.tiles.size();
		for (int lo = 1; lo <= c->L[i]; lo += T) pl.tiles.push_back(VitTile{row_off[i], lo, std::min(c->L[i], lo + T - 1)});
		pl.seg_tile[n_seg + i] = (int32_t)pl.tiles.size() - pl.seg_tile[i];
	}
	return 0;
}

// The parameters of those two calls, padded to S states: f(a) [S][S] | f(e) [3][S], the missing symbol's row `miss` | f(a0) [S], `pad`
// in the padding.  One call of f per entry, in this order.
std::vector<double> path_params(int n, int S, const double *a, const double *e, const double *a0, double (*f)(double), double pad, double miss)
{
	std::vector<double> tab((size_t)S * S + 4 * (size_t)S, pad);
	double *pa = tab.data(), *pe = pa + (size_t)S * S, *p0 = pe + 3 * (size_t)S;
	for (int l = 0; l < n; ++l)
		for (int k = 0; k < n; ++k) pa[(size_t)l * S + k] = f(a[(size_t)l * n + k]);
	for (int k = 0; k < n; ++k) {
		pe[k] = f(e[k]);
		pe[S + k] = f(e[n + k]);
		pe[2 * S + k] = miss;
		p0[k] = f(a0[k]);
	}
	return tab;
}

extern "C" int psmc_hip_viterbi(psmc_hip_ctx *c, const double *a, const double *e, const double *a0, int32_t *path, double *score)
{
	if (!c) return PSMC_HIP_EINVAL;
	if (!a || !e || !a0) return fail(c, PSMC_HIP_EINVAL, "viterbi: null parameters");
	if (!path && !score) return fail(c, PSMC_HIP_EINVAL, "viterbi: neither a path nor a score is asked for");
	if (c->n_seg < 1 || !c->d_obs) return fail(c, PSMC_HIP_ESTATE, "viterbi: no segments loaded");
	HIPCHK(c, hipSetDevice(c->device));
	const int n = c->n, S = 64 * ((n + 63) / 64), n_seg = c->n_seg, T = c->vit_tile;
	const bool wide_bp = S > 256;
	char msg[256];

	// the log tables: one libm log() per entry, -inf in the padding
	const std::vector<double> tab = path_params(n, S, a, e, a0, log, -HUGE_VAL, 0.0);
	PathPlan pl;
	if (int rc = path_plan(c, "viterbi", path != nullptr, pl)) return rc;
	const std::vector<VitSeg> &segs = pl.segs;
	const std::vector<VitTile> &tiles = pl.tiles;
	const std::vector<int32_t> &seg_tile = pl.seg_tile;
	const int64_t bins = pl.bins;
	const size_t n_tiles = tiles.size();

	Scratch sc;
	VitLaunch v;
	memset(&v, 0, sizeof v);
	const size_t bp_bytes = path ? (size_t)bins * S * (wide_bp ? 2 : 1) : 0;
	if (path) {
		v.bp = sc.get<uint8_t>(bp_bytes);
		if (!v.bp) {
			snprintf(msg, sizeof msg, "viterbi: no device memory for the back-pointer table: %.3f GB (%lld bins x %d states x %d)", bp_bytes * 1e-9,
			         (long long)bins, S, wide_bp ? 2 : 1);
			return fail(c, PSMC_HIP_ENOMEM, msg);
		}
	}
	double *d_tab = sc.get<double>(tab.size());
	VitSeg *d_segs = sc.get<VitSeg>(n_seg);
	double *d_score = sc.get<double>(n_seg);
	int32_t *d_end = sc.get<int32_t>(n_seg), *d_bad = sc.get<int32_t>(n_seg);
	VitTile *d_tiles = path ? sc.get<VitTile>(n_tiles) : nullptr;
	int32_t *d_seg_tile = path ? sc.get<int32_t>(seg_tile.size()) : nullptr;
	uint16_t *d_map = path ? sc.get<uint16_t>(n_tiles * S) : nullptr;
	int32_t *d_tile_end = path ? sc.get<int32_t>(n_tiles) : nullptr;
	int32_t *d_path = path ? sc.get<int32_t>((size_t)bins) : nullptr;
	if (!d_tab || !d_segs || !d_score || !d_end || !d_bad || (path && (!d_tiles || !d_seg_tile || !d_map || !d_tile_end || !d_path))) {
		snprintf(msg, sizeof msg, "viterbi: no device memory beside the back-pointer table of %.3f GB (maps of %zu tiles, %lld path entries)",
		         bp_bytes * 1e-9, n_tiles, (long long)bins);
		return fail(c, PSMC_HIP_ENOMEM, msg);
	}

	static const bool dbg_t = getenv("PSMC_HIP_DEBUG_TIMES") != nullptr;
	hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	if (dbg_t)
		for (int i = 0; i < 6; ++i) (void)hipEventCreate(&ev[i]);
	hipStream_t st = c->stream;
	hipError_t err = hipMemcpyAsync(d_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, st);
	if (err == hipSuccess) err = hipMemcpyAsync(d_segs, segs.data(), sizeof(VitSeg) * n_seg, hipMemcpyHostToDevice, st);
	if (err == hipSuccess) err = hipMemsetAsync(d_bad, 0, sizeof(int32_t) * n_seg, st);
	if (err == hipSuccess && path) err = hipMemcpyAsync(d_tiles, tiles.data(), sizeof(VitTile) * n_tiles, hipMemcpyHostToDevice, st);
	if (err == hipSuccess && path) err = hipMemcpyAsync(d_seg_tile, seg_tile.data(), sizeof(int32_t) * seg_tile.size(), hipMemcpyHostToDevice, st);
	int rc = 0;
	std::vector<double> h_score(n_seg);
	std::vector<int32_t> h_bad(n_seg);
	if (err == hipSuccess) {
		v.stream = st; v.n = n; v.S = S; v.wide_bp = wide_bp;
		v.la = d_tab; v.le = d_tab + (size_t)S * S; v.l0 = v.le + 3 * (size_t)S;
		v.obs = c->d_obs; v.segs = d_segs; v.n_seg = n_seg;
		v.score = d_score; v.end_state = d_end; v.bad = d_bad;
		v.tiles = d_tiles; v.n_tiles = (int)n_tiles; v.seg_tile0 = d_seg_tile; v.seg_nt = path ? d_seg_tile + n_seg : nullptr;
		v.map = d_map; v.tile_end = d_tile_end; v.path = d_path;
		for (int i = 0; i < 5; ++i) v.ev[i] = ev[i];
		rc = launch_viterbi(v);
		err = hipMemcpyAsync(h_bad.data(), d_bad, sizeof(int32_t) * n_seg, hipMemcpyDeviceToHost, st);
		if (err == hipSuccess) err = hipMemcpyAsync(h_score.data(), d_score, sizeof(double) * n_seg, hipMemcpyDeviceToHost, st);
		if (err == hipSuccess && path) err = hipMemcpyAsync(path, d_path, sizeof(int32_t) * (size_t)bins, hipMemcpyDeviceToHost, st);
		if (ev[5]) (void)hipEventRecord(ev[5], st);
	}
	const hipError_t esync = hipStreamSynchronize(st); // (the host tables live until here)
	if (dbg_t && rc == 0 && err == hipSuccess && esync == hipSuccess) {
		float ms[5] = {0, 0, 0, 0, 0};
		(void)hipEventElapsedTime(&ms[0], ev[0], ev[1]);
		if (path) {
			for (int i = 1; i < 4; ++i) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
			(void)hipEventElapsedTime(&ms[4], ev[4], ev[5]);
		} else (void)hipEventElapsedTime(&ms[4], ev[1], ev[5]);
		fprintf(stderr, "[psmc_hip] viterbi: %d states, %lld bins, %d segments, vit_tile %d: sweep %.3f ms, pass A %.3f, pass B %.3f, pass C %.3f, copy-out %.3f\n",
		        n, (long long)bins, n_seg, T, ms[0], ms[1], ms[2], ms[3], ms[4]);
	}
	for (int i = 0; i < 6; ++i)
		if (ev[i]) (void)hipEventDestroy(ev[i]);
	if (rc || err != hipSuccess || esync != hipSuccess) return fail(c, PSMC_HIP_EDEVICE, "viterbi", err != hipSuccess ? err : esync);
	for (int i = 0; i < n_seg; ++i)
		if (h_bad[i]) {
			snprintf(msg, sizeof msg, "viterbi: segment %d has no path of finite probability under these parameters (khmm.c's assert(max_l >= 0))", i);
			return fail(c, PSMC_HIP_EINVAL, msg);
		}
	if (score) memcpy(score, h_score.data(), sizeof(double) * n_seg);
	return PSMC_HIP_OK;
}
