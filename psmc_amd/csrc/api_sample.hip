// api_sample.hip -- psmc_hip_sample_paths: state paths of every loaded segment drawn from the posterior (forward filtering, backward
// sampling; the definition is pinned in include/psmc_hip.h) on the sweep of estep_sample.hip and the tiled backtrace of
// estep_viterbi.hip.  Like psmc_hip_viterbi it reads the context's observations and nothing else of it: no table, plan, selection or
// learned state is touched, in either mode, and the device memory of the call is released before it returns.
#include "psmc_hip_ctx.h"

extern "C" int psmc_hip_sample_paths(psmc_hip_ctx *c, const double *a, const double *e, const double *a0, uint64_t seed, int32_t n_samp,
                                     const uint64_t *stream, int32_t *path)
{
	if (!c) return PSMC_HIP_EINVAL;
	if (!a || !e || !a0) return fail(c, PSMC_HIP_EINVAL, "sample_paths: null parameters");
	if (!path) return fail(c, PSMC_HIP_EINVAL, "sample_paths: null path");
	if (n_samp < 1) return fail(c, PSMC_HIP_EINVAL, "sample_paths: n_samp < 1");
	if (c->n_seg < 1 || !c->d_obs) return fail(c, PSMC_HIP_ESTATE, "sample_paths: no segments loaded");
	HIPCHK(c, hipSetDevice(c->device));
	const int n = c->n, S = 64 * ((n + 63) / 64), n_seg = c->n_seg, T = c->vit_tile;
	const bool wide_bp = S > 256;
	char msg[256];

	// the parameters padded with zeros: a [S][S] as it is, e [3][S] with the missing symbol's row of ones, a0 [S]
	const std::vector<double> tab = path_params(n, S, a, e, a0, [](double x) { return x; }, 0.0, 1.0);
	// segments, rows and backtrace tiles as psmc_hip_viterbi has them; the stream ids
	PathPlan pl;
	if (int rc = path_plan(c, "sample_paths", true, pl)) return rc;
	const std::vector<VitSeg> &segs = pl.segs;
	const std::vector<VitTile> &tiles = pl.tiles;
	const std::vector<int32_t> &seg_tile = pl.seg_tile;
	const int64_t bins = pl.bins;
	const size_t n_tiles = tiles.size();
	std::vector<uint64_t> sid(n_seg);
	for (int i = 0; i < n_seg; ++i) sid[i] = stream ? stream[i] : (uint64_t)i;

	// the group: one map table per sample
	const size_t tab_bytes = (size_t)bins * S * (wide_bp ? 2 : 1);
	const size_t side_bytes = sizeof(int32_t) * (size_t)bins + sizeof(int32_t) * n_seg; // path and end states, per sample of the group
	int G = c->samp_group;
	if (G == 0) {
		size_t free_b = 0, total_b = 0;
		G = 8;
		if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
			const size_t fixed = sizeof(double) * tab.size() + (sizeof(VitSeg) + 24) * (size_t)n_seg + (sizeof(VitTile) + 4 + 2 * (size_t)S) * n_tiles + (64u << 20);
			const size_t room = free_b > fixed ? free_b - fixed : 0;
			G = (int)std::min<size_t>(8, room / (tab_bytes + side_bytes));
		}
	}
	G = std::max(1, std::min(G, (int)std::min<int32_t>(n_samp, SAMP_MAX_GROUP)));
	Scratch sc;
	uint8_t *d_map = nullptr;
	for (;; G = (G + 1) / 2) { // (a group that does not fit after all: half of it)
		if ((d_map = sc.get<uint8_t>(tab_bytes * G))) break;
		if (G == 1) {
			snprintf(msg, sizeof msg, "sample_paths: no device memory for one sample's map table: %.3f GB (%lld bins x %d states x %d)", tab_bytes * 1e-9,
			         (long long)bins, S, wide_bp ? 2 : 1);
			return fail(c, PSMC_HIP_ENOMEM, msg);
		}
	}
	double *d_tab = sc.get<double>(tab.size());
	VitSeg *d_segs = sc.get<VitSeg>(n_seg);
	uint64_t *d_sid = sc.get<uint64_t>(n_seg);
	int32_t *d_end = sc.get<int32_t>((size_t)G * n_seg);
	VitTile *d_tiles = sc.get<VitTile>(n_tiles);
	int32_t *d_seg_tile = sc.get<int32_t>(seg_tile.size());
	uint16_t *d_tmap = sc.get<uint16_t>(n_tiles * S);
	int32_t *d_tile_end = sc.get<int32_t>(n_tiles);
	int32_t *d_path = sc.get<int32_t>((size_t)G * bins);
	if (!d_tab || !d_segs || !d_sid || !d_end || !d_tiles || !d_seg_tile || !d_tmap || !d_tile_end || !d_path) {
		snprintf(msg, sizeof msg, "sample_paths: no device memory beside %d map tables of %.3f GB (maps of %zu tiles, %lld path entries per sample)", G,
		         tab_bytes * 1e-9, n_tiles, (long long)bins);
		return fail(c, PSMC_HIP_ENOMEM, msg);
	}

	static const bool dbg_t = getenv("PSMC_HIP_DEBUG_TIMES") != nullptr;
	hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
	if (dbg_t)
		for (int i = 0; i < 3; ++i) (void)hipEventCreate(&ev[i]);
	double ms_sweep = 0.0, ms_back = 0.0;
	hipStream_t st = c->stream;
	hipError_t err = hipMemcpyAsync(d_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, st);
	if (err == hipSuccess) err = hipMemcpyAsync(d_segs, segs.data(), sizeof(VitSeg) * n_seg, hipMemcpyHostToDevice, st);
	if (err == hipSuccess) err = hipMemcpyAsync(d_sid, sid.data(), sizeof(uint64_t) * n_seg, hipMemcpyHostToDevice, st);
	if (err == hipSuccess) err = hipMemcpyAsync(d_tiles, tiles.data(), sizeof(VitTile) * n_tiles, hipMemcpyHostToDevice, st);
	if (err == hipSuccess) err = hipMemcpyAsync(d_seg_tile, seg_tile.data(), sizeof(int32_t) * seg_tile.size(), hipMemcpyHostToDevice, st);
	int rc = 0, n_groups = 0;
	for (int j0 = 0; err == hipSuccess && rc == 0 && j0 < n_samp; j0 += G, ++n_groups) {
		const int g_now = std::min<int>(G, n_samp - j0);
		SampLaunch p;
		memset(&p, 0, sizeof p);
		p.stream = st; p.n = n; p.S = S; p.wide_bp = wide_bp;
		p.a = d_tab; p.e = d_tab + (size_t)S * S; p.a0 = p.e + 3 * (size_t)S;
		p.obs = c->d_obs; p.segs = d_segs; p.n_seg = n_seg; p.sid = d_sid;
		p.seed = seed; p.first = j0; p.group = g_now;
		p.map = d_map; p.map_stride = tab_bytes; p.end_state = d_end;
		if (ev[0]) (void)hipEventRecord(ev[0], st);
		rc = launch_sample_sweep(p);
		if (ev[1]) (void)hipEventRecord(ev[1], st);
		for (int g = 0; rc == 0 && g < g_now; ++g) { // the backtrace of sample j0 + g over its own table
			VitLaunch v;
			memset(&v, 0, sizeof v);
			v.stream = st; v.n = n; v.S = S; v.wide_bp = wide_bp;
			v.bp = d_map + (size_t)g * tab_bytes; v.n_seg = n_seg; v.end_state = d_end + (size_t)g * n_seg;
			v.tiles = d_tiles; v.n_tiles = (int)n_tiles; v.seg_tile0 = d_seg_tile; v.seg_nt = d_seg_tile + n_seg;
			v.map = d_tmap; v.tile_end = d_tile_end; v.path = d_path + (size_t)g * bins;
			rc = launch_vit_backtrace(v);
		}
		if (ev[2]) (void)hipEventRecord(ev[2], st);
		if (rc == 0) err = hipMemcpyAsync(path + (size_t)j0 * bins, d_path, sizeof(int32_t) * (size_t)g_now * bins, hipMemcpyDeviceToHost, st);
		if (dbg_t && rc == 0 && err == hipSuccess && hipStreamSynchronize(st) == hipSuccess) {
			float m0 = 0, m1 = 0;
			(void)hipEventElapsedTime(&m0, ev[0], ev[1]);
			(void)hipEventElapsedTime(&m1, ev[1], ev[2]);
			ms_sweep += m0; ms_back += m1;
		}
	}
	const hipError_t esync = hipStreamSynchronize(st); // (the host tables live until here)
	if (dbg_t && rc == 0 && err == hipSuccess && esync == hipSuccess)
		fprintf(stderr, "[psmc_hip] sample_paths: %d states, %lld bins, %d segments, %d samples in %d groups of %d, vit_tile %d: sweeps %.3f ms, backtraces %.3f ms\n",
		        n, (long long)bins, n_seg, (int)n_samp, n_groups, G, T, ms_sweep, ms_back);
	for (int i = 0; i < 3; ++i)
		if (ev[i]) (void)hipEventDestroy(ev[i]);
	if (rc || err != hipSuccess || esync != hipSuccess) return fail(c, PSMC_HIP_EDEVICE, "sample_paths", err != hipSuccess ? err : esync);
	return PSMC_HIP_OK;
}
