// api_viterbi.hip -- psmc_hip_viterbi: the jointly most probable state path of every loaded segment (khmm.c:83-141) on the kernels of
// estep_viterbi.hip.  It reads the context's observations and nothing else of it: no table, plan, selection or learned state is
// touched, in either mode, and the device memory of the call is released before it returns.
#include "psmc_hip_ctx.h"

namespace {
struct VitScratch { // device memory of one call
	std::vector<void *> bufs;
	~VitScratch() { for (void *p : bufs) (void)hipFree(p); }
	template <class T> T *get(size_t n)
	{
		void *p = nullptr;
		if (hipMalloc(&p, sizeof(T) * (n ? n : 1)) != hipSuccess) return nullptr;
		bufs.push_back(p);
		return (T *)p;
	}
};
} // namespace

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
	const double ninf = -HUGE_VAL;
	std::vector<double> tab((size_t)S * S + 4 * (size_t)S, ninf);
	double *la = tab.data(), *le = la + (size_t)S * S, *l0 = le + 3 * (size_t)S;
	for (int l = 0; l < n; ++l)
		for (int k = 0; k < n; ++k) la[(size_t)l * S + k] = log(a[(size_t)l * n + k]);
	for (int k = 0; k < n; ++k) {
		le[k] = log(e[k]);
		le[S + k] = log(e[n + k]);
		le[2 * S + k] = 0.0;
		l0[k] = log(a0[k]);
	}

	// segments longest first; rows and path entries in load order; the tiles of the backtrace
	std::vector<int64_t> row_off(n_seg);
	int64_t bins = 0;
	for (int i = 0; i < n_seg; ++i) { row_off[i] = bins; bins += c->L[i]; }
	std::vector<VitSeg> segs(n_seg);
	for (int i = 0; i < n_seg; ++i) segs[i] = VitSeg{c->off[i], row_off[i], c->L[i], i};
	std::stable_sort(segs.begin(), segs.end(), [](const VitSeg &x, const VitSeg &y) { return x.L > y.L; });
	std::vector<VitTile> tiles;
	std::vector<int32_t> seg_tile((size_t)2 * n_seg);
	if (path) {
		int64_t n_tiles = 0;
		for (int i = 0; i < n_seg; ++i) n_tiles += (c->L[i] + T - 1) / T;
		if (n_tiles > 0x7fffffff) return fail(c, PSMC_HIP_EINVAL, "viterbi: more than 2^31 backtrace tiles (\"vit_tile\" is too small for this input)");
		tiles.reserve((size_t)n_tiles);
		for (int i = 0; i < n_seg; ++i) {
			seg_tile[i] = (int32_t)tiles.size();
			for (int lo = 1; lo <= c->L[i]; lo += T) tiles.push_back(VitTile{row_off[i], lo, std::min(c->L[i], lo + T - 1)});
			seg_tile[n_seg + i] = (int32_t)tiles.size() - seg_tile[i];
		}
	}
	const size_t n_tiles = tiles.size();

	VitScratch sc;
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
