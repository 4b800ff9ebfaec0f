// api_probes.hip -- libpsmc_hip_diag.so (include/psmc_hip_diag.h): device self-test, instruction microbenchmarks, the pipe /
// placement / compute-unit-mask / HBM probes that DESIGN.md cites, and the HIP-event timing of a context's last E-step.
// Not part of an E-step and not part of the drop-in library: it links against libpsmc_hip.so.
#include "psmc_hip_ctx.h"
#include "psmc_hip_diag.h"

extern "C" int psmc_hip_selftest(int device)
{
	int nd = psmc_hip_device_count();
	if (nd <= 0 || device < 0 || device >= nd) return PSMC_HIP_EDEVICE;
	if (hipSetDevice(device) != hipSuccess) return PSMC_HIP_EDEVICE;
	unsigned *d = nullptr, h = 0xffffffffu;
	if (hipMalloc((void **)&d, sizeof(unsigned)) != hipSuccess) return PSMC_HIP_ENOMEM;
	(void)hipMemset(d, 0, sizeof(unsigned));
	int rc = run_selftest(nullptr, d);
	if (rc == 0 && hipDeviceSynchronize() == hipSuccess && hipMemcpy(&h, d, sizeof(unsigned), hipMemcpyDeviceToHost) == hipSuccess)
		rc = (int)h;
	else
		rc = PSMC_HIP_EDEVICE;
	(void)hipFree(d);
	return rc;
}

extern "C" int psmc_hip_microbench(int device, double *out, int n)
{
	int nd = psmc_hip_device_count();
	if (!out || n < 1) return PSMC_HIP_EINVAL;
	if (nd <= 0 || device < 0 || device >= nd) return PSMC_HIP_EDEVICE;
	if (hipSetDevice(device) != hipSuccess) return PSMC_HIP_EDEVICE;
	double *d = nullptr, h[64];
	if (hipMalloc((void **)&d, sizeof(h)) != hipSuccess) return PSMC_HIP_ENOMEM;
	(void)hipMemset(d, 0, sizeof(h));
	int rc = run_microbench(nullptr, d); // first launch warms the clocks / instruction cache
	if (rc == 0) rc = run_microbench(nullptr, d);
	if (rc == 0 && hipDeviceSynchronize() == hipSuccess && hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess) {
		for (int i = 0; i < n && i < 64; ++i) out[i] = h[i];
		rc = PSMC_HIP_OK;
	} else rc = PSMC_HIP_EDEVICE;
	(void)hipFree(d);
	return rc;
}

extern "C" int psmc_hip_pipe_probe(int device, double *out, int n)
{
	// configurations: (waves, mask of matrix waves)
	static const struct { int waves; unsigned mask; } cfg[PSMC_HIP_PIPE_PROBE_CONFIGS] = {
		{4, 0xFu}, {4, 0x0u}, {8, 0xFFu}, {8, 0x00u}, {8, 0x0Fu}, {8, 0x55u}};
	int nd = psmc_hip_device_count();
	if (!out || n < PSMC_HIP_PIPE_PROBE_CONFIGS * 8) return PSMC_HIP_EINVAL;
	if (nd <= 0 || device < 0 || device >= nd) return PSMC_HIP_EDEVICE;
	if (hipSetDevice(device) != hipSuccess) return PSMC_HIP_EDEVICE;
	double *d = nullptr;
	if (hipMalloc((void **)&d, sizeof(double) * 8) != hipSuccess) return PSMC_HIP_ENOMEM;
	int rc = 0;
	for (int i = 0; i < PSMC_HIP_PIPE_PROBE_CONFIGS && rc == 0; ++i) {
		(void)hipMemset(d, 0, sizeof(double) * 8);
		rc = run_pipe_probe(nullptr, d, cfg[i].waves, cfg[i].mask, 8);        // warm: clocks, instruction cache
		if (rc == 0) rc = run_pipe_probe(nullptr, d, cfg[i].waves, cfg[i].mask, 64);
		if (rc == 0 && (hipDeviceSynchronize() != hipSuccess ||
		                hipMemcpy(out + 8 * i, d, sizeof(double) * 8, hipMemcpyDeviceToHost) != hipSuccess)) rc = 1;
		for (int w = cfg[i].waves; w < 8; ++w) out[8 * i + w] = 0.0;
	}
	(void)hipFree(d);
	return rc ? PSMC_HIP_EDEVICE : PSMC_HIP_OK;
}

extern "C" int psmc_hip_pipe_probe2(int device, const int *kinds8, int rounds, double *out8)
{
	int nd = psmc_hip_device_count();
	if (!kinds8 || !out8 || rounds < 1) return PSMC_HIP_EINVAL;
	for (int i = 0; i < 8; ++i) if (kinds8[i] < 0 || kinds8[i] > 9) return PSMC_HIP_EINVAL;
	if (nd <= 0 || device < 0 || device >= nd) return PSMC_HIP_EDEVICE;
	if (hipSetDevice(device) != hipSuccess) return PSMC_HIP_EDEVICE;
	double *d = nullptr; void *src = nullptr;
	if (hipMalloc((void **)&d, sizeof(double) * 8) != hipSuccess || hipMalloc(&src, 4096) != hipSuccess) { if (d) (void)hipFree(d); return PSMC_HIP_ENOMEM; }
	(void)hipMemset(d, 0, sizeof(double) * 8); (void)hipMemset(src, 1, 4096);
	int rc = run_pipe_probe2(nullptr, d, kinds8, std::max(1, rounds / 8), src); // warm: clocks, instruction cache
	if (rc == 0) rc = run_pipe_probe2(nullptr, d, kinds8, rounds, src);
	if (rc == 0 && (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out8, d, sizeof(double) * 8, hipMemcpyDeviceToHost) != hipSuccess)) rc = 1;
	(void)hipFree(d); (void)hipFree(src);
	return rc ? PSMC_HIP_EDEVICE : PSMC_HIP_OK;
}

extern "C" int psmc_hip_place_probe(int device, int n_waves, int waves_per_block, int n_kernels, int steps, double *out, double *ms_out)
{
	int nd = psmc_hip_device_count();
	if (n_waves < 1 || n_waves > (1 << 16) || waves_per_block < 1 || waves_per_block > 4 || n_kernels < 1 || n_kernels > 4 || steps < 4 || !out) return PSMC_HIP_EINVAL;
	if (nd <= 0 || device < 0 || device >= nd) return PSMC_HIP_EDEVICE;
	if (hipSetDevice(device) != hipSuccess) return PSMC_HIP_EDEVICE;
	const size_t per = (size_t)3 * ((n_waves + waves_per_block - 1) / waves_per_block) * waves_per_block;
	double *d = nullptr;
	if (hipMalloc((void **)&d, sizeof(double) * per * n_kernels) != hipSuccess) return PSMC_HIP_ENOMEM;
	hipStream_t st[4] = {nullptr, nullptr, nullptr, nullptr};
	hipEvent_t e0, e1[4];
	int rc = 0;
	(void)hipEventCreate(&e0);
	for (int k = 0; k < n_kernels; ++k) { if (hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking) != hipSuccess) rc = 1; (void)hipEventCreate(&e1[k]); }
	for (int pass = 0; pass < 2 && rc == 0; ++pass) { // pass 0 warms clocks and the instruction cache
		(void)hipDeviceSynchronize();
		(void)hipEventRecord(e0, st[0]);
		for (int k = 1; k < n_kernels; ++k) (void)hipStreamWaitEvent(st[k], e0, 0);
		for (int k = 0; k < n_kernels && rc == 0; ++k) { rc = run_place_probe(st[k], d + per * k, n_waves, waves_per_block, steps & ~3); (void)hipEventRecord(e1[k], st[k]); }
	}
	if (rc == 0 && hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, d, sizeof(double) * per * n_kernels, hipMemcpyDeviceToHost) == hipSuccess) {
		float worst = 0;
		for (int k = 0; k < n_kernels; ++k) { float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1[k]); worst = std::max(worst, ms); }
		if (ms_out) *ms_out = worst;
	} else rc = 1;
	(void)hipEventDestroy(e0);
	for (int k = 0; k < n_kernels; ++k) { (void)hipEventDestroy(e1[k]); if (st[k]) (void)hipStreamDestroy(st[k]); }
	(void)hipFree(d);
	return rc ? PSMC_HIP_EDEVICE : PSMC_HIP_OK;
}

extern "C" int psmc_hip_stream_probe(int device, long long n_doubles, double *ms_out)
{
	int nd = psmc_hip_device_count();
	if (n_doubles < 1) return PSMC_HIP_EINVAL;
	if (nd <= 0 || device < 0 || device >= nd) return PSMC_HIP_EDEVICE;
	if (hipSetDevice(device) != hipSuccess) return PSMC_HIP_EDEVICE;
	double *a = nullptr, *b = nullptr;
	if (hipMalloc((void **)&a, sizeof(double) * n_doubles) != hipSuccess) return PSMC_HIP_ENOMEM;
	if (hipMalloc((void **)&b, sizeof(double) * n_doubles) != hipSuccess) { (void)hipFree(a); return PSMC_HIP_ENOMEM; }
	(void)hipMemset(a, 0, sizeof(double) * n_doubles);
	hipEvent_t e0, e1;
	(void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
	int rc = run_stream_probe(nullptr, a, b, (size_t)n_doubles); // warm
	(void)hipEventRecord(e0, nullptr);
	for (int i = 0; i < 4 && rc == 0; ++i) rc = run_stream_probe(nullptr, a, b, (size_t)n_doubles);
	(void)hipEventRecord(e1, nullptr);
	float ms = 0;
	if (rc == 0 && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) { if (ms_out) *ms_out = ms / 4; rc = PSMC_HIP_OK; }
	else rc = PSMC_HIP_EDEVICE;
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(a); (void)hipFree(b);
	return rc;
}

extern "C" int psmc_hip_hbm_probe(int device, long long bytes, double *gbps_out)
{
	int nd = psmc_hip_device_count();
	if (bytes < (1 << 24) || !gbps_out) return PSMC_HIP_EINVAL;
	if (nd <= 0 || device < 0 || device >= nd) return PSMC_HIP_EDEVICE;
	if (hipSetDevice(device) != hipSuccess) return PSMC_HIP_EDEVICE;
	bytes &= ~(long long)((1 << 23) - 1); // whole 8 MB: four 2 MB streams per wave in the sweep-store probe
	double *a = nullptr, *b = nullptr;
	if (hipMalloc((void **)&a, (size_t)bytes) != hipSuccess) return PSMC_HIP_ENOMEM;
	if (hipMalloc((void **)&b, (size_t)bytes) != hipSuccess) { (void)hipFree(a); return PSMC_HIP_ENOMEM; }
	(void)hipMemset(a, 0, (size_t)bytes); (void)hipMemset(b, 0, (size_t)bytes);
	hipEvent_t e0, e1;
	(void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
	int rc = 0;
	for (int which = 0; which < 4 && rc == 0; ++which) {
		rc = run_hbm_probe(nullptr, which, a, b, (size_t)bytes); // warm
		(void)hipEventRecord(e0, nullptr);
		for (int i = 0; i < 3 && rc == 0; ++i) rc = run_hbm_probe(nullptr, which, a, b, (size_t)bytes);
		(void)hipEventRecord(e1, nullptr);
		float ms = 0;
		if (rc == 0 && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess)
			gbps_out[which] = (which == 2 ? 2.0 : 1.0) * (double)bytes / (ms / 3 * 1e-3) / 1e9;
		else rc = PSMC_HIP_EDEVICE;
	}
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(a); (void)hipFree(b);
	return rc ? PSMC_HIP_EDEVICE : PSMC_HIP_OK;
}

extern "C" int psmc_hip_load_probe(int device, int n_waves, int steps, double *out)
{
	int nd = psmc_hip_device_count();
	if (n_waves < 1 || n_waves > (1 << 20) || steps < 4 || !out) return PSMC_HIP_EINVAL;
	if (nd <= 0 || device < 0 || device >= nd) return PSMC_HIP_EDEVICE;
	if (hipSetDevice(device) != hipSuccess) return PSMC_HIP_EDEVICE;
	double *d = nullptr;
	if (hipMalloc((void **)&d, sizeof(double) * 2 * (size_t)n_waves) != hipSuccess) return PSMC_HIP_ENOMEM;
	std::vector<double> h((size_t)2 * n_waves);
	hipEvent_t e0, e1;
	(void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
	const int arg = steps & ~3;
	int rc = run_load_probe(nullptr, d, n_waves, arg); // warm
	(void)hipEventRecord(e0, nullptr);
	if (rc == 0) rc = run_load_probe(nullptr, d, n_waves, arg);
	(void)hipEventRecord(e1, nullptr);
	float ms = 0;
	if (rc == 0 && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess &&
	    hipMemcpy(h.data(), d, sizeof(double) * h.size(), hipMemcpyDeviceToHost) == hipSuccess) {
		double cyc = 0, mhz = 0, cmax = 0;
		for (int i = 0; i < n_waves; ++i) { cyc += h[2 * (size_t)i]; mhz += h[2 * (size_t)i + 1]; cmax = std::max(cmax, h[2 * (size_t)i]); }
		out[0] = ms; out[1] = cyc / n_waves; out[2] = cmax; out[3] = mhz / n_waves;
		rc = PSMC_HIP_OK;
	} else rc = PSMC_HIP_EDEVICE;
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(d);
	return rc;
}

// Diagnostic: load_probe with the table stores of a sweep; modes: see include/psmc_hip.h and microbench.hip
extern "C" int psmc_hip_load_probe_st(int device, int n_waves, int steps, int store_steps, int mode, double *out)
{
	int nd = psmc_hip_device_count();
	if (n_waves < 1 || n_waves > (1 << 16) || steps < 4 || store_steps < 4 || store_steps > steps || !out) return PSMC_HIP_EINVAL;
	if (nd <= 0 || device < 0 || device >= nd) return PSMC_HIP_EDEVICE;
	if (hipSetDevice(device) != hipSuccess) return PSMC_HIP_EDEVICE;
	steps &= ~3; store_steps &= ~3;
	double *d = nullptr, *tbl = nullptr;
	const size_t tb = (size_t)n_waves * 4 * (size_t)store_steps * 512;
	if (hipMalloc((void **)&d, sizeof(double) * 2 * (size_t)n_waves) != hipSuccess) return PSMC_HIP_ENOMEM;
	if (hipMalloc((void **)&tbl, tb) != hipSuccess) { (void)hipFree(d); return PSMC_HIP_ENOMEM; }
	(void)hipMemset(tbl, 0, tb);
	std::vector<double> h((size_t)2 * n_waves);
	hipEvent_t e0, e1;
	(void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
	int rc = run_load_probe_st(nullptr, d, n_waves, steps, tbl, store_steps, mode);
	(void)hipEventRecord(e0, nullptr);
	if (rc == 0) rc = run_load_probe_st(nullptr, d, n_waves, steps, tbl, store_steps, mode);
	(void)hipEventRecord(e1, nullptr);
	float ms = 0;
	if (rc == 0 && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess &&
	    hipMemcpy(h.data(), d, sizeof(double) * h.size(), hipMemcpyDeviceToHost) == hipSuccess) {
		double cyc = 0, mhz = 0, cmax = 0;
		for (int i = 0; i < n_waves; ++i) { cyc += h[2 * (size_t)i]; mhz += h[2 * (size_t)i + 1]; cmax = std::max(cmax, h[2 * (size_t)i]); }
		out[0] = ms; out[1] = cyc / n_waves; out[2] = cmax; out[3] = mhz / n_waves; out[4] = (double)tb / (ms * 1e-3) / 1e9;
		rc = PSMC_HIP_OK;
	} else rc = PSMC_HIP_EDEVICE;
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(d); (void)hipFree(tbl);
	return rc;
}

// Two streams with complementary compute-unit masks (or none), the placement probe on both at once.
extern "C" int psmc_hip_cumask_probe(int device, int n_cus_a, int n_waves_a, int n_waves_b, int steps, double *out, double *ms_out)
{
	int nd = psmc_hip_device_count();
	if (n_cus_a < 0 || n_waves_a < 1 || n_waves_b < 1 || n_waves_a > (1 << 16) || n_waves_b > (1 << 16) || steps < 4 || !out) return PSMC_HIP_EINVAL;
	if (nd <= 0 || device < 0 || device >= nd) return PSMC_HIP_EDEVICE;
	if (hipSetDevice(device) != hipSuccess) return PSMC_HIP_EDEVICE;
	int cus = 0;
	if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) return PSMC_HIP_EDEVICE;
	if (n_cus_a >= cus) return PSMC_HIP_EINVAL;
	double *d = nullptr;
	if (hipMalloc((void **)&d, sizeof(double) * 3 * (size_t)(n_waves_a + n_waves_b)) != hipSuccess) return PSMC_HIP_ENOMEM;
	hipStream_t st[2] = {nullptr, nullptr};
	int rc = 0;
	if (n_cus_a > 0) {
		const int words = (cus + 31) / 32;
		std::vector<uint32_t> ma(words, 0u), mb(words, 0u);
		for (int i = 0; i < cus; ++i) (i < n_cus_a ? ma : mb)[i >> 5] |= 1u << (i & 31);
		if (hipExtStreamCreateWithCUMask(&st[0], (uint32_t)words, ma.data()) != hipSuccess) rc = 1;
		if (rc == 0 && hipExtStreamCreateWithCUMask(&st[1], (uint32_t)words, mb.data()) != hipSuccess) rc = 1;
	} else {
		if (hipStreamCreateWithFlags(&st[0], hipStreamNonBlocking) != hipSuccess) rc = 1;
		if (rc == 0 && hipStreamCreateWithFlags(&st[1], hipStreamNonBlocking) != hipSuccess) rc = 1;
	}
	hipEvent_t e0, e1[2];
	(void)hipEventCreate(&e0); (void)hipEventCreate(&e1[0]); (void)hipEventCreate(&e1[1]);
	for (int pass = 0; pass < 2 && rc == 0; ++pass) { // pass 0 warms clocks and the instruction cache
		(void)hipDeviceSynchronize();
		(void)hipEventRecord(e0, st[0]);
		(void)hipStreamWaitEvent(st[1], e0, 0);
		rc = run_place_probe(st[0], d, n_waves_a, 1, steps & ~3); (void)hipEventRecord(e1[0], st[0]);
		if (rc == 0) { rc = run_place_probe(st[1], d + 3 * (size_t)n_waves_a, n_waves_b, 1, steps & ~3); (void)hipEventRecord(e1[1], st[1]); }
	}
	if (rc == 0 && hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, d, sizeof(double) * 3 * (size_t)(n_waves_a + n_waves_b), hipMemcpyDeviceToHost) == hipSuccess) {
		float a = 0, b = 0;
		(void)hipEventElapsedTime(&a, e0, e1[0]); (void)hipEventElapsedTime(&b, e0, e1[1]);
		if (ms_out) *ms_out = std::max(a, b);
	} else rc = 1;
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1[0]); (void)hipEventDestroy(e1[1]);
	for (int k = 0; k < 2; ++k) if (st[k]) (void)hipStreamDestroy(st[k]);
	(void)hipFree(d);
	return rc ? PSMC_HIP_EDEVICE : PSMC_HIP_OK;
}

extern "C" int psmc_hip_last_timing(psmc_hip_ctx *c, double ms[7])
{
	if (!c || !ms) return PSMC_HIP_EINVAL;
	if (!c->timing_valid) {
		HIPCHK(c, hipSetDevice(c->device));
		if (hipEventSynchronize(c->ev[4]) != hipSuccess) return fail(c, PSMC_HIP_ESTATE, "last_timing: nothing recorded");
		collect_timing(c);
		if (!c->timing_valid) return fail(c, PSMC_HIP_ESTATE, "last_timing: events incomplete");
	}
	for (int i = 0; i < 7; ++i) ms[i] = c->last_ms[i];
	return PSMC_HIP_OK;
}

extern "C" int psmc_hip_plan_tiles(psmc_hip_ctx *c, int32_t *cls, int32_t *glue, int cap)
{
	if (!c || cap < 0 || (cap > 0 && (!cls || !glue))) return PSMC_HIP_EINVAL;
	// (as psmc_hip_fast_plan: the plan is made by the first fast E-step after load / select / an option that changes it)
	if (c->plan_dirty || c->chunks.empty()) return fail(c, PSMC_HIP_ESTATE, "plan_tiles: no current plan (run a fast E-step first)");
	const int nc = (int)c->chunks.size();
	for (int b = 0; b < nc && b < cap; ++b) {
		const int hom = b < (int)c->hom.size() ? c->hom[b] : 0;
		cls[b] = (b < (int)c->gap.size() && c->gap[b]) ? 1 : (hom >= 2 ? 3 : (hom == 1 ? 2 : 0));
		glue[b] = (c->glue_f[b] ? 1 : 0) | (c->glue_b[b] ? 2 : 0);
	}
	return nc;
}

extern "C" int psmc_hip_wide_plan_tiles(psmc_hip_ctx *c, int32_t *cls, int32_t *glue, int cap)
{
	if (!c || cap < 0 || (cap > 0 && (!cls || !glue))) return PSMC_HIP_EINVAL;
	// (the wide plan is made by the first wide fast E-step after load / select / an option that changes it: api_wide_fast.hip plan_wide)
	if (c->plan_dirty || c->wf_chunks.empty()) return fail(c, PSMC_HIP_ESTATE, "wide_plan_tiles: no current wide plan (run a wide fast E-step first)");
	const int nc = (int)c->wf_chunks.size();
	const bool have = (int)c->wg_cls.size() == nc; // ("wide_gap_tiles" = 0: nothing was classified)
	for (int b = 0; b < nc && b < cap; ++b) {
		cls[b] = have ? c->wg_cls[b] : 0;
		glue[b] = have ? c->wg_glue[b] & 3 : 0;
	}
	return nc;
}

// ---- what "wide_gap_tiles" planned and did (api_wide_fast.hip): host reads and plain copies behind a stream synchronise, no kernel
static int no_wide_plan(psmc_hip_ctx *c, const char *who)
{
	std::string msg = std::string(who) + ": no current wide plan (run a wide fast E-step first)";
	return fail(c, PSMC_HIP_ESTATE, msg.c_str());
}

extern "C" int psmc_hip_wide_gap_chains(psmc_hip_ctx *c, int dir, int32_t *first, int32_t *count, int32_t *walk, int32_t *level, int cap)
{
	if (!c || dir < 0 || dir > 1 || cap < 0 || (cap > 0 && (!first || !count || !walk || !level))) return PSMC_HIP_EINVAL;
	if (c->plan_dirty || c->wf_chunks.empty() || !c->wf_ran) return no_wide_plan(c, "wide_gap_chains");
	const psmc_hip_ctx::WgDir &D = c->wg[dir];
	const int nr = (int)D.runs.size();
	int lev = 0;
	for (int i = 0; i < nr && i < cap; ++i) {
		while (lev + 1 < (int)D.run_off.size() && i >= D.run_off[lev + 1]) ++lev; // (run_off: [levels + 1], ascending)
		first[i] = D.runs[i].first; count[i] = D.runs[i].count; walk[i] = D.walk[i]; level[i] = lev;
	}
	return nr;
}

extern "C" int psmc_hip_wide_gap_rechained(psmc_hip_ctx *c, int out[2])
{
	if (!c || !out) return PSMC_HIP_EINVAL;
	if (c->plan_dirty || c->wf_chunks.empty() || !c->wf_ran) return no_wide_plan(c, "wide_gap_rechained");
	out[0] = c->wg_rechained[0]; out[1] = c->wg_rechained[1];
	return PSMC_HIP_OK;
}

extern "C" int64_t psmc_hip_wide_gap_matrix(psmc_hip_ctx *c, double *M, int64_t cap)
{
	if (!c || cap < 0 || (cap > 0 && !M)) return PSMC_HIP_EINVAL;
	if (c->plan_dirty || c->wf_chunks.empty() || !c->wf_ran) return no_wide_plan(c, "wide_gap_matrix");
	if (!c->wg_m_valid || !c->d_wg_M) return fail(c, PSMC_HIP_ESTATE, "wide_gap_matrix: the last wide fast E-step built no transfer matrix (no qualifying run, or \"wide_gap_tiles\" = 0)");
	const int64_t len = (int64_t)c->n * wf_width(c);
	if (cap > 0) {
		HIPCHK(c, hipSetDevice(c->device));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		HIPCHK(c, hipMemcpy(M, c->d_wg_M, sizeof(double) * (size_t)std::min(cap, len), hipMemcpyDeviceToHost));
	}
	return len;
}

extern "C" int64_t psmc_hip_wide_hom_matrix(psmc_hip_ctx *c, double *M, int64_t cap)
{
	if (!c || cap < 0 || (cap > 0 && !M)) return PSMC_HIP_EINVAL;
	if (c->plan_dirty || c->wf_chunks.empty() || !c->wf_ran) return no_wide_plan(c, "wide_hom_matrix");
	if (!c->wg_mh_T || !c->d_wg_Mh) return fail(c, PSMC_HIP_ESTATE, "wide_hom_matrix: the last wide fast E-step built no matrix of a homozygous tile (no qualifying run with a hom tile, or \"wide_hom_tiles\" = 0)");
	const int64_t len = (int64_t)c->n * wf_width(c) + (c->wg_mh_T + 3) / 4; // M_h, then the pilot's factors
	if (cap > 0) {
		HIPCHK(c, hipSetDevice(c->device));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		HIPCHK(c, hipMemcpy(M, c->d_wg_Mh, sizeof(double) * (size_t)std::min(cap, len), hipMemcpyDeviceToHost));
	}
	return len;
}

extern "C" int64_t psmc_hip_wide_mix_matrix(psmc_hip_ctx *c, int tile, int dir, double *out, int64_t cap)
{
	if (!c || cap < 0 || (cap > 0 && !out)) return PSMC_HIP_EINVAL;
	if (c->plan_dirty || c->wf_chunks.empty() || !c->wf_ran) return no_wide_plan(c, "wide_mix_matrix");
	if (!c->wg_mx_T || !c->wg_mx_n || !c->d_wg_Mx) return fail(c, PSMC_HIP_ESTATE, "wide_mix_matrix: the last wide fast E-step built no matrix of a mix tile (no qualifying run with a mix tile, or \"wide_mix_tiles\" = 0)");
	if (dir < 0 || dir > 1 || tile < 0 || tile >= (int)c->wg_cls.size() || c->wg_cls[tile] != 6 || c->wg_mix_slot[tile] < 0)
		return fail(c, PSMC_HIP_EINVAL, "wide_mix_matrix: not a mix tile of a qualifying run (class 6 of psmc_hip_wide_plan_tiles), or dir is not 0 or 1");
	const int64_t ms = (int64_t)c->n * wf_width(c), nf = (c->wg_mx_T + 3) / 4, at = 2 * (int64_t)c->wg_mix_slot[tile] + dir;
	if (std::find(c->wg_mix_jobs.begin(), c->wg_mix_jobs.end(), (int32_t)at) == c->wg_mix_jobs.end())
		return fail(c, PSMC_HIP_ESTATE, "wide_mix_matrix: no chain of the plan crosses this tile in this direction (psmc_hip_wide_gap_chains), so the last wide fast E-step built no such matrix");
	if (cap > 0) { // the matrix, then its pilot's factors (which lie behind all matrices)
		HIPCHK(c, hipSetDevice(c->device));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		HIPCHK(c, hipMemcpy(out, c->d_wg_Mx + at * ms, sizeof(double) * (size_t)std::min(cap, ms), hipMemcpyDeviceToHost));
		if (cap > ms) HIPCHK(c, hipMemcpy(out + ms, c->d_wg_Mx + 2 * (int64_t)c->wg_mx_n * ms + at * nf, sizeof(double) * (size_t)std::min(cap - ms, nf), hipMemcpyDeviceToHost));
	}
	return ms + nf;
}

extern "C" int64_t psmc_hip_wide_tile_vectors(psmc_hip_ctx *c, int which, double *out, int64_t cap)
{
	if (!c || which < 0 || which > 1 || cap < 0 || (cap > 0 && !out)) return PSMC_HIP_EINVAL;
	if (c->plan_dirty || c->wf_chunks.empty() || !c->wf_ran) return no_wide_plan(c, "wide_tile_vectors");
	const double *src = which ? c->d_wf_bentry : c->d_wf_entry;
	if (!src) return no_wide_plan(c, "wide_tile_vectors");
	const int64_t len = (int64_t)c->wf_chunks.size() * wf_width(c);
	if (cap > 0) {
		HIPCHK(c, hipSetDevice(c->device));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		HIPCHK(c, hipMemcpy(out, src, sizeof(double) * (size_t)std::min(cap, len), hipMemcpyDeviceToHost));
	}
	return len;
}

// ---- the transfer-matrix chains of the fast path up to 128 states (api_fast.hip build_items, estep_struct.hip k_kcol_struct / k_kcol2_struct /
// k_kchain_struct): host reads and plain copies behind a stream synchronise, no kernel.  build_items keeps its lists on the device only:
// they are copied from d_items at the offsets enqueue_fast hands to the launch.
static int no_fast_lists(psmc_hip_ctx *c, const char *who)
{
	std::string msg = std::string(who) + ": no current fast plan with built item lists (run a structured fast E-step at up to 128 states first)";
	return fail(c, PSMC_HIP_ESTATE, msg.c_str());
}
static bool fast_lists_ok(const psmc_hip_ctx *c)
{
	// (dec_kind: the last fast E-step of this context succeeded, so build_items has run for the current plan)
	return c->mode == PSMC_HIP_MODE_FAST && c->ns <= 128 && !c->wf_ran && !c->plan_dirty && !c->chunks.empty() && c->use_struct && c->planned_struct &&
	       c->d_items && c->dec_kind != DEC_NONE && c->dec_kind != DEC_EXACT;
}

extern "C" int psmc_hip_fast_chain_info(psmc_hip_ctx *c, int out[8])
{
	if (!c || !out) return PSMC_HIP_EINVAL;
	if (!fast_lists_ok(c)) return no_fast_lists(c, "fast_chain_info");
	out[0] = c->n_chain_f; out[1] = c->n_chain_b; out[2] = c->n_kc; out[3] = c->n_kuniq;
	out[4] = kcol2_on(c) ? c->kc_sub_used : 1; out[5] = c->ns; out[6] = (int)c->chunks.size(); out[7] = c->chunk_used;
	return PSMC_HIP_OK;
}

extern "C" int psmc_hip_fast_chain_list(psmc_hip_ctx *c, int which, int32_t *out, int cap)
{
	if (!c || which < 0 || which > 3 || cap < 0 || (cap > 0 && !out)) return PSMC_HIP_EINVAL;
	if (!fast_lists_ok(c)) return no_fast_lists(c, "fast_chain_list");
	const size_t nc = c->chunks.size();
	// d_items + 16 nc: KcTile (tile, dir) | + 20 nc: KcRun (first, count, kc0, pad), forward runs then backward | + 26 nc: kslot | + 28 nc: kuniq
	const size_t off = which == 0 ? 20 * nc : (which == 1 ? 16 * nc : (which == 2 ? 26 * nc : 28 * nc));
	const int len = c->n_kc <= 0 ? 0 : (which == 0 ? 4 * (c->n_chain_f + c->n_chain_b) : (which == 1 ? 2 * c->n_kc : (which == 2 ? c->n_kc : c->n_kuniq)));
	if (cap > 0 && len > 0) {
		HIPCHK(c, hipSetDevice(c->device));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		HIPCHK(c, hipMemcpy(out, c->d_items + off, sizeof(int) * (size_t)std::min(cap, len), hipMemcpyDeviceToHost));
	}
	return len;
}

extern "C" int64_t psmc_hip_fast_chain_matrices(psmc_hip_ctx *c, double *out, int64_t cap)
{
	if (!c || cap < 0 || (cap > 0 && !out)) return PSMC_HIP_EINVAL;
	if (!fast_lists_ok(c)) return no_fast_lists(c, "fast_chain_matrices");
	const int64_t sub = kcol2_on(c) ? c->kc_sub_used : 1;
	const int64_t len = c->n_kc <= 0 || !c->d_Kcol ? 0 : (int64_t)c->n_kuniq * sub * ((int64_t)c->ns * c->ns + c->ns);
	if (cap > 0 && len > 0) {
		HIPCHK(c, hipSetDevice(c->device));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		HIPCHK(c, hipMemcpy(out, c->d_Kcol, sizeof(double) * (size_t)std::min(cap, len), hipMemcpyDeviceToHost));
	}
	return len;
}

extern "C" int64_t psmc_hip_fast_tile_vectors(psmc_hip_ctx *c, int which, double *out, int64_t cap)
{
	if (!c || which < 0 || which > 2 || cap < 0 || (cap > 0 && !out)) return PSMC_HIP_EINVAL;
	if (!fast_lists_ok(c)) return no_fast_lists(c, "fast_tile_vectors");
	const double *src = which == 0 ? c->d_entry : (which == 1 ? c->d_bentry : c->d_bexit);
	if (!src) return no_fast_lists(c, "fast_tile_vectors");
	const int64_t len = (int64_t)c->chunks.size() * c->ns;
	if (cap > 0) {
		HIPCHK(c, hipSetDevice(c->device));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		HIPCHK(c, hipMemcpy(out, src, sizeof(double) * (size_t)std::min(cap, len), hipMemcpyDeviceToHost));
	}
	return len;
}
