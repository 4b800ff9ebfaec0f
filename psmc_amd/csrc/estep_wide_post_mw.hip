// estep_wide_post_mw.hip -- decoding on the multi-wave wide fast path (257..1024 states, options "wide_fast" = 2 + "wide_decode";
// api_decode.hip drives it): psmc_hip_decode / _posterior / _post_counts / _scales from what the last multi-wave wide fast E-step
// (estep_wide_fast_mw.hip) left, without a backward table.  The formulas are those of estep_wide_post.hip:
//   g_p(k) = X_p(k) y(k) with y = a bt_{p+1},  G_p = sum_k g_p(k):  gamma_p(k) = g_p(k) / G_p,
//   recomb_p = 1 - sum_l X_p(l) a_ll bt_{p+1}(l) / G_p,  and at p = L: gamma_L = X_L / sum X_L, recomb_L = 0.
// A tile is ONE work-group of W = 2, 3 or 4 waves at the padded width S = 256 W, thread t holds the states 4t .. 4t+3
// (wide_mw_prims.h).  The backward step is mw_step of the E-step with the emission and scaling of mw_bstep, so bt is the E-step's bt.
//   k_mwp_dec    the sweep from the tile's converged bentry: posterior rows | recombination | argmax and its value | per-tile
//                partial posterior-weighted counts, CB count columns per sweep.  Two exchanges per position: the step's own, in
//                which r = sum X a_kk bt_{p+1} rides (slot 3, free in mw_step: it does not depend on y), and one for G and, for
//                the path, every wave's maximum and the state that holds it (an index up to 1023 is exact in a double).  The tie rule: within
//                a wave the lowest state of the lowest lane, across waves the lowest wave whose maximum equals the tile's -- the
//                lowest state wins.  iG comes from exchanged values only: the same bits in every wave.  Position L: one exchange.
//   k_wp_cnt_add (estep_wide_post.hip, at S = 512 / 768 / 1024) the tiles' partials added in tile order
//   k_mwp_scales s_p = sum X_p / sum X_{p-1} / inv_p; ONE wave per tile adds the W blocks of 256 states of a row, lowest block
//                first: no LDS, no barrier
// Posterior rows have stride n; padded states are never written, and a tile writes the positions lo .. hi it owns and nothing else.
//
// What keeps a work-group from hanging (the rule of estep_wide_fast_mw.hip): every branch that encloses an exchange depends only
// on values that are the same in all waves of the work-group.  In k_mwp_dec these are: `c.hi == c.L` and `top >= lo` (the tile
// descriptor, global memory nobody writes during the launch), the bounds of the loop over groups of four positions (top, lo),
// `p > top || p < lo` (p from the loop counters) and the template flags.  `p <= min_l` (the counts) and `k0 + i < n`, `tid == 0`
// (the stores) enclose no exchange.  k_mwp_scales has no exchange and no barrier.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; scratch is 0 everywhere; LDS = 2 x 6 x W doubles):
//   kernel                       W=2: VGPRs  LDS    W=3: VGPRs  LDS    W=4: VGPRs  LDS
//   k_mwp_dec  path                     124   192          128   288          132   384
//   k_mwp_dec  posterior                124   192          128   288          130   384
//   k_mwp_dec  recombination            130   192          134   288          138   384
//   k_mwp_dec  posterior + recomb.      132   192          136   288          138   384
//   k_mwp_dec  counts                   156   192          160   288          162   384
//   k_mwp_scales                    22 / 30 / 40 VGPRs at W = 2 / 3 / 4, no LDS
// "wide_decode_ckpt" (compile-time variants CKPT of k_mwp_dec, and k_mwp_scales_ck; the full-table kernels keep their code): after a
// "wide_ckpt" E-step X holds the rows at p % 8 == 0 only and xhi[b] every tile's last row.  k_mwp_dec CKPT sweeps the tile in blocks
// of eight positions, the top block first: the block's rows recomputed forward with mw_fstep and the stored scale factors into LDS
// (7 rows of S doubles beside the exchange slots, as k_mw_acc CKPT of estep_wide_fast_mw.hip), then the same backward step and
// mw_emit over them.  k_mwp_scales_ck: the tile's W waves step forward once and sum every row through the exchange, lowest block of
// 256 states first -- the order of k_mwp_scales.  The hang rule holds: the block bounds (q, pb, pe), the recompute's start
// (`q >= lo`, `lo > 1`) and `p & 3` come from the tile descriptor and the loop counters only, the same in every wave; in
// k_mwp_scales_ck `c.lo > 1` and the loop over lo .. hi likewise.
//   k_mwp_dec  path, CKPT               140   28864        136   43296        138   57728
//   k_mwp_dec  posterior, CKPT          124   28864        128   43296        128   57728
//   k_mwp_dec  recombination, CKPT      132   28864        136   43296        136   57728
//   k_mwp_dec  posterior + recomb., CKPT 132  28864        136   43296        136   57728
//   k_mwp_dec  counts, CKPT             156   28864        160   43296        160   57728
//   k_mwp_scales_ck                     106   192          110   288          112   384
// With CKPT the staged rows bound a compute unit at five (W = 2), three (W = 3) or two (W = 4) work-groups of its 160 KB of LDS.
#include <hip/hip_runtime.h>
#include "wide_fast.h"
#include "wide_prims.h"
#include "wide_mw_prims.h"

namespace psmc {
namespace wide {

constexpr int MWP_CB = 4; // count columns one sweep of k_mwp_dec carries (as CB of estep_wide_post.hip)

// what one position hands out: g = unnormalised posterior of the thread's states, r = sum_l X a_ll bt_{p+1} over the TILE (from the
// step's exchange), last: position L, whose recombination probability is 0.  One exchange; every wave of the tile calls it.
template <int W, bool POST, bool REC, bool PATH, bool CNT>
__device__ __forceinline__ void mw_emit(int p, int tid, int n, const double (&g)[MW_NPL], double r, bool last, Xchg<W> &xc,
                                        double *__restrict__ post, double *__restrict__ recomb, int32_t *__restrict__ path,
                                        double *__restrict__ maxp, const int32_t *__restrict__ cnt1, int n_cnt, int j0, int min_l,
                                        double (&acc)[MWP_CB][MW_NPL])
{
	constexpr int NPL = MW_NPL;
	const int k0 = NPL * tid;
	xc.put(0, wave_total(lsum<NPL>(g)));
	if (PATH) { // the wave's first maximum: the lowest i of the lane, then the lowest lane that holds the wave's maximum
		double best = g[0]; int arg = 0;
#pragma unroll
		for (int i = 1; i < NPL; ++i)
			if (g[i] > best) { best = g[i]; arg = i; }
		const double wtop = wave_maxv(best);
		const unsigned long long who = __ballot(best == wtop);
		const int src = who ? __ffsll((long long)who) - 1 : 0;
		const int k = __shfl(k0 + arg, src, 64);
		xc.put(1, wtop); xc.put(2, (double)k);
	}
	xc.sync();
	const double iG = rcp_newton(xc.sum(0));
	double top = 0.0, ktop = 0.0;
	if (PATH) { // the lowest wave whose maximum is the tile's
		top = xc.vmax(1);
		ktop = xc.get(2, 0);
#pragma unroll
		for (int w = W - 1; w >= 1; --w)
			if (xc.get(1, w) == top) ktop = xc.get(2, w);
		if (xc.get(1, 0) == top) ktop = xc.get(2, 0); // (no wave's maximum equals it -- a NaN: wave 0's, as the one-wave kernel's lane 0)
	}
	xc.next();
	if (POST) {
		double *row = post + (int64_t)(p - 1) * n;
#pragma unroll
		for (int i = 0; i < NPL; ++i)
			if (k0 + i < n) row[k0 + i] = g[i] * iG;
	}
	if (REC && tid == 0) recomb[p - 1] = last ? 0.0 : 1.0 - r * iG;
	if (PATH && tid == 0) { path[p - 1] = (int32_t)ktop; maxp[p - 1] = top * iG; }
	if (CNT && p <= min_l) {
		const int32_t *c1 = cnt1 + (int64_t)(p - 1) * n_cnt + j0;
#pragma unroll
		for (int j = 0; j < MWP_CB; ++j) {
			const double w = j0 + j < n_cnt ? (double)c1[j] : 0.0;
#pragma unroll
			for (int i = 0; i < NPL; ++i) acc[j][i] = __builtin_fma(g[i] * iG, w, acc[j][i]);
		}
	}
}

// Tile t0 + blockIdx.x of the plan (the tiles of one segment are consecutive).  Output pointers are the SEGMENT's (position 1 first).
// CNT: part[(blockIdx.x * n_cnt + j) * S + k] for the columns j0 .. j0 + MWP_CB - 1 that exist.
// CKPT ("wide_decode_ckpt" after a "wide_ckpt" E-step): as k_mw_acc CKPT (estep_wide_fast_mw.hip) -- block by block from the tile's top
// block down, the block's rows recomputed forward with mw_fstep and the stored scale factors (every recomputed step's exchange as
// k_mw_fwd does it) into LDS (7 S doubles beside the exchange slots; every thread reads back what it wrote itself), then the
// backward step and mw_emit of the full-table sweep over them, X_{8m} read from the table, X_L from xhi[b].  The block bounds come from
// the tile descriptor and the loop counters alone, so every wave of the work-group goes through the same exchanges.
template <int W, bool POST, bool REC, bool PATH, bool CNT, bool CKPT>
__global__ __launch_bounds__(64 * W) void k_mwp_dec(const double *__restrict__ par, const uint8_t *__restrict__ obs,
                                                      const Chunk *__restrict__ chunks, int t0, const double *__restrict__ X,
                                                      const double *__restrict__ inv, const double *__restrict__ entry,
                                                      const double *__restrict__ xhi, const double *__restrict__ bentry, int n,
                                                      double *__restrict__ post, double *__restrict__ recomb, int32_t *__restrict__ path,
                                                      double *__restrict__ maxp, const int32_t *__restrict__ cnt1, int n_cnt, int j0,
                                                      int min_l, double *__restrict__ part)
{
	constexpr int NPL = MW_NPL, S = 64 * NPL * W;
	__shared__ double xs[2 * MW_SLOTS * W];
	Xchg<W> xc = mw_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid, b = t0 + (int)blockIdx.x;
	const WaveScanMasks wm = wave_scan_masks(xc.lane);
	const Chunk c = chunks[b];
	const int lo = c.lo, top = min(c.hi, c.L - 1);
	StructParN<NPL> sc;
	mw_load_bwd<S>(par, k0, sc);
	double e0[NPL], e1[NPL], acc[MWP_CB][NPL];
	ld<NPL>(par + WP_E0 * S + k0, e0); ld<NPL>(par + WP_E1 * S + k0, e1);
#pragma unroll
	for (int j = 0; j < MWP_CB; ++j)
#pragma unroll
		for (int i = 0; i < NPL; ++i) acc[j][i] = 0.0;
	const uint8_t *o = obs + c.off;
	const double *fo = X + c.off * S + k0;
	if (c.hi == c.L) { // position L: beta_L = 1 (the same in every wave)
		double g[NPL];
		if (CKPT) ld<NPL>(xhi + (int64_t)b * S + k0, g); else ld<NPL>(fo + (int64_t)(c.L - 1) * S, g);
		mw_emit<W, POST, REC, PATH, CNT>(c.L, tid, n, g, 0.0, true, xc, post, recomb, path, maxp, cnt1, n_cnt, j0, min_l, acc);
	}
	if (CKPT && top >= lo) { // (the same in every wave, and so is every bound below: lo, top and the loop counters)
		__shared__ double rows[(WCK - 1) * S];
		double *my = rows + k0;
		const double *io = inv + c.off;
		double x[NPL];
		ld<NPL>(bentry + (int64_t)b * S + k0, x);
		for (int q = top & ~(WCK - 1); q + WCK - 1 >= lo; q -= WCK) { // the block of the positions q .. q+7, within lo .. top
			const int pb = max(lo, q), pe = min(top, q + WCK - 1);
			{
				StructParN<NPL> fs;
				fwd_roles<NPL>(sc, fs);
				double xf[NPL];
				int p;
				if (q >= lo) { ld<NPL>(X + ckpt_row(c.off, q) * S + k0, xf); p = q + 1; }
				else if (lo > 1) { ld<NPL>(entry + (int64_t)b * S + k0, xf); p = lo; }
				else { // X_1 = a0 e[o_1], as the forward sweep starts a segment
					double ev[NPL];
					ld<NPL>(par + WP_A0 * S + k0, xf);
					emis<NPL>((int)o[0] & 3, e0, e1, ev);
#pragma unroll
					for (int i = 0; i < NPL; ++i) xf[i] *= ev[i];
					st<NPL>(my, xf);
					p = 2;
				}
				for (; p <= pe; ++p) { // (one exchange per step, in every wave)
					const int sym = (int)o[p - 1] & 3;
					if ((p & 3) == 0) mw_fstep<W, true, true>(fs, wm, sym, e0, e1, xf, io[p - 1], xc);
					else mw_fstep<W, false, true>(fs, wm, sym, e0, e1, xf, 1.0, xc);
					st<NPL>(my + ((p & (WCK - 1)) - 1) * S, xf);
				}
			}
			for (int p = pe; p >= pb; --p) { // (two exchanges per position, in every wave)
				double Xc[NPL], ev[NPL], y[NPL], g[NPL];
				if (p & (WCK - 1)) ld<NPL>(my + ((p & (WCK - 1)) - 1) * S, Xc); else ld<NPL>(X + ckpt_row(c.off, p) * S + k0, Xc);
				emis<NPL>((int)o[p - 1] & 3, e0, e1, ev);
				double r = 0.0;
#pragma unroll
				for (int i = 0; i < NPL; ++i) {
					y[i] = x[i];
					if (REC) r = __builtin_fma(Xc[i] * (sc.dd[i] + sc.wP[i] * sc.mP[i] + sc.wS[i] * sc.mS[i]), x[i], r); // a[k][k]
				}
				const Xchg<W> ex = xc; // r rides in slot 3 of the step's own exchange, as in the full-table sweep below
				if (REC) ex.put(3, wave_total(r));
				const bool norm = (p & 3) == 0; // the backward sweep's own scaling 1 / sum(bt_{p+1}), as mw_bstep
				const double tot = norm ? mw_step<W, true>(sc, y, wm, xc) : mw_step<W, false>(sc, y, wm, xc);
				if (REC) r = ex.sum(3);
				if (norm) {
					const double sb = rcp_newton(tot);
#pragma unroll
					for (int i = 0; i < NPL; ++i) ev[i] *= sb;
				}
#pragma unroll
				for (int i = 0; i < NPL; ++i) { g[i] = Xc[i] * y[i]; x[i] = y[i] * ev[i]; }
				mw_emit<W, POST, REC, PATH, CNT>(p, tid, n, g, r, false, xc, post, recomb, path, maxp, cnt1, n_cnt, j0, min_l, acc);
			}
		}
	}
	if (!CKPT && top >= lo) { // (the same in every wave)
		double x[NPL], Xc[NPL], Xn[NPL];
		ld<NPL>(bentry + (int64_t)b * S + k0, x);
		ld<NPL>(fo + (int64_t)(top - 1) * S, Xc);
		for (int g4 = (top - 1) >> 2; g4 >= 0 && 4 * g4 + 4 >= lo; --g4) {
			const unsigned w = *reinterpret_cast<const unsigned *>(o + 4 * (int64_t)g4);
#pragma unroll
			for (int j = 3; j >= 0; --j) {
				const int p = 4 * g4 + j + 1;
				if (p > top || p < lo) continue; // (the same in every wave: both exchanges below are reached by all or none)
				if (p > lo) ld<NPL>(fo + (int64_t)(p - 2) * S, Xn); // X_{p-1}, for the next step
				double ev[NPL], y[NPL], g[NPL];
				emis<NPL>((int)((w >> (8 * j)) & 3u), e0, e1, ev);
				double r = 0.0;
#pragma unroll
				for (int i = 0; i < NPL; ++i) {
					y[i] = x[i];
					if (REC) r = __builtin_fma(Xc[i] * (sc.dd[i] + sc.wP[i] * sc.mP[i] + sc.wS[i] * sc.mS[i]), x[i], r); // a[k][k]
				}
				// r rides in slot 3 of the step's own exchange, which mw_step leaves free: published before the step's barrier, read
				// after it through a copy of the exchange as it stood (that buffer is written again only two barriers later)
				const Xchg<W> ex = xc;
				if (REC) ex.put(3, wave_total(r));
				// y <- a bt_{p+1}; p % 4 == 0: the backward sweep's own scaling 1 / sum(bt_{p+1}), as mw_bstep
				const double tot = j == 3 ? mw_step<W, true>(sc, y, wm, xc) : mw_step<W, false>(sc, y, wm, xc);
				if (REC) r = ex.sum(3);
				if (j == 3) {
					const double sb = rcp_newton(tot);
#pragma unroll
					for (int i = 0; i < NPL; ++i) ev[i] *= sb;
				}
#pragma unroll
				for (int i = 0; i < NPL; ++i) { g[i] = Xc[i] * y[i]; x[i] = y[i] * ev[i]; }
				mw_emit<W, POST, REC, PATH, CNT>(p, tid, n, g, r, false, xc, post, recomb, path, maxp, cnt1, n_cnt, j0, min_l, acc);
#pragma unroll
				for (int i = 0; i < NPL; ++i) Xc[i] = Xn[i];
			}
		}
	}
	if (CNT) {
#pragma unroll
		for (int j = 0; j < MWP_CB; ++j)
			if (j0 + j < n_cnt) st<NPL>(part + ((int64_t)blockIdx.x * n_cnt + j0 + j) * S + k0, acc[j]);
	}
}

// one wave per tile; the sum of a row: the W blocks of 256 states, lowest first (every lane holds the same bits)
template <int W> __device__ __forceinline__ double mwp_rowsum(const double *__restrict__ row)
{
	double u[MW_NPL];
	ld<MW_NPL>(row, u);
	double t = wave_total(lsum<MW_NPL>(u));
#pragma unroll
	for (int w = 1; w < W; ++w) {
		ld<MW_NPL>(row + 256 * w, u);
		t += wave_total(lsum<MW_NPL>(u));
	}
	return t;
}
template <int W>
__global__ __launch_bounds__(64) void k_mwp_scales(const Chunk *__restrict__ chunks, int t0, const double *__restrict__ X,
                                                     const double *__restrict__ inv, const double *__restrict__ entry, double *__restrict__ s)
{
	constexpr int S = 256 * W;
	const int lane = threadIdx.x, k0 = MW_NPL * lane, b = t0 + (int)blockIdx.x;
	const Chunk c = chunks[b];
	const double *fo = X + c.off * S + k0, *io = inv + c.off;
	double prev = 1.0;
	if (c.lo > 1) prev = mwp_rowsum<W>(entry + (int64_t)b * S + k0);
	for (int p = c.lo; p <= c.hi; ++p) {
		const double cur = mwp_rowsum<W>(fo + (int64_t)(p - 1) * S);
		double v = p == 1 ? cur : cur / prev; // X_1 = a0 e[o_1] as it stands
		if (p > 1 && (p & (NORM_EVERY - 1)) == 0) v /= io[p - 1];
		if (lane == 0) s[p - 1] = v;
		prev = cur;
	}
}

// CKPT: the scales without the table -- the tile's W waves step forward from entry[b] (or X_1 = a0 e[o_1], stored as it stands) with
// mw_fstep and the stored factors: the forward sweep's rows.  A row's sum goes through the exchange, which adds the waves' blocks
// of 256 states lowest block first -- the order of mwp_rowsum.  Two exchanges per position, reached by every wave: the loop bounds
// come from the tile descriptor alone, and `c.lo > 1` is the same in every wave.
template <int W>
__global__ __launch_bounds__(64 * W) void k_mwp_scales_ck(const double *__restrict__ par, const uint8_t *__restrict__ obs,
                                                            const Chunk *__restrict__ chunks, int t0, const double *__restrict__ inv,
                                                            const double *__restrict__ entry, double *__restrict__ s)
{
	constexpr int NPL = MW_NPL, S = 64 * NPL * W;
	__shared__ double xs[2 * MW_SLOTS * W];
	Xchg<W> xc = mw_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid, b = t0 + (int)blockIdx.x;
	const WaveScanMasks wm = wave_scan_masks(xc.lane);
	const Chunk c = chunks[b];
	StructParN<NPL> sc, fs;
	mw_load_bwd<S>(par, k0, sc);
	fwd_roles<NPL>(sc, fs);
	double e0[NPL], e1[NPL], x[NPL], prev;
	ld<NPL>(par + WP_E0 * S + k0, e0); ld<NPL>(par + WP_E1 * S + k0, e1);
	const uint8_t *o = obs + c.off;
	const double *io = inv + c.off;
	int p = c.lo;
	if (c.lo > 1) { ld<NPL>(entry + (int64_t)b * S + k0, x); prev = mw_vsum<W>(xc, x); }
	else {
		double ev[NPL];
		ld<NPL>(par + WP_A0 * S + k0, x);
		emis<NPL>((int)o[0] & 3, e0, e1, ev);
#pragma unroll
		for (int i = 0; i < NPL; ++i) x[i] *= ev[i];
		prev = mw_vsum<W>(xc, x);
		if (tid == 0) s[0] = prev;
		p = 2;
	}
	for (; p <= c.hi; ++p) {
		const int sym = (int)o[p - 1] & 3;
		const bool norm = (p & (NORM_EVERY - 1)) == 0;
		if (norm) mw_fstep<W, true, true>(fs, wm, sym, e0, e1, x, io[p - 1], xc);
		else mw_fstep<W, false, true>(fs, wm, sym, e0, e1, x, 1.0, xc);
		const double cur = mw_vsum<W>(xc, x);
		double v = cur / prev;
		if (norm) v /= io[p - 1];
		if (tid == 0) s[p - 1] = v;
		prev = cur;
	}
}

template <int W, bool CKPT> static int launch_post_mw(const WidePost &w)
{
	const dim3 grid(w.n_tiles), blk(64 * W);
	hipStream_t st = w.stream;
#define MWP_DEC(POST, REC, PATH, CNT, j0) \
	hipLaunchKernelGGL((k_mwp_dec<W, POST, REC, PATH, CNT, CKPT>), grid, blk, 0, st, w.par, w.obs, w.chunks, w.t0, w.X, w.inv, w.entry, w.xhi, \
	                   w.bentry, w.n_states, w.post, w.recomb, w.path, w.maxp, w.cnt1, w.n_cnt, j0, w.min_l, w.part)
	switch (w.what) {
	case WP_PATH: MWP_DEC(false, false, true, false, 0); break;
	case WP_POST: MWP_DEC(true, false, false, false, 0); break;
	case WP_REC: MWP_DEC(false, true, false, false, 0); break;
	case WP_POST_REC: MWP_DEC(true, true, false, false, 0); break;
	case WP_COUNTS:
		for (int j0 = 0; j0 < w.n_cnt; j0 += MWP_CB) MWP_DEC(false, false, false, true, j0);
		if (hipGetLastError() != hipSuccess) return -1;
		return launch_wide_post_cnt_add(w);
	case WP_SCALES:
		if (CKPT) hipLaunchKernelGGL(k_mwp_scales_ck<W>, grid, blk, 0, st, w.par, w.obs, w.chunks, w.t0, w.inv, w.entry, w.s);
		else hipLaunchKernelGGL(k_mwp_scales<W>, grid, dim3(64), 0, st, w.chunks, w.t0, w.X, w.inv, w.entry, w.s);
		break;
	default: return -1;
	}
#undef MWP_DEC
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace wide

int launch_wide_post_mw(const WidePost &w)
{
	if (w.ns != 256 * w.waves) return -1;
	const bool ck = w.ckpt == wide::WCK; // as launch_wide_post
	if (w.ckpt != 1 && !(ck && w.xhi)) return -1;
	if (w.waves == 2) return ck ? wide::launch_post_mw<2, true>(w) : wide::launch_post_mw<2, false>(w);
	if (w.waves == 3) return ck ? wide::launch_post_mw<3, true>(w) : wide::launch_post_mw<3, false>(w);
	if (w.waves == 4) return ck ? wide::launch_post_mw<4, true>(w) : wide::launch_post_mw<4, false>(w);
	return -1;
}

} // namespace psmc
