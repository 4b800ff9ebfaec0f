// estep_wide_post.hip -- decoding on the wide fast path (129..1024 states, options "wide_fast" + "wide_decode"; api_decode.hip
// drives it): psmc_hip_decode / _posterior / _post_counts / _scales / _post_mean / _post_quantile from what the last wide fast E-step left, without a backward table.
//
// The E-step keeps the lag-normalised forward table X (and 1/d_p at p % 4 == 0), every tile's forward start vector `entry` and its
// backward start vector bentry = bt_{top+1}, converged to "warm_tol" by the verify / repair rounds.  One more backward sweep per
// tile from bentry -- bstep_parts of wide_prims.h, the step of k_wf_bwarm, with the scaling of k_wf_acc, so the bt of the E-step --
// gives at every position p, with y = a bt_{p+1} (O(N)),
//   g_p(k) = X_p(k) y(k),  G_p = sum_k g_p(k):  posterior gamma_p(k) = g_p(k) / G_p  (what E0 / E1 of the E-step add up; no division
//            by an emission, so zero emissions and padded states are no special case),
//   recomb_p = 1 - sum_l X_p(l) a_ll bt_{p+1}(l) / G_p  (aux.c:189-193),  and at p = L: gamma_L = X_L / sum X_L, recomb_L = 0.
// A tile is one work-group of W waves, thread t holds the states NPL t .. NPL t + NPL - 1, as in estep_wide_fast.hip (wide_prims.h:
// the exchange between the waves and the hang rule, which holds here -- see k_wp_dec).  Nothing of 8 S bytes per bin is written:
// only what was asked for (template flags) -- -d moves 12 bytes per bin.  Posterior rows have stride n; padded states are never
// written, and a tile writes the positions lo .. hi it owns and nothing else.
//   k_wp_dec     the sweep: posterior rows | recombination | argmax (lowest state wins a tie) and its value | per-tile partial
//                posterior-weighted counts, CB count columns per sweep.  Two exchanges per position: the step's own, in which
//                r = sum X a_kk bt_{p+1} rides (it does not depend on y), and one for G and, for the path, every wave's maximum
//                and the state that holds it (an index up to 1023 is exact in a double).  iG comes from exchanged values only:
//                the same bits in every wave.  Position L: one exchange.
//                MEAN (psmc_hip_post_mean): instead of rows, up to four posterior expectations sum_k gamma_p(k) w_j(k) per position.  A
//                thread keeps the NPL x n_w weights of its states in registers; a wave's share of sum_k g_p(k) w_j(k) rides in slot
//                1 + j of the exchange that carries G (WX_SLOTS = 6: G and four columns), and mean_j = that sum * iG, stored by thread 0
//                QUANT (psmc_hip_post_quantile): instead of rows, per position the state at up to four posterior quantiles, from the
//                prefix sums of g and G alone -- no division and NO further exchange: the waves' totals that make G also tell every
//                wave which wave holds the quantile (see emit)
//   k_wp_cnt_add the tiles' partials added in tile order (deterministic)
//   k_wp_scales  s_p = sum X_p / sum X_{p-1} / inv_p from X alone (X_{lo-1}: the tile's own `entry`), s_1 = sum_k a0_k e_k(o_1).
//                ONE wave per tile at every width adds the W blocks of 64 NPL states of a row, lowest block first: no LDS, no barrier
//
// "wide_decode_ckpt" (compile-time variants CKPT of k_wp_dec, and k_wp_scales_ck): after a "wide_ckpt" E-step X holds the rows at
// p % 8 == 0 only (wide_prims.h ckpt_row) and xhi[b] every tile's last row.  k_wp_dec CKPT sweeps the tile in blocks of eight
// positions, the top block first, recomputing the block's rows forward into LDS with fstep -- the forward sweep's own step and its
// stored scale factors, as k_wf_acc CKPT of estep_wide_fast.hip -- and then runs the same backward step and emit over them;
// k_wp_scales_ck makes one forward pass per tile, all W waves, and sums every row through the exchange, lowest block first -- the
// order of k_wp_scales.  The same bits as from the full table.
//
// Resources (hipcc -O3, gfx950, make resources; scratch is 0 everywhere).  Per shape (NPL, W): VGPRs | LDS bytes per work-group |
// waves per SIMD.  LDS = the exchange slots, 2 x 6 x W doubles at W > 1, plus with CKPT 7 rows of S doubles in k_wp_dec.
//   kernel                               (3,1) S=192      (4,1) S=256      (4,2) S=512      (4,3) S=768      (4,4) S=1024
//   k_wp_dec  path                           98     0 4      122     0 4      124   192 4      128   288 4      132   384 3
//   k_wp_dec  path, CKPT                    102 10752 4      124 14336 3      136 28864 3      132 43296 3      136 57728 2
//   k_wp_dec  posterior                      96     0 5      122     0 4      124   192 4      128   288 4      130   384 3
//   k_wp_dec  posterior, CKPT                92 10752 4      116 14336 3      118 28864 3      124 43296 3      128 57728 2
//   k_wp_dec  recombination                 100     0 4      126     0 4      130   192 3      134   288 3      138   384 3
//   k_wp_dec  recombination, CKPT           102 10752 4      128 14336 3      130 28864 3      134 43296 3      136 57728 2
//   k_wp_dec  posterior + recomb.           102     0 4      130     0 3      132   192 3      136   288 3      138   384 3
//   k_wp_dec  posterior + recomb., CKPT     102 10752 4      128 14336 3      130 28864 3      134 43296 3      136 57728 2
//   k_wp_dec  counts                        118     0 4      152     0 3      156   192 3      160   288 3      162   384 3
//   k_wp_dec  counts, CKPT                  116 10752 4      148 14336 3      150 28864 3      156 43296 3      160 57728 2
//   k_wp_dec  mean                          126     0 4      158     0 3      154   192 3      158   288 3      162   384 3
//   k_wp_dec  mean, CKPT                    124 10752 4      156 14336 3      150 28864 3      156 43296 3      160 57728 2
//   k_wp_dec  quantiles                      94     0 5      118     0 4      124   192 4      126   288 4      130   384 3
//   k_wp_dec  quantiles, CKPT                92 10752 4      116 14336 3      118 28864 3      124 43296 3      128 57728 2
//   k_wp_scales (64 threads)                16     0 8       16     0 8       22     0 8       30     0 8       40     0 8
//   k_wp_scales_ck                           80     0 6      102     0 4      106   192 4      110   288 4      112   384 4
//   k_wp_cnt_add                         8 VGPRs at every width, no LDS
// With CKPT the staged rows bound a compute unit at 15 tiles (S = 192), 11 (256), five (512), three (768) or two (1024) of its
// 160 KB of LDS.
#include <hip/hip_runtime.h>
#include "wide_fast.h"
#include "wide_prims.h"

namespace psmc {
namespace wide {

constexpr int CB = 4; // count columns one sweep of k_wp_dec carries (CB x NPL accumulators per thread)

// what one position hands out: g = unnormalised posterior of the thread's states, r = sum_l X a_ll bt_{p+1} over the TILE (from the
// step's exchange), last: position L, whose recombination probability is 0.  One exchange (G; PATH: the waves' maxima); every wave
// of the tile calls it.  The tie rule of the path: within a wave the lowest state of the lowest lane that holds the wave's
// maximum, across waves the lowest wave whose maximum equals the tile's -- the lowest state wins (a NaN: wave 0's, lane 0's).
// MEAN (psmc_hip_post_mean): wt = the weights of the thread's states, column by column; the wave's share of sum_k g(k) w_j(k) rides
// in slot 1 + j of the same exchange (PATH, which uses the slots 1 and 2, is never on with it), and mean_j = that sum * iG.
// QUANT (psmc_hip_post_quantile; never on with PATH or MEAN): state_j = min(n - 1, #{k < n : c_k < x_j}), x_j = q_j G, over the prefix
// sums c_k = (the totals of the waves below + the sums of the lanes below) + the lane's running sum up to k.  With P_w = the totals
// of the waves 0 .. w added lowest first (what below(0) of wave w + 1 is), every wave finds from the exchanged totals alone
// w* = the lowest wave whose P_w is not below x_j (the last wave when there is none), and wave w* stores
//   min(n, 64 NPL w*) + #{k of wave w*, k < n : c_k < x_j}:
// every state of a wave below w* counts (its prefix is at most P_{w*-1} < x_j up to the rounding of the sums) and none above.  One
// wave stores each column, from exchanged values and its own registers: unique, and the same on every run.  A NaN total: P_0 is not
// below it, wave 0 stores its count, 0.  Padded states are left out by the test k < n itself.
template <int NPL, int W, bool POST, bool REC, bool PATH, bool CNT, bool MEAN, bool QUANT>
__device__ __forceinline__ void emit(int p, int tid, int n, const double (&g)[NPL], double r, bool last, Xchg<W> &xc,
                                     double *__restrict__ post, double *__restrict__ recomb, int32_t *__restrict__ path,
                                     double *__restrict__ maxp, const int32_t *__restrict__ cnt1, int n_cnt, int j0, int min_l,
                                     double (&acc)[CB][NPL], const double (&wt)[MEAN_COLS][NPL], int n_w, double *__restrict__ mean,
                                     const QuantQ &qq, int n_q, int32_t *__restrict__ qstate)
{
	static_assert(!(MEAN && PATH) && 1 + MEAN_COLS <= WX_SLOTS, "G takes slot 0 and every column of weights one more slot");
	static_assert(!(QUANT && (PATH || MEAN)), "the quantiles are a sweep of their own");
	const int k0 = NPL * tid;
	xc.put(0, wave_total(lsum<NPL>(g)));
	double run[NPL], lanes_below = 0.0; // QUANT: the lane's running sums (run[NPL - 1] is lsum's own sequence) and the sum of the lanes below
	if (QUANT) {
		run[0] = g[0];
#pragma unroll
		for (int i = 1; i < NPL; ++i) run[i] = run[i - 1] + g[i];
		lanes_below = wave_excl_prefix(run[NPL - 1]);
	}
	if (MEAN) { // (n_w is a kernel argument: the same in every wave)
#pragma unroll
		for (int j = 0; j < MEAN_COLS; ++j)
			if (j < n_w) {
				double t = g[0] * wt[j][0];
#pragma unroll
				for (int i = 1; i < NPL; ++i) t = __builtin_fma(g[i], wt[j][i], t);
				xc.put(1 + j, wave_total(t));
			}
	}
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
		if (xc.get(1, 0) == top) ktop = xc.get(2, 0); // (no wave's maximum equals it -- a NaN: wave 0's)
	}
	double mj[MEAN_COLS];
	if (MEAN) { // from exchanged values only: the same bits in every wave
#pragma unroll
		for (int j = 0; j < MEAN_COLS; ++j) mj[j] = j < n_w ? xc.sum(1 + j) * iG : 0.0;
	}
	if (QUANT) { // (n_q is a kernel argument; the stores sit under wave == w*, the exchange is behind us)
		const double G = xc.sum(0);
		double base = lanes_below;
		int wave = 0;
		if constexpr (W > 1) { base += xc.below(0); wave = xc.wave; }
#pragma unroll
		for (int j = 0; j < QUANT_COLS; ++j)
			if (j < n_q) {
				const double x = qq.q[j] * G;
				int ws = W - 1;
				if constexpr (W > 1) {
					double P = xc.get(0, 0);
					bool found = !(P < x);
					ws = found ? 0 : W - 1;
#pragma unroll
					for (int w = 1; w < W - 1; ++w) {
						P += xc.get(0, w);
						if (!found && !(P < x)) { found = true; ws = w; }
					}
				}
				int cnt = 0;
#pragma unroll
				for (int i = 0; i < NPL; ++i) cnt += __popcll(__ballot(k0 + i < n && base + run[i] < x));
				if (wave == ws && xc.lane == 0) qstate[(int64_t)(p - 1) * n_q + j] = min(min(n, 64 * NPL * ws) + cnt, n - 1);
			}
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
	if (MEAN && tid == 0) {
#pragma unroll
		for (int j = 0; j < MEAN_COLS; ++j)
			if (j < n_w) mean[(int64_t)(p - 1) * n_w + j] = mj[j];
	}
	if (CNT && p <= min_l) {
		const int32_t *c1 = cnt1 + (int64_t)(p - 1) * n_cnt + j0;
#pragma unroll
		for (int j = 0; j < CB; ++j) {
			const double w = j0 + j < n_cnt ? (double)c1[j] : 0.0;
#pragma unroll
			for (int i = 0; i < NPL; ++i) acc[j][i] = __builtin_fma(g[i] * iG, w, acc[j][i]);
		}
	}
}

// the backward step of one position p of the sweep: x = bt_{p+1} -> bt_p (bstep_parts: the E-step's backward step), Xc = X_p; g and
// r for emit.  One exchange, in which r rides: a wave's share goes in and the tile's sum comes back.
template <int NPL, int W, bool NORM, bool REC>
__device__ __forceinline__ void dstep(const StructParN<NPL> &sc, const WaveScanMasks &wm, int sym, const double (&e0)[NPL],
                                      const double (&e1)[NPL], const double (&akk)[NPL], const double (&Xc)[NPL], double (&x)[NPL],
                                      double (&g)[NPL], double &r, Xchg<W> &xc)
{
	double y[NPL], ev[NPL];
	r = 0.0;
	if (REC) {
#pragma unroll
		for (int i = 0; i < NPL; ++i) r = __builtin_fma(Xc[i] * akk[i], x[i], r);
		r = wave_total(r);
	}
	bstep_parts<NPL, W, NORM, REC>(sc, wm, sym, e0, e1, x, y, ev, xc, r);
#pragma unroll
	for (int i = 0; i < NPL; ++i) { g[i] = Xc[i] * y[i]; x[i] = y[i] * ev[i]; }
}

// Tile t0 + blockIdx.x of the plan (the tiles of one segment are consecutive).  Output pointers are the SEGMENT's (position 1 first).
// CNT: part[(blockIdx.x * n_cnt + j) * S + k] for the columns j0 .. j0 + CB - 1 that exist.
// CKPT ("wide_decode_ckpt" after a "wide_ckpt" E-step): X holds the rows at p % 8 == 0 only.  As k_wf_acc CKPT (estep_wide_fast.hip) the
// tile is swept in blocks of the positions 8m .. 8m+7, the top block first: the block's rows are recomputed forward with fstep and
// the stored scale factors -- the forward sweep's own bits, every recomputed step's exchange as k_wf_fwd does it -- from the
// checkpoint X_{8m}, or in the tile's lowest block from entry[b] or from X_1 = a0 e[o_1], into LDS (7 S doubles beside the exchange
// slots; every thread reads back what it wrote itself, so no barrier); then dstep and emit run over them, highest position first, X_{8m}
// read from the table.  X_L: xhi[b].  With CNT every sweep of CB columns recomputes the rows again.
// The hang rule: the branches that enclose an exchange are `c.hi == c.L` and `top >= lo` (the tile descriptor), the bounds of the
// loops (top, lo, the block bounds q, pb, pe), `p > top || p < lo`, `q >= lo`, `lo > 1` and `p & 3` (the loop counters) and the
// template flags -- the same in every wave.
template <int NPL, int W, bool POST, bool REC, bool PATH, bool CNT, bool CKPT, bool MEAN, bool QUANT>
__global__ __launch_bounds__(64 * W) void k_wp_dec(const double *__restrict__ par, const uint8_t *__restrict__ obs,
                                                     const Chunk *__restrict__ chunks, int t0, const double *__restrict__ X,
                                                     const double *__restrict__ inv, const double *__restrict__ entry,
                                                     const double *__restrict__ xhi, const double *__restrict__ bentry, int n,
                                                     double *__restrict__ post, double *__restrict__ recomb, int32_t *__restrict__ path,
                                                     double *__restrict__ maxp, const int32_t *__restrict__ cnt1, int n_cnt, int j0,
                                                     int min_l, double *__restrict__ part, const double *__restrict__ wts, int n_w,
                                                     double *__restrict__ mean, QuantQ qq, int n_q, int32_t *__restrict__ qstate)
{
	constexpr int S = 64 * NPL * W;
	__shared__ double xs[2 * WX_SLOTS * W];
	Xchg<W> xc = make_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid, b = t0 + (int)blockIdx.x;
	const WaveScanMasks wm = wave_scan_masks(xc.lane);
	const Chunk c = chunks[b];
	const int lo = c.lo, top = min(c.hi, c.L - 1);
	StructParN<NPL> sc;
	load_par<NPL, S>(par, k0, false, sc);
	double e0[NPL], e1[NPL], akk[NPL], acc[CB][NPL];
	ld<NPL>(par + WP_E0 * S + k0, e0); ld<NPL>(par + WP_E1 * S + k0, e1);
#pragma unroll
	for (int i = 0; i < NPL; ++i) akk[i] = sc.dd[i] + sc.wP[i] * sc.mP[i] + sc.wS[i] * sc.mS[i]; // a[k][k]
#pragma unroll
	for (int j = 0; j < CB; ++j)
#pragma unroll
		for (int i = 0; i < NPL; ++i) acc[j][i] = 0.0;
	double wt[MEAN_COLS][NPL]; // MEAN: the weights of the thread's states, from wts [n_w][S] (zeros beyond n)
#pragma unroll
	for (int j = 0; j < MEAN_COLS; ++j)
#pragma unroll
		for (int i = 0; i < NPL; ++i) wt[j][i] = MEAN && j < n_w ? wts[j * S + k0 + i] : 0.0;
	const uint8_t *o = obs + c.off;
	const double *fo = X + c.off * S + k0;
#define WP_EMIT(p, g, r, last) \
	emit<NPL, W, POST, REC, PATH, CNT, MEAN, QUANT>(p, tid, n, g, r, last, xc, post, recomb, path, maxp, cnt1, n_cnt, j0, min_l, acc, wt, n_w, mean, \
	                                                qq, n_q, qstate)
	if (c.hi == c.L) { // position L: beta_L = 1
		double g[NPL];
		if (CKPT) ld<NPL>(xhi + (int64_t)b * S + k0, g); else ld<NPL>(fo + (int64_t)(c.L - 1) * S, g);
		WP_EMIT(c.L, g, 0.0, true);
	}
	if (CKPT && top >= lo) {
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
				for (; p <= pe; ++p) {
					const int sym = (int)o[p - 1] & 3;
					if ((p & 3) == 0) fstep<NPL, W, true, true>(fs, wm, sym, e0, e1, xf, io[p - 1], xc);
					else fstep<NPL, W, false, true>(fs, wm, sym, e0, e1, xf, 1.0, xc);
					st<NPL>(my + ((p & (WCK - 1)) - 1) * S, xf);
				}
			}
			for (int p = pe; p >= pb; --p) {
				double Xc[NPL], g[NPL], r;
				if (p & (WCK - 1)) ld<NPL>(my + ((p & (WCK - 1)) - 1) * S, Xc); else ld<NPL>(X + ckpt_row(c.off, p) * S + k0, Xc);
				const int sym = (int)o[p - 1] & 3;
				if ((p & 3) == 0) dstep<NPL, W, true, REC>(sc, wm, sym, e0, e1, akk, Xc, x, g, r, xc);
				else dstep<NPL, W, false, REC>(sc, wm, sym, e0, e1, akk, Xc, x, g, r, xc);
				WP_EMIT(p, g, r, false);
			}
		}
	}
	if (!CKPT && top >= lo) {
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
				double g[NPL], r;
				const int sym = (int)((w >> (8 * j)) & 3u);
				if (j == 3) dstep<NPL, W, true, REC>(sc, wm, sym, e0, e1, akk, Xc, x, g, r, xc);
				else dstep<NPL, W, false, REC>(sc, wm, sym, e0, e1, akk, Xc, x, g, r, xc);
				WP_EMIT(p, g, r, false);
#pragma unroll
				for (int i = 0; i < NPL; ++i) Xc[i] = Xn[i];
			}
		}
	}
#undef WP_EMIT
	if (CNT) {
#pragma unroll
		for (int j = 0; j < CB; ++j)
			if (j0 + j < n_cnt) st<NPL>(part + ((int64_t)blockIdx.x * n_cnt + j0 + j) * S + k0, acc[j]);
	}
}

template <int S>
__global__ __launch_bounds__(256) void k_wp_cnt_add(const double *__restrict__ part, int n_tiles, int n_cnt, int n, double *__restrict__ cnt)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n * n_cnt) return;
	const int k = i / n_cnt, j = i % n_cnt;
	double t = 0.0;
	for (int q = 0; q < n_tiles; ++q) t += part[((int64_t)q * n_cnt + j) * S + k];
	cnt[i] += t;
}

// one wave per tile; the sum of a row: the W blocks of 64 NPL states, lowest first (every lane holds the same bits)
template <int NPL, int W> __device__ __forceinline__ double rowsum(const double *__restrict__ row)
{
	double u[NPL];
	ld<NPL>(row, u);
	double t = wave_total(lsum<NPL>(u));
#pragma unroll
	for (int w = 1; w < W; ++w) {
		ld<NPL>(row + 64 * NPL * w, u);
		t += wave_total(lsum<NPL>(u));
	}
	return t;
}
template <int NPL, int W>
__global__ __launch_bounds__(64) void k_wp_scales(const Chunk *__restrict__ chunks, int t0, const double *__restrict__ X,
                                                    const double *__restrict__ inv, const double *__restrict__ entry, double *__restrict__ s)
{
	constexpr int S = 64 * NPL * W;
	const int lane = threadIdx.x, k0 = NPL * lane, b = t0 + (int)blockIdx.x;
	const Chunk c = chunks[b];
	const double *fo = X + c.off * S + k0, *io = inv + c.off;
	double prev = 1.0;
	if (c.lo > 1) prev = rowsum<NPL, W>(entry + (int64_t)b * S + k0);
	for (int p = c.lo; p <= c.hi; ++p) {
		const double cur = rowsum<NPL, W>(fo + (int64_t)(p - 1) * S);
		double v = p == 1 ? cur : cur / prev; // X_1 = a0 e[o_1] as it stands
		if (p > 1 && (p & (NORM_EVERY - 1)) == 0) v /= io[p - 1];
		if (lane == 0) s[p - 1] = v;
		prev = cur;
	}
}

// CKPT: the scales without the table -- the tile's W waves step forward from entry[b] (or X_1 = a0 e[o_1], stored as it stands) with
// fstep and the stored factors: the forward sweep's rows.  A row's sum goes through the exchange, which adds the waves' blocks
// lowest block first -- the order of rowsum.  Two exchanges per position, reached by every wave: the loop bounds come from the
// tile descriptor alone, and `c.lo > 1` is the same in every wave.
template <int NPL, int W>
__global__ __launch_bounds__(64 * W) void k_wp_scales_ck(const double *__restrict__ par, const uint8_t *__restrict__ obs,
                                                           const Chunk *__restrict__ chunks, int t0, const double *__restrict__ inv,
                                                           const double *__restrict__ entry, double *__restrict__ s)
{
	constexpr int S = 64 * NPL * W;
	__shared__ double xs[2 * WX_SLOTS * W];
	Xchg<W> xc = make_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid, b = t0 + (int)blockIdx.x;
	const WaveScanMasks wm = wave_scan_masks(xc.lane);
	const Chunk c = chunks[b];
	StructParN<NPL> fs;
	load_par<NPL, S>(par, k0, true, fs);
	double e0[NPL], e1[NPL], x[NPL], prev;
	ld<NPL>(par + WP_E0 * S + k0, e0); ld<NPL>(par + WP_E1 * S + k0, e1);
	const uint8_t *o = obs + c.off;
	const double *io = inv + c.off;
	int p = c.lo;
	if (c.lo > 1) { ld<NPL>(entry + (int64_t)b * S + k0, x); prev = tile_vsum<NPL, W>(xc, x); }
	else {
		double ev[NPL];
		ld<NPL>(par + WP_A0 * S + k0, x);
		emis<NPL>((int)o[0] & 3, e0, e1, ev);
#pragma unroll
		for (int i = 0; i < NPL; ++i) x[i] *= ev[i];
		prev = tile_vsum<NPL, W>(xc, x);
		if (tid == 0) s[0] = prev;
		p = 2;
	}
	for (; p <= c.hi; ++p) {
		const int sym = (int)o[p - 1] & 3;
		const bool norm = (p & (NORM_EVERY - 1)) == 0;
		if (norm) fstep<NPL, W, true, true>(fs, wm, sym, e0, e1, x, io[p - 1], xc);
		else fstep<NPL, W, false, true>(fs, wm, sym, e0, e1, x, 1.0, xc);
		const double cur = tile_vsum<NPL, W>(xc, x);
		double v = cur / prev;
		if (norm) v /= io[p - 1];
		if (tid == 0) s[p - 1] = v;
		prev = cur;
	}
}

template <int NPL, int W, bool CKPT> static int launch_post(const WidePost &w)
{
	const dim3 grid(w.n_tiles), blk(64 * W);
	hipStream_t st = w.stream;
#define WP_DEC(POST, REC, PATH, CNT, MEAN, QUANT, j0) \
	hipLaunchKernelGGL((k_wp_dec<NPL, W, POST, REC, PATH, CNT, CKPT, MEAN, QUANT>), grid, blk, 0, st, w.par, w.obs, w.chunks, w.t0, w.X, w.inv, w.entry, w.xhi, \
	                   w.bentry, w.n_states, w.post, w.recomb, w.path, w.maxp, w.cnt1, w.n_cnt, j0, w.min_l, w.part, w.wts, w.n_w, w.mean, w.q, w.n_q, w.qstate)
	switch (w.what) {
	case WP_PATH: WP_DEC(false, false, true, false, false, false, 0); break;
	case WP_POST: WP_DEC(true, false, false, false, false, false, 0); break;
	case WP_REC: WP_DEC(false, true, false, false, false, false, 0); break;
	case WP_POST_REC: WP_DEC(true, true, false, false, false, false, 0); break;
	case WP_MEAN:
		if (w.n_w < 1 || w.n_w > MEAN_COLS || !w.wts || !w.mean) return -1;
		WP_DEC(false, false, false, false, true, false, 0);
		break;
	case WP_QUANT:
		if (w.n_q < 1 || w.n_q > QUANT_COLS || !w.qstate) return -1;
		WP_DEC(false, false, false, false, false, true, 0);
		break;
	case WP_COUNTS:
		for (int j0 = 0; j0 < w.n_cnt; j0 += CB) WP_DEC(false, false, false, true, false, false, j0);
		if (hipGetLastError() != hipSuccess) return -1;
		return launch_wide_post_cnt_add(w);
	case WP_SCALES:
		if (CKPT) hipLaunchKernelGGL((k_wp_scales_ck<NPL, W>), grid, blk, 0, st, w.par, w.obs, w.chunks, w.t0, w.inv, w.entry, w.s);
		else hipLaunchKernelGGL((k_wp_scales<NPL, W>), grid, dim3(64), 0, st, w.chunks, w.t0, w.X, w.inv, w.entry, w.s);
		break;
	default: return -1;
	}
#undef WP_DEC
	return hipGetLastError() == hipSuccess ? 0 : -1;
}
template <int NPL, int W> static int launch_post(const WidePost &w, bool ck) { return ck ? launch_post<NPL, W, true>(w) : launch_post<NPL, W, false>(w); }

template <int S> static int launch_cnt_add(const WidePost &w)
{
	hipLaunchKernelGGL(k_wp_cnt_add<S>, dim3((w.n_states * w.n_cnt + 255) / 256), dim3(256), 0, w.stream, w.part, w.n_tiles, w.n_cnt, w.n_states, w.cnt);
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace wide

int launch_wide_post_cnt_add(const WidePost &w)
{
	switch (w.ns) {
	case 192: return wide::launch_cnt_add<192>(w);
	case 256: return wide::launch_cnt_add<256>(w);
	case 512: return wide::launch_cnt_add<512>(w);
	case 768: return wide::launch_cnt_add<768>(w);
	case 1024: return wide::launch_cnt_add<1024>(w);
	}
	return -1;
}

int launch_wide_post(const WidePost &w)
{
	const bool ck = w.ckpt == wide::WCK; // the E-step kept checkpoints ("wide_ckpt"): X at every 8th position, the tiles' last rows in w.xhi
	if (w.ckpt != 1 && !(ck && w.xhi)) return -1;
	if (w.waves > 1 ? w.ns != 256 * w.waves : (w.ns != 192 && w.ns != 256)) return -1;
	switch (w.ns) {
	case 192: return wide::launch_post<3, 1>(w, ck);
	case 256: return wide::launch_post<4, 1>(w, ck);
	case 512: return wide::launch_post<4, 2>(w, ck);
	case 768: return wide::launch_post<4, 3>(w, ck);
	case 1024: return wide::launch_post<4, 4>(w, ck);
	}
	return -1;
}

} // namespace psmc
