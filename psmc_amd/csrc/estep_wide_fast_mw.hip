// estep_wide_fast_mw.hip -- FAST mode, factored statistics, 257..1024 states (option "wide_fast" = 2; api_wide_fast.hip drives it).
//
// The kernels of estep_wide_fast.hip with a tile that spans W = 2, 3 or 4 waves of ONE work-group: the padded widths are
// S = 256 W = 512, 768 and 1024 states (NPL = 4 only; there are no NPL = 3 widths here).  Wave w holds the padded states
// [256 w, 256 (w + 1)), lane j of it holds k = 256 w + 4 j + i, i.e. thread t holds k = 4 t + i -- the layout of wide_prims.h
// continued over the work-group.  Padded states have zero matrix entries and zero emissions, so they stay zero.
//
// Every wave does its in-wave scans exactly as wstep / bstep / astep of the one-wave path, then the waves EXCHANGE one small
// record per position through LDS (Xchg, wide_mw_prims.h: shared with the decoding kernels of estep_wide_post_mw.hip): the wave totals of the scans (and the wave's sum of the state vector where the
// position is scaled, p % 4 == 0), one barrier, and every wave adds the totals of the waves above it (suffix scans) or below it
// (prefix scans), lowest wave index first.  Sums over the whole tile (the scale factors, I of a tile, the mismatch of a boundary,
// the logarithms of k_mw_ll) go through the same exchange in the same fixed order, so every wave holds the same bits and the path
// is bit-reproducible from call to call like the one-wave path.
//
// The slots are double-buffered on the parity of an exchange counter that every wave advances alike, so ONE barrier per exchange
// is enough: a wave cannot reach the write of exchange t+2 before every wave has passed the barrier of exchange t+1, and that
// barrier comes after every wave's reads of exchange t.
//
// What keeps a work-group from hanging: every branch that encloses an exchange depends only on values that are the same in all
// waves of the work-group -- the tile descriptors and verify flags (global memory nobody writes during the launch), the loop
// bounds derived from them, and the mismatch of a chain's next boundary, which is computed from EXCHANGED values (mw_mismatch),
// never from one wave's share.  As in estep_wide_fast.hip, a chain never enters a tile that is itself the head of a repair in
// the same launch, nor the neighbour whose boundary vector such a head starts from: no work-group of a repair launch reads or
// writes what another work-group of it writes.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; scratch is 0 everywhere; LDS = 2 x 6 x W doubles):
//   kernel                W=2: VGPRs  LDS    W=3: VGPRs  LDS    W=4: VGPRs  LDS
//   k_mw_fwd                    114   192          118   288          126   384
//   k_mw_fwd   (repair)         120   192          124   288          130   384
//   k_mw_bwarm                  106   192          108   288          112   384
//   k_mw_acc                    216   192          220   288          226   384
//   k_mw_acc   (repair)         234   192          238   288          244   384
//   k_mw_verify                  40   192           40   288           40   384
//   k_mw_ll                      38   192           38   288           38   384
//   k_mw_reduce1 / 2           8 / 42 VGPRs at every width, no LDS
// "wide_ckpt" (compile-time variants CKPT, as in estep_wide_fast.hip: X at p % 8 == 0 only, the tiles' last rows in xhi, the accumulate
// sweep recomputes the rest with mw_fstep); LDS = the exchange slots + 7 rows of S doubles:
//   k_mw_fwd   CKPT             116   192          120   288          128   384
//   k_mw_fwd   CKPT (repair)    126   192          130   288          138   384
//   k_mw_acc   CKPT             220   28864        224   43296        226   57728
//   k_mw_acc   CKPT (repair)    248   28864        252   43296        252   57728
// Two waves per SIMD as without CKPT: four (W = 2) or two (W = 3, 4) work-groups per compute unit, at most 115 KB of its 160 KB of LDS.
#include <hip/hip_runtime.h>
#include "wave_prims.h"
#include "struct_prims.h"
#include "psmc_hip_internal.h"
#include "wide_fast.h"
#include "wide_prims.h"
#include "wide_mw_prims.h"

namespace psmc {
namespace wide {

constexpr int MW_ACC = 7;   // SL SU DG CL CU E0 E1

// wmismatch of wide_prims.h over the tile: max_k |u/|u| - v/|v|| / max_k v/|v|; NaN anywhere: +inf.  Two exchanges.
template <int W> __device__ __forceinline__ double mw_mismatch(const double (&u)[MW_NPL], const double (&v)[MW_NPL], Xchg<W> &xc)
{
	constexpr int NPL = MW_NPL;
	xc.put(0, wave_total(lsum<NPL>(u))); xc.put(1, wave_total(lsum<NPL>(v)));
	xc.sync();
	const double iu = 1.0 / xc.sum(0), iv = 1.0 / xc.sum(1);
	xc.next();
	double num = 0.0, den = 0.0;
	bool bad = iu != iu || iv != iv;
#pragma unroll
	for (int i = 0; i < NPL; ++i) {
		num = fmax(num, fabs(u[i] * iu - v[i] * iv)); den = fmax(den, fabs(v[i] * iv));
		bad = bad || u[i] != u[i] || v[i] != v[i];
	}
	xc.put(0, wave_maxv(num)); xc.put(1, wave_maxv(den)); xc.put(2, __any(bad) ? 1.0 : 0.0);
	xc.sync();
	num = xc.vmax(0); den = xc.vmax(1);
	const bool any_bad = xc.vmax(2) != 0.0;
	xc.next();
	return any_bad ? __builtin_inf() : num / den;
}

// ------------------------------------------------------------------ forward
// CKPT ("wide_ckpt"): as k_wf_fwd -- X keeps the rows at p % 8 == 0 only, the tile's last row goes to xhi[b]
template <int W, bool REPAIR, bool CKPT>
__global__ __launch_bounds__(64 * W) void k_mw_fwd(const double *__restrict__ par, const uint8_t *__restrict__ obs,
                                                     const Chunk *__restrict__ chunks, int n, const int *__restrict__ list,
                                                     const int *__restrict__ dirty, int chain, double tol, double *__restrict__ X,
                                                     double *__restrict__ inv, double *__restrict__ entry, double *__restrict__ xhi)
{
	constexpr int NPL = MW_NPL, S = 64 * NPL * W;
	__shared__ double xs[2 * MW_SLOTS * W];
	Xchg<W> xc = mw_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid;
	const WaveScanMasks wm = wave_scan_masks(xc.lane);
	StructParN<NPL> sc;
	{ // forward roles of P | R | qa | c | dd (wide_prims.h load_par, at the tile's width): mS = P, wS = qa, mP = R, wP = c
		const double *sp = par + WP_SP * S + k0;
		ld<NPL>(sp, sc.mS); ld<NPL>(sp + 2 * S, sc.wS); ld<NPL>(sp + S, sc.mP); ld<NPL>(sp + 3 * S, sc.wP); ld<NPL>(sp + 4 * S, sc.dd);
	}
	double e0[NPL], e1[NPL];
	ld<NPL>(par + WP_E0 * S + k0, e0); ld<NPL>(par + WP_E1 * S + k0, e1);
	if (REPAIR) __builtin_amdgcn_s_setprio(3);
	int b = REPAIR ? list[blockIdx.x] : (int)blockIdx.x;
	Chunk c = chunks[b];
	double x[NPL];
	int p0;
	if (REPAIR) { // from the neighbour's X_{lo-1} (a repaired tile is never a segment's first)
		if (CKPT) ld<NPL>(xhi + (int64_t)(b - 1) * S + k0, x); else ld<NPL>(X + (c.off + c.lo - 2) * S + k0, x);
		p0 = c.lo;
	} else {
		const int ws = max(1, c.lo - c.wf);
		ld<NPL>(par + WP_A0 * S + k0, x);
		if (ws == 1) { // true start: X_1 = a0 e[o_1]
			double ev[NPL];
			emis<NPL>((int)obs[c.off] & 3, e0, e1, ev);
#pragma unroll
			for (int i = 0; i < NPL; ++i) x[i] *= ev[i];
			if (CKPT) { if (c.lo == 1 && c.hi == 1) st<NPL>(xhi + (int64_t)b * S + k0, x); } // (the accumulate sweep recomputes X_1)
			else if (c.lo == 1) st<NPL>(X + c.off * S + k0, x);
			p0 = 2;
		} else p0 = ws;
	}
	for (;;) {
		const uint8_t *o = obs + c.off;
		double *fo = X + c.off * S + k0, *io = inv + c.off;
		const int lo = c.lo, hi = c.hi;
		if (p0 == lo) st<NPL>(entry + (int64_t)b * S + k0, x); // the X_{lo-1} this tile builds on
		for (int g = (p0 - 1) >> 2; 4 * g < hi; ++g) { // positions 4g+1 .. 4g+4 (indices 4g .. 4g+3)
			const unsigned w = *reinterpret_cast<const unsigned *>(o + 4 * (int64_t)g);
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				const int p = 4 * g + j + 1;
				if (p < p0 || p > hi) continue; // (the same in every wave: the exchange below is reached by all or none)
				if (p == lo && p != p0) st<NPL>(entry + (int64_t)b * S + k0, x);
				const int sym = (int)((w >> (8 * j)) & 3u);
				if (j == 3) { // p % 4 == 0: scaled by 1/d_p, a power of two (struct_prims.h pow2_rcp)
					const double iv = mw_fstep<W, true, false>(sc, wm, sym, e0, e1, x, 1.0, xc);
					if (p >= lo && tid == 0) io[p - 1] = iv;
				} else mw_fstep<W, false, false>(sc, wm, sym, e0, e1, x, 1.0, xc);
				if (!CKPT) { if (p >= lo) st<NPL>(fo + (int64_t)(p - 1) * S, x); }
				else if (p >= lo) {
					if (j == 3 && (p & (WCK - 1)) == 0) st<NPL>(X + ckpt_row(c.off, p) * S + k0, x);
					if (p == hi) st<NPL>(xhi + (int64_t)b * S + k0, x);
				}
			}
		}
		if (!REPAIR || !chain) break;
		// glued run: go on into the next tile while its start vector disagrees with this exit vector -- but not into a head of this
		// launch, nor into the tile before one (that head reads the tile's last X row as its start vector)
		const int nb = b + 1;
		if (nb >= n || !same_seg(chunks, b, nb) || (chunks[nb].flags & CHUNK_ANCHOR_F) || head_f(chunks, dirty, nb)) break;
		if (nb + 1 < n && same_seg(chunks, nb, nb + 1) && head_f(chunks, dirty, nb + 1)) break;
		double u[NPL];
		ld<NPL>(entry + (int64_t)nb * S + k0, u);
		if (mw_mismatch<W>(u, x, xc) <= tol) break; // from exchanged values: the same decision in every wave
		b = nb; c = chunks[b]; p0 = c.lo;
	}
}

// ------------------------------------------------------------------ backward
template <int W>
__global__ __launch_bounds__(64 * W) void k_mw_bwarm(const double *__restrict__ par, const uint8_t *__restrict__ obs,
                                                       const Chunk *__restrict__ chunks, double *__restrict__ bentry)
{
	constexpr int NPL = MW_NPL, S = 64 * NPL * W;
	__shared__ double xs[2 * MW_SLOTS * W];
	Xchg<W> xc = mw_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid, b = blockIdx.x;
	const WaveScanMasks wm = wave_scan_masks(xc.lane);
	const Chunk c = chunks[b];
	const int top = min(c.hi, c.L - 1);
	if (top < c.lo) return; // a tile holding only position L owns no transition (every wave of the tile leaves here)
	StructParN<NPL> sc;
	mw_load_bwd<S>(par, k0, sc);
	double e0[NPL], e1[NPL];
	ld<NPL>(par + WP_E0 * S + k0, e0); ld<NPL>(par + WP_E1 * S + k0, e1);
	const uint8_t *o = obs + c.off;
	const int q = min(c.hi + c.wb + 1, c.L); // B_q := 1: bt_q = e[o_q]
	double x[NPL];
	emis<NPL>((int)o[q - 1] & 3, e0, e1, x);
	for (int g = (q - 2) >> 2; g >= 0 && 4 * g + 4 > top; --g) { // positions q-1 .. top+1, highest first (group g holds 4g+1 .. 4g+4)
		const unsigned w = *reinterpret_cast<const unsigned *>(o + 4 * (int64_t)g);
#pragma unroll
		for (int j = 3; j >= 0; --j) {
			const int p = 4 * g + j + 1;
			if (p > q - 1 || p <= top) continue;
			const int sym = (int)((w >> (8 * j)) & 3u);
			if (j == 3) mw_bstep<W, true>(sc, wm, sym, e0, e1, x, xc); else mw_bstep<W, false>(sc, wm, sym, e0, e1, x, xc);
		}
	}
	st<NPL>(bentry + (int64_t)b * S + k0, x);
}

// One position p of the accumulate sweep (astep of estep_wide_fast.hip plus the exchange of the four scan totals and, NORM, of
// the sum of bt_{p+1}): x = bt_{p+1} on entry, bt_p on exit; X = X_p; inv = the forward scale factor at p (NORM: p % 4 == 0).
// The partial sums are kept in units of the current I; I_lane is this thread's share of it.
template <int W, bool NORM>
__device__ __forceinline__ void mw_astep(const StructParN<MW_NPL> &sc, const WaveScanMasks &wm, int sym, const double (&e0)[MW_NPL],
                                         const double (&e1)[MW_NPL], const double (&X)[MW_NPL], double (&x)[MW_NPL], double inv,
                                         double (&acc)[MW_ACC][MW_NPL], double &I_lane, Xchg<W> &xc)
{
	constexpr int NPL = MW_NPL;
	double ev[NPL];
	emis<NPL>(sym, e0, e1, ev);
	const double m0 = sym == 0 ? 1.0 : 0.0, m1 = sym == 1 ? 1.0 : 0.0;
	double su[NPL + 1], pv[NPL + 1], sx[NPL + 1], px[NPL + 1];
	su[NPL] = 0.0; sx[NPL] = 0.0; pv[0] = 0.0; px[0] = 0.0; // pv / px shifted by one: pv[i+1] = inclusive at i
#pragma unroll
	for (int i = NPL - 1; i >= 0; --i) { su[i] = __builtin_fma(x[i], sc.mS[i], su[i + 1]); sx[i] = __builtin_fma(X[i], sc.wP[i], sx[i + 1]); }
#pragma unroll
	for (int i = 0; i < NPL; ++i) { pv[i + 1] = __builtin_fma(x[i], sc.mP[i], pv[i]); px[i + 1] = __builtin_fma(X[i], sc.wS[i], px[i]); }
	double ES = wave_excl_suffix(su[0], wm), EP = wave_excl_prefix(pv[NPL]);
	double EX = wave_excl_suffix(sx[0], wm), PX = wave_excl_prefix(px[NPL]);
	xc.put(0, readlane_f64(ES + su[0], 0)); xc.put(1, readlane_f64(EP + pv[NPL], 63));
	xc.put(2, readlane_f64(EX + sx[0], 0)); xc.put(3, readlane_f64(PX + px[NPL], 63));
	if (NORM) xc.put(4, wave_total(lsum<NPL>(x)));
	xc.sync();
	ES += xc.above(0); EP += xc.below(1); EX += xc.above(2); PX += xc.below(3);
	double f = 1.0;
	if (NORM) {
		const double sb = rcp_newton(xc.sum(4));
#pragma unroll
		for (int i = 0; i < NPL; ++i) ev[i] *= sb;
		f = sb * pow2_rcp(inv);
	}
	xc.next();
	double Il = 0.0;
#pragma unroll
	for (int i = 0; i < NPL; ++i) {
		const double t = __builtin_fma(sc.wS[i], su[i], __builtin_fma(sc.wP[i], pv[i + 1], sc.dd[i] * x[i]));
		const double y = __builtin_fma(sc.wS[i], ES, __builtin_fma(sc.wP[i], EP, t)); // (a bt_{p+1})[k]
		const double gk = X[i] * y;                                                    // I * posterior of state k at p
		acc[0][i] = __builtin_fma(X[i], EP + pv[i], acc[0][i]);     // SL: strictly below k
		acc[1][i] = __builtin_fma(X[i], ES + su[i + 1], acc[1][i]); // SU: strictly above k
		acc[2][i] = __builtin_fma(X[i], x[i], acc[2][i]);           // DG
		acc[3][i] = __builtin_fma(x[i], EX + sx[i + 1], acc[3][i]); // CL: rows k > l
		acc[4][i] = __builtin_fma(x[i], PX + px[i], acc[4][i]);     // CU: rows k < l
		acc[5][i] = __builtin_fma(gk, m0, acc[5][i]);
		acc[6][i] = __builtin_fma(gk, m1, acc[6][i]);
		Il += gk;
		x[i] = y * ev[i];
	}
	I_lane = Il;
	if (NORM) { // ... now in units of I_{p-1}
#pragma unroll
		for (int q = 0; q < MW_ACC; ++q)
#pragma unroll
			for (int i = 0; i < NPL; ++i) acc[q][i] *= f;
		I_lane *= f;
	}
}
// CKPT ("wide_ckpt"): as k_wf_acc -- block by block from the tile's top block down, the block's rows recomputed forward with
// mw_fstep (every recomputed step's exchange as k_mw_fwd does it) into LDS (7 S doubles: 56 KB at W = 4, beside the exchange slots;
// every thread reads back what it wrote itself), X_{8m} read from the table.  The block bounds come from the tile descriptor
// alone, so every wave of the work-group goes through the same exchanges.
template <int W, bool REPAIR, bool CKPT>
__global__ __launch_bounds__(64 * W) void k_mw_acc(const double *__restrict__ par, const uint8_t *__restrict__ obs,
                                                     const Chunk *__restrict__ chunks, int n, const int *__restrict__ list,
                                                     const int *__restrict__ dirty, int chain, double tol, const double *__restrict__ X,
                                                     const double *__restrict__ inv, const double *__restrict__ entry, double *__restrict__ bentry,
                                                     double *__restrict__ bexit, double *__restrict__ part)
{
	constexpr int NPL = MW_NPL, S = 64 * NPL * W;
	__shared__ double xs[2 * MW_SLOTS * W];
	Xchg<W> xc = mw_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid;
	const WaveScanMasks wm = wave_scan_masks(xc.lane);
	StructParN<NPL> sc;
	mw_load_bwd<S>(par, k0, sc);
	double e0[NPL], e1[NPL];
	ld<NPL>(par + WP_E0 * S + k0, e0); ld<NPL>(par + WP_E1 * S + k0, e1);
	if (REPAIR) __builtin_amdgcn_s_setprio(3);
	int b = REPAIR ? list[blockIdx.x] : (int)blockIdx.x;
	double x[NPL];
	if (REPAIR) { ld<NPL>(bexit + (int64_t)(b + 1) * S + k0, x); st<NPL>(bentry + (int64_t)b * S + k0, x); }
	else ld<NPL>(bentry + (int64_t)b * S + k0, x);
	for (;;) {
		const Chunk c = chunks[b];
		const int lo = c.lo, top = min(c.hi, c.L - 1);
		const uint8_t *o = obs + c.off;
		const double *fo = X + c.off * S + k0, *io = inv + c.off;
		double acc[MW_ACC][NPL], accI = 1.0;
#pragma unroll
		for (int q = 0; q < MW_ACC; ++q)
#pragma unroll
			for (int i = 0; i < NPL; ++i) acc[q][i] = 0.0;
		if (CKPT && top >= lo) { // (the same in every wave, and so is every bound below)
			__shared__ double rows[(WCK - 1) * S];
			double *my = rows + k0;
			StructParN<NPL> fs;
			fwd_roles<NPL>(sc, fs);
			for (int q = top & ~(WCK - 1); q + WCK - 1 >= lo; q -= WCK) { // the block of the positions q .. q+7, within lo .. top
				const int pb = max(lo, q), pe = min(top, q + WCK - 1);
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
					if ((p & 3) == 0) mw_fstep<W, true, true>(fs, wm, sym, e0, e1, xf, io[p - 1], xc);
					else mw_fstep<W, false, true>(fs, wm, sym, e0, e1, xf, 1.0, xc);
					st<NPL>(my + ((p & (WCK - 1)) - 1) * S, xf);
				}
				for (p = pe; p >= pb; --p) {
					double Xc[NPL];
					if (p & (WCK - 1)) ld<NPL>(my + ((p & (WCK - 1)) - 1) * S, Xc); else ld<NPL>(X + ckpt_row(c.off, p) * S + k0, Xc);
					const int sym = (int)o[p - 1] & 3;
					if ((p & 3) == 0) mw_astep<W, true>(sc, wm, sym, e0, e1, Xc, x, io[p - 1], acc, accI, xc);
					else mw_astep<W, false>(sc, wm, sym, e0, e1, Xc, x, 1.0, acc, accI, xc);
				}
			}
			st<NPL>(bexit + (int64_t)b * S + k0, x); // bt_lo
		}
		if (!CKPT && top >= lo) { // (the same in every wave)
			double Xc[NPL], Xn[NPL];
			ld<NPL>(fo + (int64_t)(top - 1) * S, Xc);
			for (int g = (top - 1) >> 2; g >= 0 && 4 * g + 4 >= lo; --g) {
				const unsigned w = *reinterpret_cast<const unsigned *>(o + 4 * (int64_t)g);
				const double ivg = io[4 * g + 3]; // the forward scale factor of position 4g+4 (read only where that lies inside the tile)
#pragma unroll
				for (int j = 3; j >= 0; --j) {
					const int p = 4 * g + j + 1;
					if (p > top || p < lo) continue;
					if (p > lo) ld<NPL>(fo + (int64_t)(p - 2) * S, Xn); // X_{p-1}, for the next step
					const int sym = (int)((w >> (8 * j)) & 3u);
					if (j == 3) mw_astep<W, true>(sc, wm, sym, e0, e1, Xc, x, ivg, acc, accI, xc);
					else mw_astep<W, false>(sc, wm, sym, e0, e1, Xc, x, 1.0, acc, accI, xc);
#pragma unroll
					for (int i = 0; i < NPL; ++i) Xc[i] = Xn[i];
				}
			}
			st<NPL>(bexit + (int64_t)b * S + k0, x); // bt_lo
		}
		const double iI = top >= lo ? rcp_newton(mw_total<W>(xc, wave_total(accI))) : 1.0;
		const double mult = (double)c.mult * iI;
		double *out = part + (int64_t)b * (MW_ACC * S) + k0;
#pragma unroll
		for (int i = 0; i < NPL; ++i) {
			const double akk = sc.dd[i] + sc.wP[i] * sc.mP[i] + sc.wS[i] * sc.mS[i]; // a[k][k]
			acc[0][i] *= sc.wP[i] * mult; acc[1][i] *= sc.wS[i] * mult; acc[2][i] *= akk * mult;
			acc[3][i] *= sc.mP[i] * mult; acc[4][i] *= sc.mS[i] * mult; acc[5][i] *= mult; acc[6][i] *= mult;
		}
#pragma unroll
		for (int q = 0; q < MW_ACC; ++q) st<NPL>(out + q * S, acc[q]);
		if (!REPAIR || !chain || top < lo) break;
		// glued run: go on into the tile below while its start vector disagrees with this exit vector -- but not into a head of this
		// launch, nor into the tile above one (that head reads the tile's bexit as its start vector)
		const int nb = b - 1;
		if (nb < 0 || !same_seg(chunks, nb, b) || (chunks[nb].flags & CHUNK_ANCHOR_B) || head_b(chunks, dirty, n, nb)) break;
		if (nb - 1 >= 0 && same_seg(chunks, nb - 1, nb) && head_b(chunks, dirty, n, nb - 1)) break;
		double u[NPL];
		ld<NPL>(bentry + (int64_t)nb * S + k0, u);
		if (mw_mismatch<W>(u, x, xc) <= tol) break; // from exchanged values: the same decision in every wave
		b = nb;
		st<NPL>(bentry + (int64_t)b * S + k0, x);
	}
}

// ------------------------------------------------------------------ verify, LL, reduce
template <int W, bool BWD>
__global__ __launch_bounds__(64 * W) void k_mw_verify(const Chunk *__restrict__ chunks, int n, double tol, const double *__restrict__ X,
                                                        const double *__restrict__ xhi, const double *__restrict__ mine, const double *__restrict__ bexit,
                                                        int *__restrict__ dirty, int *__restrict__ cnt, unsigned long long *__restrict__ warm)
{
	constexpr int NPL = MW_NPL, S = 64 * NPL * W;
	__shared__ double xs[2 * MW_SLOTS * W];
	Xchg<W> xc = mw_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid, b = blockIdx.x;
	const Chunk c = chunks[b];
	bool check;
	if (!BWD) check = c.lo > 1 && !(c.flags & CHUNK_ANCHOR_F);
	else check = !(c.flags & (CHUNK_ANCHOR_B | CHUNK_LAST)) && min(c.hi, c.L - 1) >= c.lo && b + 1 < n && chunks[b + 1].off == c.off;
	double m = 0.0;
	if (check) { // (the same in every wave)
		double u[NPL], v[NPL];
		ld<NPL>(mine + (int64_t)b * S + k0, u);
		// (xhi: "wide_ckpt" -- the neighbour's last row X_{lo-1} is in the per-tile array, not in X)
		ld<NPL>(BWD ? bexit + (int64_t)(b + 1) * S + k0 : (xhi ? xhi + (int64_t)(b - 1) * S + k0 : X + (c.off + c.lo - 2) * S + k0), v);
		m = mw_mismatch<W>(u, v, xc);
	}
	if (tid == 0) {
		const int bad = check && !(m <= tol);
		dirty[b] = bad;
		if (bad) atomicAdd(cnt, 1);
		if (check) atomicMax(warm, (unsigned long long)__double_as_longlong(m));
	}
}

// wave_total_comp of wide_prims.h as its unevaluated pair (the same bits in every lane)
__device__ __forceinline__ void mw_wave_comp(const double (&x)[MW_NPL], double &h, double &l) {
	double t;
	h = x[0]; l = 0.0;
#pragma unroll
	for (int i = 1; i < MW_NPL; ++i) { two_sum(h, x[i], h, t); l += t; }
#pragma unroll
	for (int m = 1; m <= 32; m <<= 1) {
		const double oh = __shfl_xor(h, m, 64), ol = __shfl_xor(l, m, 64);
		two_sum(h, oh, h, t);
		l = (l + ol) + t;
	}
}

template <int W>
__global__ __launch_bounds__(64 * W) void k_mw_ll(const Chunk *__restrict__ chunks, const double *__restrict__ X, const double *__restrict__ xhi, const double *__restrict__ inv,
                                                    const double *__restrict__ entry, double *__restrict__ LLpart)
{
	constexpr int NPL = MW_NPL, S = 64 * NPL * W;
	__shared__ double xs[2 * MW_SLOTS * W];
	Xchg<W> xc = mw_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid, b = blockIdx.x;
	const Chunk c = chunks[b];
	const double *io = inv + c.off;
	double prod = 1.0, ll = 0.0;
	const int first = (max(c.lo, 2) + NORM_EVERY - 1) & ~(NORM_EVERY - 1);
	for (int p = first + NORM_EVERY * tid; p <= c.hi; p += NORM_EVERY * 64 * W) {
		prod *= io[p - 1];
		if (prod > 1e280 || prod < 1e-280) { ll -= log(prod); prod = 1.0; }
	}
	ll -= log(prod);
	ll = mw_total<W>(xc, wave_total(ll));
	double u[NPL];
	if (c.lo > 1) { // the tile was computed from entry = X_{lo-1} up to a factor: put the telescoping sum back in step
		double v[NPL];
		ld<NPL>(xhi ? xhi + (int64_t)(b - 1) * S + k0 : X + (c.off + c.lo - 2) * S + k0, u); ld<NPL>(entry + (int64_t)b * S + k0, v); // (xhi: "wide_ckpt", as k_mw_verify)
		const double su = mw_vsum<W>(xc, u), sv = mw_vsum<W>(xc, v);
		ll += log(su) - log(sv);
	}
	if (c.hi == c.L) {
		ld<NPL>(xhi ? xhi + (int64_t)b * S + k0 : X + (c.off + c.L - 1) * S + k0, u);
		if (c.L == 1) { // a segment of one bin: LL is this logarithm alone -- add the sum up without a rounding (estep_wide_fast.hip k_wf_ll)
			double h, l, t;
			mw_wave_comp(u, h, l);
			xc.put(0, h); xc.put(1, l);
			xc.sync();
			h = xc.get(0, 0); l = xc.get(1, 0);
#pragma unroll
			for (int w = 1; w < W; ++w) { two_sum(h, xc.get(0, w), h, t); l = (l + xc.get(1, w)) + t; }
			xc.next();
			ll += log(h + l);
		} else ll += log(mw_vsum<W>(xc, u));
	}
	if (tid == 0) LLpart[b] = ll * (double)c.mult;
}

// fixed-order two-stage sum over the tiles (k_wf_reduce1/2 of estep_wide_fast.hip at S = 512 / 768 / 1024: one thread per state)
template <int S>
__global__ __launch_bounds__(S) void k_mw_reduce1(const double *__restrict__ part, int n_tiles, const double *__restrict__ LLpart,
                                                    double *__restrict__ stage)
{
	constexpr int FSL = MW_ACC * S + 1;
	const int k = threadIdx.x, q = blockIdx.x, y = blockIdx.y;
	if (q < MW_ACC) {
		double s = 0.0;
		for (int j = y; j < n_tiles; j += RED_ROWS) s += part[(int64_t)j * (MW_ACC * S) + q * S + k];
		stage[(int64_t)y * FSL + q * S + k] = s;
	} else if (k == 0) {
		double s = 0.0;
		for (int j = y; j < n_tiles; j += RED_ROWS) s += LLpart[j];
		stage[(int64_t)y * FSL + MW_ACC * S] = s;
	}
}
template <int S>
__global__ __launch_bounds__(S) void k_mw_reduce2(const double *__restrict__ stage, double tiny_total, int n, double *__restrict__ out)
{
	constexpr int FSL = MW_ACC * S + 1;
	const int k = threadIdx.x, q = blockIdx.x;
	if (q == MW_ACC) {
		if (k == 0) {
			double s = 0.0;
			for (int y = 0; y < RED_ROWS; ++y) s += stage[(int64_t)y * FSL + MW_ACC * S];
			out[MW_ACC * n] = s;
		}
		return;
	}
	double s = 0.0;
	for (int y = 0; y < RED_ROWS; ++y) s += stage[(int64_t)y * FSL + q * S + k];
	if (k < n) { // the HMM_TINY seeds of khmm.c:305-308, per cell
		const double cells = q == 0 ? k : (q == 1 ? n - 1 - k : (q == 2 ? 1 : (q == 3 ? n - 1 - k : (q == 4 ? k : 1))));
		out[q * n + k] = s + cells * tiny_total;
	}
}

template <int W> static int launch_mw(const WideLaunch &w, int what, int n_list)
{
	constexpr int S = 64 * MW_NPL * W, T = 64 * W;
	const int nc = w.n_tiles;
	hipStream_t st = w.stream;
	const bool ck = w.ckpt == WCK;                      // "wide_ckpt": X at every 8th position, the tiles' last rows in w.xhi
	const double *xhi = ck ? w.xhi : nullptr;
	if (w.ckpt != 1 && !(ck && w.xhi)) return -1;
	switch (what) {
	case WF_FWD:
		if (ck) hipLaunchKernelGGL((k_mw_fwd<W, false, true>), dim3(nc), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.xhi);
		else hipLaunchKernelGGL((k_mw_fwd<W, false, false>), dim3(nc), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.xhi);
		break;
	case WF_FWD_REPAIR:
		if (ck) hipLaunchKernelGGL((k_mw_fwd<W, true, true>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.xhi);
		else hipLaunchKernelGGL((k_mw_fwd<W, true, false>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.xhi);
		break;
	case WF_BWARM: hipLaunchKernelGGL(k_mw_bwarm<W>, dim3(nc), dim3(T), 0, st, w.par, w.obs, w.chunks, w.bentry); break;
	case WF_ACC:
		if (ck) hipLaunchKernelGGL((k_mw_acc<W, false, true>), dim3(nc), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part);
		else hipLaunchKernelGGL((k_mw_acc<W, false, false>), dim3(nc), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part);
		break;
	case WF_ACC_REPAIR:
		if (ck) hipLaunchKernelGGL((k_mw_acc<W, true, true>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part);
		else hipLaunchKernelGGL((k_mw_acc<W, true, false>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part);
		break;
	case WF_VERIFY_F: hipLaunchKernelGGL((k_mw_verify<W, false>), dim3(nc), dim3(T), 0, st, w.chunks, nc, w.tol, w.X, xhi, w.entry, w.bexit, w.dirty, w.cnt, w.warm); break;
	case WF_VERIFY_B: hipLaunchKernelGGL((k_mw_verify<W, true>), dim3(nc), dim3(T), 0, st, w.chunks, nc, w.tol, w.X, xhi, w.bentry, w.bexit, w.dirty, w.cnt + 1, w.warm + 1); break;
	case WF_FINISH:
		hipLaunchKernelGGL(k_mw_ll<W>, dim3(nc), dim3(T), 0, st, w.chunks, w.X, xhi, w.inv, w.entry, w.LLpart);
		hipLaunchKernelGGL(k_mw_reduce1<S>, dim3(MW_ACC + 1, RED_ROWS), dim3(S), 0, st, w.part, nc, w.LLpart, w.stage);
		hipLaunchKernelGGL(k_mw_reduce2<S>, dim3(MW_ACC + 1), dim3(S), 0, st, w.stage, w.tiny_total, w.n_states, w.out);
		break;
	default: return -1;
	}
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace wide

int launch_wide_fast_mw(const WideLaunch &w, int what, int n_list)
{
	if (w.ns != 256 * w.waves) return -1;
	if (w.waves == 2) return wide::launch_mw<2>(w, what, n_list);
	if (w.waves == 3) return wide::launch_mw<3>(w, what, n_list);
	if (w.waves == 4) return wide::launch_mw<4>(w, what, n_list);
	return -1;
}

} // namespace psmc
