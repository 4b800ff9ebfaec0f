// estep_wide_fast.hip -- FAST mode, factored statistics, 129..256 states (option "wide_fast"; api_wide_fast.hip drives it).
//
// The algebra is the one of estep_struct.hip (forward / backward step in O(N): two scans) and estep_factored.hip (the five
// triangular sums of A, E and LL straight from the backward sweep).  Only the layout differs: a state vector of S = 192 or 256
// padded states is ONE tile per wave, 64 lanes x NPL adjacent states (NPL = 3 or 4, lane j holds k = NPL j + i), so the
// cross-lane part of a scan is a whole-wave scan (wave_shr / wave_shl by one lane, then the row scans of struct_prims.h) instead
// of a 16-lane row scan.  Nothing goes through LDS: the five structure vectors and the two emission rows stay in registers.
// Padded states have zero matrix entries and zero emissions, so they stay zero.
//
// One wave per tile and direction:
//   k_wf_fwd    speculative forward sweep (warm-up from a0, the stationary vector, `wf` bins before the tile; a segment's first tile
//               from X_1 = a0 e[o_1]); stores X (one row of 8 S bytes per position), 1/d_p at p % 4 == 0 (a power of two: pow2_rcp)
//               and the start vector `entry`.  REPAIR: from the neighbour's X_{lo-1}; with `chain` the wave walks on into the next
//               tile while that tile's start vector disagrees with the new exit vector (a glued run: one round instead of one per tile).
//   k_wf_bwarm  speculative backward warm-up: bentry = bt_{top+1} of every tile, from bt_q = e[o_q] `wb` bins above it.
//   k_wf_acc    the tile's backward sweep from bentry, reading X: the seven per-lane sums of estep_factored.hip, bexit = bt_lo,
//               the tile's partials (a repaired tile OVERWRITES them: nothing is counted twice).  REPAIR: from the exit vector of the
//               tile above, chaining downwards like the forward repair.
//   k_wf_verify every tile's start vector against its neighbour's exit vector (the test of estep_fast.hip k_verify).
//   k_wf_ll, k_wf_reduce1/2: the log-likelihood of a tile (as estep_fast.hip k_ll) and the fixed-order sum of the partials.
// A chain never enters a tile that is itself the head of a repair in the same launch, nor the neighbour whose boundary vector such a
// head starts from: no wave of a repair launch reads or writes what another wave of it writes, so the result does not depend on
// scheduling.  A tile a chain stops in front of is flagged again by the next verify round.
//
// "wide_ckpt" (compile-time variants CKPT of k_wf_fwd and k_wf_acc; the full-table kernels keep their code): X keeps the rows at
// p % 8 == 0 only, by absolute position (wide_prims.h ckpt_row), and every tile's last row goes to xhi[b], which k_wf_verify, the
// start of a forward repair and k_wf_ll read instead of X_{lo-1} / X_L.  The accumulate sweep recomputes the seven rows between two
// checkpoints into LDS with fstep (wide_prims.h), the forward sweep's own step, from the scale factors that sweep stored: the same
// bits as the full table.  A chained repair rewrites the checkpoints and last rows of the tiles it walks through; what it may
// not enter is unchanged (a head reads its neighbour's xhi row where it read the neighbour's last X row).
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; scratch is 0 everywhere; LDS in bytes per wave):
//   kernel                      S=192: VGPRs  LDS     S=256: VGPRs       LDS
//   k_wf_fwd    / repair             86 /  90   0          108 / 112       0
//   k_wf_fwd    / repair, CKPT       88 /  92   0          110 / 114       0
//   k_wf_acc    / repair            154 / 178   0          206 / 228       0
//   k_wf_acc    / repair, CKPT      196 / 220   10752      256 / 256+24 AGPRs  14336
//   k_wf_verify                      33 /  36 (backward)    36 /  39       0
//   k_wf_ll                          37          0           38            0
// The CKPT accumulate sweep runs two tiles per SIMD at either width (the full-table one three at 192 states): eight waves' staged
// rows are 84 / 112 KB of the compute unit's 160 KB.
#include <hip/hip_runtime.h>
#include "wave_prims.h"
#include "struct_prims.h"
#include "psmc_hip_internal.h"
#include "wide_fast.h"
#include "wide_prims.h"

namespace psmc {
namespace wide {

constexpr int WACC = 7; // SL SU DG CL CU E0 E1

// ------------------------------------------------------------------ forward
// CKPT ("wide_ckpt"): X keeps the rows at p % 8 == 0 only (ckpt_row), and the tile's last row X_hi goes to xhi[b] -- what the
// neighbour's verify and repair and k_wf_ll read; the accumulate sweep recomputes the rest.
template <int NPL, bool REPAIR, bool CKPT>
__global__ __launch_bounds__(64) void k_wf_fwd(const double *__restrict__ par, const uint8_t *__restrict__ obs,
                                                 const Chunk *__restrict__ chunks, int n, const int *__restrict__ list,
                                                 const int *__restrict__ dirty, int chain, double tol, double *__restrict__ X,
                                                 double *__restrict__ inv, double *__restrict__ entry, double *__restrict__ xhi)
{
	constexpr int S = 64 * NPL;
	const int lane = threadIdx.x, k0 = NPL * lane;
	const WaveScanMasks wm = wave_scan_masks(lane);
	StructParN<NPL> sc;
	load_par<NPL>(par, k0, true, sc);
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
				if (p < p0 || p > hi) continue;
				if (p == lo && p != p0) st<NPL>(entry + (int64_t)b * S + k0, x);
				const int sym = (int)((w >> (8 * j)) & 3u);
				if (j == 3) { // p % 4 == 0: scaled by 1/d_p
					const double iv = fstep<NPL, true, false>(sc, wm, sym, e0, e1, x, 1.0);
					if (p >= lo && lane == 0) io[p - 1] = iv;
				} else fstep<NPL, false, false>(sc, wm, sym, e0, e1, x, 1.0);
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
		if (wmismatch<NPL>(u, x) <= tol) break;
		b = nb; c = chunks[b]; p0 = c.lo;
	}
}

// ------------------------------------------------------------------ backward
template <int NPL>
__global__ __launch_bounds__(64) void k_wf_bwarm(const double *__restrict__ par, const uint8_t *__restrict__ obs,
                                                   const Chunk *__restrict__ chunks, double *__restrict__ bentry)
{
	constexpr int S = 64 * NPL;
	const int lane = threadIdx.x, k0 = NPL * lane, b = blockIdx.x;
	const WaveScanMasks wm = wave_scan_masks(lane);
	const Chunk c = chunks[b];
	const int top = min(c.hi, c.L - 1);
	if (top < c.lo) return; // a tile holding only position L owns no transition
	StructParN<NPL> sc;
	load_par<NPL>(par, k0, false, sc);
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
			if (j == 3) bstep<NPL, true>(sc, wm, sym, e0, e1, x); else bstep<NPL, false>(sc, wm, sym, e0, e1, x);
		}
	}
	st<NPL>(bentry + (int64_t)b * S + k0, x);
}

// One position p of the accumulate sweep (estep_factored.hip acc_step with whole-wave scans): x = bt_{p+1} on entry, bt_p on exit;
// X = X_p; inv = the forward scale factor at p (NORM: p % 4 == 0).  The partial sums are kept in units of the current I.
template <int NPL, bool NORM>
__device__ __forceinline__ void astep(const StructParN<NPL> &sc, const WaveScanMasks &wm, int sym, const double (&e0)[NPL],
                                      const double (&e1)[NPL], const double (&X)[NPL], double (&x)[NPL], double inv,
                                      double (&acc)[WACC][NPL], double &I_lane)
{
	double ev[NPL];
	emis<NPL>(sym, e0, e1, ev);
	const double m0 = sym == 0 ? 1.0 : 0.0, m1 = sym == 1 ? 1.0 : 0.0;
	double f = 1.0;
	if (NORM) {
		const double sb = rcp_newton(wave_total(lsum<NPL>(x)));
#pragma unroll
		for (int i = 0; i < NPL; ++i) ev[i] *= sb;
		f = sb * pow2_rcp(inv);
	}
	double su[NPL + 1], pv[NPL + 1], sx[NPL + 1], px[NPL + 1];
	su[NPL] = 0.0; sx[NPL] = 0.0; pv[0] = 0.0; px[0] = 0.0; // pv / px shifted by one: pv[i+1] = inclusive at i
#pragma unroll
	for (int i = NPL - 1; i >= 0; --i) { su[i] = __builtin_fma(x[i], sc.mS[i], su[i + 1]); sx[i] = __builtin_fma(X[i], sc.wP[i], sx[i + 1]); }
#pragma unroll
	for (int i = 0; i < NPL; ++i) { pv[i + 1] = __builtin_fma(x[i], sc.mP[i], pv[i]); px[i + 1] = __builtin_fma(X[i], sc.wS[i], px[i]); }
	const double ES = wave_excl_suffix(su[0], wm), EP = wave_excl_prefix(pv[NPL]);
	const double EX = wave_excl_suffix(sx[0], wm), PX = wave_excl_prefix(px[NPL]);
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
		for (int q = 0; q < WACC; ++q)
#pragma unroll
			for (int i = 0; i < NPL; ++i) acc[q][i] *= f;
		I_lane *= f;
	}
}
// CKPT ("wide_ckpt"): X holds the rows at p % 8 == 0 only.  The tile is swept in blocks of the positions 8m .. 8m+7, the top block
// first: the block's rows are recomputed forward with fstep -- the forward sweep's own step and its stored scale factors, so its
// bits -- from the checkpoint X_{8m}, or in the tile's lowest block from entry[b] (the X_{lo-1} the tile was built on) or from
// X_1 = a0 e[o_1], into LDS (rows 8m+1 .. 8m+7: 7 S doubles, every lane reads back what it wrote itself, so no barrier); then astep runs
// over them, highest position first, X_{8m} read from the table.
template <int NPL, bool REPAIR, bool CKPT>
__global__ __launch_bounds__(64) void k_wf_acc(const double *__restrict__ par, const uint8_t *__restrict__ obs,
                                                 const Chunk *__restrict__ chunks, int n, const int *__restrict__ list,
                                                 const int *__restrict__ dirty, int chain, double tol, const double *__restrict__ X,
                                                 const double *__restrict__ inv, const double *__restrict__ entry, double *__restrict__ bentry,
                                                 double *__restrict__ bexit, double *__restrict__ part)
{
	constexpr int S = 64 * NPL;
	const int lane = threadIdx.x, k0 = NPL * lane;
	const WaveScanMasks wm = wave_scan_masks(lane);
	StructParN<NPL> sc;
	load_par<NPL>(par, k0, false, sc);
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
		double acc[WACC][NPL], accI = 1.0;
#pragma unroll
		for (int q = 0; q < WACC; ++q)
#pragma unroll
			for (int i = 0; i < NPL; ++i) acc[q][i] = 0.0;
		if (CKPT && top >= lo) {
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
					if ((p & 3) == 0) fstep<NPL, true, true>(fs, wm, sym, e0, e1, xf, io[p - 1]);
					else fstep<NPL, false, true>(fs, wm, sym, e0, e1, xf, 1.0);
					st<NPL>(my + ((p & (WCK - 1)) - 1) * S, xf);
				}
				for (p = pe; p >= pb; --p) {
					double Xc[NPL];
					if (p & (WCK - 1)) ld<NPL>(my + ((p & (WCK - 1)) - 1) * S, Xc); else ld<NPL>(X + ckpt_row(c.off, p) * S + k0, Xc);
					const int sym = (int)o[p - 1] & 3;
					if ((p & 3) == 0) astep<NPL, true>(sc, wm, sym, e0, e1, Xc, x, io[p - 1], acc, accI);
					else astep<NPL, false>(sc, wm, sym, e0, e1, Xc, x, 1.0, acc, accI);
				}
			}
			st<NPL>(bexit + (int64_t)b * S + k0, x); // bt_lo
		}
		if (!CKPT && top >= lo) {
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
					if (j == 3) astep<NPL, true>(sc, wm, sym, e0, e1, Xc, x, ivg, acc, accI);
					else astep<NPL, false>(sc, wm, sym, e0, e1, Xc, x, 1.0, acc, accI);
#pragma unroll
					for (int i = 0; i < NPL; ++i) Xc[i] = Xn[i];
				}
			}
			st<NPL>(bexit + (int64_t)b * S + k0, x); // bt_lo
		}
		const double iI = top >= lo ? rcp_newton(wave_total(accI)) : 1.0;
		const double mult = (double)c.mult * iI;
		double *out = part + (int64_t)b * (WACC * S) + k0;
#pragma unroll
		for (int i = 0; i < NPL; ++i) {
			const double akk = sc.dd[i] + sc.wP[i] * sc.mP[i] + sc.wS[i] * sc.mS[i]; // a[k][k]
			acc[0][i] *= sc.wP[i] * mult; acc[1][i] *= sc.wS[i] * mult; acc[2][i] *= akk * mult;
			acc[3][i] *= sc.mP[i] * mult; acc[4][i] *= sc.mS[i] * mult; acc[5][i] *= mult; acc[6][i] *= mult;
		}
#pragma unroll
		for (int q = 0; q < WACC; ++q) st<NPL>(out + q * S, acc[q]);
		if (!REPAIR || !chain || top < lo) break;
		// glued run: go on into the tile below while its start vector disagrees with this exit vector -- but not into a head of this
		// launch, nor into the tile above one (that head reads the tile's bexit as its start vector)
		const int nb = b - 1;
		if (nb < 0 || !same_seg(chunks, nb, b) || (chunks[nb].flags & CHUNK_ANCHOR_B) || head_b(chunks, dirty, n, nb)) break;
		if (nb - 1 >= 0 && same_seg(chunks, nb - 1, nb) && head_b(chunks, dirty, n, nb - 1)) break;
		double u[NPL];
		ld<NPL>(bentry + (int64_t)nb * S + k0, u);
		if (wmismatch<NPL>(u, x) <= tol) break;
		b = nb;
		st<NPL>(bentry + (int64_t)b * S + k0, x);
	}
}

// ------------------------------------------------------------------ verify, LL, reduce
template <int NPL, bool BWD>
__global__ __launch_bounds__(64) void k_wf_verify(const Chunk *__restrict__ chunks, int n, double tol, const double *__restrict__ X,
                                                    const double *__restrict__ xhi, const double *__restrict__ mine, const double *__restrict__ bexit,
                                                    int *__restrict__ dirty, int *__restrict__ cnt, unsigned long long *__restrict__ warm)
{
	constexpr int S = 64 * NPL;
	const int lane = threadIdx.x, k0 = NPL * lane, b = blockIdx.x;
	const Chunk c = chunks[b];
	bool check;
	if (!BWD) check = c.lo > 1 && !(c.flags & CHUNK_ANCHOR_F);
	else check = !(c.flags & (CHUNK_ANCHOR_B | CHUNK_LAST)) && min(c.hi, c.L - 1) >= c.lo && b + 1 < n && chunks[b + 1].off == c.off;
	double m = 0.0;
	if (check) {
		double u[NPL], v[NPL];
		ld<NPL>(mine + (int64_t)b * S + k0, u);
		// (xhi: "wide_ckpt" -- the neighbour's last row X_{lo-1} is in the per-tile array, not in X)
		ld<NPL>(BWD ? bexit + (int64_t)(b + 1) * S + k0 : (xhi ? xhi + (int64_t)(b - 1) * S + k0 : X + (c.off + c.lo - 2) * S + k0), v);
		m = wmismatch<NPL>(u, v);
	}
	if (lane == 0) {
		const int bad = check && !(m <= tol);
		dirty[b] = bad;
		if (bad) atomicAdd(cnt, 1);
		if (check) atomicMax(warm, (unsigned long long)__double_as_longlong(m));
	}
}

template <int NPL>
__global__ __launch_bounds__(64) void k_wf_ll(const Chunk *__restrict__ chunks, const double *__restrict__ X, const double *__restrict__ xhi,
                                                const double *__restrict__ inv, const double *__restrict__ entry, double *__restrict__ LLpart)
{
	constexpr int S = 64 * NPL;
	const int lane = threadIdx.x, k0 = NPL * lane, b = blockIdx.x;
	const Chunk c = chunks[b];
	const double *io = inv + c.off;
	double prod = 1.0, ll = 0.0;
	const int first = (max(c.lo, 2) + NORM_EVERY - 1) & ~(NORM_EVERY - 1);
	for (int p = first + NORM_EVERY * lane; p <= c.hi; p += NORM_EVERY * 64) {
		prod *= io[p - 1];
		if (prod > 1e280 || prod < 1e-280) { ll -= log(prod); prod = 1.0; }
	}
	ll -= log(prod);
	ll = wave_total(ll);
	double u[NPL];
	if (c.lo > 1) { // the tile was computed from entry = X_{lo-1} up to a factor: put the telescoping sum back in step
		double v[NPL];
		ld<NPL>(xhi ? xhi + (int64_t)(b - 1) * S + k0 : X + (c.off + c.lo - 2) * S + k0, u); ld<NPL>(entry + (int64_t)b * S + k0, v); // (xhi: "wide_ckpt", as k_wf_verify)
		ll += log(wave_total(lsum<NPL>(u))) - log(wave_total(lsum<NPL>(v)));
	}
	if (c.hi == c.L) {
		ld<NPL>(xhi ? xhi + (int64_t)b * S + k0 : X + (c.off + c.L - 1) * S + k0, u);
		// a segment of one bin: LL is this logarithm alone, log sum_k a0[k] e[o_1][k], and the rounding of the sum is all its
		// error (log at 0.93 magnifies one unit in the last place 14 times) -- add it up without one.  Longer segments keep
		// the plain sum: their LL adds hundreds of logarithms, and the last unit of this one is far below what those leave.
		ll += log(c.L == 1 ? wave_total_comp<NPL>(u) : wave_total(lsum<NPL>(u)));
	}
	if (lane == 0) LLpart[b] = ll * (double)c.mult;
}

// fixed-order two-stage sum over the tiles (estep_factored.hip k_reduce_factored1/2 at S = 192 / 256)
template <int S>
__global__ __launch_bounds__(S) void k_wf_reduce1(const double *__restrict__ part, int n_tiles, const double *__restrict__ LLpart,
                                                    double *__restrict__ stage)
{
	constexpr int FSL = WACC * S + 1;
	const int k = threadIdx.x, q = blockIdx.x, y = blockIdx.y;
	if (q < WACC) {
		double s = 0.0;
		for (int j = y; j < n_tiles; j += RED_ROWS) s += part[(int64_t)j * (WACC * S) + q * S + k];
		stage[(int64_t)y * FSL + q * S + k] = s;
	} else if (k == 0) {
		double s = 0.0;
		for (int j = y; j < n_tiles; j += RED_ROWS) s += LLpart[j];
		stage[(int64_t)y * FSL + WACC * S] = s;
	}
}
template <int S>
__global__ __launch_bounds__(S) void k_wf_reduce2(const double *__restrict__ stage, double tiny_total, int n, double *__restrict__ out)
{
	constexpr int FSL = WACC * S + 1;
	const int k = threadIdx.x, q = blockIdx.x;
	if (q == WACC) {
		if (k == 0) {
			double s = 0.0;
			for (int y = 0; y < RED_ROWS; ++y) s += stage[(int64_t)y * FSL + WACC * S];
			out[WACC * n] = s;
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

template <int NPL> static int launch_all(const WideLaunch &w, int what, int n_list)
{
	constexpr int S = 64 * NPL;
	const int nc = w.n_tiles;
	hipStream_t st = w.stream;
	const bool ck = w.ckpt == WCK;                      // "wide_ckpt": X at every 8th position, the tiles' last rows in w.xhi
	const double *xhi = ck ? w.xhi : nullptr;
	if (w.ckpt != 1 && !(ck && w.xhi)) return -1;
	switch (what) {
	case WF_FWD:
		if (ck) hipLaunchKernelGGL((k_wf_fwd<NPL, false, true>), dim3(nc), dim3(64), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.xhi);
		else hipLaunchKernelGGL((k_wf_fwd<NPL, false, false>), dim3(nc), dim3(64), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.xhi);
		break;
	case WF_FWD_REPAIR:
		if (ck) hipLaunchKernelGGL((k_wf_fwd<NPL, true, true>), dim3(n_list), dim3(64), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.xhi);
		else hipLaunchKernelGGL((k_wf_fwd<NPL, true, false>), dim3(n_list), dim3(64), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.xhi);
		break;
	case WF_BWARM: hipLaunchKernelGGL(k_wf_bwarm<NPL>, dim3(nc), dim3(64), 0, st, w.par, w.obs, w.chunks, w.bentry); break;
	case WF_ACC:
		if (ck) hipLaunchKernelGGL((k_wf_acc<NPL, false, true>), dim3(nc), dim3(64), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part);
		else hipLaunchKernelGGL((k_wf_acc<NPL, false, false>), dim3(nc), dim3(64), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part);
		break;
	case WF_ACC_REPAIR:
		if (ck) hipLaunchKernelGGL((k_wf_acc<NPL, true, true>), dim3(n_list), dim3(64), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part);
		else hipLaunchKernelGGL((k_wf_acc<NPL, true, false>), dim3(n_list), dim3(64), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part);
		break;
	case WF_VERIFY_F: hipLaunchKernelGGL((k_wf_verify<NPL, false>), dim3(nc), dim3(64), 0, st, w.chunks, nc, w.tol, w.X, xhi, w.entry, w.bexit, w.dirty, w.cnt, w.warm); break;
	case WF_VERIFY_B: hipLaunchKernelGGL((k_wf_verify<NPL, true>), dim3(nc), dim3(64), 0, st, w.chunks, nc, w.tol, w.X, xhi, w.bentry, w.bexit, w.dirty, w.cnt + 1, w.warm + 1); break;
	case WF_FINISH:
		hipLaunchKernelGGL(k_wf_ll<NPL>, dim3(nc), dim3(64), 0, st, w.chunks, w.X, xhi, w.inv, w.entry, w.LLpart);
		hipLaunchKernelGGL(k_wf_reduce1<S>, dim3(WACC + 1, RED_ROWS), dim3(S), 0, st, w.part, nc, w.LLpart, w.stage);
		hipLaunchKernelGGL(k_wf_reduce2<S>, dim3(WACC + 1), dim3(S), 0, st, w.stage, w.tiny_total, w.n_states, w.out);
		break;
	default: return -1;
	}
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace wide

int launch_wide_fast(const WideLaunch &w, int what, int n_list)
{
	if (w.waves > 1) return launch_wide_fast_mw(w, what, n_list); // 257..1024 states: estep_wide_fast_mw.hip
	if (w.ns == 192) return wide::launch_all<3>(w, what, n_list);
	if (w.ns == 256) return wide::launch_all<4>(w, what, n_list);
	return -1;
}

} // namespace psmc
