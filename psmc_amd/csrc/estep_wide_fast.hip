// estep_wide_fast.hip -- FAST mode, factored statistics, 129..1024 states (option "wide_fast"; api_wide_fast.hip drives it).
//
// The algebra is the one of estep_struct.hip (forward / backward step in O(N): two scans) and estep_factored.hip (the five
// triangular sums of A, E and LL straight from the backward sweep).  Only the layout differs: a state vector of S padded states is
// ONE tile per work-group of W waves, thread t holds the NPL adjacent states k = NPL t + i (wide_prims.h): S = 192 and 256 as one
// wave, (NPL, W) = (3, 1) and (4, 1); S = 512, 768 and 1024 as W = 2, 3 and 4 waves of NPL = 4.  The cross-lane part of a scan is a
// whole-wave scan (wave_shr / wave_shl by one lane, then the row scans of struct_prims.h); what crosses the waves of a tile -- the
// totals of the scans, the sums behind the scale factors, I of a tile, the mismatch of a boundary, the logarithms of k_wf_ll --
// goes through the exchange of wide_prims.h (Xchg) in a fixed order, and at W = 1 that exchange does nothing: no LDS, no barrier.
// The five structure vectors and the two emission rows stay in registers.  Padded states have zero matrix entries and zero
// emissions, so they stay zero -- but for the emission of a missing bin, which emis() (wide_prims.h) answers with 1 on every lane: the
// one start vector made of an emission alone, k_wf_bwarm's bt_q = e[o_q], is zeroed on the states n .. where it is stored.  The hang rule of
// wide_prims.h holds in every kernel here; the comments "(the same in every wave)" mark the branches it bears on.
//
// One work-group per tile and direction:
//   k_wf_fwd    speculative forward sweep (warm-up from a0, the stationary vector, `wf` bins before the tile; a segment's first tile
//               from X_1 = a0 e[o_1]); stores X (one row of 8 S bytes per position), 1/d_p at p % 4 == 0 (a power of two: pow2_rcp)
//               and the start vector `entry`.  REPAIR: from the neighbour's X_{lo-1}; with `chain` the tile walks on into the next
//               tile while that tile's start vector disagrees with the new exit vector (a glued run: one round instead of one per tile).
//   k_wf_bwarm  speculative backward warm-up: bentry = bt_{top+1} of every tile, from bt_q = e[o_q] `wb` bins above it.
//   k_wf_acc    the tile's backward sweep from bentry, reading X: the seven per-thread sums of estep_factored.hip, bexit = bt_lo,
//               the tile's partials (a repaired tile OVERWRITES them: nothing is counted twice).  REPAIR: from the exit vector of the
//               tile above, chaining downwards like the forward repair.
//   k_wf_verify every tile's start vector against its neighbour's exit vector (the test of estep_fast.hip k_verify).
//   k_wf_ll, k_wf_reduce1/2: the log-likelihood of a tile (as estep_fast.hip k_ll) and the fixed-order sum of the partials.
// A chain never enters a tile that is itself the head of a repair in the same launch, nor the neighbour whose boundary vector such a
// head starts from: no work-group of a repair launch reads or writes what another work-group of it writes, so the result does not
// depend on scheduling.  A tile a chain stops in front of is flagged again by the next verify round.
//
// "wide_ckpt" (compile-time variants CKPT of k_wf_fwd and k_wf_acc): X keeps the rows at p % 8 == 0 only, by absolute position
// (wide_prims.h ckpt_row), and every tile's last row goes to xhi[b], which k_wf_verify, the start of a forward repair and k_wf_ll
// read instead of X_{lo-1} / X_L.  The accumulate sweep recomputes the seven rows between two checkpoints into LDS with fstep
// (wide_prims.h), the forward sweep's own step, from the scale factors that sweep stored: the same bits as the full table.  A
// chained repair rewrites the checkpoints and last rows of the tiles it walks through; what it may not enter is unchanged (a head
// reads its neighbour's xhi row where it read the neighbour's last X row).
//
// Resources (hipcc -O3, gfx950, make resources; scratch is 0 everywhere).  Per shape (NPL, W): VGPRs (+ AGPRs) | LDS bytes per
// work-group | waves per SIMD.  LDS = the exchange slots, 2 x 6 x W doubles at W > 1, plus with CKPT 7 rows of S doubles in k_wf_acc.
//   kernel                               (3,1) S=192      (4,1) S=256      (4,2) S=512      (4,3) S=768      (4,4) S=1024
//   k_wf_fwd                                 86     0 5      108     0 4      114   192 4      118   288 4      126   384 4
//   k_wf_fwd    repair                       90     0 5      112     0 4      120   192 4      124   288 4      130   384 3
//   k_wf_fwd    CKPT                         88     0 5      110     0 4      116   192 4      120   288 4      128   384 4
//   k_wf_fwd    CKPT, repair                 92     0 5      114     0 4      126   192 4      130   288 3      138   384 3
//   k_wf_bwarm                               80     0 6      102     0 4      106   192 4      108   288 4      112   384 4
//   k_wf_acc                                154     0 3      206     0 2      216   192 2      220   288 2      226   384 2
//   k_wf_acc    repair                      178     0 2      228     0 2      234   192 2      238   288 2      244   384 2
//   k_wf_acc    CKPT                        196 10752 2      256 14336 2      220 28864 2      224 43296 2      226 57728 2
//   k_wf_acc    CKPT, repair                220 10752 2   256+24 14336 1      248 28864 2      252 43296 2      252 57728 2
//   k_wf_verify forward                      33     0 8       36     0 8       40   192 8       40   288 8       40   384 8
//   k_wf_verify backward                     36     0 8       39     0 8       40   192 8       40   288 8       40   384 8
//   k_wf_ll                                  37     0 8       38     0 8       38   192 8       38   288 8       38   384 8
//   k_wf_reduce1 / 2                     8 / 42 VGPRs at every width, no LDS
// "wide_gap_tiles" (GAP = 1: the listed tiles only, the registers of the plain kernels; GAP = 2: sweeps from a tile's own start
// vector and the repairs of a plan with qualifying runs, the registers of the repairs; LDS as the kernel above them):
//   k_wf_fwd    GAP 1 | CKPT, GAP 1     86  |  88   5      108  | 110  4      114  | 116  4      118  | 120  4      126  | 128  4
//   k_wf_fwd    GAP 2 | CKPT, GAP 2     90  |  92   5      112  | 114  4      120  | 122  4      124  | 126  4      130  | 134  3
//   k_wf_bwarm  LIST                         80     6           102    4           106    4           108    4           112    4
//   k_wf_acc    GAP 1 | CKPT, GAP 1    154 3 | 196 2       206 2 | 256 2       216 2 | 220 2       220 2 | 224 2       226 2 | 226 2
//   k_wf_acc    GAP 2 | CKPT, GAP 2    178 2 | 220 2       228 2 | 256+24 1    234 2 | 248 2       238 2 | 252 2       244 2 | 252 2
// The kernels of the transfer-matrix chain itself: estep_wide_gap.hip.
// The CKPT accumulate sweep at (4, 1) sits on the register edge (256 VGPRs; its repair takes 24 AGPRs and one wave per SIMD): the
// one-wave order of astep and of the scaled steps of wide_prims.h is what keeps it there.  With CKPT the staged rows are at most
// 115 KB of a compute unit's 160 KB of LDS (eight tiles of S = 256; four, two and two work-groups at W = 2, 3, 4).
#include <hip/hip_runtime.h>
#include "wave_prims.h"
#include "struct_prims.h"
#include "psmc_hip_internal.h"
#include "wide_fast.h"
#include "wide_prims.h"

namespace psmc {
namespace wide {

// ------------------------------------------------------------------ forward
// CKPT ("wide_ckpt"): X keeps the rows at p % 8 == 0 only (ckpt_row), and the tile's last row X_hi goes to xhi[b] -- what the
// neighbour's verify and repair and k_wf_ll read; the accumulate sweep recomputes the rest.
// GAP ("wide_gap_tiles"; 0: the kernels as they were, the two last arguments unused): 1 = the speculative sweep over the listed tiles only
// (the unglued tiles of the plan); 2 = the repair of a plan with qualifying runs -- a list entry is a tile and two flags, WG_OWN: start from
// the tile's own entry[b] (what the transfer-matrix chain of estep_wide_gap.hip left there) instead of the neighbour's last row, WG_SINGLE:
// do not walk on (a gap tile of a run: the chain has given every one its own start).  The walk never enters the first chained tile of a
// run (glue & WG_FIRST_F): the chain crosses the run, not the walk.  `init`: the launch behind the chain at the start of an E-step -- no
// verify has run, so there are no heads to respect, and a tile glued forward (glue & 1) has no start vector to compare with: walk on.
template <int NPL, int W, bool REPAIR, bool CKPT, int GAP = 0>
__global__ __launch_bounds__(64 * W) void k_wf_fwd(const double *__restrict__ par, const uint8_t *__restrict__ obs,
                                                     const Chunk *__restrict__ chunks, int n, const int *__restrict__ list,
                                                     const int *__restrict__ dirty, int chain, double tol, double *__restrict__ X,
                                                     double *__restrict__ inv, double *__restrict__ entry, double *__restrict__ xhi,
                                                     const int *__restrict__ glue, int init)
{
	constexpr int S = 64 * NPL * W;
	__shared__ double xs[2 * WX_SLOTS * W];
	Xchg<W> xc = make_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid;
	const WaveScanMasks wm = wave_scan_masks(xc.lane);
	StructParN<NPL> sc;
	load_par<NPL, S>(par, k0, true, sc);
	double e0[NPL], e1[NPL];
	ld<NPL>(par + WP_E0 * S + k0, e0); ld<NPL>(par + WP_E1 * S + k0, e1);
	if (REPAIR) __builtin_amdgcn_s_setprio(3);
	int b = REPAIR || GAP ? list[blockIdx.x] : (int)blockIdx.x;
	int own = 0, single = 0; // (GAP == 2; from the list: the same in every wave)
	if (GAP == 2) { own = b & WG_OWN; single = b & WG_SINGLE; b &= WG_TILE; }
	Chunk c = chunks[b];
	double x[NPL];
	int p0;
	if (REPAIR) { // from the neighbour's X_{lo-1} (a repaired tile is never a segment's first)
		if (GAP == 2 && own) ld<NPL>(entry + (int64_t)b * S + k0, x);
		else if (CKPT) ld<NPL>(xhi + (int64_t)(b - 1) * S + k0, x); else ld<NPL>(X + (c.off + c.lo - 2) * S + k0, x);
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
					const double iv = fstep<NPL, W, true, false>(sc, wm, sym, e0, e1, x, 1.0, xc);
					if (p >= lo && tid == 0) io[p - 1] = iv;
				} else fstep<NPL, W, false, false>(sc, wm, sym, e0, e1, x, 1.0, xc);
				if (!CKPT) { if (p >= lo) st<NPL>(fo + (int64_t)(p - 1) * S, x); }
				else if (p >= lo) {
					if (j == 3 && (p & (WCK - 1)) == 0) st<NPL>(X + ckpt_row(c.off, p) * S + k0, x);
					if (p == hi) st<NPL>(xhi + (int64_t)b * S + k0, x);
				}
			}
		}
		if (!REPAIR || (GAP != 2 && !chain)) break;
		// glued run: go on into the next tile while its start vector disagrees with this exit vector -- but not into a head of this
		// launch, nor into the tile before one (that head reads the tile's last X row as its start vector)
		const int nb = b + 1;
		if (GAP == 2) { // (every condition from the list, the plan or the verify flags: the same in every wave)
			if (single || nb >= n || !same_seg(chunks, b, nb) || (chunks[nb].flags & CHUNK_ANCHOR_F) || (glue[nb] & WG_FIRST_F)) break;
			const bool through = init && (glue[nb] & 1); // glued at plan time and not swept yet: nothing to compare with
			if (!through && !chain) break;
			if (!init) {
				if (head_f(chunks, dirty, nb)) break;
				if (nb + 1 < n && same_seg(chunks, nb, nb + 1) && head_f(chunks, dirty, nb + 1)) break;
			}
			if (!through) {
				double u[NPL];
				ld<NPL>(entry + (int64_t)nb * S + k0, u);
				if (tile_mismatch<NPL, W>(u, x, xc) <= tol) break;
			}
			b = nb; c = chunks[b]; p0 = c.lo;
			continue;
		}
		if (nb >= n || !same_seg(chunks, b, nb) || (chunks[nb].flags & CHUNK_ANCHOR_F) || head_f(chunks, dirty, nb)) break;
		if (nb + 1 < n && same_seg(chunks, nb, nb + 1) && head_f(chunks, dirty, nb + 1)) break;
		double u[NPL];
		ld<NPL>(entry + (int64_t)nb * S + k0, u);
		if (tile_mismatch<NPL, W>(u, x, xc) <= tol) break; // from exchanged values: the same decision in every wave
		b = nb; c = chunks[b]; p0 = c.lo;
	}
}

// ------------------------------------------------------------------ backward
// LIST ("wide_gap_tiles"): the listed tiles only (those not glued backward; the chain of estep_wide_gap.hip gives the others their start vectors)
template <int NPL, int W, bool LIST = false>
__global__ __launch_bounds__(64 * W) void k_wf_bwarm(const double *__restrict__ par, const uint8_t *__restrict__ obs,
                                                       const Chunk *__restrict__ chunks, double *__restrict__ bentry, const int *__restrict__ list)
{
	constexpr int S = 64 * NPL * W;
	__shared__ double xs[2 * WX_SLOTS * W];
	Xchg<W> xc = make_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid, b = LIST ? list[blockIdx.x] : (int)blockIdx.x;
	const WaveScanMasks wm = wave_scan_masks(xc.lane);
	const Chunk c = chunks[b];
	const int top = min(c.hi, c.L - 1);
	if (top < c.lo) return; // a tile holding only position L owns no transition (every wave of the tile leaves here)
	StructParN<NPL> sc;
	load_par<NPL, S>(par, k0, false, sc);
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
			if (j == 3) bstep<NPL, W, true>(sc, wm, sym, e0, e1, x, xc); else bstep<NPL, W, false>(sc, wm, sym, e0, e1, x, xc);
		}
	}
	// The start vector leaves with zeros on the padded states n ..: a missing bin's emission is 1 on every lane (emis), and where no step
	// follows the seed (q = top + 1: a segment's last tile) it would go out as it stands, into the first scaling of every sweep that starts
	// from bentry and into V's padded columns.  A step clears the padded states, so behind one this changes nothing -- which is why the
	// zeros are put here and not at the seed: there they would change the factor of a warm-up's first scaled step when bin q is missing,
	// a factor that any positive number can be, and with it the last bits of every speculated start vector at the sizes with padded states.
	// A padded state is one whose row of the matrix is zero -- P, R and dd, which the loop above holds in registers (a state of an HMM has
	// a row that sums to 1) -- so the kernel needs neither n nor another register.
#pragma unroll
	for (int i = 0; i < NPL; ++i) x[i] = sc.wP[i] != 0.0 || sc.wS[i] != 0.0 || sc.dd[i] != 0.0 ? x[i] : 0.0;
	st<NPL>(bentry + (int64_t)b * S + k0, x);
}

// One position p of the accumulate sweep (estep_factored.hip acc_step with whole-wave scans, and one exchange: the four scan
// totals and, NORM, the sum of bt_{p+1}): x = bt_{p+1} on entry, bt_p on exit; X = X_p; inv = the forward scale factor at p (NORM:
// p % 4 == 0).  The partial sums are kept in units of the current I; I_lane is this thread's share of it.
template <int NPL, int W, bool NORM>
__device__ __forceinline__ void astep(const StructParN<NPL> &sc, const WaveScanMasks &wm, int sym, const double (&e0)[NPL],
                                      const double (&e1)[NPL], const double (&X)[NPL], double (&x)[NPL], double inv,
                                      double (&acc)[WACC][NPL], double &I_lane, Xchg<W> &xc)
{
	double ev[NPL];
	emis<NPL>(sym, e0, e1, ev);
	const double m0 = sym == 0 ? 1.0 : 0.0, m1 = sym == 1 ? 1.0 : 0.0;
	double f = 1.0;
	if constexpr (W == 1) { // (one wave: the factor before the scans, as bstep_parts of wide_prims.h)
		if (NORM) {
			const double sb = rcp_newton(wave_total(lsum<NPL>(x)));
#pragma unroll
			for (int i = 0; i < NPL; ++i) ev[i] *= sb;
			f = sb * pow2_rcp(inv);
		}
	}
	double su[NPL + 1], pv[NPL + 1], sx[NPL + 1], px[NPL + 1];
	su[NPL] = 0.0; sx[NPL] = 0.0; pv[0] = 0.0; px[0] = 0.0; // pv / px shifted by one: pv[i+1] = inclusive at i
#pragma unroll
	for (int i = NPL - 1; i >= 0; --i) { su[i] = __builtin_fma(x[i], sc.mS[i], su[i + 1]); sx[i] = __builtin_fma(X[i], sc.wP[i], sx[i + 1]); }
#pragma unroll
	for (int i = 0; i < NPL; ++i) { pv[i + 1] = __builtin_fma(x[i], sc.mP[i], pv[i]); px[i + 1] = __builtin_fma(X[i], sc.wS[i], px[i]); }
	double ES = wave_excl_suffix(su[0], wm), EP = wave_excl_prefix(pv[NPL]);
	double EX = wave_excl_suffix(sx[0], wm), PX = wave_excl_prefix(px[NPL]);
	if constexpr (W > 1) {
		xc.put(0, readlane_f64(ES + su[0], 0)); xc.put(1, readlane_f64(EP + pv[NPL], 63));
		xc.put(2, readlane_f64(EX + sx[0], 0)); xc.put(3, readlane_f64(PX + px[NPL], 63));
		if (NORM) xc.put(4, wave_total(lsum<NPL>(x)));
		xc.sync();
		ES += xc.above(0); EP += xc.below(1); EX += xc.above(2); PX += xc.below(3);
		if (NORM) {
			const double sb = rcp_newton(xc.sum(4));
#pragma unroll
			for (int i = 0; i < NPL; ++i) ev[i] *= sb;
			f = sb * pow2_rcp(inv);
		}
		xc.next();
	}
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
// bits, every recomputed step's exchange as k_wf_fwd does it -- from the checkpoint X_{8m}, or in the tile's lowest block from
// entry[b] (the X_{lo-1} the tile was built on) or from X_1 = a0 e[o_1], into LDS (rows 8m+1 .. 8m+7: 7 S doubles, 56 KB at
// W = 4, beside the exchange slots; every thread reads back what it wrote itself, so no barrier); then astep runs over them,
// highest position first, X_{8m} read from the table.  The block bounds come from the tile descriptor alone.
// GAP: as k_wf_fwd, mirrored -- WG_OWN starts from the tile's own bentry[b], the walk goes down, never into the first chained tile
// of a run from above (glue & WG_FIRST_B), and with `init` through the tiles glued backward (glue & 2).
template <int NPL, int W, bool REPAIR, bool CKPT, int GAP = 0>
__global__ __launch_bounds__(64 * W) void k_wf_acc(const double *__restrict__ par, const uint8_t *__restrict__ obs,
                                                     const Chunk *__restrict__ chunks, int n, const int *__restrict__ list,
                                                     const int *__restrict__ dirty, int chain, double tol, const double *__restrict__ X,
                                                     const double *__restrict__ inv, const double *__restrict__ entry, double *__restrict__ bentry,
                                                     double *__restrict__ bexit, double *__restrict__ part, const int *__restrict__ glue, int init)
{
	constexpr int S = 64 * NPL * W;
	__shared__ double xs[2 * WX_SLOTS * W];
	Xchg<W> xc = make_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid;
	const WaveScanMasks wm = wave_scan_masks(xc.lane);
	StructParN<NPL> sc;
	load_par<NPL, S>(par, k0, false, sc);
	double e0[NPL], e1[NPL];
	ld<NPL>(par + WP_E0 * S + k0, e0); ld<NPL>(par + WP_E1 * S + k0, e1);
	if (REPAIR) __builtin_amdgcn_s_setprio(3);
	int b = REPAIR || GAP ? list[blockIdx.x] : (int)blockIdx.x;
	int own = 0, single = 0; // (GAP == 2; from the list: the same in every wave)
	if (GAP == 2) { own = b & WG_OWN; single = b & WG_SINGLE; b &= WG_TILE; }
	double x[NPL];
	if (REPAIR && !(GAP == 2 && own)) { ld<NPL>(bexit + (int64_t)(b + 1) * S + k0, x); st<NPL>(bentry + (int64_t)b * S + k0, x); }
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
					if ((p & 3) == 0) fstep<NPL, W, true, true>(fs, wm, sym, e0, e1, xf, io[p - 1], xc);
					else fstep<NPL, W, false, true>(fs, wm, sym, e0, e1, xf, 1.0, xc);
					st<NPL>(my + ((p & (WCK - 1)) - 1) * S, xf);
				}
				for (p = pe; p >= pb; --p) {
					double Xc[NPL];
					if (p & (WCK - 1)) ld<NPL>(my + ((p & (WCK - 1)) - 1) * S, Xc); else ld<NPL>(X + ckpt_row(c.off, p) * S + k0, Xc);
					const int sym = (int)o[p - 1] & 3;
					if ((p & 3) == 0) astep<NPL, W, true>(sc, wm, sym, e0, e1, Xc, x, io[p - 1], acc, accI, xc);
					else astep<NPL, W, false>(sc, wm, sym, e0, e1, Xc, x, 1.0, acc, accI, xc);
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
					if (j == 3) astep<NPL, W, true>(sc, wm, sym, e0, e1, Xc, x, ivg, acc, accI, xc);
					else astep<NPL, W, false>(sc, wm, sym, e0, e1, Xc, x, 1.0, acc, accI, xc);
#pragma unroll
					for (int i = 0; i < NPL; ++i) Xc[i] = Xn[i];
				}
			}
			st<NPL>(bexit + (int64_t)b * S + k0, x); // bt_lo
		}
		const double iI = top >= lo ? rcp_newton(tile_total<W>(xc, wave_total(accI))) : 1.0;
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
		if (!REPAIR || (GAP != 2 && !chain) || top < lo) break;
		// glued run: go on into the tile below while its start vector disagrees with this exit vector -- but not into a head of this
		// launch, nor into the tile above one (that head reads the tile's bexit as its start vector)
		const int nb = b - 1;
		if (GAP == 2) { // (every condition from the list, the plan or the verify flags: the same in every wave)
			if (single || nb < 0 || !same_seg(chunks, nb, b) || (chunks[nb].flags & CHUNK_ANCHOR_B) || (glue[nb] & WG_FIRST_B)) break;
			const bool through = init && (glue[nb] & 2); // glued at plan time and not swept yet: nothing to compare with
			if (!through && !chain) break;
			if (!init) {
				if (head_b(chunks, dirty, n, nb)) break;
				if (nb - 1 >= 0 && same_seg(chunks, nb - 1, nb) && head_b(chunks, dirty, n, nb - 1)) break;
			}
			if (!through) {
				double u[NPL];
				ld<NPL>(bentry + (int64_t)nb * S + k0, u);
				if (tile_mismatch<NPL, W>(u, x, xc) <= tol) break;
			}
			b = nb;
			st<NPL>(bentry + (int64_t)b * S + k0, x);
			continue;
		}
		if (nb < 0 || !same_seg(chunks, nb, b) || (chunks[nb].flags & CHUNK_ANCHOR_B) || head_b(chunks, dirty, n, nb)) break;
		if (nb - 1 >= 0 && same_seg(chunks, nb - 1, nb) && head_b(chunks, dirty, n, nb - 1)) break;
		double u[NPL];
		ld<NPL>(bentry + (int64_t)nb * S + k0, u);
		if (tile_mismatch<NPL, W>(u, x, xc) <= tol) break; // from exchanged values: the same decision in every wave
		b = nb;
		st<NPL>(bentry + (int64_t)b * S + k0, x);
	}
}

// ------------------------------------------------------------------ verify, LL, reduce
template <int NPL, int W, bool BWD>
__global__ __launch_bounds__(64 * W) void k_wf_verify(const Chunk *__restrict__ chunks, int n, double tol, const double *__restrict__ X,
                                                        const double *__restrict__ xhi, const double *__restrict__ mine, const double *__restrict__ bexit,
                                                        int *__restrict__ dirty, int *__restrict__ cnt, unsigned long long *__restrict__ warm)
{
	constexpr int S = 64 * NPL * W;
	__shared__ double xs[2 * WX_SLOTS * W];
	Xchg<W> xc = make_xchg<W>(xs);
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
		m = tile_mismatch<NPL, W>(u, v, xc);
	}
	if (tid == 0) {
		const int bad = check && !(m <= tol);
		dirty[b] = bad;
		if (bad) atomicAdd(cnt, 1);
		if (check) atomicMax(warm, (unsigned long long)__double_as_longlong(m));
	}
}

template <int NPL, int W>
__global__ __launch_bounds__(64 * W) void k_wf_ll(const Chunk *__restrict__ chunks, const double *__restrict__ X, const double *__restrict__ xhi, const double *__restrict__ inv,
                                                    const double *__restrict__ entry, double *__restrict__ LLpart)
{
	constexpr int S = 64 * NPL * W;
	__shared__ double xs[2 * WX_SLOTS * W];
	Xchg<W> xc = make_xchg<W>(xs);
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
	ll = tile_total<W>(xc, wave_total(ll));
	double u[NPL];
	if (c.lo > 1) { // the tile was computed from entry = X_{lo-1} up to a factor: put the telescoping sum back in step
		double v[NPL];
		ld<NPL>(xhi ? xhi + (int64_t)(b - 1) * S + k0 : X + (c.off + c.lo - 2) * S + k0, u); ld<NPL>(entry + (int64_t)b * S + k0, v); // (xhi: "wide_ckpt", as k_wf_verify)
		const double su = tile_vsum<NPL, W>(xc, u), sv = tile_vsum<NPL, W>(xc, v);
		ll += log(su) - log(sv);
	}
	if (c.hi == c.L) {
		ld<NPL>(xhi ? xhi + (int64_t)b * S + k0 : X + (c.off + c.L - 1) * S + k0, u);
		// a segment of one bin: LL is this logarithm alone, log sum_k a0[k] e[o_1][k], and the rounding of the sum is all its
		// error (log at 0.93 magnifies one unit in the last place 14 times) -- add it up without one.  Longer segments keep
		// the plain sum: their LL adds hundreds of logarithms, and the last unit of this one is far below what those leave.
		ll += log(c.L == 1 ? tile_total_comp<NPL, W>(xc, u) : tile_vsum<NPL, W>(xc, u)); // (c.L: the same in every wave)
	}
	if (tid == 0) LLpart[b] = ll * (double)c.mult;
}

// fixed-order two-stage sum over the tiles (estep_factored.hip k_reduce_factored1/2 at the tile's width: one thread per state)
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

template <int NPL, int W> static int launch_all(const WideLaunch &w, int what, int n_list)
{
	constexpr int S = 64 * NPL * W, T = 64 * W;
	const int nc = w.n_tiles;
	hipStream_t st = w.stream;
	const bool ck = w.ckpt == WCK;                      // "wide_ckpt": X at every 8th position, the tiles' last rows in w.xhi
	const double *xhi = ck ? w.xhi : nullptr;
	if (w.ckpt != 1 && !(ck && w.xhi)) return -1;
	if (what >= WF_FWD_LIST && (n_list <= 0 || !w.list || !w.glue)) return n_list == 0 ? 0 : -1; // (an empty list: nothing to launch)
	switch (what) {
	case WF_FWD:
		if (ck) hipLaunchKernelGGL((k_wf_fwd<NPL, W, false, true>), dim3(nc), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.xhi, nullptr, 0);
		else hipLaunchKernelGGL((k_wf_fwd<NPL, W, false, false>), dim3(nc), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.xhi, nullptr, 0);
		break;
	case WF_FWD_REPAIR:
		if (ck) hipLaunchKernelGGL((k_wf_fwd<NPL, W, true, true>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.xhi, nullptr, 0);
		else hipLaunchKernelGGL((k_wf_fwd<NPL, W, true, false>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.xhi, nullptr, 0);
		break;
	case WF_BWARM: hipLaunchKernelGGL((k_wf_bwarm<NPL, W>), dim3(nc), dim3(T), 0, st, w.par, w.obs, w.chunks, w.bentry, nullptr); break;
	case WF_ACC:
		if (ck) hipLaunchKernelGGL((k_wf_acc<NPL, W, false, true>), dim3(nc), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part, nullptr, 0);
		else hipLaunchKernelGGL((k_wf_acc<NPL, W, false, false>), dim3(nc), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part, nullptr, 0);
		break;
	case WF_ACC_REPAIR:
		if (ck) hipLaunchKernelGGL((k_wf_acc<NPL, W, true, true>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part, nullptr, 0);
		else hipLaunchKernelGGL((k_wf_acc<NPL, W, true, false>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part, nullptr, 0);
		break;
	// "wide_gap_tiles": the listed speculative sweeps (w.list, n_list tiles) and the sweeps / repairs of a plan with qualifying runs
	case WF_FWD_LIST:
		if (ck) hipLaunchKernelGGL((k_wf_fwd<NPL, W, false, true, 1>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.xhi, w.glue, 0);
		else hipLaunchKernelGGL((k_wf_fwd<NPL, W, false, false, 1>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.xhi, w.glue, 0);
		break;
	case WF_FWD_GAP:
		if (ck) hipLaunchKernelGGL((k_wf_fwd<NPL, W, true, true, 2>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.xhi, w.glue, w.init);
		else hipLaunchKernelGGL((k_wf_fwd<NPL, W, true, false, 2>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.xhi, w.glue, w.init);
		break;
	case WF_BWARM_LIST: hipLaunchKernelGGL((k_wf_bwarm<NPL, W, true>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, w.bentry, w.list); break;
	case WF_ACC_LIST:
		if (ck) hipLaunchKernelGGL((k_wf_acc<NPL, W, false, true, 1>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part, w.glue, 0);
		else hipLaunchKernelGGL((k_wf_acc<NPL, W, false, false, 1>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, 0, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part, w.glue, 0);
		break;
	case WF_ACC_GAP:
		if (ck) hipLaunchKernelGGL((k_wf_acc<NPL, W, true, true, 2>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part, w.glue, w.init);
		else hipLaunchKernelGGL((k_wf_acc<NPL, W, true, false, 2>), dim3(n_list), dim3(T), 0, st, w.par, w.obs, w.chunks, nc, w.list, w.dirty, w.chain, w.tol, w.X, w.inv, w.entry, w.bentry, w.bexit, w.part, w.glue, w.init);
		break;
	case WF_VERIFY_F: hipLaunchKernelGGL((k_wf_verify<NPL, W, false>), dim3(nc), dim3(T), 0, st, w.chunks, nc, w.tol, w.X, xhi, w.entry, w.bexit, w.dirty, w.cnt, w.warm); break;
	case WF_VERIFY_B: hipLaunchKernelGGL((k_wf_verify<NPL, W, true>), dim3(nc), dim3(T), 0, st, w.chunks, nc, w.tol, w.X, xhi, w.bentry, w.bexit, w.dirty, w.cnt + 1, w.warm + 1); break;
	case WF_FINISH:
		hipLaunchKernelGGL((k_wf_ll<NPL, W>), dim3(nc), dim3(T), 0, st, w.chunks, w.X, xhi, w.inv, w.entry, w.LLpart);
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
	if (w.waves > 1 ? w.ns != 256 * w.waves : (w.ns != 192 && w.ns != 256)) return -1;
	switch (w.ns) {
	case 192: return wide::launch_all<3, 1>(w, what, n_list);
	case 256: return wide::launch_all<4, 1>(w, what, n_list);
	case 512: return wide::launch_all<4, 2>(w, what, n_list);
	case 768: return wide::launch_all<4, 3>(w, what, n_list);
	case 1024: return wide::launch_all<4, 4>(w, what, n_list);
	}
	return -1;
}

} // namespace psmc
