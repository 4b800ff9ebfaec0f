// estep_wide_gap.hip -- the wide fast path (estep_wide_fast.hip, 129..1024 states) across runs of missing data: option
// "wide_gap_tiles" (api_wide_fast.hip plans and drives it).
//
// Inside a run of `N` bins the emission is 1 for every state, so a full tile of T missing bins maps its start vector by one fixed
// matrix, M = a^T to the power T, whatever the tile: forward X_{hi} = X_{lo-1} M, backward bt_{lo} = M bt_{hi+1}, both up to the
// positive factors the sweeps scale by.  A speculative warm-up cannot cross such a run (the chain forgets at the matrix's second
// eigenvalue alone), and a repair walks it position by position.  Here the run is crossed tile by tile:
//   k_wf_gapmat    once per E-step (the parameters move): row k of M is the unit vector of state k swept T bins through fstep
//                  (wide_prims.h), the forward sweep's own step, under the missing symbol; one work-group per row, in the layout of
//                  the sweeps.  The steps are the UNSCALED ones: what the sweep does at p % 4 == 0 on top is a multiplication of every
//                  state by one power of two, which is exact -- so a row here is the sweep's row with those factors undone, and all
//                  rows are on one scale (the matrix is stochastic under the missing symbol: a row's sum stays 1 up to rounding).
//   k_wf_gapchain  one work-group of 1024 threads per qualifying run and direction: reads the vector the run is entered with,
//                  applies M once per tile and writes every tile's start vector (wide_fast.h GapRun).  Forward x <- x M: one thread
//                  per column, the rows split into 1024 / S contiguous ranges whose partial sums are added lowest range first.
//                  Backward y <- M y: one wave per row (rows wave, wave + 16, ...), every lane the columns lane, lane + 64, ...
//                  in ascending order, then wave_total's fixed order.  The vector is normalised to sum 1 after every application
//                  (every consumer of entry / bentry is invariant to a positive factor).  No atomics, every sum in a fixed order:
//                  the same bits at every call.
// Correctness does not rest on the chain: k_wf_verify tests the boundaries of the chained tiles like any other, and the structured
// sweep of a gap tile from the chain's vector is what fills X, inv and the statistics.
//
// Resources (hipcc -O3, gfx950, make resources; scratch is 0 everywhere): VGPRs | LDS bytes | waves per SIMD
//   kernel                               (3,1) S=192      (4,1) S=256      (4,2) S=512      (4,3) S=768      (4,4) S=1024
//   k_wf_gapmat                              62     0 8       78     0 6       82   192 5       85   288 5       89   384 5
//   k_wf_gapchain forward                    68  9224 7       68 10248 7       68 12296 7       48 12296 8       46 16392 8
//   k_wf_gapchain backward                   28  9224 8       30 10248 8       46 12296 8       64 12296 8       82 16392 5
//   k_wf_hompilot                            72     0 7       94     0 5       94   192 5       98   288 4      106   384 4
//   k_wf_hommat                              78     0 6       98     0 4       90   192 5       93   288 5       97   384 4
//   k_wf_gapchain forward  HOM               70  9224 7       68 10248 7       68 12296 7       48 12296 8       44 16392 8
//   k_wf_gapchain backward HOM               34  9224 8       36 10248 8       52 12296 8       70 12296 7       88 16392 5
//   k_wf_mixpilot                            82     0 5      104     0 4      110   192 4      114   288 4      122   384 4
//   k_wf_mixmat                              80     0 6      102     0 4      104   192 4      109   288 4      113   384 4
//   k_wf_gapchain forward  MIX               70  9224 7       68 10248 7       68 12296 7       48 12296 8       44 16392 8
//   k_wf_gapchain backward MIX               34  9224 8       36 10248 8       52 12296 8       70 12296 7       88 16392 5
// (the chain is one work-group of 16 waves whatever the width: four waves per SIMD of one compute unit)
//
// "wide_hom_tiles": the same across runs of homozygosity (symbol 0 only).  A full tile of T homozygous bins maps its start vector by
// M_h = (a D)^T-th power forward and (D a)^T-th power = D M_h D^-1 backward, D = diag(e0):
//   k_wf_hompilot  once per E-step, one work-group: the uniform vector swept T bins under symbol 0, which yields the power-of-two
//                  factors of a sweep through such a tile (M_h is far from stochastic: e0 < 1 at every bin);
//   k_wf_hommat    row k of M_h = the unit vector of state k swept T bins under symbol 0 with the pilot's factors: all rows on one
//                  scale, none can overflow (the argument: at the kernel);
//   k_wf_gapchain HOM  the chain of a plan whose qualifying runs hold hom tiles: per tile the matrix of the tile's class (a device
//                  copy of wg_cls), backward across a hom tile D M_h D^-1 v.  Read order, summation order and normalisation are the
//                  plain chain's; a run of gap tiles alone gives the same bits through either instantiation.
//
// "wide_mix_tiles": the same across het-free tiles that hold BOTH symbol 0 and `N` (class 3 of k_tile_class, wg_cls 6).  Such a tile has
// maps of its own, and no diagonal relation ties the backward one to the forward one, so every mix tile owns TWO matrices.  With
// D_p = diag(e0) at a homozygous bin p and D_p = I at a missing one, over the tile's bins lo .. hi:
//   forward   F = a D_lo a D_lo+1 ... a D_hi,  X_hi = X_{lo-1} F;      row k of F = e_k swept through the symbols o_lo .. o_hi
//   backward  B = D_lo a D_lo+1 a ... D_hi a,  bt_lo = B bt_{hi+1};    row k of B = D_lo(k) e_k swept through o_lo+1 .. o_hi, N
// -- both are FORWARD sweeps of unit vectors through fstep, the second through the sequence shifted by one bin with `N` appended.
//   k_wf_mixpilot  once per E-step, one work-group per JOB -- a mix tile and a direction in which a chain of the plan crosses it (a tile
//                  anchored in a direction, or of a run whose chain was dropped, needs no matrix there): the uniform vector swept
//                  through that direction's sequence, which yields the power-of-two factors of that sweep;
//   k_wf_mixmat    one work-group per row and job: the unit vector (direction 1: times D_lo(k)) swept through the same sequence
//                  with that pilot's factors.  All matrices of an E-step are built by these two launches, side by side.  Both read
//                  the symbols of four bins at a time, ahead of the four steps that use them;
//   k_wf_gapchain MIX  the chain of a plan whose qualifying runs hold mix tiles: across a tile of class 6 the tile's own F (forward) or
//                  B (backward) through a device table tile -> slot, no D scaling; across classes 2 and 4 what the HOM chain applies.
//                  Read order, summation order and normalisation are the plain chain's.
#include <hip/hip_runtime.h>
#include "wave_prims.h"
#include "struct_prims.h"
#include "psmc_hip_internal.h"
#include "wide_fast.h"
#include "wide_prims.h"

namespace psmc {
namespace wide {

template <int NPL, int W>
__global__ __launch_bounds__(64 * W) void k_wf_gapmat(const double *__restrict__ par, int T, double *__restrict__ M)
{
	constexpr int S = 64 * NPL * W;
	__shared__ double xs[2 * WX_SLOTS * W];
	Xchg<W> xc = make_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid, k = blockIdx.x;
	const WaveScanMasks wm = wave_scan_masks(xc.lane);
	StructParN<NPL> sc;
	load_par<NPL, S>(par, k0, true, sc);
	double e0[NPL], e1[NPL]; // (the missing symbol reads neither)
	ld<NPL>(par + WP_E0 * S + k0, e0); ld<NPL>(par + WP_E1 * S + k0, e1);
	double x[NPL];
#pragma unroll
	for (int i = 0; i < NPL; ++i) x[i] = k0 + i == k ? 1.0 : 0.0;
	for (int p = 0; p < T; ++p) fstep<NPL, W, false, false>(sc, wm, 2, e0, e1, x, 1.0, xc); // (T: the same in every wave)
	st<NPL>(M + (int64_t)k * S + k0, x);
}

// "wide_hom_tiles": the pilot of the matrix of a full tile of homozygous bins (symbol 0).  Under symbol 0 a step multiplies by e0 < 1,
// so that matrix is far from stochastic and an unscaled row would drift towards underflow on long tiles.  ONE work-group sweeps the
// uniform vector 1/n through T bins of symbol 0 exactly as the forward sweep steps (fstep, the power-of-two factor at every fourth
// bin computed from the vector) and stores the factors it used: fac[j] scaled bin 4 j, ceil(T / 4) of them.
template <int NPL, int W>
__global__ __launch_bounds__(64 * W) void k_wf_hompilot(const double *__restrict__ par, int n, int T, double *__restrict__ fac)
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
	double x[NPL];
#pragma unroll
	for (int i = 0; i < NPL; ++i) x[i] = k0 + i < n ? 1.0 / n : 0.0;
	for (int p = 0; p < T; ++p) { // (T, p: the same in every wave)
		if ((p & 3) == 0) {
			const double iv = fstep<NPL, W, true, false>(sc, wm, 0, e0, e1, x, 1.0, xc);
			if (tid == 0) fac[p >> 2] = iv;
		} else fstep<NPL, W, false, false>(sc, wm, 0, e0, e1, x, 1.0, xc);
	}
}

// ... and the matrix: row k of M_h is the unit vector of state k swept T bins under symbol 0 with the PILOT's factors (fstep GIVEN), one
// work-group per row as k_wf_gapmat.  Every row is multiplied by the same powers of two, which is exact: M_h is the sweep's own tile
// map, x -> e0 . (a^T x) taken T times, on one common scale -- and the chain normalises after every application, so the scale drops
// out.  No row can overflow: all entries are non-negative and e_k <= n u elementwise (u the uniform vector), so by linearity
// e_k M_h <= n (u M_h) elementwise, and u M_h is the pilot's own vector, which its factors hold at a sum below 2 at every scaled bin
// (it only shrinks in between: every step's column sums are at most max e0 <= 1).  A row underflows only where it is negligible
// against the pilot by the whole range of a double -- a state the chain's product could not see either.
template <int NPL, int W>
__global__ __launch_bounds__(64 * W) void k_wf_hommat(const double *__restrict__ par, int T, const double *__restrict__ fac, double *__restrict__ M)
{
	constexpr int S = 64 * NPL * W;
	__shared__ double xs[2 * WX_SLOTS * W];
	Xchg<W> xc = make_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid, k = blockIdx.x;
	const WaveScanMasks wm = wave_scan_masks(xc.lane);
	StructParN<NPL> sc;
	load_par<NPL, S>(par, k0, true, sc);
	double e0[NPL], e1[NPL];
	ld<NPL>(par + WP_E0 * S + k0, e0); ld<NPL>(par + WP_E1 * S + k0, e1);
	double x[NPL];
#pragma unroll
	for (int i = 0; i < NPL; ++i) x[i] = k0 + i == k ? 1.0 : 0.0;
	for (int p = 0; p < T; ++p) { // (T, p: the same in every wave)
		if ((p & 3) == 0) fstep<NPL, W, true, true>(sc, wm, 0, e0, e1, x, fac[p >> 2], xc);
		else fstep<NPL, W, false, false>(sc, wm, 0, e0, e1, x, 1.0, xc);
	}
	st<NPL>(M + (int64_t)k * S + k0, x);
}

// "wide_mix_tiles": the sequence of symbols a mix tile's matrix of direction `dir` is swept through -- the tile's own bins o[0 .. T - 1]
// forward, and backward the same shifted by one bin with the missing symbol appended (B = D_lo a D_lo+1 ... D_hi a: the first bin's
// emission is the row's start value, the last step has none).  p, dir, T and o are the same in every thread of the work-group: one read
// per bin, the same in every lane.  The sweeps below fetch the symbols of bins p .. p + 3 together at p % 4 == 0, so the four loads
// are in flight at once and off the steps' dependency chain (past the tile's end the answer is the missing symbol, and it is not used).
__device__ __forceinline__ int mix_sym(const uint8_t *__restrict__ o, int dir, int p, int T)
{
	const int q = p + dir;
	return q < T ? (int)o[q] & 3 : 2;
}

// The pilots of the matrices of the mix tiles: work-group j does job jobs[j] = 2 slot + dir -- it sweeps the uniform vector 1/n through
// the sequence of tile tiles[slot] in direction dir exactly as k_wf_hompilot does through symbol 0, and stores the ceil(T / 4)
// factors it used at fac[(2 slot + dir) nf ..].
template <int NPL, int W>
__global__ __launch_bounds__(64 * W) void k_wf_mixpilot(const double *__restrict__ par, const uint8_t *__restrict__ obs, const Chunk *__restrict__ chunks,
                                                         const int *__restrict__ tiles, const int *__restrict__ jobs, int n, int T, double *__restrict__ fac)
{
	constexpr int S = 64 * NPL * W;
	__shared__ double xs[2 * WX_SLOTS * W];
	Xchg<W> xc = make_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid, job = jobs[blockIdx.x], dir = job & 1;
	const WaveScanMasks wm = wave_scan_masks(xc.lane);
	const Chunk c = chunks[tiles[job >> 1]];
	const uint8_t *o = obs + c.off + c.lo - 1; // the tile's bins o[0 .. T - 1] (a full tile: hi - lo + 1 == T)
	fac += (int64_t)job * ((T + 3) / 4);
	StructParN<NPL> sc;
	load_par<NPL, S>(par, k0, true, sc);
	double e0[NPL], e1[NPL];
	ld<NPL>(par + WP_E0 * S + k0, e0); ld<NPL>(par + WP_E1 * S + k0, e1);
	double x[NPL];
#pragma unroll
	for (int i = 0; i < NPL; ++i) x[i] = k0 + i < n ? 1.0 / n : 0.0;
	for (int p = 0; p < T; p += 4) { // (T, p, the symbols: the same in every wave)
		int sym[4];
#pragma unroll
		for (int j = 0; j < 4; ++j) sym[j] = mix_sym(o, dir, p + j, T);
		const double iv = fstep<NPL, W, true, false>(sc, wm, sym[0], e0, e1, x, 1.0, xc);
		if (tid == 0) fac[p >> 2] = iv;
#pragma unroll
		for (int j = 1; j < 4; ++j)
			if (p + j < T) fstep<NPL, W, false, false>(sc, wm, sym[j], e0, e1, x, 1.0, xc);
	}
}

// ... and the matrices: work-group (job, k), job = 2 slot + dir as above, sweeps row k of F (dir 0: e_k through o_lo .. o_hi) or of B (dir 1: D_lo(k) e_k through
// o_lo+1 .. o_hi, N) with the factors of THAT direction's pilot (fstep GIVEN), into Mx[(2 slot + dir)][k][.].  Every row of one matrix is
// multiplied by the same powers of two, which is exact, and the chain normalises after every application, so the scale drops out.
// No row can overflow -- the argument of k_wf_hommat, word for word, because each direction's matrix is swept with its own pilot through
// its own sequence: all entries are non-negative and the start row is at most e_k (D_lo(k) <= 1), and e_k <= n u elementwise (u the
// uniform vector), so by linearity the row is at most n times the pilot's vector elementwise at every bin, and the pilot's factors hold
// its sum below 2 at every scaled bin (it only shrinks in between: every step's column sums are at most max(e0, 1) <= 1).  A row
// underflows only where it is negligible against the pilot by the whole range of a double.
template <int NPL, int W>
__global__ __launch_bounds__(64 * W) void k_wf_mixmat(const double *__restrict__ par, const uint8_t *__restrict__ obs, const Chunk *__restrict__ chunks,
                                                       const int *__restrict__ tiles, const int *__restrict__ jobs, int n, int T, const double *__restrict__ fac,
                                                       double *__restrict__ Mx)
{
	constexpr int S = 64 * NPL * W;
	__shared__ double xs[2 * WX_SLOTS * W];
	Xchg<W> xc = make_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid, k = blockIdx.y, job = jobs[blockIdx.x], dir = job & 1;
	const WaveScanMasks wm = wave_scan_masks(xc.lane);
	const Chunk c = chunks[tiles[job >> 1]];
	const uint8_t *o = obs + c.off + c.lo - 1;
	fac += (int64_t)job * ((T + 3) / 4);
	StructParN<NPL> sc;
	load_par<NPL, S>(par, k0, true, sc);
	double e0[NPL], e1[NPL];
	ld<NPL>(par + WP_E0 * S + k0, e0); ld<NPL>(par + WP_E1 * S + k0, e1);
	const bool d_lo = dir == 1 && ((int)o[0] & 3) == 0; // backward: the first bin's emission starts the row
	double x[NPL];
#pragma unroll
	for (int i = 0; i < NPL; ++i) x[i] = k0 + i == k ? (d_lo ? e0[i] : 1.0) : 0.0;
	for (int p = 0; p < T; p += 4) { // (T, p, the symbols: the same in every wave)
		int sym[4];
#pragma unroll
		for (int j = 0; j < 4; ++j) sym[j] = mix_sym(o, dir, p + j, T);
		fstep<NPL, W, true, true>(sc, wm, sym[0], e0, e1, x, fac[p >> 2], xc);
#pragma unroll
		for (int j = 1; j < 4; ++j)
			if (p + j < T) fstep<NPL, W, false, false>(sc, wm, sym[j], e0, e1, x, 1.0, xc);
	}
	st<NPL>(Mx + ((int64_t)job * n + k) * S + k0, x);
}

constexpr int WG_THREADS = 1024;

// HOM ("wide_hom_tiles", a plan whose qualifying runs hold hom tiles; false: the kernel as it was, the three last arguments unused): the
// matrix of every application is the crossed tile's own -- M_h where cls says 4, else M -- and the backward product of a hom tile is
// bt_lo = D M_h D^-1 bt_{hi+1}, D = diag(e0): the sweep's backward map is (D a)^T = D (a D)^T D^-1, and (a D)^T is what k_wf_hommat built.
// KIND: 0 the plain chain, 1 HOM, 2 MIX ("wide_mix_tiles", a plan whose qualifying runs hold mix tiles): what HOM does, and across a tile of
// class 6 the matrix is the tile's own of this direction, Mx[2 slot[tile] + BWD] (F forward, B backward), with no D scaling.
template <int S, bool BWD, int KIND = 0>
__global__ __launch_bounds__(WG_THREADS) void k_wf_gapchain(const double *__restrict__ M, int n, const Chunk *__restrict__ chunks,
                                                              const GapRun *__restrict__ runs, const double *__restrict__ X,
                                                              const double *__restrict__ xhi, const double *__restrict__ bexit,
                                                              double *__restrict__ dst, const double *__restrict__ Mh = nullptr,
                                                              const int *__restrict__ cls = nullptr, const double *__restrict__ e0 = nullptr,
                                                              const double *__restrict__ Mx = nullptr, const int *__restrict__ slot = nullptr)
{
	constexpr bool HOM = KIND >= 1;
	constexpr int KS = WG_THREADS / S; // forward: ranges of rows (5 at S = 192, 4, 2, 1, 1)
	__shared__ double v[S], y[KS * S], tot;
	const GapRun r = runs[blockIdx.x];
	const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
	const double *src;
	if (BWD) src = bexit + (int64_t)(r.first + 1) * S;
	else if (xhi) src = xhi + (int64_t)(r.first - 1) * S;
	else { const Chunk c = chunks[r.first - 1]; src = X + (c.off + c.hi - 1) * S; }
	if (t < S) {
		const double a = src[t];
		v[t] = a; y[t] = 0.0; // (backward: rows n .. S - 1 of M do not exist, those states stay 0)
		dst[(int64_t)r.first * S + t] = a;
	}
	__syncthreads();
	for (int i = 1; i <= r.count; ++i) { // (r, n: the same in every thread -- every barrier below is reached by all)
		const double *Mt = M;
		bool hom = false; // (the crossed tile's class: the same in every thread)
		if constexpr (KIND == 1) { hom = cls[BWD ? r.first - i + 1 : r.first + i - 1] == 4; if (hom) Mt = Mh; }
		if constexpr (KIND == 2) {
			const int tile = BWD ? r.first - i + 1 : r.first + i - 1, cl = cls[tile];
			hom = cl == 4;
			if (hom) Mt = Mh;
			else if (cl == 6) Mt = Mx + (int64_t)(2 * slot[tile] + (BWD ? 1 : 0)) * n * S;
		}
		if constexpr (HOM && BWD) {
			if (hom) { // D^-1 bt_{hi+1}, in place (states n .. S - 1 are 0 and stay so)
				if (t < n) v[t] = v[t] / e0[t];
				__syncthreads();
			}
		}
		if (!BWD) {
			const int g = t / S, col = t - g * S, kc = (n + KS - 1) / KS;
			if (g < KS) {
				const int k1 = min(n, (g + 1) * kc);
				double acc = 0.0;
#pragma unroll 8
				for (int k = g * kc; k < k1; ++k) acc = __builtin_fma(v[k], Mt[(int64_t)k * S + col], acc);
				y[g * S + col] = acc;
			}
			__syncthreads();
			if (KS > 1 && t < S) {
				double acc = y[t];
#pragma unroll
				for (int q = 1; q < KS; ++q) acc += y[q * S + t];
				y[t] = acc; // (only this thread reads the column's partial sums)
			}
		} else {
			for (int k = wave; k < n; k += WG_THREADS / 64) {
				const double *row = Mt + (int64_t)k * S;
				double acc = 0.0;
#pragma unroll
				for (int j = 0; j < S / 64; ++j) acc = __builtin_fma(row[lane + 64 * j], v[lane + 64 * j], acc);
				acc = wave_total(acc);
				if (lane == 0) y[k] = HOM && hom ? acc * e0[k] : acc;
			}
		}
		__syncthreads();
		if (wave == 0) { // the sum of the new vector: per lane ascending, then wave_total
			double s = 0.0;
#pragma unroll
			for (int j = 0; j < S / 64; ++j) s += y[lane + 64 * j];
			s = wave_total(s);
			if (lane == 0) tot = 1.0 / s;
		}
		__syncthreads();
		if (t < S) {
			const double a = y[t] * tot;
			v[t] = a;
			dst[(int64_t)(BWD ? r.first - i : r.first + i) * S + t] = a;
		}
		__syncthreads();
	}
}

template <int NPL, int W> static int launch_gap(const WideGap &w, int what)
{
	constexpr int S = 64 * NPL * W;
	hipStream_t st = w.stream;
	switch (what) {
	case WG_MAT:
		if (w.mats & 1) hipLaunchKernelGGL((k_wf_gapmat<NPL, W>), dim3(w.n_states), dim3(64 * W), 0, st, w.par, w.T, w.M);
		if (w.mats & 2) { // the pilot, then the rows of M_h with its factors (behind M_h in the same buffer)
			double *fac = w.Mh + (int64_t)w.n_states * S;
			hipLaunchKernelGGL((k_wf_hompilot<NPL, W>), dim3(1), dim3(64 * W), 0, st, w.par, w.n_states, w.T, fac);
			hipLaunchKernelGGL((k_wf_hommat<NPL, W>), dim3(w.n_states), dim3(64 * W), 0, st, w.par, w.T, fac, w.Mh);
		}
		if ((w.mats & 4) && w.n_jobs > 0) { // the pilots of the jobs, then the rows of their matrices (the factors behind the matrices in the same buffer)
			double *fac = w.Mx + (int64_t)2 * w.n_mix * w.n_states * S;
			hipLaunchKernelGGL((k_wf_mixpilot<NPL, W>), dim3(w.n_jobs), dim3(64 * W), 0, st, w.par, w.obs, w.chunks, w.mix_tiles, w.mix_jobs, w.n_states, w.T, fac);
			hipLaunchKernelGGL((k_wf_mixmat<NPL, W>), dim3(w.n_jobs, w.n_states), dim3(64 * W), 0, st, w.par, w.obs, w.chunks, w.mix_tiles, w.mix_jobs, w.n_states, w.T, fac, w.Mx);
		}
		break;
	case WG_CHAIN_F:
		if (w.n_runs > 0 && (w.mats & 4)) hipLaunchKernelGGL((k_wf_gapchain<S, false, 2>), dim3(w.n_runs), dim3(WG_THREADS), 0, st, w.M, w.n_states, w.chunks, w.runs, w.X, w.ckpt == WCK ? w.xhi : nullptr, w.bexit, w.entry, w.Mh, w.cls, w.par + WP_E0 * S, w.Mx, w.mix_slot);
		else if (w.n_runs > 0 && (w.mats & 2)) hipLaunchKernelGGL((k_wf_gapchain<S, false, 1>), dim3(w.n_runs), dim3(WG_THREADS), 0, st, w.M, w.n_states, w.chunks, w.runs, w.X, w.ckpt == WCK ? w.xhi : nullptr, w.bexit, w.entry, w.Mh, w.cls, w.par + WP_E0 * S);
		else if (w.n_runs > 0) hipLaunchKernelGGL((k_wf_gapchain<S, false>), dim3(w.n_runs), dim3(WG_THREADS), 0, st, w.M, w.n_states, w.chunks, w.runs, w.X, w.ckpt == WCK ? w.xhi : nullptr, w.bexit, w.entry);
		break;
	case WG_CHAIN_B:
		if (w.n_runs > 0 && (w.mats & 4)) hipLaunchKernelGGL((k_wf_gapchain<S, true, 2>), dim3(w.n_runs), dim3(WG_THREADS), 0, st, w.M, w.n_states, w.chunks, w.runs, w.X, nullptr, w.bexit, w.bentry, w.Mh, w.cls, w.par + WP_E0 * S, w.Mx, w.mix_slot);
		else if (w.n_runs > 0 && (w.mats & 2)) hipLaunchKernelGGL((k_wf_gapchain<S, true, 1>), dim3(w.n_runs), dim3(WG_THREADS), 0, st, w.M, w.n_states, w.chunks, w.runs, w.X, nullptr, w.bexit, w.bentry, w.Mh, w.cls, w.par + WP_E0 * S);
		else if (w.n_runs > 0) hipLaunchKernelGGL((k_wf_gapchain<S, true>), dim3(w.n_runs), dim3(WG_THREADS), 0, st, w.M, w.n_states, w.chunks, w.runs, w.X, nullptr, w.bexit, w.bentry);
		break;
	default: return -1;
	}
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace wide

int launch_wide_gap(const WideGap &w, int what)
{
	if (w.waves > 1 ? w.ns != 256 * w.waves : (w.ns != 192 && w.ns != 256)) return -1;
	if (w.ckpt != 1 && !(w.ckpt == wide::WCK && w.xhi)) return -1;
	if (!(w.mats & 7) || ((w.mats & 2) && !(w.Mh && w.cls))) return -1;
	if ((w.mats & 4) && !(w.Mx && w.cls && w.mix_slot && w.mix_tiles && w.mix_jobs && w.obs && w.n_mix > 0 && w.n_mix <= 65535 && w.n_jobs >= 0 && w.n_jobs <= 2 * w.n_mix)) return -1;
	switch (w.ns) {
	case 192: return wide::launch_gap<3, 1>(w, what);
	case 256: return wide::launch_gap<4, 1>(w, what);
	case 512: return wide::launch_gap<4, 2>(w, what);
	case 768: return wide::launch_gap<4, 3>(w, what);
	case 1024: return wide::launch_gap<4, 4>(w, what);
	}
	return -1;
}

} // namespace psmc
