// estep_wide_counts.hip -- the full count matrix A on the wide fast path (129..1024 states, options "wide_fast" + "wide_counts";
// api_wide_fast.hip estep_counts_wide drives it): what psmc_hip_estep of such a context returns beside E and LL.
//
// The factored wide E-step leaves the lag-normalised forward table X (every row: a wide-counts E-step keeps interval 1 -- unless
// "wide_ckpt" + "wide_counts_ckpt": then the rows at p % 8 == 0 only, see below) and every tile's backward start vector bentry = bt_{top+1}, converged to "warm_tol".  The counts are
//   A[k][l] = a[k][l] C[k][l],   C[k][l] = sum_p X_p(k) V_p(l),   V_p(l) = mult bt_{p+1}(l) / G_p,   G_p = sum_k X_p(k) (a bt_{p+1})(k)
// over the positions p = 1 .. L - 1 of every selected segment (position L owns no transition), so every transition adds exactly
// mult to the sum of A.  No S x S accumulator lives inside a sweep: the pass is cut into slabs of whole tiles in plan order, and per slab
//   k_wc_v             one more backward sweep per tile from bentry -- the backward step of the E-step (wide_prims.h bstep_parts,
//                      as k_wp_dec of estep_wide_post.hip), so the E-step's own bt -- that writes V_p for p = lo .. min(hi, L - 1)
//                      into the slab's V rows (8 S bytes per position; a tile that holds only position L writes nothing).  A
//                      tile is one work-group of W waves as in the E-step: one wave at S = 192 / 256, W = 2, 3, 4 at S = 256 W.
//   k_wc_gemm          C += X^T V on v_mfma_f64_16x16x4 (lane (t, i) supplies A[M = i][K = t] and B[K = t][N = i]; result q of the
//                      lane is D[t + 4 q][i]: estep_fused.hip).  M = N = S, a multiple of 64: one wave owns a 64 x 64 block (4 x 4
//                      instructions per four rows of K).  K is a list of row ranges (KRange: where the rows start in X and in the
//                      slab, how many -- never across a tile's end, so the alignment gaps between segments, position L and
//                      segments outside the selection are in no range); a ragged range ends in one masked step (rows past its
//                      end supply zeros and are not read).  Split-K: split s of n_split takes the ranges
//                      [n s / n_split, n (s + 1) / n_split) of the slab and owns the partial matrix P[s] -- ONE work-group per
//                      block of a partial, which reads it back (first slab: zeros) and adds slab after slab in stream order.
//                      No atomics; the order of every sum is fixed by the plan.
//   k_wc_finish        A[k][l] = a[k][l] (P[0][k][l] + P[1][k][l] + ...) + tiny_total in split order, the n x n block at row stride n
//                      (tiny_total: HMM_TINY per selected segment, what the reference's counts start from).
// The ranges, the slabs and n_split are functions of the plan and the options alone (api_wide_fast.hip plan_counts): the result
// does not depend on the device, on timing or on earlier calls.
//
// "wide_counts_ckpt" (compile-time variant CKPT of k_wc_v): after a "wide_ckpt" E-step X holds the rows at p % 8 == 0 only
// (wide_prims.h ckpt_row).  k_wc_v CKPT sweeps the tile in blocks of eight positions, the top block first, recomputing the block's
// rows forward into LDS with fstep -- the forward sweep's own step and its stored scale factors, as k_wp_dec CKPT of
// estep_wide_post.hip and k_wf_acc CKPT of estep_wide_fast.hip -- runs the same backward step, G_p and V_p store over them, and
// writes every owned row X_p into the slab-sized buffer Xs at the row of V_p.  k_wc_gemm and k_wc_finish are the same kernels: the
// GEMM gets Xs for X and ranges whose xrow is their vrow -- the same ranges in the same order and the same n_split, so every MFMA
// sees the same operands in the same order: the bits of the full-table pass.
//
// Resources (hipcc -O3, gfx950, make resources; scratch is 0 everywhere).  k_wc_v per shape (NPL, W): VGPRs | LDS bytes per
// work-group | waves per SIMD:
//   kernel                               (3,1) S=192      (4,1) S=256      (4,2) S=512      (4,3) S=768      (4,4) S=1024
//   k_wc_v                                   98     0 4      126     0 4      128   192 4      136   288 3      140   384 3
//   k_wc_v  CKPT                             96 10752 4      118 14336 3      122 28864 3      128 43296 3      130 57728 2
//   (CKPT: LDS = the exchange slots plus 7 rows of S doubles, as k_wp_dec CKPT; the non-CKPT variant is what it was before CKPT existed)
//   k_wc_gemm       162 .. 164 VGPRs (of them 128 accumulators; no AGPRs) at every width, no LDS: three waves per SIMD
//                   (amdgpu_waves_per_eu(2): without it the compiler takes 134 VGPRs + 128 AGPRs, one wave per SIMD)
//   k_wc_finish     8 VGPRs, no LDS
// Measured on an MI355X (profiles/wide_fast_timing.txt, stress fixture of 2.2 M bins): the whole pass 9 ms at 200 states, 37 ms at
// 300, 138 ms at 1024 -- 2 S^2 flop per bin (S = 256, 512, 1024) at 31 / 31 / 33 Tflop/s, beside factored E-steps of 273 / 422 / 547 ms;
// 30 M-bin genome at 200 states: 180 ms (22 Tflop/s) beside 158.  From checkpoints, same fixture: the pass 12 / 39 / 141 ms beside
// checkpointed factored E-steps of 328 / 515 / 657 ms, for 0.57 / 1.14 / 2.28 GB of X instead of 4.5 / 9.0 / 18.0 GB.
#include <hip/hip_runtime.h>
#include "wide_fast.h"
#include "wide_prims.h"

namespace psmc {
namespace wide {

typedef double d4c_t __attribute__((ext_vector_type(4)));

// Tile t0 + blockIdx.x of the plan; its V rows start at row vrow[b] of the slab (position lo first).  The tile is one work-group of
// W waves (wide_prims.h).  Two exchanges per position (the step's own, and G), reached by every wave: `top < lo`, the loop bounds
// and `p > top || p < lo` come from the tile descriptor and the loop counters.
// CKPT ("wide_counts_ckpt" after a "wide_ckpt" E-step): X holds the rows at p % 8 == 0 only.  As k_wp_dec CKPT (estep_wide_post.hip)
// and k_wf_acc CKPT (estep_wide_fast.hip) the tile is swept in blocks of the positions 8m .. 8m+7, the top block first: the block's
// rows are recomputed forward with fstep and the stored scale factors -- the forward sweep's own bits, every recomputed step's
// exchange as k_wf_fwd does it -- from the checkpoint X_{8m}, or in the tile's lowest block from entry[b] or from X_1 = a0 e[o_1],
// into LDS (7 S doubles beside the exchange slots; every thread reads back what it wrote itself, so no barrier); then the same
// backward step, G_p and V_p store run over them, highest position first, X_{8m} read from the table.  Every owned row X_p also goes
// to row vrow[b] + p - lo of the slab-sized buffer Xs -- the row of V_p -- which the GEMM reads in place of the table.
// The hang rule: the branches that enclose an exchange are `top < lo` (the tile descriptor), the bounds of the loops (top, lo, the
// block bounds q, pb, pe), `q >= lo`, `lo > 1` and `p & 3` (the loop counters) and the template flag -- the same in every wave.
template <int NPL, int W, bool CKPT>
__global__ __launch_bounds__(64 * W) void k_wc_v(const double *__restrict__ par, const uint8_t *__restrict__ obs,
                                                   const Chunk *__restrict__ chunks, int t0, const double *__restrict__ X,
                                                   const double *__restrict__ inv, const double *__restrict__ entry,
                                                   const double *__restrict__ bentry, const int32_t *__restrict__ vrow,
                                                   double *__restrict__ V, double *__restrict__ Xs)
{
	constexpr int S = 64 * NPL * W;
	__shared__ double xs[2 * WX_SLOTS * W];
	Xchg<W> xc = make_xchg<W>(xs);
	const int tid = threadIdx.x, k0 = NPL * tid, b = t0 + (int)blockIdx.x;
	const WaveScanMasks wm = wave_scan_masks(xc.lane);
	const Chunk c = chunks[b];
	const int lo = c.lo, top = min(c.hi, c.L - 1);
	if (top < lo) return; // the tile holds position L only: no transition (the same in every wave)
	StructParN<NPL> sc;
	load_par<NPL, S>(par, k0, false, sc);
	double e0[NPL], e1[NPL];
	ld<NPL>(par + WP_E0 * S + k0, e0); ld<NPL>(par + WP_E1 * S + k0, e1);
	const double mult = (double)c.mult;
	const uint8_t *o = obs + c.off;
	double *vo = V + (int64_t)vrow[b] * S + k0;
	double x[NPL];
	ld<NPL>(bentry + (int64_t)b * S + k0, x);
	if constexpr (CKPT) {
		__shared__ double rows[(WCK - 1) * S];
		double *my = rows + k0;
		double *xo = Xs + (int64_t)vrow[b] * S + k0;
		const double *io = inv + c.off;
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
				double Xc[NPL], ev[NPL], y[NPL], g[NPL], none = 0.0;
				if (p & (WCK - 1)) ld<NPL>(my + ((p & (WCK - 1)) - 1) * S, Xc); else ld<NPL>(X + ckpt_row(c.off, p) * S + k0, Xc);
				st<NPL>(xo + (int64_t)(p - lo) * S, Xc);
				const int sym = (int)o[p - 1] & 3;
				if ((p & 3) == 0) bstep_parts<NPL, W, true, false>(sc, wm, sym, e0, e1, x, y, ev, xc, none);
				else bstep_parts<NPL, W, false, false>(sc, wm, sym, e0, e1, x, y, ev, xc, none);
#pragma unroll
				for (int i = 0; i < NPL; ++i) g[i] = Xc[i] * y[i];
				const double s = mult * rcp_newton(tile_vsum<NPL, W>(xc, g)); // exchanged values only: the same bits in every wave
#pragma unroll
				for (int i = 0; i < NPL; ++i) { g[i] = x[i] * s; x[i] = y[i] * ev[i]; }
				st<NPL>(vo + (int64_t)(p - lo) * S, g);
			}
		}
	} else {
		const double *fo = X + c.off * S + k0;
		double Xc[NPL], Xn[NPL];
		ld<NPL>(fo + (int64_t)(top - 1) * S, Xc);
		for (int g4 = (top - 1) >> 2; g4 >= 0 && 4 * g4 + 4 >= lo; --g4) {
			const unsigned w = *reinterpret_cast<const unsigned *>(o + 4 * (int64_t)g4);
#pragma unroll
			for (int j = 3; j >= 0; --j) {
				const int p = 4 * g4 + j + 1;
				if (p > top || p < lo) continue; // (the same in every wave)
				if (p > lo) ld<NPL>(fo + (int64_t)(p - 2) * S, Xn); // X_{p-1}, for the next step
				double ev[NPL], y[NPL], g[NPL], none = 0.0;
				// y = a bt_{p+1}; p % 4 == 0: the backward sweep's own scaling 1 / sum(bt_{p+1}) in ev
				const int sym = (int)((w >> (8 * j)) & 3u);
				if (j == 3) bstep_parts<NPL, W, true, false>(sc, wm, sym, e0, e1, x, y, ev, xc, none);
				else bstep_parts<NPL, W, false, false>(sc, wm, sym, e0, e1, x, y, ev, xc, none);
#pragma unroll
				for (int i = 0; i < NPL; ++i) g[i] = Xc[i] * y[i];
				const double s = mult * rcp_newton(tile_vsum<NPL, W>(xc, g)); // exchanged values only: the same bits in every wave
#pragma unroll
				for (int i = 0; i < NPL; ++i) { g[i] = x[i] * s; x[i] = y[i] * ev[i]; }
				st<NPL>(vo + (int64_t)(p - lo) * S, g);
#pragma unroll
				for (int i = 0; i < NPL; ++i) Xc[i] = Xn[i];
			}
		}
	}
}

// blockIdx.x: the 64 x 64 block (mb, nb) of C, blockIdx.y: the split.  One wave.
template <int S>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_wc_gemm(const double *__restrict__ X, const double *__restrict__ V,
                                                  const KRange *__restrict__ kr, int n_kr, int n_split, int first, double *__restrict__ P)
{
	constexpr int NB = S / 64;
	const int lane = threadIdx.x, t = lane >> 4, i = lane & 15;
	const int mb = (int)blockIdx.x / NB, nb = (int)blockIdx.x % NB, s = (int)blockIdx.y;
	const int r0 = (int)((int64_t)n_kr * s / n_split), r1 = (int)((int64_t)n_kr * (s + 1) / n_split);
	double *Pb = P + ((int64_t)s * S + 64 * mb + t) * S + 64 * nb + i; // result q of block (m, n): Pb[(16 m + 4 q) S + 16 n]
	d4c_t acc[4][4];
#pragma unroll
	for (int m = 0; m < 4; ++m)
#pragma unroll
		for (int n = 0; n < 4; ++n)
#pragma unroll
			for (int q = 0; q < 4; ++q) acc[m][n][q] = first ? 0.0 : Pb[(int64_t)(16 * m + 4 * q) * S + 16 * n];
	for (int r = r0; r < r1; ++r) {
		const KRange k = kr[r];
		const double *xa = X + (k.xrow + t) * S + 64 * mb + i;     // row t of the step, columns i, i + 16, i + 32, i + 48 of the block
		const double *vb = V + ((int64_t)k.vrow + t) * S + 64 * nb + i;
		int kk = 0;
		for (; kk + 4 <= k.rows; kk += 4) {
			double a[4], bb[4];
#pragma unroll
			for (int m = 0; m < 4; ++m) { a[m] = xa[(int64_t)kk * S + 16 * m]; bb[m] = vb[(int64_t)kk * S + 16 * m]; }
#pragma unroll
			for (int m = 0; m < 4; ++m)
#pragma unroll
				for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], bb[n], acc[m][n], 0, 0, 0);
		}
		if (kk < k.rows) { // the ragged end: rows past it are not read and supply zeros
			const bool ok = kk + t < k.rows;
			double a[4], bb[4];
#pragma unroll
			for (int m = 0; m < 4; ++m) {
				a[m] = ok ? xa[(int64_t)kk * S + 16 * m] : 0.0;
				bb[m] = ok ? vb[(int64_t)kk * S + 16 * m] : 0.0;
			}
#pragma unroll
			for (int m = 0; m < 4; ++m)
#pragma unroll
				for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], bb[n], acc[m][n], 0, 0, 0);
		}
	}
#pragma unroll
	for (int m = 0; m < 4; ++m)
#pragma unroll
		for (int n = 0; n < 4; ++n)
#pragma unroll
			for (int q = 0; q < 4; ++q) Pb[(int64_t)(16 * m + 4 * q) * S + 16 * n] = acc[m][n][q];
}

template <int S>
__global__ __launch_bounds__(256) void k_wc_finish(const double *__restrict__ P, int n_split, const double *__restrict__ a, double tiny_total,
                                                     int n, double *__restrict__ out)
{
	const int idx = blockIdx.x * 256 + threadIdx.x;
	if (idx >= n * n) return;
	const int k = idx / n, l = idx % n;
	double t = 0.0;
	for (int s = 0; s < n_split; ++s) t += P[((int64_t)s * S + k) * S + l];
	out[idx] = a[idx] * t + tiny_total; // (hmm_expect starts every segment's counts at HMM_TINY, khmm.c: as k_reduce2 of estep_fast.hip)
}

template <int S> static int launch_counts(const WideCounts &w, int what)
{
	constexpr int WV = S <= 256 ? 1 : S / 256; // waves per tile of k_wc_v
	hipStream_t st = w.stream;
	switch (what) {
	case WC_V:
		if (w.ckpt == WCK)
			hipLaunchKernelGGL((k_wc_v<S / (64 * WV), WV, true>), dim3(w.n_tiles), dim3(64 * WV), 0, st, w.par, w.obs, w.chunks, w.t0, w.X, w.inv, w.entry, w.bentry, w.vrow, w.V, w.Xs);
		else
			hipLaunchKernelGGL((k_wc_v<S / (64 * WV), WV, false>), dim3(w.n_tiles), dim3(64 * WV), 0, st, w.par, w.obs, w.chunks, w.t0, w.X, w.inv, w.entry, w.bentry, w.vrow, w.V, w.Xs);
		break;
	case WC_GEMM: // ckpt == 8: the X rows of the slab, which k_wc_v wrote (the ranges' xrow are rows of Xs then)
		hipLaunchKernelGGL(k_wc_gemm<S>, dim3((S / 64) * (S / 64), w.n_split), dim3(64), 0, st, w.ckpt == WCK ? w.Xs : w.X, w.V, w.kr, w.n_kr, w.n_split, w.first, w.P);
		break;
	case WC_FINISH:
		hipLaunchKernelGGL(k_wc_finish<S>, dim3((w.n_states * w.n_states + 255) / 256), dim3(256), 0, st, w.P, w.n_split, w.a, w.tiny_total, w.n_states, w.out);
		break;
	default: return -1;
	}
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace wide

int launch_wide_counts(const WideCounts &w, int what)
{
	if (w.waves > 1 ? w.ns != 256 * w.waves : (w.ns != 192 && w.ns != 256)) return -1;
	if (w.ckpt != 1 && !(w.ckpt == wide::WCK && w.inv && w.entry && w.Xs)) return -1;
	switch (w.ns) {
	case 192: return wide::launch_counts<192>(w, what);
	case 256: return wide::launch_counts<256>(w, what);
	case 512: return wide::launch_counts<512>(w, what);
	case 768: return wide::launch_counts<768>(w, what);
	case 1024: return wide::launch_counts<1024>(w, what);
	}
	return -1;
}

} // namespace psmc
