// estep_wide_counts.hip -- the full count matrix A on the wide fast path (129..1024 states, options "wide_fast" + "wide_counts";
// api_wide_fast.hip estep_counts_wide drives it): what psmc_hip_estep of such a context returns beside E and LL.
//
// The factored wide E-step leaves the lag-normalised forward table X (every row: a wide-counts E-step keeps interval 1) and every
// tile's backward start vector bentry = bt_{top+1}, converged to "warm_tol".  The counts are
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
// Resources (hipcc -O3, gfx950, make resources; scratch is 0 everywhere).  k_wc_v per shape (NPL, W): VGPRs | LDS bytes per
// work-group | waves per SIMD:
//   kernel                               (3,1) S=192      (4,1) S=256      (4,2) S=512      (4,3) S=768      (4,4) S=1024
//   k_wc_v                                   98     0 4      126     0 4      128   192 4      136   288 3      140   384 3
//   k_wc_gemm       162 .. 164 VGPRs (of them 128 accumulators; no AGPRs) at every width, no LDS: three waves per SIMD
//                   (amdgpu_waves_per_eu(2): without it the compiler takes 134 VGPRs + 128 AGPRs, one wave per SIMD)
//   k_wc_finish     8 VGPRs, no LDS
// Measured on an MI355X (profiles/wide_fast_timing.txt, stress fixture of 2.2 M bins): the whole pass 9 ms at 200 states, 37 ms at
// 300, 138 ms at 1024 -- 2 S^2 flop per bin (S = 256, 512, 1024) at 31 / 31 / 33 Tflop/s, beside factored E-steps of 273 / 422 / 547 ms;
// 30 M-bin genome at 200 states: 180 ms (22 Tflop/s) beside 158.
#include <hip/hip_runtime.h>
#include "wide_fast.h"
#include "wide_prims.h"

namespace psmc {
namespace wide {

typedef double d4c_t __attribute__((ext_vector_type(4)));

// Tile t0 + blockIdx.x of the plan; its V rows start at row vrow[b] of the slab (position lo first).  The tile is one work-group of
// W waves (wide_prims.h).  Two exchanges per position (the step's own, and G), reached by every wave: `top < lo`, the loop bounds
// and `p > top || p < lo` come from the tile descriptor and the loop counters.
template <int NPL, int W>
__global__ __launch_bounds__(64 * W) void k_wc_v(const double *__restrict__ par, const uint8_t *__restrict__ obs,
                                                   const Chunk *__restrict__ chunks, int t0, const double *__restrict__ X,
                                                   const double *__restrict__ bentry, const int32_t *__restrict__ vrow,
                                                   double *__restrict__ V)
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
	const double *fo = X + c.off * S + k0;
	double *vo = V + (int64_t)vrow[b] * S + k0;
	double x[NPL], Xc[NPL], Xn[NPL];
	ld<NPL>(bentry + (int64_t)b * S + k0, x);
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
		hipLaunchKernelGGL((k_wc_v<S / (64 * WV), WV>), dim3(w.n_tiles), dim3(64 * WV), 0, st, w.par, w.obs, w.chunks, w.t0, w.X, w.bentry, w.vrow, w.V);
		break;
	case WC_GEMM:
		hipLaunchKernelGGL(k_wc_gemm<S>, dim3((S / 64) * (S / 64), w.n_split), dim3(64), 0, st, w.X, w.V, w.kr, w.n_kr, w.n_split, w.first, w.P);
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
