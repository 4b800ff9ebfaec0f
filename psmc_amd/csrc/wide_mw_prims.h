// wide_mw_prims.h -- what the multi-wave kernels of the wide fast path share (estep_wide_fast_mw.hip: the E-step at 257..1024
// states; estep_wide_post_mw.hip: decoding from its tables): a tile is ONE work-group of W = 2, 3 or 4 waves at the padded width
// S = 256 W, thread t holds the states 4t .. 4t+3 (the layout of wide_prims.h continued over the work-group).  Here: the exchange
// of wave-uniform values between the waves of a tile through LDS (Xchg), sums over the tile, the O(N) step x <- M x over the tile
// and the backward step with its scaling at p % 4 == 0.  The rules of the exchange (one barrier per exchange, every wave goes
// through the same sequence of exchanges) are stated at the top of estep_wide_fast_mw.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "wave_prims.h"
#include "struct_prims.h"
#include "psmc_hip_internal.h"
#include "wide_prims.h"

namespace psmc {
namespace wide {

constexpr int MW_NPL = 4;   // states per lane
constexpr int MW_SLOTS = 6; // values one wave publishes per exchange, at most

// The exchange between the W waves of a tile.  put(): lane 0 publishes a wave-uniform value; sync(): the one barrier; above() /
// below() / sum() / vmax(): the other waves' values in a fixed order (the same bits in every wave); next(): the other buffer.
// Every wave of the work-group must go through the same sequence of exchanges.
template <int W> struct Xchg {
	double *lds;
	int wave, lane;
	unsigned t;
	__device__ __forceinline__ double *buf() const { return lds + (t & 1u) * (MW_SLOTS * W); }
	__device__ __forceinline__ void put(int s, double v) const { if (lane == 0) buf()[s * W + wave] = v; }
	__device__ __forceinline__ void sync() const { __syncthreads(); }
	__device__ __forceinline__ void next() { ++t; }
	__device__ __forceinline__ double get(int s, int w) const { return buf()[s * W + w]; }
	__device__ __forceinline__ double above(int s) const { // waves w' > wave, lowest first
		double r = 0.0;
#pragma unroll
		for (int w = 1; w < W; ++w) r += w > wave ? get(s, w) : 0.0;
		return r;
	}
	__device__ __forceinline__ double below(int s) const { // waves w' < wave, lowest first
		double r = 0.0;
#pragma unroll
		for (int w = 0; w < W - 1; ++w) r += w < wave ? get(s, w) : 0.0;
		return r;
	}
	__device__ __forceinline__ double sum(int s) const {
		double r = get(s, 0);
#pragma unroll
		for (int w = 1; w < W; ++w) r += get(s, w);
		return r;
	}
	__device__ __forceinline__ double vmax(int s) const {
		double r = get(s, 0);
#pragma unroll
		for (int w = 1; w < W; ++w) r = fmax(r, get(s, w));
		return r;
	}
};
template <int W> __device__ __forceinline__ Xchg<W> mw_xchg(double *lds) {
	Xchg<W> xc;
	xc.lds = lds; xc.lane = threadIdx.x & 63; xc.wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); xc.t = 0u;
	return xc;
}
// sum over the tile of a per-wave value (wave-uniform on entry), the same bits in every wave
template <int W> __device__ __forceinline__ double mw_total(Xchg<W> &xc, double wave_value) {
	xc.put(0, wave_value);
	xc.sync();
	const double r = xc.sum(0);
	xc.next();
	return r;
}
template <int W> __device__ __forceinline__ double mw_vsum(Xchg<W> &xc, const double (&x)[MW_NPL]) { return mw_total<W>(xc, wave_total(lsum<MW_NPL>(x))); }

// x <- M x over the tile (wstep of wide_prims.h plus the exchange); NORM: returns the sum of x over the tile BEFORE the step
template <int W, bool NORM>
__device__ __forceinline__ double mw_step(const StructParN<MW_NPL> &c, double (&x)[MW_NPL], const WaveScanMasks &wm, Xchg<W> &xc)
{
	constexpr int NPL = MW_NPL;
	double su[NPL], pv[NPL];
	su[NPL - 1] = x[NPL - 1] * c.mS[NPL - 1];
#pragma unroll
	for (int i = NPL - 2; i >= 0; --i) su[i] = __builtin_fma(x[i], c.mS[i], su[i + 1]);
	pv[0] = x[0] * c.mP[0];
#pragma unroll
	for (int i = 1; i < NPL; ++i) pv[i] = __builtin_fma(x[i], c.mP[i], pv[i - 1]);
	double ES = wave_excl_suffix(su[0], wm), EP = wave_excl_prefix(pv[NPL - 1]);
	xc.put(0, readlane_f64(ES + su[0], 0));        // the wave's whole suffix sum: lane 0's inclusive one
	xc.put(1, readlane_f64(EP + pv[NPL - 1], 63)); // the wave's whole prefix sum: lane 63's inclusive one
	if (NORM) xc.put(2, wave_total(lsum<NPL>(x)));
	double t[NPL];
#pragma unroll
	for (int i = 0; i < NPL; ++i) t[i] = __builtin_fma(c.wS[i], su[i], __builtin_fma(c.wP[i], pv[i], c.dd[i] * x[i]));
	xc.sync();
	ES += xc.above(0); EP += xc.below(1);
	const double tot = NORM ? xc.sum(2) : 0.0;
	xc.next();
#pragma unroll
	for (int i = 0; i < NPL; ++i) x[i] = __builtin_fma(c.wS[i], ES, __builtin_fma(c.wP[i], EP, t[i]));
	return tot;
}
// one forward position over the tile (fstep of wide_prims.h with mw_step): x = X_{p-1} -> X_p, scaled at p % 4 == 0 (NORM) by
// 1/d_p -- GIVEN: the factor the forward sweep stored, else computed from x.  Returns the factor.  One exchange either way.
template <int W, bool NORM, bool GIVEN>
__device__ __forceinline__ double mw_fstep(const StructParN<MW_NPL> &sc, const WaveScanMasks &wm, int sym, const double (&e0)[MW_NPL],
                                           const double (&e1)[MW_NPL], double (&x)[MW_NPL], double given, Xchg<W> &xc)
{
	double ev[MW_NPL];
	emis<MW_NPL>(sym, e0, e1, ev);
	double iv = 1.0;
	if (NORM && !GIVEN) iv = pow2_rcp(mw_step<W, true>(sc, x, wm, xc));
	else { mw_step<W, false>(sc, x, wm, xc); if (NORM) iv = given; }
	if (NORM) {
#pragma unroll
		for (int i = 0; i < MW_NPL; ++i) ev[i] *= iv;
	}
#pragma unroll
	for (int i = 0; i < MW_NPL; ++i) x[i] *= ev[i];
	return iv;
}
// one backward step at position p: x = bt_{p+1} -> bt_p (own scaling at p % 4 == 0: 1/sum(bt_{p+1}))
template <int W, bool NORM>
__device__ __forceinline__ void mw_bstep(const StructParN<MW_NPL> &sc, const WaveScanMasks &wm, int sym, const double (&e0)[MW_NPL],
                                         const double (&e1)[MW_NPL], double (&x)[MW_NPL], Xchg<W> &xc)
{
	double ev[MW_NPL];
	emis<MW_NPL>(sym, e0, e1, ev);
	const double tot = mw_step<W, NORM>(sc, x, wm, xc);
	if (NORM) {
		const double sb = rcp_newton(tot);
#pragma unroll
		for (int i = 0; i < MW_NPL; ++i) ev[i] *= sb;
	}
#pragma unroll
	for (int i = 0; i < MW_NPL; ++i) x[i] *= ev[i];
}

// the per-lane constants of the backward direction at the tile's width: mS = c, wS = R, mP = qa, wP = P (wide_prims.h load_par)
template <int S> __device__ __forceinline__ void mw_load_bwd(const double *__restrict__ par, int k0, StructParN<MW_NPL> &sc) {
	const double *sp = par + WP_SP * S + k0;
	ld<MW_NPL>(sp + 3 * S, sc.mS); ld<MW_NPL>(sp + S, sc.wS); ld<MW_NPL>(sp + 2 * S, sc.mP); ld<MW_NPL>(sp, sc.wP); ld<MW_NPL>(sp + 4 * S, sc.dd);
}

} // namespace wide
} // namespace psmc
