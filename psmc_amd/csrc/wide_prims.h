// wide_prims.h -- what the kernels of the wide fast path share (estep_wide_fast.hip: the E-step; estep_wide_post.hip: decoding
// from its tables; estep_wide_counts.hip: the V rows of the count matrix; estep_wide_gap.hip: the rows of the transfer matrix of a tile
// of missing data).  A tile is ONE work-group of W waves at the padded width
// S = 64 NPL W: (NPL, W) = (3, 1), (4, 1) at 192 / 256 states, (4, 2), (4, 3), (4, 4) at 512 / 768 / 1024.  Thread t holds the NPL
// adjacent states k = NPL t + i, so wave w holds [64 NPL w, 64 NPL (w + 1)).  Here: the whole-wave scans, the exchange of
// wave-uniform values between the waves of a tile (Xchg), what crosses the tile through it (sum, mismatch), the parameter block,
// the O(N) step x <- M x and the forward and backward steps with their scaling at p % 4 == 0.
//
// THE EXCHANGE (W > 1).  Every wave does its in-wave scans, then the waves exchange one small record through LDS: lane 0 of each
// wave publishes wave-uniform values (put), ONE barrier (sync), and every wave reads the others' values in a fixed order, lowest
// wave first (above / below / sum / vmax / get), so every wave holds the same bits and the path is bit-reproducible from call to
// call.  The slots are double-buffered on the parity of an exchange counter that every wave advances alike (next), so one barrier
// per exchange is enough: a wave cannot reach the write of exchange t+2 before every wave has passed the barrier of exchange t+1,
// and that barrier comes after every wave's reads of exchange t.
// THE HANG RULE.  Every wave of a work-group must go through the same sequence of exchanges: every branch that encloses an
// exchange depends only on values that are the same in all waves of the work-group -- template flags, the tile descriptors and
// verify flags (global memory nobody writes during the launch), loop bounds and counters derived from them, and values that came
// out of an exchange (the mismatch of a chain's next boundary), never one wave's share.  Branches on the thread index, on
// `k0 + i < n` or on `p <= min_l` enclose stores only.
// ONE WAVE (W == 1) is the case of an exchange that does nothing: Xchg<1> keeps what is put in registers, has no LDS and no
// barrier, and has no above() / below() -- adding their 0.0 would turn a -0.0 into +0.0, so the steps skip the addition.
#pragma once
#include <hip/hip_runtime.h>
#include "wave_prims.h"
#include "struct_prims.h"
#include "psmc_hip_internal.h"

namespace psmc {
namespace wide {

// parameter block of the wide fast path, S doubles each: e0 | e1 | a0 | P | R | qa | c | dd
constexpr int WP_E0 = 0, WP_E1 = 1, WP_A0 = 2, WP_SP = 3;
constexpr int WACC = 7;     // the factored sums of the accumulate sweep: SL SU DG CL CU E0 E1
constexpr int WX_SLOTS = 6; // values one wave publishes per exchange, at most

// sums over lanes m' < m / m' > m of the whole wave (0 in lane 0 / 63): shift by one lane, then the inclusive scans
__device__ __forceinline__ double wave_excl_prefix(double t) { return wave_prefix_incl_bc(dpp_z<0x138>(t)); } // wave_shr:1
__device__ __forceinline__ double wave_excl_suffix(double t, const WaveScanMasks &m) { return wave_suffix_incl(dpp_z<0x130>(t), m); } // wave_shl:1
// sum over the wave, the same bits in every lane (row sums, then the four rows in a fixed order)
__device__ __forceinline__ double wave_total(double t) {
	t = row_sum16(t);
	return (readlane_f64(t, 0) + readlane_f64(t, 16)) + (readlane_f64(t, 32) + readlane_f64(t, 48));
}
__device__ __forceinline__ double wave_maxv(double v) {
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
	return v;
}
template <int NPL> __device__ __forceinline__ double lsum(const double (&x)[NPL]) {
	double t = x[0];
#pragma unroll
	for (int i = 1; i < NPL; ++i) t += x[i];
	return t;
}
template <int NPL> __device__ __forceinline__ void ld(const double *p, double (&v)[NPL]) {
#pragma unroll
	for (int i = 0; i < NPL; ++i) v[i] = p[i];
}
template <int NPL> __device__ __forceinline__ void st(double *p, const double (&v)[NPL]) {
#pragma unroll
	for (int i = 0; i < NPL; ++i) p[i] = v[i];
}

// The exchange between the W waves of a tile (the rules: top of this file).
template <int W> struct Xchg {
	double *lds; // [2][WX_SLOTS][W]
	int wave, lane;
	unsigned t;
	__device__ __forceinline__ double *buf() const { return lds + (t & 1u) * (WX_SLOTS * W); }
	__device__ __forceinline__ void put(int s, double v) { if (lane == 0) buf()[s * W + wave] = v; }
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
template <> struct Xchg<1> {
	double v[WX_SLOTS];
	int lane;
	__device__ __forceinline__ void put(int s, double x) { v[s] = x; }
	__device__ __forceinline__ void sync() const {}
	__device__ __forceinline__ void next() {}
	__device__ __forceinline__ double get(int s, int) const { return v[s]; }
	__device__ __forceinline__ double sum(int s) const { return v[s]; }
	__device__ __forceinline__ double vmax(int s) const { return v[s]; }
};
// the exchange of this work-group over the kernel's slots, __shared__ double [2 * WX_SLOTS * W] (W == 1: unused, so not allocated)
template <int W> __device__ __forceinline__ Xchg<W> make_xchg(double *lds) {
	Xchg<W> xc;
	if constexpr (W > 1) { xc.lds = lds; xc.wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); xc.t = 0u; xc.lane = threadIdx.x & 63; }
	else xc.lane = threadIdx.x;
	return xc;
}

// sum over the tile of a per-wave value (wave-uniform on entry), the same bits in every wave.  One exchange.
template <int W> __device__ __forceinline__ double tile_total(Xchg<W> &xc, double wave_value) {
	xc.put(0, wave_value);
	xc.sync();
	const double r = xc.sum(0);
	xc.next();
	return r;
}
template <int NPL, int W> __device__ __forceinline__ double tile_vsum(Xchg<W> &xc, const double (&x)[NPL]) { return tile_total<W>(xc, wave_total(lsum<NPL>(x))); }

// Knuth's two-sum: s + err = a + b exactly
__device__ __forceinline__ void two_sum(double a, double b, double &s, double &err) {
	s = a + b;
	const double bb = s - a;
	err = (a - (s - bb)) + (b - bb);
}
// sum over the tile of NPL values per thread, carried as an unevaluated pair (two-sum at every addition, the error terms added up
// beside; across waves lowest wave first): the rounded result is the exact sum's nearest double but for ties, the same bits in
// every thread.  One exchange.
template <int NPL, int W> __device__ __forceinline__ double tile_total_comp(Xchg<W> &xc, const double (&x)[NPL]) {
	double h = x[0], l = 0.0, t;
#pragma unroll
	for (int i = 1; i < NPL; ++i) { two_sum(h, x[i], h, t); l += t; }
#pragma unroll
	for (int m = 1; m <= 32; m <<= 1) {
		const double oh = __shfl_xor(h, m, 64), ol = __shfl_xor(l, m, 64);
		two_sum(h, oh, h, t);
		l = (l + ol) + t;
	}
	xc.put(0, h); xc.put(1, l);
	xc.sync();
	h = xc.get(0, 0); l = xc.get(1, 0);
#pragma unroll
	for (int w = 1; w < W; ++w) { two_sum(h, xc.get(0, w), h, t); l = (l + xc.get(1, w)) + t; }
	xc.next();
	return h + l;
}
// max_k |u/|u| - v/|v|| / max_k v/|v| over the tile (u: the vector a tile built on, v: what its neighbour computed); NaN anywhere:
// +inf.  Two exchanges; from exchanged values only, so the same decision in every wave.
template <int NPL, int W> __device__ __forceinline__ double tile_mismatch(const double (&u)[NPL], const double (&v)[NPL], Xchg<W> &xc)
{
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

// the five vectors in the roles load_struct_par (estep_struct.hip) gives them: forward mS = P, wS = qa, mP = R, wP = c;
// backward mS = c, wS = R, mP = qa, wP = P
template <int NPL, int S> __device__ __forceinline__ void load_par(const double *__restrict__ par, int k0, bool fwd, StructParN<NPL> &c) {
	const double *sp = par + WP_SP * S + k0; // P | R | qa | c | dd
	ld<NPL>(sp + (fwd ? 0 : 3 * S), c.mS); ld<NPL>(sp + (fwd ? 2 * S : S), c.wS);
	ld<NPL>(sp + (fwd ? S : 2 * S), c.mP); ld<NPL>(sp + (fwd ? 3 * S : 0), c.wP); ld<NPL>(sp + 4 * S, c.dd);
}
// the forward roles of the five vectors, from a backward set (load_par: the same vectors in other roles)
template <int NPL> __device__ __forceinline__ void fwd_roles(const StructParN<NPL> &b, StructParN<NPL> &f) {
#pragma unroll
	for (int i = 0; i < NPL; ++i) { f.mS[i] = b.wP[i]; f.wS[i] = b.mP[i]; f.mP[i] = b.wS[i]; f.wP[i] = b.mS[i]; f.dd[i] = b.dd[i]; }
}
template <int NPL> __device__ __forceinline__ void emis(int sym, const double (&e0)[NPL], const double (&e1)[NPL], double (&ev)[NPL]) {
#pragma unroll
	for (int i = 0; i < NPL; ++i) ev[i] = sym == 0 ? e0[i] : (sym == 1 ? e1[i] : 1.0);
}
// x <- M x over the tile: wS.SUF(x.mS) + wP.PRE(x.mP) + dd.x (inclusive scans over the S states).  One exchange: the wave totals
// of the two scans; NORM: also the sum of x over the tile BEFORE the step, which is returned; RIDE: also `ride`, a wave's share on
// entry and the tile's sum on exit (it must not depend on the step's result).
template <int NPL, int W, bool NORM, bool RIDE>
__device__ __forceinline__ double step_ride(const StructParN<NPL> &c, double (&x)[NPL], const WaveScanMasks &wm, Xchg<W> &xc, double &ride)
{
	double su[NPL], pv[NPL];
	su[NPL - 1] = x[NPL - 1] * c.mS[NPL - 1];
#pragma unroll
	for (int i = NPL - 2; i >= 0; --i) su[i] = __builtin_fma(x[i], c.mS[i], su[i + 1]);
	pv[0] = x[0] * c.mP[0];
#pragma unroll
	for (int i = 1; i < NPL; ++i) pv[i] = __builtin_fma(x[i], c.mP[i], pv[i - 1]);
	double ES = wave_excl_suffix(su[0], wm), EP = wave_excl_prefix(pv[NPL - 1]);
	if (RIDE) xc.put(3, ride);
	if constexpr (W > 1) {
		xc.put(0, readlane_f64(ES + su[0], 0));        // the wave's whole suffix sum: lane 0's inclusive one
		xc.put(1, readlane_f64(EP + pv[NPL - 1], 63)); // the wave's whole prefix sum: lane 63's inclusive one
	}
	if (NORM) xc.put(2, wave_total(lsum<NPL>(x)));
	double t[NPL]; // the part of the result that needs no other wave: before the barrier (one wave: in the last loop, the order that keeps the one-wave sweeps' code)
	if constexpr (W > 1) {
#pragma unroll
		for (int i = 0; i < NPL; ++i) t[i] = __builtin_fma(c.wS[i], su[i], __builtin_fma(c.wP[i], pv[i], c.dd[i] * x[i]));
	}
	xc.sync();
	if constexpr (W > 1) { ES += xc.above(0); EP += xc.below(1); }
	const double tot = NORM ? xc.sum(2) : 0.0;
	if (RIDE) ride = xc.sum(3);
	xc.next();
#pragma unroll
	for (int i = 0; i < NPL; ++i) {
		if constexpr (W == 1) t[i] = __builtin_fma(c.wS[i], su[i], __builtin_fma(c.wP[i], pv[i], c.dd[i] * x[i]));
		x[i] = __builtin_fma(c.wS[i], ES, __builtin_fma(c.wP[i], EP, t[i]));
	}
	return tot;
}
template <int NPL, int W, bool NORM>
__device__ __forceinline__ double step(const StructParN<NPL> &c, double (&x)[NPL], const WaveScanMasks &wm, Xchg<W> &xc)
{
	double none = 0.0;
	return step_ride<NPL, W, NORM, false>(c, x, wm, xc, none);
}
// The scaled steps below take the sum they scale by from the step's own exchange.  One wave has no exchange to save, and there the
// factor is computed BEFORE the matrix step: the same bits, and the order that holds the registers of the one-wave sweeps.
//
// one forward position p: x = X_{p-1} -> X_p = e[o_p] . (M x), scaled at p % 4 == 0 (NORM) by 1/d_p, a power of two (struct_prims.h
// pow2_rcp) -- GIVEN: the factor the forward sweep stored (`given`), else computed from x.  Returns the factor.  One exchange.  The
// forward sweep and the recomputation from checkpoints (accumulate sweep, decoding) both step through here: the same arithmetic,
// so the same bits.
template <int NPL, int W, bool NORM, bool GIVEN>
__device__ __forceinline__ double fstep(const StructParN<NPL> &c, const WaveScanMasks &wm, int sym, const double (&e0)[NPL],
                                        const double (&e1)[NPL], double (&x)[NPL], double given, Xchg<W> &xc)
{
	double ev[NPL];
	emis<NPL>(sym, e0, e1, ev);
	double iv = NORM && GIVEN ? given : 1.0;
	if constexpr (W == 1) {
		if (NORM && !GIVEN) iv = pow2_rcp(wave_total(lsum<NPL>(x)));
		if (NORM) {
#pragma unroll
			for (int i = 0; i < NPL; ++i) ev[i] *= iv;
		}
		step<NPL, W, false>(c, x, wm, xc);
	} else {
		if (NORM && !GIVEN) iv = pow2_rcp(step<NPL, W, true>(c, x, wm, xc));
		else step<NPL, W, false>(c, x, wm, xc);
		if (NORM) {
#pragma unroll
			for (int i = 0; i < NPL; ++i) ev[i] *= iv;
		}
	}
#pragma unroll
	for (int i = 0; i < NPL; ++i) x[i] *= ev[i];
	return iv;
}
// one backward step at position p in its parts: from x = bt_{p+1}, y = a bt_{p+1} and ev = e[o_p] with the sweep's own scaling
// at p % 4 == 0 (NORM: 1/sum(bt_{p+1})), so that bt_p = y . ev; the sweeps that decode read y.  One exchange; RIDE: as step_ride.
template <int NPL, int W, bool NORM, bool RIDE>
__device__ __forceinline__ void bstep_parts(const StructParN<NPL> &sc, const WaveScanMasks &wm, int sym, const double (&e0)[NPL],
                                            const double (&e1)[NPL], const double (&x)[NPL], double (&y)[NPL], double (&ev)[NPL],
                                            Xchg<W> &xc, double &ride)
{
	emis<NPL>(sym, e0, e1, ev);
#pragma unroll
	for (int i = 0; i < NPL; ++i) y[i] = x[i];
	if constexpr (W == 1) {
		if (NORM) {
			const double sb = rcp_newton(wave_total(lsum<NPL>(x)));
#pragma unroll
			for (int i = 0; i < NPL; ++i) ev[i] *= sb;
		}
		step_ride<NPL, W, false, RIDE>(sc, y, wm, xc, ride);
	} else {
		const double tot = step_ride<NPL, W, NORM, RIDE>(sc, y, wm, xc, ride);
		if (NORM) {
			const double sb = rcp_newton(tot);
#pragma unroll
			for (int i = 0; i < NPL; ++i) ev[i] *= sb;
		}
	}
}
// ... and whole: x = bt_{p+1} -> bt_p
template <int NPL, int W, bool NORM>
__device__ __forceinline__ void bstep(const StructParN<NPL> &sc, const WaveScanMasks &wm, int sym, const double (&e0)[NPL],
                                      const double (&e1)[NPL], double (&x)[NPL], Xchg<W> &xc)
{
	double y[NPL], ev[NPL], none = 0.0;
	bstep_parts<NPL, W, NORM, false>(sc, wm, sym, e0, e1, x, y, ev, xc, none);
#pragma unroll
	for (int i = 0; i < NPL; ++i) x[i] = y[i] * ev[i];
}

// the checkpointed X table ("wide_ckpt"): one row per position p with p % 8 == 0.  Segments start at off % 64 == 0, so the rows of
// all segments lie in one table by absolute position: the row of position p of the segment at `off`
constexpr int WCK = 8;
__device__ __forceinline__ int64_t ckpt_row(int64_t off, int p) { return (off >> 3) + (p >> 3) - 1; }
__device__ __forceinline__ bool same_seg(const Chunk *__restrict__ ch, int a, int b) { return ch[a].off == ch[b].off; }
// a tile that a repair launch of this round starts a work-group on (dirty, and its predecessor in the sweep direction is not)
__device__ __forceinline__ bool head_f(const Chunk *__restrict__ ch, const int *__restrict__ dirty, int b) {
	return dirty[b] && !(b > 0 && same_seg(ch, b - 1, b) && dirty[b - 1]);
}
__device__ __forceinline__ bool head_b(const Chunk *__restrict__ ch, const int *__restrict__ dirty, int n, int b) {
	return dirty[b] && !(b + 1 < n && same_seg(ch, b, b + 1) && dirty[b + 1]);
}

} // namespace wide
} // namespace psmc
