// wide_prims.h -- what the kernels of the wide fast path share (estep_wide_fast.hip: the E-step; estep_wide_post.hip: decoding
// from its tables): S = 192 or 256 padded states as ONE tile per wave, 64 lanes x NPL adjacent states (lane j holds k = NPL j + i),
// the whole-wave scans, the parameter block, the O(N) step x <- M x and the backward step with its scaling at p % 4 == 0.
#pragma once
#include <hip/hip_runtime.h>
#include "wave_prims.h"
#include "struct_prims.h"
#include "psmc_hip_internal.h"

namespace psmc {
namespace wide {

// parameter block of the wide fast path, S doubles each: e0 | e1 | a0 | P | R | qa | c | dd
constexpr int WP_E0 = 0, WP_E1 = 1, WP_A0 = 2, WP_SP = 3;

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
// sum over the wave of NPL values per lane, carried as an unevaluated pair (Knuth's two-sum at every addition, the error terms
// added up beside): the rounded result is the exact sum's nearest double but for ties, the same bits in every lane
__device__ __forceinline__ void two_sum(double a, double b, double &s, double &err) {
	s = a + b;
	const double bb = s - a;
	err = (a - (s - bb)) + (b - bb);
}
template <int NPL> __device__ __forceinline__ double wave_total_comp(const double (&x)[NPL]) {
	double h = x[0], l = 0.0, t;
#pragma unroll
	for (int i = 1; i < NPL; ++i) { two_sum(h, x[i], h, t); l += t; }
#pragma unroll
	for (int m = 1; m <= 32; m <<= 1) {
		const double oh = __shfl_xor(h, m, 64), ol = __shfl_xor(l, m, 64);
		two_sum(h, oh, h, t);
		l = (l + ol) + t;
	}
	return h + l;
}
template <int NPL> __device__ __forceinline__ void ld(const double *p, double (&v)[NPL]) {
#pragma unroll
	for (int i = 0; i < NPL; ++i) v[i] = p[i];
}
template <int NPL> __device__ __forceinline__ void st(double *p, const double (&v)[NPL]) {
#pragma unroll
	for (int i = 0; i < NPL; ++i) p[i] = v[i];
}
// the five vectors in the roles load_struct_par (estep_struct.hip) gives them: forward mS = P, wS = qa, mP = R, wP = c;
// backward mS = c, wS = R, mP = qa, wP = P
template <int NPL> __device__ __forceinline__ void load_par(const double *__restrict__ par, int k0, bool fwd, StructParN<NPL> &c) {
	constexpr int S = 64 * NPL;
	const double *sp = par + WP_SP * S + k0; // P | R | qa | c | dd
	ld<NPL>(sp + (fwd ? 0 : 3 * S), c.mS); ld<NPL>(sp + (fwd ? 2 * S : S), c.wS);
	ld<NPL>(sp + (fwd ? S : 2 * S), c.mP); ld<NPL>(sp + (fwd ? 3 * S : 0), c.wP); ld<NPL>(sp + 4 * S, c.dd);
}
template <int NPL> __device__ __forceinline__ void emis(int sym, const double (&e0)[NPL], const double (&e1)[NPL], double (&ev)[NPL]) {
#pragma unroll
	for (int i = 0; i < NPL; ++i) ev[i] = sym == 0 ? e0[i] : (sym == 1 ? e1[i] : 1.0);
}
// x <- M x: wS.SUF(x.mS) + wP.PRE(x.mP) + dd.x (inclusive scans over the S states)
template <int NPL> __device__ __forceinline__ void wstep(const StructParN<NPL> &c, double (&x)[NPL], const WaveScanMasks &wm) {
	double su[NPL], pv[NPL];
	su[NPL - 1] = x[NPL - 1] * c.mS[NPL - 1];
#pragma unroll
	for (int i = NPL - 2; i >= 0; --i) su[i] = __builtin_fma(x[i], c.mS[i], su[i + 1]);
	pv[0] = x[0] * c.mP[0];
#pragma unroll
	for (int i = 1; i < NPL; ++i) pv[i] = __builtin_fma(x[i], c.mP[i], pv[i - 1]);
	const double ES = wave_excl_suffix(su[0], wm), EP = wave_excl_prefix(pv[NPL - 1]);
#pragma unroll
	for (int i = 0; i < NPL; ++i) {
		const double t = __builtin_fma(c.wS[i], su[i], __builtin_fma(c.wP[i], pv[i], c.dd[i] * x[i]));
		x[i] = __builtin_fma(c.wS[i], ES, __builtin_fma(c.wP[i], EP, t));
	}
}
// one forward position p: x = X_{p-1} -> X_p = e[o_p] . (M x), scaled at p % 4 == 0 (NORM) by 1/d_p, a power of two (struct_prims.h
// pow2_rcp) -- GIVEN: the factor the forward sweep stored (`given`), else computed from x.  Returns the factor.  The forward sweep
// and the checkpointed accumulate sweep's recomputation (estep_wide_fast.hip) both step through here: the same arithmetic, so the same bits.
template <int NPL, bool NORM, bool GIVEN>
__device__ __forceinline__ double fstep(const StructParN<NPL> &c, const WaveScanMasks &wm, int sym, const double (&e0)[NPL],
                                        const double (&e1)[NPL], double (&x)[NPL], double given)
{
	double ev[NPL];
	emis<NPL>(sym, e0, e1, ev);
	double iv = 1.0;
	if (NORM) {
		iv = GIVEN ? given : pow2_rcp(wave_total(lsum<NPL>(x)));
#pragma unroll
		for (int i = 0; i < NPL; ++i) ev[i] *= iv;
	}
	wstep<NPL>(c, x, wm);
#pragma unroll
	for (int i = 0; i < NPL; ++i) x[i] *= ev[i];
	return iv;
}
// the checkpointed X table ("wide_ckpt"): one row per position p with p % 8 == 0.  Segments start at off % 64 == 0, so the rows of
// all segments lie in one table by absolute position: the row of position p of the segment at `off`
constexpr int WCK = 8;
__device__ __forceinline__ int64_t ckpt_row(int64_t off, int p) { return (off >> 3) + (p >> 3) - 1; }
// the forward roles of the five vectors, from a backward set (load_par: the same vectors in other roles)
template <int NPL> __device__ __forceinline__ void fwd_roles(const StructParN<NPL> &b, StructParN<NPL> &f) {
#pragma unroll
	for (int i = 0; i < NPL; ++i) { f.mS[i] = b.wP[i]; f.wS[i] = b.mP[i]; f.mP[i] = b.wS[i]; f.wP[i] = b.mS[i]; f.dd[i] = b.dd[i]; }
}
// max_k |u/|u| - v/|v|| / max_k v/|v| (u: the vector a tile built on, v: what its neighbour computed); NaN anywhere: +inf
template <int NPL> __device__ __forceinline__ double wmismatch(const double (&u)[NPL], const double (&v)[NPL]) {
	const double iu = 1.0 / wave_total(lsum<NPL>(u)), iv = 1.0 / wave_total(lsum<NPL>(v));
	double num = 0.0, den = 0.0;
	bool bad = iu != iu || iv != iv;
#pragma unroll
	for (int i = 0; i < NPL; ++i) {
		num = fmax(num, fabs(u[i] * iu - v[i] * iv)); den = fmax(den, fabs(v[i] * iv));
		bad = bad || u[i] != u[i] || v[i] != v[i];
	}
	num = wave_maxv(num); den = wave_maxv(den);
	return __any(bad) ? __builtin_inf() : num / den;
}
__device__ __forceinline__ bool same_seg(const Chunk *__restrict__ ch, int a, int b) { return ch[a].off == ch[b].off; }
// a tile that a repair launch of this round starts a wave on (dirty, and its predecessor in the sweep direction is not)
__device__ __forceinline__ bool head_f(const Chunk *__restrict__ ch, const int *__restrict__ dirty, int b) {
	return dirty[b] && !(b > 0 && same_seg(ch, b - 1, b) && dirty[b - 1]);
}
__device__ __forceinline__ bool head_b(const Chunk *__restrict__ ch, const int *__restrict__ dirty, int n, int b) {
	return dirty[b] && !(b + 1 < n && same_seg(ch, b, b + 1) && dirty[b + 1]);
}

// one backward step at position p: x = bt_{p+1} -> bt_p (own scaling at p % 4 == 0: 1/sum(bt_{p+1}))
template <int NPL, bool NORM>
__device__ __forceinline__ void bstep(const StructParN<NPL> &sc, const WaveScanMasks &wm, int sym, const double (&e0)[NPL],
                                      const double (&e1)[NPL], double (&x)[NPL])
{
	double ev[NPL];
	emis<NPL>(sym, e0, e1, ev);
	if (NORM) {
		const double sb = rcp_newton(wave_total(lsum<NPL>(x)));
#pragma unroll
		for (int i = 0; i < NPL; ++i) ev[i] *= sb;
	}
	wstep<NPL>(sc, x, wm);
#pragma unroll
	for (int i = 0; i < NPL; ++i) x[i] *= ev[i];
}

} // namespace wide
} // namespace psmc
