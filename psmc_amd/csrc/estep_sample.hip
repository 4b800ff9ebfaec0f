// estep_sample.hip -- state paths drawn from the posterior P(path | data, parameters): forward filtering, backward sampling.
// psmc_hip_sample_paths, api_sample.hip; the arithmetic is pinned in include/psmc_hip.h.
//
// The forward vectors are khmm.c:170-185's bit for bit: tmp_k = sum_l f_{u-1}[l] * a[l][k] from 0.0 in ascending l, every product
// rounded once, f_u[k] = e(o_u)[k] * tmp_k divided by the ascending sum over k.  Given the state k at position u, the state at u - 1 is
// drawn from the weights w_l = f_{u-1}[l] * a[l][k]: with c_l their running sum -- the very sum whose last value is tmp_k -- and
// x = r * c_{n-1}, it is the number of l with c_l < x.  r depends on (seed, sample, segment, position) alone, not on the sample's history,
// so the draw is a MAP from the state at u to the state at u - 1, and the sweep stores that map for every k, one or two bytes per entry,
// exactly as the Viterbi sweep stores its back-pointers: the tiled backtrace of estep_viterbi.hip composes them.
//
// Sweep: one work-group per segment, all segments in one launch, longest first; positions are sequential.  A work-group is P parts of S
// threads; thread (k, part) owns column k of a -- in registers up to 192 padded states, streamed beyond -- and forms the ordered sum
// over l itself: ascending order is part of the definition, the range of l cannot be split.  Every part runs the same forward pass
// (same operations on the same LDS vector: same bits, nothing to exchange); part 0 publishes f_u.  The samples of the group are dealt
// round robin to the parts, and a part counts for up to four of its samples in one more pass over l that forms the same running sum
// again.  The r's are uniform over the work-group: thread g < group computes sample g's r of the next position into LDS.  Padded
// states carry zeros: adding +0.0 changes no sum, and what the padded l would add to a count is taken off again.
// Everything is stored with ordinary vector stores.
#include "psmc_hip_internal.h"

namespace psmc {

namespace {

constexpr uint64_t SAMP_GOLD = 0x9e3779b97f4a7c15ull;

__device__ __forceinline__ uint64_t samp_mix(uint64_t z)
{
	z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
	z ^= z >> 27; z *= 0x94d049bb133111ebull;
	z ^= z >> 31;
	return z;
}
// r of position u in (0, 1]: (z >> 11) + 1 <= 2^53 is a double as it stands, and so is its product with 2^-53
__device__ __forceinline__ double samp_r(uint64_t key, int u)
{
	const uint64_t z = samp_mix(key + SAMP_GOLD * (uint64_t)u);
	return (double)((z >> 11) + 1) * 0x1p-53;
}
// the drawn index from the count of c_l < x: 0 when the total is 0 or NaN; never beyond n - 1 (only weights below zero could get there)
__device__ __forceinline__ int samp_index(int cnt, double total, int n)
{
	if (!(total > 0.0 || total < 0.0)) return 0;
	return min(cnt, n - 1);
}

// strict left-to-right sum of v[0..n) from 0.0 (the normaliser, khmm.c:177-181)
__device__ __forceinline__ double samp_sum(const double *v, int n)
{
	double s = 0.0;
	int k = 0;
	for (; k + 8 <= n; k += 8) { // the reads are independent, the adds are the chain
		const double v0 = v[k], v1 = v[k + 1], v2 = v[k + 2], v3 = v[k + 3], v4 = v[k + 4], v5 = v[k + 5], v6 = v[k + 6], v7 = v[k + 7];
		s += v0; s += v1; s += v2; s += v3; s += v4; s += v5; s += v6; s += v7;
	}
	for (; k < n; ++k) s += v[k];
	return s;
}

// the register-resident passes read x from LDS a chunk of rows ahead; a scheduling barrier per chunk keeps the compiler from hoisting
// every read of a pass to its top (a register pair per l beside the column's: spills)
constexpr int samp_chunk(int SR) { return SR >= 192 ? 8 : 16; }

// tmp = sum_l x[l] * a[l][k], ascending from 0.0.  SR > 0: the column in registers, all SR = S rows (the padded ones add +0.0);
// SR == 0: the column streamed from m (row stride S), rows 0 .. n - 1
template <int SR> __device__ __forceinline__ double samp_dot(const double *x, const double *col, const double *__restrict__ m, int n, int S)
{
	double acc = 0.0;
	if constexpr (SR > 0) {
		constexpr int CH = samp_chunk(SR);
		double cur[CH], nxt[CH];
#pragma unroll
		for (int j = 0; j < CH; ++j) cur[j] = x[j];
#pragma unroll
		for (int l0 = 0; l0 < SR; l0 += CH) {
			if (l0 + CH < SR) {
#pragma unroll
				for (int j = 0; j < CH; ++j) nxt[j] = x[l0 + CH + j];
			}
#pragma unroll
			for (int j = 0; j < CH; ++j) acc += cur[j] * col[l0 + j];
			__builtin_amdgcn_sched_barrier(0);
#pragma unroll
			for (int j = 0; j < CH; ++j) cur[j] = nxt[j];
		}
	} else {
		int l = 0;
		for (; l + 8 <= n; l += 8) {
			double mv[8], xv[8];
#pragma unroll
			for (int j = 0; j < 8; ++j) { mv[j] = m[(size_t)(l + j) * S]; xv[j] = x[l + j]; }
#pragma unroll
			for (int j = 0; j < 8; ++j) acc += xv[j] * mv[j];
		}
		for (; l < n; ++l) acc += x[l] * m[(size_t)l * S];
	}
	return acc;
}

// the same running sum once more, counting for NC samples the l with c_l < xj[i]
template <int SR, int NC>
__device__ __forceinline__ void samp_count(const double *x, const double *col, const double *__restrict__ m, int n, int S, const double *xj, int *cnt)
{
	double c = 0.0;
#pragma unroll
	for (int i = 0; i < NC; ++i) cnt[i] = 0;
	if constexpr (SR > 0) {
		constexpr int CH = samp_chunk(SR);
		double cur[CH], nxt[CH];
#pragma unroll
		for (int j = 0; j < CH; ++j) cur[j] = x[j];
#pragma unroll
		for (int l0 = 0; l0 < SR; l0 += CH) {
			if (l0 + CH < SR) {
#pragma unroll
				for (int j = 0; j < CH; ++j) nxt[j] = x[l0 + CH + j];
			}
#pragma unroll
			for (int j = 0; j < CH; ++j) {
				c += cur[j] * col[l0 + j];
#pragma unroll
				for (int i = 0; i < NC; ++i) cnt[i] += c < xj[i] ? 1 : 0;
			}
			__builtin_amdgcn_sched_barrier(0);
#pragma unroll
			for (int j = 0; j < CH; ++j) cur[j] = nxt[j];
		}
		// rows n .. SR - 1 added +0.0 each: c stayed at c_{n-1}, and each of them counted what c_{n-1} < x counts
#pragma unroll
		for (int i = 0; i < NC; ++i) cnt[i] -= c < xj[i] ? SR - n : 0;
	} else {
		int l = 0;
		for (; l + 8 <= n; l += 8) {
			double mv[8], xv[8];
#pragma unroll
			for (int j = 0; j < 8; ++j) { mv[j] = m[(size_t)(l + j) * S]; xv[j] = x[l + j]; }
#pragma unroll
			for (int j = 0; j < 8; ++j) {
				c += xv[j] * mv[j];
#pragma unroll
				for (int i = 0; i < NC; ++i) cnt[i] += c < xj[i] ? 1 : 0;
			}
		}
		for (; l < n; ++l) {
			c += x[l] * m[(size_t)l * S];
#pragma unroll
			for (int i = 0; i < NC; ++i) cnt[i] += c < xj[i] ? 1 : 0;
		}
	}
}

// ---- the sweep.  SR > 0: S = SR in {64, 128, 192} with PR parts, the column in registers; SR == 0: any S (a multiple of 64, up to 1024)
// with P = 1024 / S parts, the column streamed.  Dynamic LDS: xs [2][S] doubles | gs [S] | rs [SAMP_MAX_GROUP]
template <int SR, int PR, typename BP>
__global__ __launch_bounds__(SR > 0 ? SR * PR : 1024) void k_samp_sweep(const double *__restrict__ a, const double *__restrict__ e, const double *__restrict__ a0,
                                                                         const uint8_t *__restrict__ obs, const VitSeg *__restrict__ segs,
                                                                         const uint64_t *__restrict__ sid, int n, int S_rt, int P_rt, uint64_t seed, int first,
                                                                         int group, BP *__restrict__ map, size_t stride, int32_t *__restrict__ end_state, int n_seg)
{
	extern __shared__ double samp_lds[];
	const int S = SR > 0 ? SR : S_rt, P = SR > 0 ? PR : P_rt;
	double *xs = samp_lds, *gs = samp_lds + 2 * S, *rs = samp_lds + 3 * S;
	const int t = threadIdx.x, k = t % S, part = t / S;
	const VitSeg sg = segs[blockIdx.x];
	double col[SR > 0 ? SR : 1];
	if constexpr (SR > 0) {
#pragma unroll
		for (int l = 0; l < SR; ++l) col[l] = a[(size_t)l * SR + k];
	}
	const double *m = a + k;
	const double e0 = e[k], e1 = e[S + k], e2 = e[2 * S + k];
	uint64_t key = 0;
	if (t < group) key = samp_mix(samp_mix(seed + SAMP_GOLD * (uint64_t)(first + t + 1)) + SAMP_GOLD * (sid[sg.seg] + 1));
	ObsAhead o(obs + sg.obs_off, sg.L);
	BP *row = map + (size_t)sg.row_off * S + k;
	{ // position 1: f_1 = a0 o e(o_1), normalised
		const int sym = (int)(o.cur & 3);
		const double g = a0[k] * (sym == 0 ? e0 : sym == 1 ? e1 : e2);
		if (part == 0) gs[k] = g;
		__syncthreads();
		if (part == 0) xs[S + k] = g / samp_sum(gs, n);
		if (t < group) rs[t] = samp_r(key, 1);
		__syncthreads();
	}
	for (int u = 2; u <= sg.L; ++u) {
		const int b = (u - 1) & 7;
		if (b == 0) o.advance();
		const int sym = (int)((o.cur >> (8 * b)) & 3);
		const double *xp = xs + ((u - 1) & 1) * S;
		const double tmp = samp_dot<SR>(xp, col, m, n, S);
		const double g = (sym == 0 ? e0 : sym == 1 ? e1 : e2) * tmp;
		if (part == 0) gs[k] = g;
		// the maps of this part's samples: row u - 1, the state at u - 1 given k at u, drawn with r(., u - 1)
		int xoff = ((u - 1) & 1) * S;
		asm volatile("" : "+s"(xoff)); // (the count passes read f_{u-1} through an offset of their own: left to itself the compiler keeps
		                               // the forward pass's products and running sums alive for them, a register per l)
		const double *xq = xs + xoff;
		int gi = part;
		for (; gi + 3 * P < group; gi += 4 * P) {
			double xj[4];
			int cnt[4];
#pragma unroll
			for (int i = 0; i < 4; ++i) xj[i] = rs[gi + i * P] * tmp;
			samp_count<SR, 4>(xq, col, m, n, S, xj, cnt);
#pragma unroll
			for (int i = 0; i < 4; ++i) row[(size_t)(gi + i * P) * stride + (size_t)(u - 1) * S] = (BP)samp_index(cnt[i], tmp, n);
		}
		for (; gi < group; gi += P) {
			double xj[1];
			int cnt[1];
			xj[0] = rs[gi] * tmp;
			samp_count<SR, 1>(xq, col, m, n, S, xj, cnt);
			row[(size_t)gi * stride + (size_t)(u - 1) * S] = (BP)samp_index(cnt[0], tmp, n);
		}
		__syncthreads();
		if (part == 0) xs[(u & 1) * S + k] = g / samp_sum(gs, n);
		if (t < group) rs[t] = samp_r(key, u);
		__syncthreads();
	}
	// the end draw: s_L from w = f_L with r(., L), one thread per sample
	if (t < group) {
		const double *fL = xs + (sg.L & 1) * S;
		const double total = samp_sum(fL, n), x = rs[t] * total;
		double c = 0.0;
		int cnt = 0;
		for (int l = 0; l < n; ++l) {
			c += fL[l];
			cnt += c < x ? 1 : 0;
		}
		end_state[(size_t)t * n_seg + sg.seg] = samp_index(cnt, total, n);
	}
}

} // namespace

int launch_sample_sweep(const SampLaunch &p)
{
	const int S = p.S;
	const size_t lds = sizeof(double) * (3 * (size_t)S + SAMP_MAX_GROUP);
#define SAMP_ARGS(BP, stride) p.a, p.e, p.a0, p.obs, p.segs, p.sid, p.n, S, 1024 / S, p.seed, p.first, p.group, (BP *)p.map, (size_t)(stride), p.end_state, p.n_seg
	if (p.group < 1 || p.group > SAMP_MAX_GROUP) return -1;
	if (S == 64) k_samp_sweep<64, 8, uint8_t><<<p.n_seg, 512, lds, p.stream>>>(SAMP_ARGS(uint8_t, p.map_stride));
	else if (S == 128) k_samp_sweep<128, 2, uint8_t><<<p.n_seg, 256, lds, p.stream>>>(SAMP_ARGS(uint8_t, p.map_stride));
	else if (S == 192) k_samp_sweep<192, 1, uint8_t><<<p.n_seg, 192, lds, p.stream>>>(SAMP_ARGS(uint8_t, p.map_stride));
	else if (!p.wide_bp) k_samp_sweep<0, 0, uint8_t><<<p.n_seg, (1024 / S) * S, lds, p.stream>>>(SAMP_ARGS(uint8_t, p.map_stride));
	else k_samp_sweep<0, 0, uint16_t><<<p.n_seg, (1024 / S) * S, lds, p.stream>>>(SAMP_ARGS(uint16_t, p.map_stride / 2));
#undef SAMP_ARGS
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace psmc
