// estep_post_fast.hip -- posterior decoding from the tables of a FAST-mode E-step (psmc_hip_decode / _posterior /
// _post_counts / _scales / _post_mean / _post_quantile on a fast context whose last single E-step left both X and bt: the dense sweeps, or the
// structured sweeps with the unfused back half, "fuse=0" / "fuse128=0").
//
// Conventions of the tables (estep_fast.hip, estep_struct.hip; g = seg_off + u - 1):
//   X_u  = e[o_u] * (a^T X_{u-1}) * inv_u            d_f, inv_u = d_s[g] at u % 4 == 0 (a power of two or 1/sum), 1 elsewhere
//   bt_u = e[o_u] * (a bt_{u+1}) * sb_u              d_b, sb_u  = d_sb[g] at u % 4 == 0, 1 elsewhere
// and a tile that starts at lo > 1 was swept from its own start vector entry = X_{lo-1} (d_entry), which agrees with the
// stored row lo-1 in direction only.  Neither vector has the reference's scale, so every output is a ratio in which the
// scales cancel:
//   posterior  gamma_u(k) = X_u(k) bt_u(k) / e_k(o_u) / G_u,  G_u = sum_k X_u(k) bt_u(k) / e_k(o_u)     (k_expect_mfma's g_p / G_p)
//              (u = L: beta_L = 1, gamma_L = X_L / sum X_L)
//   -D recomb  1 - sb_u sum_l X_u(l) a_ll bt_{u+1}(l) / G_u   (u < L; 0 at u = L): sum_kl X_u(k) a_kl bt_{u+1}(l) = G_u / sb_u
//   -s         s_u = sum X_u / sum X_{u-1} / inv_u  (X_{u-1} := entry at a tile's first position), s_1 = sum_k a0_k e_k(o_1)
// One wave per block of positions, lane = state (and state + 64 at 128 states); the sums are wave_sum_nat, whose total is
// taken from lane 0 so that every lane divides by the same double.
#include <hip/hip_runtime.h>
#include "wave_prims.h"
#include "struct_prims.h"
#include "psmc_hip_internal.h"

namespace psmc {

constexpr int POST_BLK = 64;    // positions per wave: posterior, decode, scales
constexpr int PCNT_BLK = 2048;  // positions per wave of the -c partial sums (the second kernel adds one partial per block)
constexpr int PCNT_J = 8;       // count columns per pass over a block

__device__ __forceinline__ double wsum(double v) { return first_lane_f64(wave_sum_nat(v)); }

template <int S> struct PostRow {
	static constexpr int PER = S / 64;
	double gam[PER]; // X bt / e (unnormalised posterior)
	double G;        // their sum over the states
};

// unnormalised posterior of position u (1-based) of the segment at off
template <int S>
__device__ __forceinline__ void post_row(const double *__restrict__ f, const double *__restrict__ b, const double *__restrict__ re,
                                         int sym, int64_t g, int u, int L, int lane, PostRow<S> &r)
{
	double t = 0.0;
#pragma unroll
	for (int j = 0; j < PostRow<S>::PER; ++j) {
		const int k = lane + 64 * j;
		const double x = f[g * S + k];
		const double rr = sym == 0 ? re[k] : (sym == 1 ? re[S + k] : 1.0);
		r.gam[j] = u < L ? x * b[g * S + k] * rr : x;
		t += r.gam[j];
	}
	r.G = wsum(t);
}

// post[(u-1)*n + k] = gamma_u(k), recomb[u-1] (-D), path / maxp (-d): any of them may be null
template <int S>
__global__ __launch_bounds__(64) void k_post_fast(const double *__restrict__ f, const double *__restrict__ b,
                                                    const double *__restrict__ sb, const double *__restrict__ re,
                                                    const double *__restrict__ a, const uint8_t *__restrict__ obs, int64_t off,
                                                    int L, int n, double *__restrict__ post, double *__restrict__ recomb,
                                                    int32_t *__restrict__ path, double *__restrict__ maxp)
{
	constexpr int PER = S / 64;
	const int lane = threadIdx.x;
	const int u0 = blockIdx.x * POST_BLK + 1, u1 = min(L, u0 + POST_BLK - 1);
	double dg[PER];
#pragma unroll
	for (int j = 0; j < PER; ++j) { const int k = lane + 64 * j; dg[j] = recomb ? a[(int64_t)k * S + k] : 0.0; }
	for (int u = u0; u <= u1; ++u) {
		const int64_t g = off + u - 1;
		PostRow<S> r;
		post_row<S>(f, b, re, (int)obs[g], g, u, L, lane, r);
		double pv[PER];
#pragma unroll
		for (int j = 0; j < PER; ++j) pv[j] = r.gam[j] / r.G;
		if (post) {
#pragma unroll
			for (int j = 0; j < PER; ++j) { const int k = lane + 64 * j; if (k < n) post[(int64_t)(u - 1) * n + k] = pv[j]; }
		}
		if (path) { // first maximum in state order (hmm_post_decode compares with `<`)
			double v = lane < n ? pv[0] : -1.0;
			int k = lane;
			if constexpr (PER == 2) { const int k2 = lane + 64; const double v2 = k2 < n ? pv[1] : -1.0; if (v2 > v) { v = v2; k = k2; } }
#pragma unroll
			for (int m = 32; m >= 1; m >>= 1) {
				const double ov = __shfl_xor(v, m, 64);
				const int ok = __shfl_xor(k, m, 64);
				if (ov > v || (ov == v && ok < k)) { v = ov; k = ok; }
			}
			if (lane == 0) { path[u - 1] = k; if (maxp) maxp[u - 1] = v; }
		}
		if (recomb) {
			double pr = 0.0;
			if (u < L) {
				double t = 0.0;
#pragma unroll
				for (int j = 0; j < PER; ++j) { const int k = lane + 64 * j; t += f[g * S + k] * dg[j] * b[(g + 1) * S + k]; }
				const double sc = (u & (NORM_EVERY - 1)) == 0 ? sb[g] : 1.0;
				const double sm = sc * wsum(t) / r.G;
				pr = sm != sm ? sm : 1.0 - sm;
			}
			if (lane == 0) recomb[u - 1] = pr;
		}
	}
}

// psmc_hip_post_mean: mean[(u-1)*n_w + j] = sum_k gamma_u(k) w[j][k], gamma the doubles k_post_fast stores (gam / G).
// w: [n_w][S], zeros beyond the n states (the padded states' gam is 0 as well).
template <int S>
__global__ __launch_bounds__(64) void k_post_mean_fast(const double *__restrict__ f, const double *__restrict__ b,
                                                         const double *__restrict__ re, const uint8_t *__restrict__ obs, int64_t off,
                                                         int L, const double *__restrict__ w, int n_w, double *__restrict__ mean)
{
	constexpr int PER = S / 64, MW = MEAN_COLS;
	const int lane = threadIdx.x;
	const int u0 = blockIdx.x * POST_BLK + 1, u1 = min(L, u0 + POST_BLK - 1);
	double wv[MW][PER];
#pragma unroll
	for (int c = 0; c < MW; ++c)
#pragma unroll
		for (int j = 0; j < PER; ++j) wv[c][j] = c < n_w ? w[c * S + lane + 64 * j] : 0.0;
	for (int u = u0; u <= u1; ++u) {
		const int64_t g = off + u - 1;
		PostRow<S> r;
		post_row<S>(f, b, re, (int)obs[g], g, u, L, lane, r);
		double pv[PER];
#pragma unroll
		for (int j = 0; j < PER; ++j) pv[j] = r.gam[j] / r.G;
#pragma unroll
		for (int c = 0; c < MW; ++c)
			if (c < n_w) {
				double t = pv[0] * wv[c][0];
#pragma unroll
				for (int j = 1; j < PER; ++j) t = __builtin_fma(pv[j], wv[c][j], t);
				const double m = wsum(t);
				if (lane == 0) mean[(int64_t)(u - 1) * n_w + c] = m;
			}
	}
}

// psmc_hip_post_quantile: state[(u-1)*n_q + j] = min(n - 1, #{k < n : c_k < q_j G}) over the prefix sums c_k of the row's
// unnormalised gam and its total G (post_row's; no division).  A lane holds the states lane + 64 j, so the prefix over the states
// is the inclusive wave scan of gam[j] plus the totals of the lower j (lane 63 of their scans); the count is a ballot per j, and
// the padded states (k >= n) are left out by the test itself.  A NaN total: every comparison is false, state 0.
template <int S>
__global__ __launch_bounds__(64) void k_post_quantile_fast(const double *__restrict__ f, const double *__restrict__ b,
                                                             const double *__restrict__ re, const uint8_t *__restrict__ obs, int64_t off,
                                                             int L, int n, QuantQ qq, int n_q, int32_t *__restrict__ state)
{
	constexpr int PER = S / 64;
	const int lane = threadIdx.x;
	const int u0 = blockIdx.x * POST_BLK + 1, u1 = min(L, u0 + POST_BLK - 1);
	for (int u = u0; u <= u1; ++u) {
		const int64_t g = off + u - 1;
		PostRow<S> r;
		post_row<S>(f, b, re, (int)obs[g], g, u, L, lane, r);
		double c[PER], base = 0.0;
#pragma unroll
		for (int j = 0; j < PER; ++j) {
			c[j] = wave_prefix_incl_bc(r.gam[j]);
			if (j) c[j] += base;
			if (j + 1 < PER) base = readlane_f64(c[j], 63);
		}
#pragma unroll
		for (int col = 0; col < QUANT_COLS; ++col)
			if (col < n_q) { // (a kernel argument: the same in every lane)
				const double x = qq.q[col] * r.G;
				int cnt = 0;
#pragma unroll
				for (int j = 0; j < PER; ++j) cnt += __popcll(__ballot(lane + 64 * j < n && c[j] < x));
				if (lane == 0) state[(int64_t)(u - 1) * n_q + col] = min(cnt, n - 1);
			}
	}
}

// -s: the reference's scaling factors s_u (hmm_forward, khmm.c:170-186).  Tiles of the segment: T bins each, the first
// one is tile `first` of the plan (its start vectors in entry).
template <int S>
__global__ __launch_bounds__(64) void k_scales_fast(const double *__restrict__ f, const double *__restrict__ invd,
                                                      const double *__restrict__ entry, const double *__restrict__ a0,
                                                      const double *__restrict__ e, const uint8_t *__restrict__ obs, int64_t off,
                                                      int L, int T, int first, double *__restrict__ s)
{
	constexpr int PER = S / 64;
	const int lane = threadIdx.x;
	const int u0 = blockIdx.x * POST_BLK + 1, u1 = min(L, u0 + POST_BLK - 1);
	auto row_sum = [&](const double *p) {
		double t = 0.0;
#pragma unroll
		for (int j = 0; j < PER; ++j) t += p[lane + 64 * j];
		return wsum(t);
	};
	double prev = u0 > 1 ? row_sum(f + (off + u0 - 2) * S) : 0.0; // sum X_{u0-1}
	for (int u = u0; u <= u1; ++u) {
		const int64_t g = off + u - 1;
		const double cur = row_sum(f + g * S);
		double su;
		if (u == 1) { // f_1 = a0 * e[o_1], s_1 = its sum (khmm.c:171-174)
			const int sym = (int)obs[g];
			double t = 0.0;
#pragma unroll
			for (int j = 0; j < PER; ++j) { const int k = lane + 64 * j; t += a0[k] * (sym == 2 ? 1.0 : e[sym * S + k]); }
			su = wsum(t);
		} else {
			const double den = (u - 1) % T == 0 ? row_sum(entry + (int64_t)(first + (u - 1) / T) * S) : prev;
			su = cur / den;
			if ((u & (NORM_EVERY - 1)) == 0) su = su / invd[g];
		}
		if (lane == 0) s[u - 1] = su;
		prev = cur;
	}
}

// -c: part[(blk * n_cnt + j) * S + k] = sum over the block's positions u of gamma_u(k) * cnt1[u-1][j]
template <int S>
__global__ __launch_bounds__(64) void k_post_counts_fast(const double *__restrict__ f, const double *__restrict__ b,
                                                           const double *__restrict__ re, const uint8_t *__restrict__ obs, int64_t off,
                                                           int L, int min_l, const int32_t *__restrict__ cnt1, int n_cnt,
                                                           double *__restrict__ part)
{
	constexpr int PER = S / 64;
	const int lane = threadIdx.x, blk = blockIdx.x;
	const int u0 = blk * PCNT_BLK + 1, u1 = min(min_l, u0 + PCNT_BLK - 1);
	for (int j0 = 0; j0 < n_cnt; j0 += PCNT_J) {
		double acc[PCNT_J][PER];
#pragma unroll
		for (int jj = 0; jj < PCNT_J; ++jj)
#pragma unroll
			for (int q = 0; q < PER; ++q) acc[jj][q] = 0.0;
		for (int u = u0; u <= u1; ++u) {
			const int64_t g = off + u - 1;
			PostRow<S> r;
			post_row<S>(f, b, re, (int)obs[g], g, u, L, lane, r);
			const int32_t *cr = cnt1 + (int64_t)(u - 1) * n_cnt + j0;
#pragma unroll
			for (int jj = 0; jj < PCNT_J; ++jj) {
				if (j0 + jj < n_cnt) {
					const double cv = (double)cr[jj];
#pragma unroll
					for (int q = 0; q < PER; ++q) acc[jj][q] += r.gam[q] / r.G * cv;
				}
			}
		}
#pragma unroll
		for (int jj = 0; jj < PCNT_J; ++jj)
			if (j0 + jj < n_cnt)
#pragma unroll
				for (int q = 0; q < PER; ++q) part[((int64_t)blk * n_cnt + j0 + jj) * S + lane + 64 * q] = acc[jj][q];
	}
}

// cnt[k * n_cnt + j] += the blocks' partials, in block order (deterministic); one thread per (k, j)
template <int S>
__global__ __launch_bounds__(256) void k_post_counts_add(const double *__restrict__ part, int n_blk, int n_cnt, int n,
                                                           double *__restrict__ cnt)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n * n_cnt) return;
	const int k = i / n_cnt, j = i % n_cnt;
	double t = 0.0;
	for (int q = 0; q < n_blk; ++q) t += part[((int64_t)q * n_cnt + j) * S + k];
	cnt[i] += t;
}

int launch_post_fast(hipStream_t st, const double *f, const double *b, const double *sb, const double *re, const double *a,
                     const uint8_t *obs, int64_t off, int L, int n, int ns, double *post, double *recomb, int32_t *path, double *maxp)
{
	const dim3 grid((L + POST_BLK - 1) / POST_BLK);
	if (ns == 128) hipLaunchKernelGGL(k_post_fast<128>, grid, dim3(64), 0, st, f, b, sb, re, a, obs, off, L, n, post, recomb, path, maxp);
	else hipLaunchKernelGGL(k_post_fast<64>, grid, dim3(64), 0, st, f, b, sb, re, a, obs, off, L, n, post, recomb, path, maxp);
	return (int)hipGetLastError();
}

int launch_post_mean_fast(hipStream_t st, const double *f, const double *b, const double *re, const uint8_t *obs, int64_t off, int L,
                          int ns, const double *w, int n_w, double *mean)
{
	const dim3 grid((L + POST_BLK - 1) / POST_BLK);
	if (ns == 128) hipLaunchKernelGGL(k_post_mean_fast<128>, grid, dim3(64), 0, st, f, b, re, obs, off, L, w, n_w, mean);
	else hipLaunchKernelGGL(k_post_mean_fast<64>, grid, dim3(64), 0, st, f, b, re, obs, off, L, w, n_w, mean);
	return (int)hipGetLastError();
}

int launch_post_quantile_fast(hipStream_t st, const double *f, const double *b, const double *re, const uint8_t *obs, int64_t off, int L,
                              int n, int ns, const QuantQ &q, int n_q, int32_t *state)
{
	const dim3 grid((L + POST_BLK - 1) / POST_BLK);
	if (ns == 128) hipLaunchKernelGGL(k_post_quantile_fast<128>, grid, dim3(64), 0, st, f, b, re, obs, off, L, n, q, n_q, state);
	else hipLaunchKernelGGL(k_post_quantile_fast<64>, grid, dim3(64), 0, st, f, b, re, obs, off, L, n, q, n_q, state);
	return (int)hipGetLastError();
}

int launch_scales_fast(hipStream_t st, const double *f, const double *invd, const double *entry, const double *a0, const double *e,
                       const uint8_t *obs, int64_t off, int L, int T, int first, int ns, double *s)
{
	const dim3 grid((L + POST_BLK - 1) / POST_BLK);
	if (ns == 128) hipLaunchKernelGGL(k_scales_fast<128>, grid, dim3(64), 0, st, f, invd, entry, a0, e, obs, off, L, T, first, s);
	else hipLaunchKernelGGL(k_scales_fast<64>, grid, dim3(64), 0, st, f, invd, entry, a0, e, obs, off, L, T, first, s);
	return (int)hipGetLastError();
}

int post_counts_fast_blocks(int min_l) { return (min_l + PCNT_BLK - 1) / PCNT_BLK; }

int launch_post_counts_fast(hipStream_t st, const double *f, const double *b, const double *re, const uint8_t *obs, int64_t off,
                            int L, int min_l, const int32_t *cnt1, int n_cnt, int n, int ns, double *part, double *cnt)
{
	const int nb = post_counts_fast_blocks(min_l);
	const dim3 g2((n * n_cnt + 255) / 256);
	if (ns == 128) {
		hipLaunchKernelGGL(k_post_counts_fast<128>, dim3(nb), dim3(64), 0, st, f, b, re, obs, off, L, min_l, cnt1, n_cnt, part);
		hipLaunchKernelGGL(k_post_counts_add<128>, g2, dim3(256), 0, st, part, nb, n_cnt, n, cnt);
	} else {
		hipLaunchKernelGGL(k_post_counts_fast<64>, dim3(nb), dim3(64), 0, st, f, b, re, obs, off, L, min_l, cnt1, n_cnt, part);
		hipLaunchKernelGGL(k_post_counts_add<64>, g2, dim3(256), 0, st, part, nb, n_cnt, n, cnt);
	}
	return (int)hipGetLastError();
}

} // namespace psmc
