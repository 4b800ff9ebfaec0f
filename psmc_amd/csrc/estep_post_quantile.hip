// estep_post_quantile.hip -- psmc_hip_post_quantile on the EXACT tables (f, b, s of estep_exact.hip / estep_wide.hip), any width S:
//   gamma_u(k) = f[u][k] * b[u][k] * s[u]   (the double psmc_hip_posterior returns),
//   c_0 = gamma_u(0), c_k = c_{k-1} + gamma_u(k)  -- one rounded addition each, in state order, the first term taken as it is --
//   x_j = q_j * c_{n-1}  (one rounded product),   state[u][j] = min(n - 1, #{k < n : c_k < x_j})
// with every product rounded once (the library is built with -ffp-contract=off: no FMA) -- bit for bit the C loop over the rows of
// psmc_hip_posterior.  A NaN total gives 0: every comparison is false.
// The layout of estep_post_mean.hip: one wave per 64 positions; the tables are read coalesced, a slab of 64 positions x 16 states at
// a time, f * b goes through LDS (row stride 17: no bank conflict either way), and then lane = position walks its row's 16 states
// in order.  The total is needed before the count, so the row is walked TWICE: the first walk keeps the running sum only, the
// second one forms the same running sums again -- the same operations on the same doubles -- and counts them against the
// thresholds (the second read of the wave's 2 x 64 x S doubles comes from the cache).  The last slab's load may take in up to 15
// padded states (k >= n; inside the row, S being a multiple of 64): they go to LDS and are never used -- the walk stops at n.
// LDS: 64 x 17 doubles.
#include <hip/hip_runtime.h>
#include "psmc_hip_internal.h"

namespace psmc {

constexpr int PQ_POS = 64, PQ_K = 16, PQ_LD = PQ_K + 1;

// state: [L][n_q] (position 1 first)
__global__ __launch_bounds__(64) void k_post_quantile_exact(const double *__restrict__ f, const double *__restrict__ b,
                                                              const double *__restrict__ s, int64_t off, int L, int n, int S,
                                                              QuantQ qq, int n_q, int32_t *__restrict__ state)
{
	__shared__ double tile[PQ_POS * PQ_LD];
	const int lane = threadIdx.x;
	const int u0 = blockIdx.x * PQ_POS, rows = min(PQ_POS, L - u0);
	const int64_t g0 = off + u0;
	const double ss = lane < rows ? s[g0 + lane] : 0.0;
	double x[QUANT_COLS] = {};
	int cnt[QUANT_COLS] = {};
	for (int pass = 0; pass < 2; ++pass) { // 0: the total; 1: the count
		double c = 0.0;
		for (int k0 = 0; k0 < n; k0 += PQ_K) {
#pragma unroll
			for (int it = 0; it < PQ_K; ++it) {
				const int el = it * PQ_POS + lane, row = el / PQ_K, col = el % PQ_K;
				if (row < rows) {
					const int64_t i = (g0 + row) * S + k0 + col; // (k0 + col < S: S is a multiple of 64)
					tile[row * PQ_LD + col] = f[i] * b[i];
				}
			}
			__syncthreads();
			const int kc = min(PQ_K, n - k0);
			if (lane < rows) {
#pragma unroll
				for (int cc = 0; cc < PQ_K; ++cc) {
					if (cc < kc) {
						const double gam = tile[lane * PQ_LD + cc] * ss; // f * b * s, left to right
						c = k0 + cc == 0 ? gam : c + gam;
						if (pass) {
#pragma unroll
							for (int j = 0; j < QUANT_COLS; ++j) cnt[j] += c < x[j] ? 1 : 0; // (x of a column beyond n_q is 0 and unused)
						}
					}
				}
			}
			__syncthreads();
		}
		if (pass == 0) {
#pragma unroll
			for (int j = 0; j < QUANT_COLS; ++j) x[j] = j < n_q ? qq.q[j] * c : 0.0;
		}
	}
	if (lane < rows) {
#pragma unroll
		for (int j = 0; j < QUANT_COLS; ++j)
			if (j < n_q) state[(int64_t)(u0 + lane) * n_q + j] = min(cnt[j], n - 1);
	}
}

int launch_post_quantile_exact(hipStream_t st, const double *f, const double *b, const double *s, int64_t off, int L, int n, int S,
                               const QuantQ &q, int n_q, int32_t *state)
{
	hipLaunchKernelGGL(k_post_quantile_exact, dim3((L + PQ_POS - 1) / PQ_POS), dim3(64), 0, st, f, b, s, off, L, n, S, q, n_q, state);
	return (int)hipGetLastError();
}

} // namespace psmc
