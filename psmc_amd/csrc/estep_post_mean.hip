// estep_post_mean.hip -- psmc_hip_post_mean on the EXACT tables (f, b, s of estep_exact.hip / estep_wide.hip), any width S:
//   mean[u][j] = sum_k gamma_u(k) * w[j][k],   gamma_u(k) = f[u][k] * b[u][k] * s[u]   (the double psmc_hip_posterior returns)
// with every product rounded once (the library is built with -ffp-contract=off: no FMA) and the sum in state order, the first term
// taken as it is: ((t_0 + t_1) + t_2) + ... -- bit for bit the C loop over the rows of psmc_hip_posterior.
// One wave per 64 positions.  The tables are read coalesced, a slab of 64 positions x 16 states at a time: element e of the slab
// goes to lane e % 64, so 16 adjacent lanes read the 128 contiguous bytes of one row; f * b goes through LDS (row stride 17: no bank
// conflict either way), and then lane = position walks its row's 16 states in order.  The weights are wave-uniform (scalar loads).
// The last slab's load may take in up to 15 padded states (k >= n; inside the row, S being a multiple of 64): they go to LDS and are
// never used -- the walk stops at n.  LDS: 64 x 17 doubles.
#include <hip/hip_runtime.h>
#include "psmc_hip_internal.h"

namespace psmc {

constexpr int PM_POS = 64, PM_K = 16, PM_LD = PM_K + 1;

// w: [n_w][S], mean: [L][n_w] (position 1 first)
__global__ __launch_bounds__(64) void k_post_mean_exact(const double *__restrict__ f, const double *__restrict__ b,
                                                          const double *__restrict__ s, int64_t off, int L, int n, int S,
                                                          const double *__restrict__ w, int n_w, double *__restrict__ mean)
{
	__shared__ double tile[PM_POS * PM_LD];
	const int lane = threadIdx.x;
	const int u0 = blockIdx.x * PM_POS, rows = min(PM_POS, L - u0);
	const int64_t g0 = off + u0;
	const double ss = lane < rows ? s[g0 + lane] : 0.0;
	double m[MEAN_COLS] = {};
	for (int k0 = 0; k0 < n; k0 += PM_K) {
#pragma unroll
		for (int it = 0; it < PM_K; ++it) {
			const int el = it * PM_POS + lane, row = el / PM_K, col = el % PM_K;
			if (row < rows) {
				const int64_t i = (g0 + row) * S + k0 + col; // (k0 + col < S: S is a multiple of 64)
				tile[row * PM_LD + col] = f[i] * b[i];
			}
		}
		__syncthreads();
		const int kc = min(PM_K, n - k0);
		if (lane < rows) {
#pragma unroll
			for (int c = 0; c < PM_K; ++c) {
				if (c < kc) {
					const double gam = tile[lane * PM_LD + c] * ss; // f * b * s, left to right
#pragma unroll
					for (int j = 0; j < MEAN_COLS; ++j)
						if (j < n_w) {
							const double t = gam * w[(int64_t)j * S + k0 + c];
							m[j] = k0 + c == 0 ? t : m[j] + t;
						}
				}
			}
		}
		__syncthreads();
	}
	if (lane < rows) {
#pragma unroll
		for (int j = 0; j < MEAN_COLS; ++j)
			if (j < n_w) mean[(int64_t)(u0 + lane) * n_w + j] = m[j];
	}
}

int launch_post_mean_exact(hipStream_t st, const double *f, const double *b, const double *s, int64_t off, int L, int n, int S,
                           const double *w, int n_w, double *mean)
{
	hipLaunchKernelGGL(k_post_mean_exact, dim3((L + PM_POS - 1) / PM_POS), dim3(64), 0, st, f, b, s, off, L, n, S, w, n_w, mean);
	return (int)hipGetLastError();
}

} // namespace psmc
