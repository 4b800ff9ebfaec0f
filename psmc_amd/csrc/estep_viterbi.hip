// estep_viterbi.hip -- the Viterbi path of every segment (khmm.c:83-141): psmc_hip_viterbi, api_viterbi.hip.
//
// The recursion in log space has no ordered sum.  With the host's log tables (one libm log() per entry)
//     V_1[k] = le[o_1][k] + l0[k]
//     V_u[k] = le[o_u][k] + max_l (V_{u-1}[l] + la[k][l]),   bp_u[k] = the lowest l that attains the maximum
// every candidate is ONE rounded addition, and "the maximum, the lowest index among equal maxima" is exact and associative: the range of l
// may be cut into parts that are reduced side by side and combined in any order, and the bits are still khmm.c's.  A part's result is
// (m, arg) of khmm.c's own loop over that part -- m = -1e300, arg = -1 to start with, `if (m < c)` taken in ascending l -- and parts are
// combined in ascending order with the same strict test, so the first maximum wins and a NaN never does.
//
// Sweep: one work-group per segment, all segments in one launch, longest first; positions are sequential.  A work-group is P parts of S
// threads: thread (k, part) reduces its S / P values of l for target state k, the P partial pairs meet in LDS, the threads of part 0
// combine them, add the emission and store V_u[k] (LDS, double-buffered) and bp_u[k] (one or two bytes).  Up to 192 states the thread's
// slice of la lives in registers (k_vit_sweep_reg); beyond, la is streamed from memory, consecutive k consecutive doubles
// (k_vit_sweep_mem; with 1024 states P = 1 and a position costs one barrier).  Padded states carry -inf and can never win.  Observations
// are read eight bins at a time, one word ahead.
//
// Backtrace: no pointer chase through memory longer than a tile ("vit_tile" bins).
//   A  k_vit_maps     per tile, one thread per state follows the back-pointers from the tile's last bin to the last bin of the tile below:
//                     the tile's map.  Rows are staged through LDS a block at a time (their addresses do not depend on the state)
//   B  k_vit_compose  per segment, the maps are composed from the top tile down: the path's state at every tile's last bin
//   C  k_vit_path     per tile, one walk from that state writes the path: rows staged through LDS, one lane chases inside LDS, the whole
//                     work-group writes the block's states out
// Everything is stored with ordinary vector stores.
#include "psmc_hip_internal.h"

namespace psmc {

namespace {

constexpr int VIT_STAGE_BYTES = 32768; // LDS a backtrace work-group stages rows in
constexpr int VIT_WAIT_VMCNT0 = 0x0F70; // s_waitcnt vmcnt(0) alone on gfx9: vmcnt = 0 (bits 3:0 and 15:14), expcnt = 7, lgkmcnt = 15

// the end of a sweep (one thread): khmm.c's rule over V_L, the lowest state among equal maxima
__device__ void vit_finish(const double *V, int S, int seg, bool bad, double *score, int32_t *end_state, int32_t *bad_out)
{
	double m = -1e300;
	int arg = -1;
	for (int k = 0; k < S; ++k) {
		const double c = V[k];
		if (m < c) { m = c; arg = k; }
	}
	score[seg] = m;
	end_state[seg] = arg < 0 ? 0 : arg;
	if (bad || arg < 0) bad_out[seg] = 1;
}

// ---- the sweep, la in registers: S in {64, 128, 192}, P parts of S threads
template <int S, int P, typename BP>
__global__ __launch_bounds__(S *P) void k_vit_sweep_reg(const double *__restrict__ la_g, const double *__restrict__ le, const double *__restrict__ l0,
                                                        const uint8_t *__restrict__ obs, const VitSeg *__restrict__ segs, int n, BP *__restrict__ bp,
                                                        double *__restrict__ score, int32_t *__restrict__ end_state, int32_t *__restrict__ bad_out)
{
	constexpr int CH = S / P;
	static_assert(S % P == 0, "parts of equal size");
	__shared__ double V[2][S];
	__shared__ double pm[P][S];
	__shared__ int pa[P][S];
	__shared__ int s_bad;
	const int t = threadIdx.x, k = t % S, part = t / S, l_first = part * CH;
	const VitSeg sg = segs[blockIdx.x];
	double la[CH];
#pragma unroll
	for (int j = 0; j < CH; ++j) la[j] = la_g[(size_t)(l_first + j) * S + k];
	const double e0 = le[k], e1 = le[S + k], e2 = le[2 * S + k];
	if (t == 0) s_bad = 0;
	ObsAhead o(obs + sg.obs_off, sg.L);
	BP *row = bp ? bp + (size_t)sg.row_off * S : nullptr;
	bool bad = false;
	{
		const int sym = (int)(o.cur & 3);
		if (part == 0) V[1][k] = (sym == 0 ? e0 : sym == 1 ? e1 : e2) + l0[k];
	}
	// every load of the prologue has landed before the loop: inside it the only memory operation left on the vector memory counter
	// is the back-pointer store, and nothing waits for that (left to itself the compiler waits for these registers at their first
	// use inside the loop, and such a wait also waits for the stores of the positions before: 0.80 -> 0.74 us per bin at 64 states)
	__builtin_amdgcn_s_waitcnt(VIT_WAIT_VMCNT0);
	__syncthreads();
	for (int u = 2; u <= sg.L; ++u) {
		const int b = (u - 1) & 7;
		if (b == 0) o.advance();
		const int sym = (int)((o.cur >> (8 * b)) & 3);
		const double *Vp = V[(u - 1) & 1];
		double m = -1e300;
		int arg = -1;
#pragma unroll
		for (int j = 0; j < CH; ++j) {
			const double c = Vp[l_first + j] + la[j];
			if (m < c) { m = c; arg = l_first + j; }
		}
		if (P > 1) {
			pm[part][k] = m;
			pa[part][k] = arg;
			__syncthreads();
		}
		if (part == 0) {
			double pq[P];
			int qw = 0;
#pragma unroll
			for (int q = 1; q < P; ++q) pq[q] = pm[q][k]; // (independent reads: one round trip)
#pragma unroll
			for (int q = 1; q < P; ++q)
				if (m < pq[q]) { m = pq[q]; qw = q; }
			if (qw) arg = pa[qw][k];
			V[u & 1][k] = (sym == 0 ? e0 : sym == 1 ? e1 : e2) + m;
			if (row) row[(size_t)(u - 1) * S + k] = (BP)(arg < 0 ? 0 : arg);
			bad = bad || (arg < 0 && k < n);
		}
		__syncthreads();
	}
	if (bad) s_bad = 1;
	__syncthreads();
	if (t == 0) vit_finish(V[sg.L & 1], S, sg.seg, s_bad != 0, score, end_state, bad_out);
}

// ---- the sweep, la streamed: any S (a multiple of 64, up to 1024), P = 1024 / S parts of S threads.  Dynamic LDS:
// V [2][S] doubles | pm [P][S] doubles | pa [P][S] ints
template <typename BP>
__global__ __launch_bounds__(1024) void k_vit_sweep_mem(const double *__restrict__ la_g, const double *__restrict__ le, const double *__restrict__ l0,
                                                        const uint8_t *__restrict__ obs, const VitSeg *__restrict__ segs, int n, int S, int P,
                                                        BP *__restrict__ bp, double *__restrict__ score, int32_t *__restrict__ end_state,
                                                        int32_t *__restrict__ bad_out)
{
	extern __shared__ double vit_lds[];
	double *V = vit_lds, *pm = vit_lds + 2 * S;
	int *pa = (int *)(pm + (size_t)P * S);
	__shared__ int s_bad;
	const int t = threadIdx.x, k = t % S, part = t / S;
	const int CH = (n + P - 1) / P;                  // the padded states beyond n hold -inf: nobody looks at them
	const int l_first = part * CH, l_end = min(n, l_first + CH);
	const VitSeg sg = segs[blockIdx.x];
	const double e0 = le[k], e1 = le[S + k], e2 = le[2 * S + k];
	if (t == 0) s_bad = 0;
	ObsAhead o(obs + sg.obs_off, sg.L);
	BP *row = bp ? bp + (size_t)sg.row_off * S : nullptr;
	bool bad = false;
	{
		const int sym = (int)(o.cur & 3);
		if (part == 0) V[S + k] = (sym == 0 ? e0 : sym == 1 ? e1 : e2) + l0[k];
	}
	__builtin_amdgcn_s_waitcnt(VIT_WAIT_VMCNT0); // (as in k_vit_sweep_reg: the emission registers are there before the loop)
	__syncthreads();
	for (int u = 2; u <= sg.L; ++u) {
		const int b = (u - 1) & 7;
		if (b == 0) o.advance();
		const int sym = (int)((o.cur >> (8 * b)) & 3);
		const double *Vp = V + ((u - 1) & 1) * S;
		const double *lap = la_g + (size_t)l_first * S + k;
		double m = -1e300;
		int arg = -1;
		int l = l_first;
		for (; l + 16 <= l_end; l += 16, lap += 16 * (size_t)S) { // sixteen loads in flight
			double av[16];
#pragma unroll
			for (int j = 0; j < 16; ++j) av[j] = lap[j * (size_t)S];
#pragma unroll
			for (int j = 0; j < 16; ++j) {
				const double c = Vp[l + j] + av[j];
				if (m < c) { m = c; arg = l + j; }
			}
		}
		for (; l + 4 <= l_end; l += 4, lap += 4 * (size_t)S) {
			const double a0 = lap[0], a1 = lap[S], a2 = lap[2 * (size_t)S], a3 = lap[3 * (size_t)S];
			const double c0 = Vp[l] + a0, c1 = Vp[l + 1] + a1, c2 = Vp[l + 2] + a2, c3 = Vp[l + 3] + a3;
			if (m < c0) { m = c0; arg = l; }
			if (m < c1) { m = c1; arg = l + 1; }
			if (m < c2) { m = c2; arg = l + 2; }
			if (m < c3) { m = c3; arg = l + 3; }
		}
		for (; l < l_end; ++l, lap += S) {
			const double c = Vp[l] + lap[0];
			if (m < c) { m = c; arg = l; }
		}
		if (P > 1) {
			pm[part * S + k] = m;
			pa[part * S + k] = arg;
			__syncthreads();
		}
		if (part == 0) {
			for (int q = 1; q < P; ++q) {
				const double c = pm[q * S + k];
				if (m < c) { m = c; arg = pa[q * S + k]; }
			}
			V[(u & 1) * S + k] = (sym == 0 ? e0 : sym == 1 ? e1 : e2) + m;
			if (row) row[(size_t)(u - 1) * S + k] = (BP)(arg < 0 ? 0 : arg);
			bad = bad || (arg < 0 && k < n);
		}
		__syncthreads();
	}
	if (bad) s_bad = 1;
	__syncthreads();
	if (t == 0) vit_finish(V + (sg.L & 1) * S, S, sg.seg, s_bad != 0, score, end_state, bad_out);
}

// rows [r0, r0 + nb) of the table into LDS, four bytes per thread and turn (a row is a multiple of 64 bytes)
template <typename BP> __device__ void vit_stage(const BP *__restrict__ bp, int64_t r0, int nb, int S, BP *buf)
{
	const uint32_t *src = (const uint32_t *)(bp + (size_t)r0 * S);
	uint32_t *dst = (uint32_t *)buf;
	const int words = (int)((size_t)nb * S * sizeof(BP) / 4);
	for (int i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
}

// ---- pass A: S threads per tile; nothing to do for a segment's first tile
template <typename BP>
__global__ __launch_bounds__(1024) void k_vit_maps(const BP *__restrict__ bp, const VitTile *__restrict__ tiles, int S, int R, uint16_t *__restrict__ map)
{
	extern __shared__ double vit_lds[];
	BP *buf = (BP *)vit_lds;
	const VitTile tl = tiles[blockIdx.x];
	if (tl.lo == 1) return;
	int s = threadIdx.x;
	for (int top = tl.hi; top >= tl.lo; top -= R) {
		const int nb = min(R, top - tl.lo + 1), first = top - nb + 1; // positions first..top: rows first - 1 .. top - 1
		vit_stage(bp, tl.row_off + first - 1, nb, S, buf);
		__syncthreads();
		for (int r = nb - 1; r >= 0; --r) s = buf[r * S + s];
		__syncthreads();
	}
	map[(size_t)blockIdx.x * S + threadIdx.x] = (uint16_t)s;
}

// ---- pass B: one thread per segment
__global__ void k_vit_compose(const int32_t *__restrict__ seg_tile0, const int32_t *__restrict__ seg_nt, const int32_t *__restrict__ end_state,
                              const uint16_t *__restrict__ map, int n_seg, int S, int32_t *__restrict__ tile_end)
{
	const int seg = blockIdx.x * blockDim.x + threadIdx.x;
	if (seg >= n_seg) return;
	const int t0 = seg_tile0[seg], nt = seg_nt[seg];
	int s = end_state[seg];
	tile_end[t0 + nt - 1] = s;
	for (int j = nt - 1; j >= 1; --j) {
		s = map[(size_t)(t0 + j) * S + s];
		tile_end[t0 + j - 1] = s;
	}
}

// ---- pass C: 256 threads per tile
template <typename BP>
__global__ __launch_bounds__(256) void k_vit_path(const BP *__restrict__ bp, const VitTile *__restrict__ tiles, const int32_t *__restrict__ tile_end, int S,
                                                  int R, int32_t *__restrict__ path)
{
	extern __shared__ double vit_lds[];
	BP *buf = (BP *)vit_lds;
	int32_t *sb = (int32_t *)((char *)vit_lds + VIT_STAGE_BYTES); // [R]
	const VitTile tl = tiles[blockIdx.x];
	int s = tile_end[blockIdx.x];
	for (int top = tl.hi; top >= tl.lo; top -= R) {
		const int nb = min(R, top - tl.lo + 1), first = top - nb + 1;
		vit_stage(bp, tl.row_off + first - 1, nb, S, buf);
		__syncthreads();
		if (threadIdx.x == 0)
			for (int r = nb - 1; r >= 0; --r) {
				sb[r] = s;
				if (first + r > 1) s = buf[r * S + s]; // (row 0 of a segment holds nothing)
			}
		__syncthreads();
		for (int r = threadIdx.x; r < nb; r += blockDim.x) path[tl.row_off + first - 1 + r] = sb[r];
		__syncthreads();
	}
}

// the backtrace over one table of [bins][S] entries: passes A, B, C from v.end_state to v.path
template <typename BP> int launch_backtrace_t(const VitLaunch &v)
{
	const int S = v.S;
	const BP *bp = (const BP *)v.bp;
	const int R = VIT_STAGE_BYTES / (S * (int)sizeof(BP)); // 16 rows at 1024 states, 512 at 64
	k_vit_maps<BP><<<v.n_tiles, S, VIT_STAGE_BYTES, v.stream>>>(bp, v.tiles, S, R, v.map);
	if (v.ev[2]) (void)hipEventRecord(v.ev[2], v.stream);
	k_vit_compose<<<(v.n_seg + 63) / 64, 64, 0, v.stream>>>(v.seg_tile0, v.seg_nt, v.end_state, v.map, v.n_seg, S, v.tile_end);
	if (v.ev[3]) (void)hipEventRecord(v.ev[3], v.stream);
	k_vit_path<BP><<<v.n_tiles, 256, VIT_STAGE_BYTES + sizeof(int32_t) * R, v.stream>>>(bp, v.tiles, v.tile_end, S, R, v.path);
	if (v.ev[4]) (void)hipEventRecord(v.ev[4], v.stream);
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <typename BP> int launch_viterbi_t(const VitLaunch &v)
{
	const int S = v.S;
	BP *bp = (BP *)v.bp;
	if (v.ev[0]) (void)hipEventRecord(v.ev[0], v.stream);
#define VIT_ARGS v.la, v.le, v.l0, v.obs, v.segs, v.n, bp, v.score, v.end_state, v.bad
	if (S == 64) k_vit_sweep_reg<64, 8, BP><<<v.n_seg, 512, 0, v.stream>>>(VIT_ARGS);
	else if (S == 128) k_vit_sweep_reg<128, 8, BP><<<v.n_seg, 1024, 0, v.stream>>>(VIT_ARGS);
	else if (S == 192) k_vit_sweep_reg<192, 4, BP><<<v.n_seg, 768, 0, v.stream>>>(VIT_ARGS);
	else {
		const int P = 1024 / S;
		const size_t lds = sizeof(double) * 2 * S + (sizeof(double) + sizeof(int)) * (size_t)P * S;
		k_vit_sweep_mem<BP><<<v.n_seg, P * S, lds, v.stream>>>(v.la, v.le, v.l0, v.obs, v.segs, v.n, S, P, bp, v.score, v.end_state, v.bad);
	}
#undef VIT_ARGS
	if (v.ev[1]) (void)hipEventRecord(v.ev[1], v.stream);
	if (bp) return launch_backtrace_t<BP>(v);
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace

int launch_viterbi(const VitLaunch &v)
{
	return v.wide_bp ? launch_viterbi_t<uint16_t>(v) : launch_viterbi_t<uint8_t>(v);
}

int launch_vit_backtrace(const VitLaunch &v)
{
	return v.wide_bp ? launch_backtrace_t<uint16_t>(v) : launch_backtrace_t<uint8_t>(v);
}

} // namespace psmc
