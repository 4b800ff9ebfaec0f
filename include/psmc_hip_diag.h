/* psmc_hip_diag.h -- C-ABI of libpsmc_hip_diag.so: the lab bench of the MI355X PSMC E-step (device self-test,
 * instruction microbenchmarks, pipe / placement / HBM probes, per-kernel HIP-event timing of the last E-step).
 *
 * NOT part of the drop-in boundary: a maintainer of lh3/psmc links libpsmc_hip.so (include/psmc_hip.h) only.  This
 * library exists for tests/, bench.py's roofline figures and the measurements DESIGN.md cites; it links against
 * libpsmc_hip.so and is built from the same tree (psmc_amd/csrc/Makefile), so it may look inside a context.
 * Every function returns 0 (or what it documents) or a negative PSMC_HIP_E* code of psmc_hip.h.
 */
#ifndef PSMC_HIP_DIAG_H
#define PSMC_HIP_DIAG_H
#include "psmc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Built-in check of the cross-lane primitives on the device (row replication
 * variants, DPP broadcasts, f64 MFMA layout).  Returns 0 when all agree;
 * a positive bitmask of failed primitives otherwise. */
int psmc_hip_selftest(int device);

/* Diagnostic: shader cycles per operation of the FP64 building blocks (dependent
 * and independent v_fmac_f64_dpp chains, row replication, f64 MFMA ...), one
 * wave; see psmc_amd/csrc/microbench.hip for the meaning of out[0..13]. */
int psmc_hip_microbench(int device, double *out, int n);

/* Diagnostic: do the f64 matrix instructions of one wave overlap with the f64 vector instructions of another wave
 * on the same SIMD?  One work-group on one CU, waves go to its four SIMDs round robin; a "matrix wave" issues 64
 * v_mfma_f64_16x16x4 per round, a "vector wave" 1024 v_fma_f64 (8 chains) -- ~4100 cycles of issue either way.
 * out[8*c + w] = shader cycles per round of wave w in configuration c (0 where the configuration has no wave w):
 *   c=0: 4 matrix waves (one per SIMD)      c=1: 4 vector waves         c=2: 8 matrix waves (two per SIMD)
 *   c=3: 8 vector waves                     c=4: waves 0-3 matrix, 4-7 vector (one of each per SIMD)
 *   c=5: even waves matrix, odd waves vector (SIMDs 0 and 2 hold two matrix waves, 1 and 3 two vector waves).
 * Separate pipes would give c=4 the times of c=0 / c=1; one shared pipe gives it their sum.  n >= 48. */
#define PSMC_HIP_PIPE_PROBE_CONFIGS 6
int psmc_hip_pipe_probe(int device, double *out, int n);

/* Diagnostic, second edition of the pipe probe: which instructions of one wave overlap with another wave's
 * v_mfma_f64 on the same SIMD?  One work-group of up to 8 waves on one CU (wave w -> SIMD w % 4); kinds8[w] says what
 * wave w issues per round (~4 k cycles of issue when alone): 0 idle, 1 v_mfma_f64_16x16x4 x 64, 2 v_fma_f64 x 1024,
 * 3 v_mov_b32_dpp x 1024, 4 DPP scan levels (2 v_mov_b32_dpp + v_add_f64, as the sweeps' row scans) ~ 1024 in all,
 * 5 ds_read_b128 x 512, 6 s_load_dwordx4 x 256 + v_readlane_b32 x 512, 7 v_add_u32 x 1024, 8 v_fma_f32 x 1024,
 * 9 v_add_f64 x 1024.  out8[w] = shader cycles per round of wave w (0 for idle waves). */
int psmc_hip_pipe_probe2(int device, const int *kinds8, int rounds, double *out8);

/* Diagnostic: where do the waves of a launch smaller than the device land?  n_kernels (1..4) launches of n_waves waves
 * of the structured sweep step (no memory traffic), in work-groups of waves_per_block (1..4) waves, side by side on
 * streams of their own.  out[3*(k*n_waves_padded + w) + 0..2] = shader cycles per step of wave w of launch k, its
 * HW_ID register (SIMD bits 5:4, CU 11:8, SH 12, SE 15:13) and its XCC_ID; n_waves_padded = n_waves rounded up to a
 * multiple of waves_per_block.  *ms_out = the slowest launch.  A shard-sized E-step has fewer waves than the device
 * has SIMDs: if they are stacked on the same SIMDs, every step costs a multiple of its latency. */
int psmc_hip_place_probe(int device, int n_waves, int waves_per_block, int n_kernels, int steps, double *out, double *ms_out);

/* Diagnostic: an 8-byte-per-lane streaming copy (reads and writes 8*n_doubles bytes, 5
 * launches) to calibrate the rocprofv3 FETCH_SIZE / WRITE_SIZE counters for the access
 * width the kernels use; *ms_out = average duration of one launch. */
int psmc_hip_stream_probe(int device, long long n_doubles, double *ms_out);

/* Diagnostic: what plain streaming kernels reach on this device with 16-byte accesses over two
 * buffers of `bytes` each: gbps_out[0] fill, [1] read, [2] copy (read + write), [3] the store
 * pattern of the structured sweeps (four 512-byte-per-step streams per wave).  GB/s. */
int psmc_hip_hbm_probe(int device, long long bytes, double *gbps_out);

/* Diagnostic: the structured sweep step (no memory traffic) on n_waves wavefronts at once, `steps`
 * steps each: out[0] kernel ms, [1] mean / [2] max shader cycles per step of a wave, [3] mean shader
 * clock in MHz the waves saw -- how far FP64 issue and clocks hold up when the whole device is busy.
 */
int psmc_hip_load_probe(int device, int n_waves, int steps, double *out);

/* Diagnostic: psmc_hip_load_probe with the table stores of a forward sweep: each wave appends 512 bytes per tile and
 * step during the last `store_steps` of its `steps` steps.  mode 1: two 16-byte stores per lane and step (what
 * k_fwd_struct does), 2: the same bytes written as 2 KB per tile every 4th step.  out[0..3] as psmc_hip_load_probe,
 * out[4] = GB/s of the stores over the whole kernel. */
int psmc_hip_load_probe_st(int device, int n_waves, int steps, int store_steps, int mode, double *out);

/* Wall time in ms of the last E-step measured with HIP events on the streams the
 * kernels ran on.  Exact mode: [0] total, [1] forward, [2] backward, [3] expect,
 * [4] host-copy tail.  Fast mode: [0] total, [1] both sweep chains (speculate +
 * repair rounds; forward and backward run concurrently), [2] LL + redo of the
 * counts after the chains, [3] the full expect kernel alone (fused back half: its one or two
 * launches, summed), [4] reductions, [5] the
 * speculative forward sweep kernel alone, [6] the speculative backward sweep alone. */
int psmc_hip_last_timing(psmc_hip_ctx *ctx, double ms[7]);

/* Diagnostic: do HIP's per-stream compute-unit masks (hipExtStreamCreateWithCUMask) partition the device?  Stream A gets
 * the first n_cus_a compute units of the mask's bit order, stream B the others; n_waves_a / n_waves_b one-wave work-groups of
 * the structured sweep step (no memory traffic) run on them at the same time.  out[3*w + 0..2] = shader cycles per step,
 * HW_ID and XCC_ID of wave w (A's waves first, then B's, as psmc_hip_place_probe); *ms_out = the slower launch.
 * n_cus_a = 0: no masks (both streams see the whole device).  psmc_boot keeps its main run out of the bootstrap
 * batch's way like this (psmc_amd/host/boot.c). */
int psmc_hip_cumask_probe(int device, int n_cus_a, int n_waves_a, int n_waves_b, int steps, double *out, double *ms_out);

/* Diagnostic: the tiles of the current fast plan (up to 128 states), as the planner classified them ("gap_tiles", "hom_tiles" of
 * psmc_hip.h).  Returns the number of tiles of the plan -- PSMC_HIP_ESTATE when there is none, as psmc_hip_fast_plan -- and fills the
 * first `cap` entries: cls[b] = 0, 1 = gap tile (a full tile of missing data inside its segment), 2 = hom tile (a full het-free tile
 * inside its segment) outside a qualifying run, 3 = hom tile of a qualifying run; glue[b] = bit 0: tile b continues the forward item
 * of tile b - 1, bit 1: it continues the backward item of tile b + 1 -- what the plan rules set and what the context has learned
 * since.  The plan of the wide fast path (129..1024 states, "wide_fast") is a different one: psmc_hip_wide_plan_tiles below. */
int psmc_hip_plan_tiles(psmc_hip_ctx *ctx, int32_t *cls, int32_t *glue, int cap);

/* Diagnostic: the tiles of the current plan of the wide fast path ("wide_fast", 129..1024 states), as "wide_gap_tiles" of psmc_hip.h
 * classified them.  Returns the number of tiles of the plan -- PSMC_HIP_ESTATE when there is none (no wide fast E-step since load /
 * select / an option that changes the plan) -- and fills the first `cap` entries: cls[b] = 0, 1 = gap tile (a full tile of missing
 * data, neither first nor last in its segment) outside a qualifying run, 2 = gap tile of a qualifying run; glue[b] = bit 0: glued
 * forward (the tile does not speculate: its start vector comes from the transfer-matrix chain across the run, or from the walk
 * behind it), bit 1: glued backward.  With "wide_hom_tiles" = 1 also 3 = hom tile (a full tile of
 * homozygous bins only, neither first nor last in its segment) outside a qualifying run, 4 = hom tile of a qualifying run.  With
 * "wide_mix_tiles" = 1 beside it also 5 = mix tile (a full het-free tile with both homozygous and missing bins, neither first nor
 * last in its segment) outside a qualifying run, or over "wide_mix_mb", 6 = mix tile of a qualifying run.  All zero
 * with "wide_gap_tiles" = 0 and "wide_hom_tiles" = 0. */
int psmc_hip_wide_plan_tiles(psmc_hip_ctx *ctx, int32_t *cls, int32_t *glue, int cap);

/* Diagnostics of "wide_gap_tiles" (psmc_hip.h): what the planner made of the qualifying runs and what the last wide fast E-step did
 * with it.  Host reads and plain device-to-host copies behind a synchronise of the context's stream; none launches a kernel.  All
 * of them return PSMC_HIP_ESTATE under the condition of psmc_hip_wide_plan_tiles (no current wide plan).
 *
 * psmc_hip_wide_gap_chains: the transfer-matrix chains of the current plan in direction dir (0 forward, 1 backward), in the order
 * they are launched (level by level).  Returns their number and fills the first `cap` entries: first[i] = the tile whose start
 * vector the chain copies from its neighbour's exit vector (the run's first tile in sweep order that is not anchored in that
 * direction), count[i] = applications of the matrix (the tiles first + 1 .. first + count forward, first - 1 .. first - count
 * backward; 0: every tile of the run is anchored, only the walk hangs on the chain), walk[i] = the tile its walk starts on (the
 * last tile the chain writes), level[i] = 0, or one more than the chain before it in the segment when its first vector comes out
 * of that chain's walk.  0 chains with "wide_gap_tiles" = 0 or without a qualifying run.
 *
 * psmc_hip_wide_gap_rechained: out[0] forward, out[1] backward: chains the repair rounds of the last wide fast E-step ran again (a
 * run whose first chained tile headed a failing run), summed over the rounds.
 *
 * psmc_hip_wide_gap_matrix: the transfer matrix of one full tile of missing data as the last wide fast E-step built it, n rows of
 * the padded width (192 or 256 up to 256 states, the next multiple of 256 beyond): row k = the unit vector of state k swept T
 * bins forward.  Returns the number of doubles and copies the first `cap`; PSMC_HIP_ESTATE when that E-step built none.
 *
 * psmc_hip_wide_hom_matrix ("wide_hom_tiles"): the matrix of one full tile of T homozygous bins as the last wide fast E-step built it,
 * n rows of the padded width -- row k = the unit vector of state k swept T bins forward under symbol 0 with the pilot's power-of-two
 * factors -- followed by those ceil(T / 4) factors (factor j was applied at bin 4 j of the tile, counted from 0): dividing every
 * entry by their product gives the unscaled matrix.  Returns the number of doubles, n x width + ceil(T / 4), and copies the first
 * `cap`; PSMC_HIP_ESTATE when that E-step built none (no qualifying run with a hom tile).  A chain applies it across the tiles of
 * class 4: forward v <- v M_h, backward v <- D M_h D^-1 v with D = diag(e0), normalised to sum 1 after every application.
 *
 * psmc_hip_wide_mix_matrix ("wide_mix_tiles"): one of the two matrices of the mix tile `tile` (class 6) as the last wide fast E-step
 * built it -- dir 0: F, row k = the unit vector of state k swept forward through the tile's own symbols; dir 1: B, row k = the unit
 * vector times the first bin's emission swept forward through the symbols from the second bin on and one missing bin -- n rows of the
 * padded width, on the scale of that direction's pilot, followed by the pilot's ceil(T / 4) factors.  Returns the number of doubles,
 * n x width + ceil(T / 4), and copies the first `cap`; PSMC_HIP_ESTATE when that E-step built none, PSMC_HIP_EINVAL for a tile that is
 * not class 6 or a dir that is not 0 or 1.  A matrix is built where a chain of the plan crosses the tile in that direction
 * (psmc_hip_wide_gap_chains: the tiles first, first +- 1, ... of a chain, `count` of them); for a class-6 tile that is anchored in
 * the direction, or whose run has no chain, there is none: PSMC_HIP_ESTATE.  A chain applies them across the tile: forward v <- v F, backward v <- B v, normalised.
 *
 * psmc_hip_wide_tile_vectors: every tile's start vector after the last wide fast E-step, forward (which = 0: entry) or backward
 * (which = 1: bentry), tiles x the padded width.  Returns the number of doubles and copies the first `cap`. */
int psmc_hip_wide_gap_chains(psmc_hip_ctx *ctx, int dir, int32_t *first, int32_t *count, int32_t *walk, int32_t *level, int cap);
int psmc_hip_wide_gap_rechained(psmc_hip_ctx *ctx, int out[2]);
int64_t psmc_hip_wide_gap_matrix(psmc_hip_ctx *ctx, double *M, int64_t cap);
int64_t psmc_hip_wide_hom_matrix(psmc_hip_ctx *ctx, double *M, int64_t cap);
int64_t psmc_hip_wide_mix_matrix(psmc_hip_ctx *ctx, int tile, int dir, double *out, int64_t cap);
int64_t psmc_hip_wide_tile_vectors(psmc_hip_ctx *ctx, int which, double *out, int64_t cap);

/* Diagnostics of the transfer-matrix chains of the fast path up to 128 states (the glued runs of the structured plan: learned runs,
 * "gap_tiles", "hom_tiles"): what the list builder made of the runs and what the last fast E-step (psmc_hip_estep, _factored, _device)
 * left behind.  Host reads and plain device-to-host copies behind a synchronise of the context's stream; none launches a kernel.  All
 * four return PSMC_HIP_ESTATE when there is no current fast plan with built item lists (no successful structured fast E-step of at
 * most 128 states since load / select / an option that changes the plan).  S below is the padded state count: 64, or 128 beyond 64.
 *
 * psmc_hip_fast_chain_info: out[0], out[1] = chained runs forward, backward; out[2] = KcTiles (one per matrix application of any
 * chain); out[3] = matrix slots; out[4] = step ranges per tile in use ("kc_sub" as planned at S = 64, 1 at S = 128); out[5] = S;
 * out[6] = tiles of the plan; out[7] = the tile length.
 *
 * psmc_hip_fast_chain_list: returns the length in ints of list `which` and copies the first `cap`:
 *   0  the chained runs in launch order, forward ones first: (first, count, kc0, 0) each -- the chain starts from the start vector of
 *      tile `first` (forward) or first + count - 1 (backward), which a walk leaves, and writes the start vectors of the run's other
 *      count - 1 tiles; kc0 = index of the run's first KcTile;
 *   1  the KcTiles (tile, dir) each, dir 0 forward, 1 backward: the tile whose steps application j of a chain crosses;
 *   2  kslot[j]: the matrix slot of KcTile j (the gap tiles of a direction share one, and so do the all-homozygous tiles of the
 *      qualifying runs of "hom_tiles", when the tile length is a multiple of four);
 *   3  kuniq[u]: the KcTile slot u's matrices are computed from.
 *
 * psmc_hip_fast_chain_matrices: slots x ranges matrices of S x S doubles, then slots x ranges x S exponents, as the last E-step left
 * them: element [(j * S + col) * S + k], j = slot * ranges + range, is state k of the unit vector of state `col` after the range's
 * steps, scaled by 2^-exponent[j * S + col].  Returns the number of doubles (0 without a chain) and copies the first `cap`.
 *
 * psmc_hip_fast_tile_vectors: which = 0 entry (forward start vectors, proportional to X at lo - 1), 1 bentry (backward start vectors,
 * proportional to bt at min(hi, L - 1) + 1), 2 bexit (backward exit vectors), tiles x S each, after the last E-step.  The entry of a
 * segment's first tile is never written (position 1 is an initial condition).  Returns the number of doubles and copies the first
 * `cap`. */
int psmc_hip_fast_chain_info(psmc_hip_ctx *ctx, int out[8]);
int psmc_hip_fast_chain_list(psmc_hip_ctx *ctx, int which, int32_t *out, int cap);
int64_t psmc_hip_fast_chain_matrices(psmc_hip_ctx *ctx, double *out, int64_t cap);
int64_t psmc_hip_fast_tile_vectors(psmc_hip_ctx *ctx, int which, double *out, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif
