/* psmc_hip.h -- C-ABI of libpsmc_hip.so: the PSMC E-step (Baum-Welch
 * forward-backward + expected counts) on AMD MI355X (gfx950).
 *
 * The reference (lh3/psmc) has no plugin/FFI seam; its E-step is the body of
 * psmc_em(), em.c:33-55, which calls khmm.h:64-92 per segment:
 *     hmm_pre_backward, hmm_new_data, hmm_forward, hmm_backward, hmm_lk,
 *     hmm_expect, hmm_add_expect
 * and psmc_decode(), aux.c:150-158, which re-runs forward/backward.  Because
 * the f/b tables must stay in HBM, the drop-in boundary sits one level up: a
 * batch E-step over all loaded segments.  Each entry point below names the
 * reference code it replaces.  Plain C types only; every function returns 0 or
 * a negative PSMC_HIP_E* code, never aborts, never prints.
 *
 * Conventions: n = number of hidden states (psmc's n+1; <= PSMC_HIP_MAX_STATES = 1024.  Up to 64: every kernel; 65..128:
 * fast mode runs the structured sweeps for matrices of the PSMC form and psmc_hip_estep falls back to the exact kernels for
 * any other matrix; 129..1024 (`psmc -p "100*2"`): the wide exact kernels of estep_wide.hip whatever the mode -- psmc_hip_estep,
 * _estep_segments, _estep_batch, the table readers and the decoding entry points; the device-resident and factored fast entry
 * points return PSMC_HIP_ENOTSUP there, except that with the option "wide_fast" = 1 or 2 a fast-mode context of 129..256 states
 * runs psmc_hip_estep_factored and _estep_factored_device on the fast kernels of estep_wide_fast.hip, and with "wide_fast" = 2 one
 * of 257..1024 states runs them on the same kernels with 2..4 waves per tile (PSMC-form matrices; psmc_hip_get_tables stays
 * exact; so do the full counts of psmc_hip_estep unless "wide_counts" = 1 is set as well -- then A comes from that E-step's tables
 * through a GEMM on the FP64 matrix cores, estep_wide_counts.hip; so does the batch unless "wide_batch" = 1 is set as well -- see psmc_hip_estep_batch --
 * and so does decoding unless "wide_decode" = 1 is -- beyond 256 states together with "wide_fast" = 2: see "Decoding on a FAST context";
 * the path's forward table X takes 8 x (192, 256, 512, 768 or 1024) bytes per bin, with the option "wide_ckpt" = 1 an eighth of that);
 * row-major FP64; a[k*n+l]=P(k->l) (khmm.h:34); e[b*n+k], b=0 hom / 1 het
 * (khmm.h:34; the missing-data row e[2][*]=1 of khmm.c:21 is implied);
 * a0[k] (khmm.h:36); observations are bytes 0/1/2 exactly as psmc_read_seq
 * decodes them (cli.c:15-32,117-125), 0-indexed as in psmc_seq_t (psmc.h:22-26).
 */
#ifndef PSMC_HIP_H
#define PSMC_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PSMC_HIP_MODE_EXACT 0 /* bit-identical to khmm.c (ordered sums, no FMA) */
#define PSMC_HIP_MODE_FAST  1 /* tiled speculative sweeps, FMA/MFMA, tree reductions; stats within 1e-10 */

#define PSMC_HIP_MAX_STATES 1024 /* exact mode; the fast kernels cover up to 128 states (beyond: a fast-mode context runs the exact ones),
                                    and the factored statistics up to 256 with the option "wide_fast" = 1, up to 1024 with "wide_fast" = 2;
                                    with "wide_decode" = 1 the decoding entry points read such an E-step's tables at the same sizes */

#define PSMC_HIP_OK        0
#define PSMC_HIP_EINVAL   -1 /* bad argument (NULL, n out of range, empty segment ...) */
#define PSMC_HIP_ENOMEM   -2 /* host or device allocation failed */
#define PSMC_HIP_EDEVICE  -3 /* HIP runtime error; see psmc_hip_last_error() */
#define PSMC_HIP_ENOTSUP  -4 /* not supported in this build (n > 1024; the device-resident / factored fast entry points with n > 128 -- the
                                factored ones with n > 256 when "wide_fast" is 1; "wide_fast" = 2 covers them all -- or with n > 64 and a
                                matrix without the PSMC form; psmc_hip_estep never answers it beyond 128 states: where "wide_counts" does
                                not apply it runs the wide exact kernels, and psmc_hip_estep_device beyond 128 states always answers it,
                                "wide_counts" or not; psmc_hip_estep_batch on the wide fast path -- "wide_batch" -- for the reasons
                                psmc_hip_estep_factored has there, the message naming the replicate).  The decoding entry points never
                                answer it beyond 128 states: where they cannot read the wide fast tables ("wide_decode") they read the
                                exact ones */
#define PSMC_HIP_ESTATE   -5 /* call order violated (no segments loaded ...) */
#define PSMC_HIP_ECONVERGE -6 /* fast mode: tile boundaries did not converge within max_rounds */

typedef struct psmc_hip_ctx psmc_hip_ctx;

/* Number of visible HIP devices (0 when none / no driver). */
int psmc_hip_device_count(void);
/* Compute units of a device (256 on an MI355X; 0 on error). */
int psmc_hip_device_cus(int device);

/* Replaces hmm_new_par/hmm_new_exp bookkeeping (khmm.c:10-23, 60-69). */
int psmc_hip_create(psmc_hip_ctx **ctx, int n_states, int device, int mode);
void psmc_hip_destroy(psmc_hip_ctx *ctx);
const char *psmc_hip_strerror(int err);
const char *psmc_hip_last_error(const psmc_hip_ctx *ctx);

/* Options.  None is needed: the defaults are what bench.py and the psmc binary run, and the plan adapts to the input
 * (see "auto").  PSMC_HIP_OPTIONS="key=value,key=value" in the environment sets them for every context of a process.
 * Unknown keys and out-of-range values return PSMC_HIP_EINVAL.  Setting any option drops the per-replicate plans a
 * fast-mode batch has learned.  Exact mode reads only "rep_impl", "batch_bins", "batch_sort", "batch_tailfill", "batch_major" and "exact_refwd" ("batch_first" is accepted and has no effect).
 *
 *  key             default  meaning
 *  --- plan of the fast mode (tiles, speculation) ---------------------------------------------------------------
 *  "chunk"         0        tile length in bins; 0 = auto: two ROUNDS of the fused back half (8192 tiles, one wave per
 *                           SIMD and four tiles per wave in each of two launches) for genome-sized inputs, ONE round
 *                           (4096 tiles, every tile speculating in both directions, one launch) below 8192 x warmup
 *                           bins (25 M) -- a single chromosome, one rank's share of a genome at 2/4/8 GPUs
 *  "warmup"        3072     bins a tile starts outside itself (from the stationary vector) in each direction
 *  "warm_tol"      1e-12    agreement demanded between the vector a tile built on and what its neighbour computed
 *  "max_rounds"    4096     verify / repair rounds before PSMC_HIP_ECONVERGE
 *  "wide_fast"     0        1: a fast-mode context of 129..256 states runs psmc_hip_estep_factored[_device] on the fast kernels of
 *                           estep_wide_fast.hip (one tile per wave, 64 lanes x 3 or 4 states; PSMC-form matrices, else ENOTSUP; more
 *                           than 256 states: ENOTSUP).  It reads "chunk" (0 = about 4096 tiles, at least 256 bins), "warmup" (16384
 *                           bins unless set: shorter warm-ups leave tiles whose repair walks a whole segment), "warm_tol",
 *                           "max_rounds" and "learn" (1: a repair walks on through the failing tiles after it in the same round;
 *                           0: one tile per wave and round); with "structured" = 0 it answers ENOTSUP, as the factored statistics
 *                           do up to 128 states.  It keeps an X table of its own: 8 x 192 or 8 x 256 bytes per bin
 *                           (46 / 61 GB at 30 M bins; with "wide_ckpt" = 1: 192 or 256 bytes per bin, 5.8 / 7.7 GB), beside the exact
 *                           tables.  psmc_hip_estep, psmc_hip_get_tables, the batch (without
 *                           "wide_batch": see psmc_hip_estep_batch) and the decoding entry points (without "wide_decode") stay on the
 *                           exact kernels, bit for bit.  Exact mode and <= 128 states: no effect.
 *                           2: the same at 129..256 states (the same kernels, the same bits as 1), and a fast-mode context of 257..1024
 *                           states runs them on the same kernels of estep_wide_fast.hip: a tile is one work-group of 2, 3 or 4 waves
 *                           (padded widths 512, 768, 1024: 64 lanes x 4 states per wave), the waves exchange their scan totals through
 *                           LDS once per position.  Plan, options, ENOTSUP / ECONVERGE and diagnostics as for 1; the X table is 8 x 512,
 *                           8 x 768 or 8 x 1024 bytes per bin -- 123, 184 or 246 GB at 30 M bins; with "wide_ckpt" = 1: 512, 768 or 1024
 *                           bytes per bin, 15, 23 or 31 GB -- (PSMC_HIP_ENOMEM, with the table's size in the message, when it does
 *                           not fit).  Everything else such a context does stays on the exact kernels -- the batch too, unless
 *                           "wide_batch" = 1 is set as well, and decoding, unless "wide_decode" = 1 is.
 *                           Other values: PSMC_HIP_EINVAL
 *  "wide_decode"   0        1, with "wide_fast" = 1 or 2 on a fast-mode context of 129..256 states, and with "wide_fast" = 2 on one of
 *                           257..1024 states: psmc_hip_decode, _posterior, _post_counts and _scales read what the LAST single E-step
 *                           left -- after a wide fast factored E-step its X table and converged tile boundaries (estep_wide_post.hip; no
 *                           backward table), after psmc_hip_estep the exact tables,
 *                           bit for bit (see "Decoding on a FAST context").  0: the exact tables whatever E-step ran last, as before
 *                           the option existed.  Anywhere else -- exact mode, up to 128 states, beyond 256 states with "wide_fast" = 1
 *                           -- no effect.  (In the one release where "wide_fast" = 2 existed without this, the pair had no effect
 *                           beyond 256 states: a decode after a wide fast E-step read the exact tables of an OLDER E-step, or
 *                           answered ESTATE.)  Other values: PSMC_HIP_EINVAL
 *  "wide_ckpt"     0        1: a wide fast E-step ("wide_fast", at every size it covers: psmc_hip_estep_factored[_device], the wide fast batch
 *                           -- "wide_batch" --, every shard of a psmc_hip_group) keeps X at every 8th position only, plus the last row
 *                           of every tile, and its accumulate sweep recomputes the seven rows between two checkpoints with the forward
 *                           sweep's own arithmetic: the results are the full table's, bit for bit.  The table then takes S bytes per bin
 *                           (S = 192, 256, 512, 768, 1024 padded states) plus 2 x 8 S bytes per tile instead of 8 S bytes per bin:
 *                           7.7 GB instead of 61 GB at 200 states and 30 M bins, 31 GB instead of 246 GB at 1024 states.  The table is
 *                           sized anew when the interval changes between two E-steps of a context (psmc_hip_wide_table_info reports it;
 *                           psmc_hip_fast_info out[5] is 1 after a checkpointed E-step).  "wide_decode" = 1 wins: the decoding kernels
 *                           read full rows, so while it is set a wide fast E-step keeps the full table whatever "wide_ckpt" says
 *                           (PSMC_HIP_ENOMEM as under "wide_fast" when that does not fit; so does a wide-counts E-step -- "wide_counts" --
 *                           unless "wide_counts_ckpt" = 1) -- set "wide_decode" before the one E-step
 *                           that is decoded, and the EM rounds before it run checkpointed -- or set "wide_decode_ckpt" = 1 as well,
 *                           and that E-step keeps checkpoints too.  Without "wide_decode_ckpt", psmc_hip_decode, _posterior,
 *                           _post_counts and _scales after a checkpointed E-step ("wide_decode" set afterwards, no new E-step) answer
 *                           PSMC_HIP_ESTATE.  Exact mode, up to 128 states (their own "ckpt"), "wide_fast" = 0: accepted, no effect.
 *                           Other values: PSMC_HIP_EINVAL
 *  "wide_decode_ckpt" 0     1: decoding from checkpoints.  A wide fast E-step with "wide_ckpt" = 1 keeps checkpoints even while
 *                           "wide_decode" = 1 (interval 8 in psmc_hip_wide_table_info, psmc_hip_fast_info out[5] = 1: the E-step's
 *                           table no longer depends on "wide_decode"), and psmc_hip_decode, _posterior, _post_counts and _scales after
 *                           such an E-step read its checkpoints, the tiles' last rows, 1/d and the tile boundaries: the CKPT kernels of
 *                           estep_wide_post.hip recompute the seven rows between two checkpoints with the
 *                           forward sweep's own arithmetic, block by block as the E-step's accumulate sweep does, and return the bits
 *                           of decoding from the full table.  "wide_decode" may be switched on after that E-step: nothing is re-run.
 *                           The option is read by every decoding call too: back at 0, a call after a checkpointed E-step answers
 *                           PSMC_HIP_ESTATE as before.  A decoding call allocates nothing proportional to bins x S (posterior rows it
 *                           was asked for aside); psmc_hip_post_counts recomputes the rows once per four count columns.  Every other
 *                           state rule of "Decoding on a FAST context" is unchanged.  Without "wide_ckpt", in exact mode, up to 128
 *                           states or with "wide_fast" = 0: accepted, no effect.  Other values: PSMC_HIP_EINVAL
 *  "wide_batch"    0        1: psmc_hip_estep_batch[_cb] of a fast-mode context of 129..1024 states whose size "wide_fast" covers, asked for
 *                           sums and not for A -- with "wide_counts" = 1: for A as well --, runs every replicate on the wide fast path (see
 *                           psmc_hip_estep_batch, "wide fast batch").
 *                           0, and every other context or call: the batch as without the option.  Other values: PSMC_HIP_EINVAL
 *  "wide_counts"   0        1: psmc_hip_estep of a fast-mode context of 129..1024 states whose size "wide_fast" covers (1: up to 256 states,
 *                           2: up to 1024), with "structured" = 1 and a matrix of the PSMC form, returns the full count matrix A from the
 *                           wide fast path: the factored wide E-step as it stands (its sweeps, verify / repair rounds, E and LL, bit for
 *                           bit), then a counts pass (estep_wide_counts.hip): per slab of whole tiles one more backward sweep from the
 *                           converged tile boundaries that writes V_p = mult bt_{p+1} / G_p, then C += X^T V as a split-K GEMM on
 *                           v_mfma_f64_16x16x4 with one owner per partial matrix and no atomics, at the end A = a . C.  A0 = zeros and
 *                           chk = 1.0 as after every fast-mode E-step; PSMC_HIP_ECONVERGE as the factored wide E-step answers it.  The
 *                           result depends on the call's inputs and the options alone -- not on the device, on timing or on earlier
 *                           calls: bit-reproducible.  That E-step keeps the full X table (interval 1) whatever "wide_ckpt" says, as
 *                           "wide_decode" without "wide_decode_ckpt" does -- unless "wide_counts_ckpt" = 1: counts from checkpoints.  Device memory the
 *                           counts pass adds, whatever the number of bins: one slab of V (8 S bytes per slab bin, S = the padded width;
 *                           auto: at most 4 GB, or one tile if that is longer), the partial matrices (at most 64 MB), a and A (8 n^2 bytes each)
 *                           and one slab's row ranges -- plus four bytes per tile of the plan; PSMC_HIP_ENOMEM with the size in the
 *                           message when it does not fit.  Afterwards the E-step is "the last single E-step" exactly as a wide factored
 *                           one is (decoding with "wide_decode", psmc_hip_get_tables: the exact tables stay what they were);
 *                           psmc_hip_fast_info out[4] is 4 ("full counts of the wide path"; 3 after the factored statistics),
 *                           psmc_hip_fast_repairs out[5] stays 2.  In every other case -- the option at 0, exact mode, up to 128 states, a
 *                           matrix without the PSMC form, "structured" = 0, 257+ states with "wide_fast" = 1 -- psmc_hip_estep runs the
 *                           wide exact kernels, bit for bit as without the option.  psmc_hip_estep_device beyond 128 states is not
 *                           covered (PSMC_HIP_ENOTSUP as before); psmc_hip_group_estep reaches the path through its per-shard
 *                           psmc_hip_estep.  With "wide_batch" = 1 the batch returns A this way too (psmc_hip_estep_batch).
 *                           Other values: PSMC_HIP_EINVAL
 *  "wide_counts_ckpt" 0     1: counts from checkpoints.  A wide-counts E-step ("wide_counts": psmc_hip_estep, the wide fast batch asked for A,
 *                           every shard of a psmc_hip_group) with "wide_ckpt" = 1 keeps checkpoints -- X at every 8th position plus every
 *                           tile's last row; interval 8 in psmc_hip_wide_table_info, psmc_hip_fast_info out[5] = 1 -- and the V pass of the
 *                           counts recomputes the seven rows between two checkpoints with the forward sweep's own arithmetic, block by
 *                           block as the accumulate sweep does, and writes the slab's X rows beside its V rows; the GEMM reads them
 *                           through the same row ranges in the same order.  A, E, LL (and the batch's factored sums) are the bits of the
 *                           full-table wide-counts E-step with the same inputs and options; A0 = zeros, chk = 1.0.  A context that
 *                           alternates psmc_hip_estep and psmc_hip_estep_factored then keeps one table: nothing is sized anew.  The
 *                           counts pass follows the interval the E-step kept: "wide_decode" = 1 without "wide_decode_ckpt" still forces
 *                           the full table, and the counts then read it; with "wide_decode_ckpt" = 1 the E-step keeps checkpoints and a
 *                           decoding call after it reads them.  Device memory the checkpoint path adds: one X slab of the V slab's size
 *                           (8 S bytes per slab bin; auto: at most 4 GB, or one tile if that is longer; "wide_counts_slab" bounds both),
 *                           allocated at the first such E-step; PSMC_HIP_ENOMEM names the buffer and its size.  At 30 M bins and 1024
 *                           states: 31 GB of X plus up to 8 GB of slabs instead of 246 GB; at 256: 7.7 GB plus up to 8 GB instead of 61 GB.
 *                           Exact mode, up to 128 states, "wide_fast" = 0, without "wide_ckpt" or without "wide_counts": accepted, no
 *                           effect.  psmc_hip_estep_device beyond 128 states stays PSMC_HIP_ENOTSUP.  Other values: PSMC_HIP_EINVAL
 *  "wide_counts_slab" 0     bins per slab of that counts pass (whole tiles in plan order; a tile longer than the slab is a slab of its
 *                           own); 0 = auto: 2^29 / S bins (fewer tiles per slab serialise the V pass).  Slabs, row ranges and the split factor are functions of the tile plan and
 *                           this option alone ("wide_counts_ckpt" changes none of them; it adds an X slab of the same rows).  Negative: PSMC_HIP_EINVAL
 *  "merge"         0        1: a forward FIX pass between the forward sweep and the back half (64 states, fused back half): every tile's start
 *                           vector is checked there, and a tile that fails is rewritten from the true vector until its trajectory has the
 *                           direction of the stored one again (the factor between the two parts is kept for the counts and the likelihood) --
 *                           nothing is counted twice.  0: verify after the back half, whole tiles and their groups of the counts again.
 *                           Built in round 6 with "adapt" and "prev_start" (VERDICT r5 item 1), measured, off: DESIGN.md section 8
 *  "adapt"         0        1, with "merge": every speculating tile's forward warm-up follows the mismatch its speculation left (shrinks while it
 *                           is more than two decades inside "warm_tol", grows by what a repair needed)
 *  "prev_start"    0        1: forward warm-ups start from the previous E-step's X at that position instead of the stationary vector
 *  "learn"         1        tiles that needed a repair are treated differently in the following E-steps of the context
 *                           (longer warm-up, then glued to their neighbour); results then depend on the call history
 *                           within the stated tolerance, two contexts with the same history agree bit for bit
 *  "warm_shift"    auto     such a tile first gets a warm-up of warmup << warm_shift bins of its own and is glued only
 *                           if that fails too; 0 = glue at once.  auto: 1 with the two-round plan, 0 with one round
 *  "group_cap"     131072   longest run of glued tiles, in bins (full tiles of missing data do not count: "gap_tiles")
 *  "gap_tiles"     1        full tiles that consist of missing data only (runs of `N`: centromeres, assembly gaps) are glued to their neighbours
 *                           when the plan is made -- inside such a run the chain forgets at the rate of the matrix's second eigenvalue alone,
 *                           ~5e5 bins, so no warm-up works -- do not count against "group_cap" / "kc_div", and share ONE transfer matrix per
 *                           direction (a^T to the tile length).  0: as rounds 1-4 (a 2e5-bin gap then costs ~50 repair rounds per E-step)
 *  "hom_tiles"     0        1: runs of homozygosity are found when the plan is made, as "gap_tiles" finds runs of missing data (structured sweeps,
 *                           up to 128 states).  A hom tile is a full tile without a heterozygous bin -- all homozygous, or homozygous and missing
 *                           bins -- that is neither the first nor the last tile of its segment; a qualifying run is a maximal sequence of
 *                           consecutive hom tiles and gap tiles of one segment that holds at least one hom tile and "hom_min" bins of hom tiles.
 *                           Every tile whose warm-up window overlaps a tile of a qualifying run -- the run's own tiles behind its head, and the
 *                           tiles up to one warm-up past its end, in either direction -- is glued to its neighbour at once instead of being
 *                           learned one repair round at a time (a 45 k-bin run at 256-bin tiles: ~290 rounds in a context's first E-step).  The
 *                           all-homozygous tiles of qualifying runs share ONE transfer matrix per direction when the tile length is a multiple
 *                           of four and then do not count against "group_cap" / "kc_div"; the others keep a matrix each and count in full.
 *                           0: the plan is bit for bit what it was without the option.  Accepted and ignored in exact mode, by the dense
 *                           sweeps ("structured" = 0, a matrix without the PSMC form) and beyond 128 states.  Other values: PSMC_HIP_EINVAL
 *  "hom_min"       auto     bins of hom tiles a run needs to qualify; 0 = auto = "warmup" / 4.  The default comes from a CPU measurement on two
 *                           parameter sets (~512 het-free bins inside a 3072-bin warm-up are harmless, ~1024 are not),
 *                           not from a GPU sweep.  Negative: PSMC_HIP_EINVAL
 *  "wide_gap_tiles" 0       1: the wide fast path ("wide_fast", 129..1024 states) finds runs of missing data when its plan is made and crosses
 *                           them with a transfer matrix instead of speculating into them and repairing them position by position.  A gap tile
 *                           is a full tile of missing data only that is neither the first nor the last tile of its segment; a qualifying run
 *                           is a maximal sequence of consecutive gap tiles of one segment that holds at least "wide_gap_min" bins.  Glued
 *                           forward: every gap tile of a qualifying run and every later tile of the segment whose warm-up window (the
 *                           "warmup" bins before it) overlaps a tile of the run; glued backward: the mirror.  A tile whose speculation
 *                           starts at the true segment end in a direction is never glued in it.  Glued tiles do not speculate: once per
 *                           E-step the matrix M of one full tile of missing data is built (n unit vectors swept through the forward
 *                           sweep's own step), one chain per run and direction applies it tile by tile from the exit vector of the run's
 *                           neighbour, the run's tiles are swept from the chain's vectors, and one walk per run goes on through the tiles
 *                           glued behind it.  Every boundary is verified as any other, a failing one is repaired as before -- a failing
 *                           run by chaining it again, which fast_diag counts as one head tile.  Results stay bit-reproducible and within
 *                           the fast-mode tolerances; with "wide_ckpt", "wide_decode[_ckpt]", "wide_counts[_ckpt]", "wide_batch" and in
 *                           group shards as without.  Device memory: n x (padded states) doubles for M, 8 MB at 1024 states.  Measured
 *                           on the stress fixture (2.2 M bins, planted runs of 2e5 missing bins): profiles/wide_fast_timing.txt.
 *                           0: plan and E-step are bit for bit what they are without the option, and nothing new is launched.  Accepted
 *                           and ignored where the wide fast path does not run.  Other values: PSMC_HIP_EINVAL
 *  "wide_gap_min"  auto     bins of missing data a run of gap tiles needs to qualify; 0 = auto = a quarter of the wide plan's warm-up (4096
 *                           at the default 16384): a shorter run leaves at least 12288 data bins in a warm-up window, which
 *                           profiles/wide_fast_timing.txt measured as sufficient.  Negative: PSMC_HIP_EINVAL
 *  "wide_hom_tiles" 0       1: the same for runs of homozygosity, which a warm-up crosses no better (two start vectors still disagree by
 *                           0.03-0.08 after 16384 homozygous bins: DESIGN.md section 7).  A hom tile is a full tile of homozygous bins only
 *                           (no het, no missing bin) that is neither the first nor the last tile of its segment.  A chain tile is a gap
 *                           tile when "wide_gap_tiles" is on, or a hom tile when this option is on; a run is a maximal sequence of
 *                           consecutive chain tiles of one segment, and it qualifies when "wide_gap_tiles" is on and its gap tiles hold
 *                           at least "wide_gap_min" bins, or this option is on and its hom tiles hold at least "wide_hom_min" bins.  Glue,
 *                           chains, levels, verification and repair are those of "wide_gap_tiles"; across a hom tile the chain applies
 *                           the matrix M_h of one full tile of homozygous bins, built once per E-step beside M: a pilot sweep of the
 *                           uniform vector yields the power-of-two scale factors of such a tile, and the n unit vectors are swept
 *                           with them (under symbol 0 every step shrinks the vector, an unscaled row would drift towards underflow).
 *                           A het-free tile that holds homozygous AND missing bins is an ordinary data tile: it ends a run, and the run
 *                           that resumes behind it is chained after the walk through it.  Device memory: n x (padded states) doubles
 *                           for M_h and a quarter of a tile's bins in factors, and four bytes per tile.  Results stay bit-reproducible
 *                           and within the fast-mode tolerances, with every option "wide_gap_tiles" goes with.  0: plan and E-step are
 *                           bit for bit what they are without the option.  Accepted and ignored where the wide fast path does not run
 *                           (exact mode, up to 128 states, "wide_fast" = 0).  Other values: PSMC_HIP_EINVAL
 *  "wide_hom_min"  auto     bins of hom tiles a run needs to qualify through them; 0 = auto = a quarter of the wide plan's warm-up, as
 *                           "wide_gap_min" and "hom_min".  Negative: PSMC_HIP_EINVAL
 *  "wide_mix_tiles" 0       1 (it has an effect only with "wide_hom_tiles" = 1): het-free tiles that hold BOTH homozygous and missing bins
 *                           join the chain -- a real .psmcfa has `N` bins scattered through its runs of homozygosity, and without this
 *                           option every such tile ends a run.  A mix tile is a full tile without a het that holds both symbols and is
 *                           neither the first nor the last tile of its segment.  Mix tiles are admitted in plan order while the
 *                           matrices of all admitted ones fit "wide_mix_mb" (and at most 65535 tiles); this happens before runs are formed, so a refused tile ends
 *                           a run as it does without the option.  Admitted mix tiles are chain tiles beside gap and hom tiles; their
 *                           bins count towards "wide_hom_min" like those of hom tiles.  Glue, chains, levels, verification and repair
 *                           are unchanged.  Every mix tile of a qualifying run owns two matrices of n x (padded states) doubles, its own
 *                           forward map F = a D_lo ... a D_hi and backward map B = D_lo a ... D_hi a (D_p = diag(e0) at a homozygous bin,
 *                           the identity at a missing one; no diagonal relation ties the two), both swept row by row through the
 *                           tile's symbols with the power-of-two factors of a pilot sweep of their own; all of them are built by two
 *                           launches per E-step.  Results stay bit-reproducible and within the fast-mode tolerances.  0, or an input
 *                           without such a tile: plan, launches and bits are those without the option.  Other values: PSMC_HIP_EINVAL
 *  "wide_mix_mb"   2048     cap, in MB (10^6 bytes), on the matrices of the mix tiles; 1 .. 262144, anything else: PSMC_HIP_EINVAL.  A
 *                           condition, not a tuned number: at 1024 states a tile's two matrices are 16.8 MB and the default holds about
 *                           120 tiles; at 200 states (256 padded) they are 0.8 MB and it holds about 2500
 *  "vit_tile"      2048     bins per backtrace tile of psmc_hip_viterbi: 16 .. 16777216, anything else: PSMC_HIP_EINVAL.  Paths and scores do
 *                           not depend on it: it sets how long the longest chain of dependent loads is (one tile) and how many maps of
 *                           2 x (padded states) bytes there are (profiles/viterbi.txt).  psmc_hip_sample_paths tiles its backtraces by it
 *                           as well; the samples do not depend on it either
 *  "samp_group"    0        samples per sweep of psmc_hip_sample_paths: one map table per sample of the group is held on the device, and
 *                           one forward sweep serves the whole group.  0 (auto): as many as the free device memory holds, at most 8;
 *                           1 .. 64: that many (fewer when n_samp is smaller or the memory does not hold them); anything else:
 *                           PSMC_HIP_EINVAL.  The samples do not depend on it
 *  "two_phase"     auto     2: the fused back half runs as two launches, odd tiles of the second list start from the exit
 *                           vector of the tile above instead of speculating backward; 0: every tile speculates, one
 *                           launch when the tiles fit one round.  auto: 2 with two rounds, 0 with one
 *  "merge1"        auto     1: bulk forward sweep and backward warm-up pass in ONE grid, so that the dispatcher puts
 *                           their waves on distinct SIMDs, and the dependent chain walks -> chains -> run tiles -> back
 *                           half on one stream; 0: side by side on streams of their own.  auto: 1 with one round
 *  "phase1"        auto     fused back half, 64 states, four tiles per wave, bulk passes on streams of their own (not "merge1"): 1 = the blocks of
 *                           the bulk forward sweep and of the backward warm-up pass form ONE work queue, longest first, that a persistent
 *                           grid of "phase1_waves" waves per SIMD pulls from; 0 = two launches, dealt out by the dispatcher.  Bit-identical.
 *                           auto: 1
 *  "phase1_waves"  2        waves per SIMD of that grid (1..4)
 *  "tail"          1        fused back half (64 and 128 states), overlapped streams: 1 = the waves of the fused counts test the backward tile
 *                           boundaries themselves, with the verify kernel's own arithmetic (the few pairs they cannot -- tiles of glued runs, an
 *                           upper tile that owns no transition -- stay with that kernel), and the reductions follow the counts instead of the
 *                           verify, list A's partial counts being summed while list B runs; 0 = verify, compaction and reductions as launches
 *                           behind list B.  Bit-identical; ignored by the factored, the unfused and the dense back half and by batches.
 *  "coarse"        auto     a bulk sweep item spans up to this many consecutive tiles of a segment: ONE speculative warm-up per item
 *                           and direction (the forward sweep runs through its tiles, the backward pass of phase 1 walks the item and
 *                           leaves every tile's start vector), so the back half keeps its ~4096 tiles while phase 1 pays half the
 *                           warm-ups.  Fused / factored back half only.  auto: 2 in the one-round plan when there are more than 2048
 *                           tiles shorter than their warm-up (1 M .. 12 M bins), else 1
 *  "lanes8"        auto     64 states, fused / factored back half: 1 = the bulk sweeps of phase 1 run EIGHT tiles per wave (8 lanes x 8 states per
 *                           tile: a scan level less, ~13 instead of 17 vector instructions per tile-step, half as many waves); 0 = four.
 *                           auto: with the factored statistics of a genome-sized input (their forward sweep stores checkpoints only, three
 *                           waves per SIMD: issue-bound); slower for the full-count E-step (forward sweep paced by its table stores) and for
 *                           shard-sized inputs (one wave per SIMD: the 8 x 8 step is a third longer)
 *  "share_learn"   1        psmc_hip_estep_batch, fast mode: the replicates tile every segment with ONE tile length (the largest
 *                           replicate's) and a replicate that plans starts from the glue flags and warm-ups its predecessors learned
 *                           at the same (segment, tile) -- the slow regions belong to the data, so replicate 2..R skip most of the repair
 *                           rounds of their first E-step; results then depend on the batch's call history (two contexts with the same
 *                           history agree bit for bit).  0: every replicate plans and learns for itself
 *  --- glued runs ---------------------------------------------------------------------------------------------------
 *  "kc_min"        auto     runs of at least this many tiles get their boundary vectors from a chain of tile transfer
 *                           matrices instead of a walk; 0 = never.  auto (-1): 4 with 64 states (5 in the two-round plan), 8 with
 *                           65..128 (12)
 *  "kc_sub"        auto     64 states: a tile's steps are cut into this many ranges with a matrix (and a pair of
 *                           waves) each; auto: ranges of about (tile + warmup) / 8 steps, at most 4
 *  --- back half ----------------------------------------------------------------------------------------------------
 *  "fuse"          1        structured sweeps, up to 64 states: the backward sweep feeds the counts' matrix
 *                           instructions directly, bt never stored; 0: bt table + separate counts kernel
 *  "fuse128"       2        the same with 65..128 states: 2 = sixteen tiles per work-group, one sweep per tile, operands of the matrix
 *                           instructions exchanged through LDS; 0 = unfused
 *  "ckpt"          1        psmc_hip_estep_factored keeps X only every 8th position and recomputes the rest
 *  "structured"    1        1 = O(N) sweeps when a[][] has the PSMC form (checked per call), 0 = always the dense sweeps
 *  "overlap"       1        forward chain, backward chain, counts and walks on streams of their own; 0: one stream
 *  --- dense sweeps / unfused counts (any matrix up to 64 states) ----------------------------------------------------
 *  --- exact mode ---------------------------------------------------------------------------------------------------
 *  "rep_impl"      auto     row replication of the ordered sums: 1 v_permlane16/32_swap, 0 ds_bpermute (bit-identical); -1 = auto:
 *                           0 when a launch has more than one wave per SIMD (bootstrap batch), else 1
 *  "batch_bins"    0        psmc_hip_estep_batch: table bins per launch; 0 = what fits the free device memory
 *  "batch_first"   0        psmc_hip_estep_batch, fast mode: replicate 0 of the calls that follow is replicate <value> of the context's
 *                           replicates -- a caller that sends its replicates in several calls names each call's first position, so that
 *                           every replicate meets the tile plan it had in the previous EM iteration.  Exact mode keeps nothing per
 *                           replicate and ignores it.
 *  "batch_sort"    1        psmc_hip_estep_batch: the entries -- (replicate, segment) sweeps -- of ALL replicates are dealt to the launches
 *                           longest first, so that the long trunks share one launch and the others end with their own, shorter, longest
 *                           entry; 0 = replicate-major order (every launch then lasts as long as the longest trunk).  Bit-identical.
 *  "batch_tailfill" 1       psmc_hip_estep_batch with "batch_sort": when memory and entry slots would allow one launch fewer than filling them
 *                           longest first gives, the shortest entries go into the spare slots of the memory-bound launches (no last launch
 *                           of a few dozen entries on an empty device); 0 = plain head fill.  Bit-identical.
 *  "batch_major"   1        psmc_hip_estep_batch_cb with "batch_sort", several launches: when half of the entry blocks or more share their longest
 *                           length (utils/splitfa.c cuts the trunks to one length), the blocks no longer than that keep the caller's replicate
 *                           order -- longer ones still first, by length -- so that replicates complete launch by launch and `done` can hand
 *                           them to the caller's M-steps while the later launches run.  Where that order alone needs a launch more than the tail
 *                           fill, the few shortest blocks of the call leave the replicates' order and go where there is room (round 6); not
 *                           when it still needs a launch more.  Bit-identical.
 *  "exact_refwd"   auto     psmc_hip_estep_batch, 64 states: 1, 2 = no f table -- the expect pass recomputes the forward sweep in its own
 *                           work-group (bit-identical), so a launch group holds twice the replicates; 2 = two entries per work-group
 *                           (two producer waves, two consumer waves: four entries per compute unit), 1 = one; 0 = f and b tables,
 *                           three kernels.  auto: 2, and only when the tables of all replicates would not fit one launch group
 *
 * With 65..128 states "lanes8", "kc_sub", "ckpt", "merge" and "adapt" are accepted and ignored (their kernels are 64-state ones);
 * beyond 128 states the exact kernels read only "batch_bins" and "batch_sort" (the wide fast path: see "wide_fast").
 * Removed after losing their A/B or settling on one value (HISTORY.md keeps the measurements) -- round 3: "count_impl", "kc_warm",
 * "walk_heads", "walk_impl", "kcol_impl", "fuse_order", "exact_lds", the value 1 of "two_phase"; round 6: "lanes8b" (with its kernel),
 * "batch_slots", "expect_impl" (with the vector-instruction counts kernel), the value 1 of "fuse128" (with round 3's 128-state kernel),
 * "struct_tiles", "target_waves", "n_sub", "runs_late", "merge_order", "gate", "kc_div", "kcol_prio" (what they chose is now what the plan does). */
int psmc_hip_set_option(psmc_hip_ctx *ctx, const char *key, double value);

/* Restrict the kernels of this context to `count` compute units starting at `first` in the bit order of HIP's compute-unit
 * masks (hipExtStreamCreateWithCUMask; on an MI355X consecutive bits go round the eight XCDs, so a range of 24 is three
 * units of every XCD); count = 0: the whole device again.  Two contexts with disjoint ranges share a device without ever
 * sharing a SIMD: psmc_boot runs the main run (README:49-53 of the reference) beside the bootstrap batch like this -- the
 * main run's 90 sequential sweeps keep a SIMD each, and the batch sizes its launches for the units it was left
 * (psmc_amd/host/boot.c).  Re-creates the context's streams: call it between E-steps, before the first for preference. */
int psmc_hip_set_cu_range(psmc_hip_ctx *ctx, int first, int count);

/* Replaces the per-segment hmm_new_data copies of em.c:38-44 / khmm.c:37-45:
 * uploads all segments once; the caller keeps ownership of seq.
 * Call order: a load (this call or psmc_hip_load_segments_device) ends what the last E-step left.  Until the next single E-step
 * psmc_hip_get_tables and the decoding entry points (psmc_hip_decode, _posterior, _scales, _post_counts, _post_mean,
 * _post_quantile) return PSMC_HIP_ESTATE ("no single E-step yet"), as on a fresh context and as after psmc_hip_estep_batch: the
 * tables hold the previous segments at the previous offsets.
 * NOT checked (open): a call that has to grow the tables after a single E-step -- psmc_hip_reserve_batch_tables with a bound
 * beyond what they hold -- frees and re-allocates them, and a decoding call or psmc_hip_get_tables before the next single E-step
 * then reads blocks nobody wrote.  Reserve before the first E-step (as psmc_boot does), or run an E-step before decoding. */
int psmc_hip_load_segments(psmc_hip_ctx *ctx, int n_seg, const uint8_t *const *seq, const int32_t *L);
/* Same, for observations already resident in HBM: d_obs holds the segments
 * back to back, segment i starting at byte off[i] (off[i] % 64 == 0) with at
 * least 64 readable bytes after the last one.  The buffer is borrowed. */
int psmc_hip_load_segments_device(psmc_hip_ctx *ctx, int n_seg, const void *d_obs, const int64_t *off,
                                  const int32_t *L);
/* Bootstrap multiset (psmc_resamp, aux.c:8-47): which loaded segments the next
 * E-steps run over, in order, repeats allowed.  Default: all, in load order. */
int psmc_hip_select(psmc_hip_ctx *ctx, int n_sel, const int32_t *seg_idx);

/* Replaces em.c:33-55 + 60: one E-step over the selected segments.
 *   A  n*n   he_sum->A            E  2*n  he_sum->E[0..1] (khmm.c:355)
 *   A0 n     he_sum->A0 (may be NULL; unused downstream)
 *   LL       sum of hmm_lk over segments (em.c:48)
 *   chk      n_sel values of the khmm.c:237-238 underflow check (may be NULL)
 * Fast mode computes neither A0 (nothing downstream reads it: khmm.c:321-322 fills it, hmm_Q never uses it) nor the
 * self-check (its speculation has its own verify / repair net): A0 comes back as zeros and chk as 1.0, from this call
 * and from psmc_hip_group_estep alike.  Exact mode returns the reference's values -- also where the parameters are no HMM
 * (negative, infinite or NaN entries): a cell that is NaN in the reference is NaN here and no other is, with the reference's
 * sign as long as no parameter is a positive NaN (x86 sets the sign bit of a NaN it makes and carries an operand's NaN along).
 * Parameters that hold NaNs of both signs are undefined: which of two NaNs an addition keeps depends on the operand order one
 * build of the reference chose. */
int psmc_hip_estep(psmc_hip_ctx *ctx, const double *a, const double *e, const double *a0, double *A, double *E,
                   double *A0, double *LL, double *chk);

/* Allocate now the tables a single E-step over the loaded segments needs (exact: f, b, s; fast: X and the scale factors),
 * instead of inside the first psmc_hip_estep: a caller that shares the device with an exact batch (psmc_boot --main) takes
 * its share BEFORE the batch sizes its own from what is free. */
int psmc_hip_reserve_tables(psmc_hip_ctx *ctx);

/* Config 4 (bootstrap): n_rep E-steps over ONE loaded segment set in a single call -- replicate r has its own
 * parameters a[r] (n*n), e[r] (2*n), a0[r] (n) and its own multiset sel_idx[sel_off[r] .. sel_off[r+1]) of loaded
 * segments (psmc_resamp, aux.c:8-47: repeats allowed, order matters for the exact sum).  Replaces n_rep runs of
 * em.c:33-55, i.e. what README:57-62 of the reference farms out with xargs.  Outputs, any may be NULL but one of
 * A / sums is needed: A n_rep*n*n, sums n_rep*5n (SL|SU|DG|CL|CU as psmc_hip_estep_factored), E n_rep*2n, LL n_rep.
 *   exact mode: an ENTRY is one (replicate, unique segment) sweep, one wave; the entries of all replicates are dealt to launches
 *     by length (options "batch_sort", "batch_tailfill", "batch_major"), as many per launch as table memory and wave slots hold,
 *     so the device holds hundreds of sweeps instead of one replicate's dozens; results are bit-identical to n_rep separate
 *     psmc_hip_select + psmc_hip_estep calls whatever the dealing.  "batch_bins" caps the table bins per launch; default: what
 *     fits the free memory.
 *   fast mode: one replicate fills the device, so they run back to back, each on its own learned tile plan (kept in
 *     a per-replicate child context that shares this context's observations and tables); sums = factored statistics.
 *   beyond 128 states: the exact launch groups above whatever the mode, bit for bit what an exact-mode context gives -- except the
 *   wide fast batch: a call takes the wide fast path ("wide_fast") if and only if "wide_batch" = 1, the context is in fast mode, has
 *     more than 128 states, "wide_fast" covers its size (1: up to 256 states, 2: up to 1024), A == NULL and sums != NULL.  A caller who
 *     wants A, alone or beside sums, gets the exact launch groups -- unless "wide_counts" = 1 (and "structured" = 1): then the call
 *     takes the wide path with A != NULL too, replicate r's A has the bits psmc_hip_select + psmc_hip_estep give on a fresh context
 *     with the same options, and its sums are the factored statistics of the same E-step.  The wide path learns nothing between E-steps (its plan depends on
 *     the selection and the options alone), so there are no replicate contexts: for r = 0 .. n_rep-1, in order, the context selects
 *     replicate r's multiset, runs the E-step of psmc_hip_estep_factored with a[r], e[r], a0[r] into the rows r of sums / E / LL --
 *     the bits psmc_hip_select + psmc_hip_estep_factored give on a fresh context with the same options -- and calls done(user, 1, &r).
 *     One X table, sized for all loaded segments, serves every replicate.  On every exit, errors included, the selection the context
 *     had before the call is back: a later single E-step gives the bits it gave before.  PSMC_HIP_ECONVERGE from a replicate's
 *     E-step: that replicate is repeated with the exact kernels (a line on stderr names it and the path that failed) and the batch
 *     goes on wide.  PSMC_HIP_ENOTSUP ("structured" = 0, a matrix without the PSMC form) ends the call, the message names the
 *     replicate.  Afterwards psmc_hip_fast_repairs / _fast_info / _fast_diag describe the last replicate's E-step, psmc_hip_batch_info
 *     answers {n_rep, 0}; "batch_first" and "share_learn" are not read.
 * Segment tables are in batch layout afterwards: decode / get_tables need a single E-step first (the wide fast batch included: with
 * "wide_decode" = 1 a decoding call after it answers PSMC_HIP_ESTATE). */
/* Exact mode: allocate the batch's tables now -- min(max_bins, what "batch_bins" allows or 0.9 of the free device memory;
 * max_bins <= 0: no upper bound), max_bins = the table bins all replicates together can need, e.g. n_rep x the padded
 * length of the loaded segments -- instead of inside the first psmc_hip_estep_batch.  The driver clears what it hands out:
 * ~250 GB take 4-6 s, which a caller can spend while it is still loading (psmc_boot does; the first EM iteration then costs
 * what the others do).  Fast mode: no-op (up to 128 states, and where "wide_batch" = 1 sends the batch down the wide fast path).
 * A SECOND call while that reservation stands (64 states, batch without the f table) adds what has become free since -- psmc_boot
 * --main: the main run that shared the device is over -- as a second chunk of table beside the first, up to max_bins in all: the batches
 * that follow plan their launches for both (an entry's table is an offset from the first chunk either way).  Growing the first chunk
 * instead would free and allocate it again: 8 s for 260 GB on this driver against 0.5 s for 31 GB more. */
int psmc_hip_reserve_batch_tables(psmc_hip_ctx *ctx, int64_t max_bins);
int psmc_hip_estep_batch(psmc_hip_ctx *ctx, int n_rep, const double *a, const double *e, const double *a0,
                         const int32_t *sel_off, const int32_t *sel_idx, double *A, double *sums, double *E, double *LL);
/* The same with a progress callback: `done(user, n, replicates)` is called on the calling thread, between two launches (exact mode)
 * or after each replicate's E-step (fast mode, the wide fast batch), with the replicates -- positions in this call -- whose rows of A / sums / E / LL are
 * final from now on; every replicate is named exactly once, the last ones before the call returns.  What em.c:56-68 does next, the
 * M-step, needs nothing else: a caller can run the finished replicates' M-steps on its own threads while the device works on the
 * rest of the batch (psmc_boot does).  The callback must not call into this context.  done = NULL: psmc_hip_estep_batch. */
typedef void (*psmc_hip_batch_done_fn)(void *user, int n_done, const int32_t *replicates);
int psmc_hip_estep_batch_cb(psmc_hip_ctx *ctx, int n_rep, const double *a, const double *e, const double *a0,
                            const int32_t *sel_off, const int32_t *sel_idx, double *A, double *sums, double *E, double *LL,
                            psmc_hip_batch_done_fn done, void *user);
/* Diagnostic: out = {launch groups of the last exact batch (fast, wide fast batch: replicates run), replicate contexts alive}. */
int psmc_hip_batch_info(psmc_hip_ctx *ctx, int out[2]);

/* Exact mode, for multi-process sharding: per selected segment the reference's
 * own `he` (em.c:49) and hmm_lk, so that the caller can add them in the global
 * input order.  segA n_sel*n*n, segE n_sel*3*n, segA0 n_sel*n, segLL n_sel. */
int psmc_hip_estep_segments(psmc_hip_ctx *ctx, const double *a, const double *e, const double *a0, double *segA,
                            double *segE, double *segA0, double *segLL, double *chk);

/* Fast mode, device-resident result for a collective: enqueues the E-step on
 * `stream` (a hipStream_t, NULL = default) and writes n*n + 2*n + 1 doubles
 * [A | E | LL] to the device buffer d_stats.  Asynchronous; the caller
 * synchronises the stream (or hands d_stats to RCCL on the same stream). */
int psmc_hip_estep_device(psmc_hip_ctx *ctx, const double *a, const double *e, const double *a0, void *d_stats,
                          void *stream);
/* Fast-mode diagnostics of the last E-step.  warm_err_fwd/bwd = largest
 * relative mismatch left between the vector a tile built on at its boundary and
 * the value its neighbour computed (after the last verify round: <= warm_tol);
 * warmup_used = speculative overlap in bins. */
int psmc_hip_fast_diag(psmc_hip_ctx *ctx, double *warm_err_fwd, double *warm_err_bwd, int *n_chunks,
                       int *warmup_used);
/* How much repair the speculation needed: verify/repair rounds and the total
 * number of tile re-runs, forward and backward, out[0..3]; out[4] = tiles
 * the forward fix pass rewrote in part ("merge"),
 * out[5] = 1 when a second pass of the counts had to run, 2 when the E-step was one of the wide path ("wide_fast": 129..256, with the value 2 up to 1024
 * states: out[0..3] are then its verify / repair rounds and the head tiles the repairs started from, out[4] = 0). */
int psmc_hip_fast_repairs(psmc_hip_ctx *ctx, int out[6]);
/* Diagnostic: the plan the NEXT fast E-step of this context will run with: out = {tiles, tile length in bins, mean forward
 * warm-up of the speculating tiles in bins, mean backward warm-up, longest forward, longest backward, tiles glued to their
 * predecessor (forward), tiles glued to their successor (backward)}. */
int psmc_hip_fast_plan(psmc_hip_ctx *ctx, double out[8]);

/* Fast mode, matrices of the PSMC form (two rank-1 triangles, core.c:112-122), any n <= 128: the E-step without the
 * N x N counts.  The EM objective needs of A only  SL_k = sum_{l<k} A[k][l],  SU_k = sum_{l>k} A[k][l],
 * DG_k = A[k][k],  CL_l = sum_{k>l} A[k][l],  CU_l = sum_{k<l} A[k][l]  (psmc_amd/host/mstep.c); they come out
 * of the backward sweep in O(N) per bin.  sums = SL | SU | DG | CL | CU (5n), E as in psmc_hip_estep (2n).
 * PSMC_HIP_ENOTSUP when the matrix does not have the form.  129..256 states: with the option "wide_fast" only, 257..1024 states: with "wide_fast" = 2 only (see there).
 * Replaces em.c:33-55 + the reads of hmm_Q. */
int psmc_hip_estep_factored(psmc_hip_ctx *ctx, const double *a, const double *e, const double *a0, double *sums,
                            double *E, double *LL);

/* Diagnostic: out = {structured sweeps used (0/1), tile length in bins, forward sweep items,
 * backward sweep items, back half (0: bt table + counts kernel, 1: backward sweep fused with the counts, 2: factored
 * statistics, 3: the factored statistics of the wide path, "wide_fast": items = tiles), checkpointed X (0/1), launches of the fused back half (2 with the two-phase plan), phase 1 as one grid
 * ("merge1": 0/1)} of the last fast-mode E-step (items = runs of glued tiles).  The O(N) structured
 * sweeps are chosen automatically when a[][] has the two rank-1
 * triangles psmc_update_hmm builds (core.c:112-122); otherwise the dense sweeps run. */
int psmc_hip_fast_info(psmc_hip_ctx *ctx, int out[8]);

/* Diagnostic: the forward table of the wide fast path ("wide_fast").  out = {rows of X currently allocated for it (the table; with
 * "wide_ckpt" also every tile's last row, kept beside it), the padded width S of a row in states (8 S bytes), the checkpoint interval
 * of the last wide fast E-step (1: every position, 8: "wide_ckpt"; 0: none ran yet), bytes held = rows x S x 8}.  All zeros on a
 * context that never ran the path. */
int psmc_hip_wide_table_info(psmc_hip_ctx *ctx, int64_t out[4]);

/* Copies the forward/backward tables of one loaded segment to the host after
 * an E-step (replaces reading hd->f, hd->b, hd->s: aux.c:159-200).  f,b: L*n,
 * s: L; any of them may be NULL (the PR line of `-s`, aux.c:159-164, needs s only: 8 bytes per bin).
 * Exact mode: the reference's values bit for bit.  Fast mode (diagnostic):
 * f = X, b = bt = e[o_p]*B_p, s = 1/d_p at p % 4 == 0; b only
 * with "fuse" = 0 (the fused back half never stores bt), all of f only without checkpointing. */
int psmc_hip_get_tables(psmc_hip_ctx *ctx, int seg, double *f, double *b, double *s);

/* Posterior decoding of one segment on the device after an exact E-step (fast mode: see below): replaces
 * hmm_post_decode (khmm.c:264-281) + the max-posterior bookkeeping of aux.c:165-182.
 * path[u-1] = argmax_k f[u][k]*b[u][k]*s[u] (first maximum wins), maxp[u-1] = its value;
 * 12 bytes per bin leave the GPU instead of the 2*8*n of the tables. */
int psmc_hip_decode(psmc_hip_ctx *ctx, int seg, int32_t *path, double *maxp);

/* Full posterior decoding of one segment on the device after an exact E-step (fast mode: see below): replaces the -D branch of psmc_decode
 * (aux.c:183-200).  post[(u-1)*n + l] = f[u][l]*b[u][l]*s[u] (hmm_post_state, khmm.c:285-292); recomb[u-1] = 1 -
 * sum_l f[u][l]*a[l][l]*b[u+1][l]*e[o_{u+1}][l] for u < L and 0 at u = L (aux.c:189-193) -- every product left to
 * right, the sum in state order: the reference's doubles.  Either output may be NULL.  8*(n+1) bytes per bin leave the
 * GPU instead of the 16*n + 8 of the tables. */
int psmc_hip_posterior(psmc_hip_ctx *ctx, int seg, double *post, double *recomb);

/* Posterior-weighted counts of one segment on the device (fast mode: see below): replaces the -c branch of psmc_decode (aux.c:202-219).
 * cnt1 = the segment's record of a cntcpg file (l positions x n_cnt int32, utils/cntcpg.c); cnt (n*n_cnt, in/out)
 * are the running totals, cnt[k*n_cnt + j] += post[u][k] * cnt1[(u-1)*n_cnt + j] for u = 1..min(L, l) in position
 * order -- call once per segment in input order with the same cnt, as the reference's loop does.  Only
 * 4*n_cnt bytes per bin go to the GPU and n*n_cnt doubles come back. */
int psmc_hip_post_counts(psmc_hip_ctx *ctx, int seg, const int32_t *cnt1, int32_t l, int32_t n_cnt, double *cnt);

/* The reference's scaling factors s[u] of one segment (hmm_forward, khmm.c:170-186; the PR line of -s, aux.c:159-164), L doubles.
 * Exact mode (and more than 128 states unless the wide fast tables are decoded -- "wide_decode" --, and the exact fallback below): a copy of the
 * table, the doubles psmc_hip_get_tables returns as s.  Fast mode: s_u = sum X_u / sum X_{u-1} / inv_u from the fast forward table, X_{u-1} being a tile's own start
 * vector at its first position and s_1 = sum_k a0_k e_k(o_1); within 1e-11 relative of the exact value. */
int psmc_hip_scales(psmc_hip_ctx *ctx, int seg, double *s);

/* Per-bin posterior expectations of one segment on the device: the local TMRCA track (what utils/dec2ctime.pl and friends make of
 * the rows of -D).  w is an n_w x n array of per-state weights, 1 <= n_w <= PSMC_HIP_MAX_MEAN_COLS, and
 *   mean[(u-1)*n_w + j] = sum_k gamma_u(k) * w[j*n + k],   u = 1..L, j = 0..n_w-1,
 * gamma_u being the posterior row psmc_hip_posterior returns for the same call state: w = t_k gives the expected coalescence time,
 * w = t_k^2 its second moment, an indicator P(T > x).  8*n_w bytes per bin leave the GPU instead of the 8*n of the rows.  The fifth
 * sibling of _decode / _posterior / _post_counts / _scales: the same state rules ("Decoding on a FAST context": which tables are
 * read, ESTATE, ENOTSUP, "wide_decode", "wide_decode_ckpt", selection and reload), and it reads tables only.  PSMC_HIP_EINVAL for a
 * NULL w or mean and for n_w outside 1..PSMC_HIP_MAX_MEAN_COLS (four: on the wide fast path every column takes one slot of the
 * exchange between a tile's waves beside the row sum, and a wave publishes six values at most).  Per source:
 *   - the exact tables (exact mode, the exact fallbacks of a fast context, beyond 128 states without "wide_decode"):
 *     gamma_u(k) = f*b*s multiplied left to right, t_k = gamma_u(k) * w[j][k] rounded once (no FMA), and the sum in state order,
 *     ((t_0 + t_1) + t_2) + ... -- bit for bit what a C loop over the rows of psmc_hip_posterior gives (estep_post_mean.hip);
 *   - the fast tables up to 128 states: the sum of gamma_u(k) w[j][k] over the doubles psmc_hip_posterior returns, in the order of
 *     the wave's reduction and with FMAs (estep_post_fast.hip): within (n + 8) * 2^-52 * max_k |w[j][k]| of the exact sum over
 *     those rows;
 *   - the wide fast tables (full or checkpoints): (sum_k g_p(k) w[j][k]) / G_p from the sweep's unnormalised g (estep_wide_post.hip),
 *     within the same bound of the sum over the rows; from checkpoints the bits of the full table.
 * Against an exact context given the same parameters, the fast sources are within 1e-9 * sum_k |w[j][k]| (the posterior's 1e-9
 * absolute per state).  Every column is computed on its own: a call with several columns returns, column by column, the bits of
 * the calls with one. */
#define PSMC_HIP_MAX_MEAN_COLS 4
int psmc_hip_post_mean(psmc_hip_ctx *ctx, int seg, const double *w, int32_t n_w, double *mean);

/* Per-bin posterior quantiles of one segment on the device: the median and a credible band of the local TMRCA (the posterior over
 * the states is skewed and often bimodal near a breakpoint, so mean +- sd is no band).  q holds n_q values in [0, 1],
 * 1 <= n_q <= PSMC_HIP_MAX_QUANT_COLS, and
 *   state[(u-1)*n_q + j] = the 0-based state at the q[j] quantile of the posterior of bin u,   u = 1..L, j = 0..n_q-1,
 * bins numbered as psmc_hip_decode numbers them.  4*n_q bytes per bin leave the GPU instead of the 8*n of the rows.  The sixth sibling
 * of _decode / _posterior / _post_counts / _scales / _post_mean: the state rules are exactly those of _post_mean ("Decoding on a
 * FAST context": which tables are read, ESTATE, ENOTSUP, "wide_decode", "wide_decode_ckpt", selection and reload); it reads tables
 * only, and its device scratch is freed before it returns.  PSMC_HIP_EINVAL for a NULL q or state, for n_q outside
 * 1..PSMC_HIP_MAX_QUANT_COLS and for any q[j] that is NaN or outside [0, 1].
 * The rule is the one psmc_hip_sample_paths uses for a draw: the number of states whose running sum lies below q times the total.
 * Per source:
 *   - the exact tables (exact mode, the exact fallbacks of a fast context, beyond 128 states without "wide_decode"):
 *     gamma_u(k) = f*b*s multiplied left to right; c_0 = gamma_u(0), c_k = c_{k-1} + gamma_u(k), one rounded addition each in
 *     ascending k (no FMA); x_j = q[j] * c_{n-1}, one rounded product; state = min(n-1, #{k < n : c_k < x_j}).  A NaN total gives 0
 *     (every comparison is false).  Bit for bit what a C loop over the rows of psmc_hip_posterior gives (estep_post_quantile.hip); so
 *     q = 0 gives state 0, and q = 1 the first state at which the running sum reaches its final value;
 *   - the fast tables up to 128 states: the same count, #{k < n : c_k < q[j] G} clipped to n-1, over the kernel's own prefix sums
 *     of the unnormalised g_u(k) = X_u(k) bt_u(k) / e_k(o_u) (a wave scan; any association, FMAs) and its own total G_u
 *     (estep_post_fast.hip); padded states (k >= n) are left out by a test of their index, not by their g being zero;
 *   - the wide fast tables (full or checkpoints): the same count over the prefix sums of the sweep's g_p(k) = X_p(k) y(k) and
 *     G_p (estep_wide_post.hip): the prefix of a state is its thread's running sum plus the sums of the lanes and of the waves
 *     below it.  Beyond 256 states the wave that holds the quantile is found from the waves' totals alone -- the lowest wave w*
 *     whose inclusive prefix is not below q[j] G -- and the state is min(n, the states of the waves below w*) + the count within
 *     w*, clipped to n-1.  From checkpoints the bits of the full table.
 * On every source the result is deterministic -- it depends on the tables and q alone -- and every column is computed on its own: a
 * call with several columns returns, column by column, the bits of the calls with one.
 * Guarantees for the fast sources (the exact ones are bit-pinned above), with C_k the cdf of a posterior row summed in state order
 * without rounding (C_{-1} = -inf) and i the returned state:  (i == 0 or C_{i-1} < q + d) and (i == n-1 or C_i >= q - d), where
 *   (Q2) against the rows psmc_hip_posterior returns on the same context in the same call state: d = 2 * (n + 8) * 2^-52 -- C_i is a
 *        _post_mean with an indicator column, whose bound for |w| <= 1 is (n + 8) * 2^-52; doubled for forming q G and comparing
 *        unnormalised;
 *   (Q3) against the rows of an exact context given the same parameters: d = 1e-9 * n (the posterior's 1e-9 absolute per state). */
#define PSMC_HIP_MAX_QUANT_COLS 4
int psmc_hip_post_quantile(psmc_hip_ctx *ctx, int seg, const double *q, int32_t n_q, int32_t *state);

/* Viterbi path of every loaded segment (khmm.c:83-141), in load order; psmc_hip_select is not read.
 * path: sum of L entries, segment i at offset L[0]+..+L[i-1]; score: n_seg doubles (hmm_Viterbi's return value).
 * Either may be NULL; with path == NULL no back-pointer table is allocated.
 * The jointly most probable state sequence, not the per-bin argmax of psmc_hip_decode; bins are numbered as psmc_hip_decode numbers
 * them.  The arithmetic is the reference's, bit for bit, on any context -- both modes run the same kernels (estep_viterbi.hip), 1..1024
 * states, any matrix:
 *   la[k][l] = log(a[l][k]), le[b][k] = log(e[b][k]) (b = 0, 1), le[2][k] = 0, l0[k] = log(a0[k]): on the host, one libm log() each
 *   (log(0) = -inf is allowed);
 *   V_1[k] = le[o_1][k] + l0[k];  at u = 2..L, for every k: m = -1e300, arg = -1, for l = 0..n-1: c = V_{u-1}[l] + la[k][l], if (m < c)
 *   m = c, arg = l -- the first maximum wins, a NaN never does -- then V_u[k] = le[o_u][k] + m, bp_u[k] = arg;
 *   the same rule over V_L gives the last state and the score; s_{u-1} = bp_u[s_u]; path[u-1] = s_u.
 * Every candidate is one IEEE addition, and "the maximum, the lowest index among equal maxima" is exact and associative, so the
 * kernels split the range of l over lanes and waves and still return the reference's bits.
 * The call reads the observations only: every table, plan, learned state and selection of the context stays as it was (an E-step or
 * a decoding call after it returns the bits it returns without it), and the device memory it allocates -- the back-pointer table,
 * 1 byte per (bin, state padded to a multiple of 64) up to 256 states and 2 bytes beyond (1.9 GB for 30 M bins x 64 states), the
 * tiles' maps, the path -- is released before it returns.  The backtrace runs tile by tile ("vit_tile"): per tile every state is
 * followed down to the tile below, the maps are composed per segment, and every tile writes its piece of the path.
 * PSMC_HIP_ESTATE: no segments loaded.  PSMC_HIP_EINVAL: a NULL parameter; both outputs NULL; a state of some segment has no
 * predecessor of finite probability (where the reference's assert(max_l >= 0) fires -- the message names the segment, the outputs are
 * unspecified, the context stays usable).  PSMC_HIP_ENOMEM: the message holds the table's size. */
int psmc_hip_viterbi(psmc_hip_ctx *ctx, const double *a, const double *e, const double *a0,
                     int32_t *path, double *score);

/* State paths drawn from the posterior P(path | data, parameters) of every loaded segment, in load order (forward filtering, backward
 * sampling); psmc_hip_select is not read.  path: n_samp * sum of L entries, sample j (0-based), segment i at offset
 * j * (sum of L) + L[0]+..+L[i-1], 0-based states, bins numbered as psmc_hip_decode numbers them.  stream: n_seg ids, one per segment,
 * or NULL: the load index (a caller that holds a shard of a larger input passes the segments' global indices).
 * The result is pinned bit for bit and depends on (a, e, a0, the observations, seed, j, the segment's stream id q) alone -- not on the
 * device, the mode, "vit_tile", "samp_group", n_samp or anything done on the context before -- 1..1024 states, any matrix; both modes
 * run the same kernels (estep_sample.hip):
 *   forward vectors: hmm_forward's (khmm.c:170-185), every product rounded once, no FMA: f_1 = a0 o e(o_1); at u = 2..L, for every k:
 *   tmp = 0.0, for l = 0..n-1: tmp += f_{u-1}[l] * a[l][k], then f_u[k] = e(o_u)[k] * tmp; each f_u is divided (IEEE division) by the
 *   sum of its entries in ascending k; the missing symbol has emission 1 (the doubles psmc_hip_get_tables returns as f in exact mode);
 *   random numbers, counter based, on 64-bit unsigned integers: mix(z): z ^= z >> 30, z *= 0xbf58476d1ce4e5b9, z ^= z >> 27,
 *   z *= 0x94d049bb133111eb, z ^= z >> 31;  G = 0x9e3779b97f4a7c15;  key = mix(mix(seed + G*(j+1)) + G*(q+1));  at position u = 1..L:
 *   z = mix(key + G*u), r = ((z >> 11) + 1) * 2^-53, in (0, 1];
 *   the draw from weights w_0..w_{n-1}: c_l = the running sum from 0.0 in ascending l, x = r * c_{n-1} (one rounded product), the index
 *   is the number of l < n with c_l < x: never a leading run of zero weights (r > 0), never beyond n - 1 (r <= 1).  A total c_{n-1} of 0
 *   or NaN gives index 0, and a count of n -- only weights below zero can produce it -- gives n - 1: there is no error path;
 *   the path of sample j: s_L is drawn with r(., L) from w = f_L; for u = L-1 down to 1, s_u is drawn with r(., u) from
 *   w_l = f_u[l] * a[l][s_{u+1}], each product rounded once (the running sum whose last value is tmp of the forward step for column
 *   s_{u+1}); path[u-1] = s_u.
 * The draw at u is a map from the state at u + 1 to the state at u that does not depend on the sample's history: the sweep stores it
 * for every state, 1 byte per (bin, state padded to a multiple of 64) up to 256 states and 2 bytes beyond, one such table per sample of
 * a group ("samp_group"), and psmc_hip_viterbi's tiled backtrace ("vit_tile") composes the maps of each sample.
 * The call reads the observations only: every table, plan, learned state and selection of the context stays as it was, and the
 * device memory it allocates is released before it returns.
 * PSMC_HIP_EINVAL: a NULL parameter or path, n_samp < 1.  PSMC_HIP_ESTATE: no segments loaded.  PSMC_HIP_ENOMEM: one sample's table does
 * not fit; the message holds its size. */
int psmc_hip_sample_paths(psmc_hip_ctx *ctx, const double *a, const double *e, const double *a0,
                          uint64_t seed, int32_t n_samp, const uint64_t *stream, int32_t *path);

/* Decoding on a FAST context (up to 128 states): psmc_hip_decode, _posterior, _post_counts, _scales, _post_mean and _post_quantile read what the last
 * single E-step (psmc_hip_estep / _estep_device) left:
 *   - the fast tables X and bt -- the dense sweeps (any matrix, <= 64 states) or the structured ones with the unfused back half
 *     ("fuse" = 0 up to 64 states, "fuse128" = 0 for 65..128): scale-free kernels (estep_post_fast.hip) compute
 *     gamma_u(k) = X_u(k) bt_u(k) / e_k(o_u) normalised over k, i.e. the posterior of k_expect_mfma, not the reference's doubles.
 *     Tolerances against an exact context given the same parameters: posterior rows, maxp and recomb within 1e-9 absolute;
 *     scales 1e-11 relative; post_counts 1e-9 relative on every cell >= 1e-6 of the largest; the path equal wherever the two
 *     largest exact posteriors differ by more than 2e-9 (a near-tie may go either way);
 *   - the exact tables (65..128 states and a matrix without the PSMC form: fast mode ran the exact kernels): the exact
 *     kernels, the reference's doubles;
 *   - PSMC_HIP_ESTATE after the fused or the factored back half (no bt: set "fuse" / "fuse128" to 0 first), after a batch,
 *     or before any single E-step; PSMC_HIP_ENOTSUP after an E-step whose forward fix pass ran ("merge" = 1).
 * A decoding call reads the tables only: it changes nothing a later E-step uses (plan, glue, warm-ups).
 *
 * 129..256 states with "wide_fast" = 1 or 2, 257..1024 states with "wide_fast" = 2, and "wide_decode" = 1: the same rule -- the
 * last single E-step decides.
 *   - a wide fast factored E-step (psmc_hip_estep_factored / _estep_factored_device) that returned 0: one more backward sweep per
 *     tile (estep_wide_post.hip; beyond 256 states a tile is one work-group of 2..4 waves over X at
 *     the padded width 512 / 768 / 1024) from the tile's converged start vector bt_{top+1}, reading X; no backward table exists
 *     or is written.  With y = a bt_{p+1}:  gamma_p(k) = X_p(k) y(k) / G_p,  G_p = sum_k X_p(k) y(k)  (the posterior the E-step's E adds
 *     up; no division by an emission);  recomb_p = 1 - sum_l X_p(l) a_ll bt_{p+1}(l) / G_p;  at p = L: gamma_L = X_L / sum X_L,
 *     recomb_L = 0;  the path takes the lowest state among equal maxima;  s_p = sum X_p / sum X_{p-1} / inv_p with a tile's own
 *     start vector for X_{lo-1}, s_1 = sum_k a0_k e_k(o_1);  post_counts adds per-tile partials in tile order.  Tolerances: the
 *     ones above (1e-9 absolute, scales 1e-11 relative, counts 1e-9 relative, path equal away from near-ties of 2e-9);
 *   - psmc_hip_estep (the wide exact kernels): the exact tables, the reference's doubles, as without the option;
 *   - PSMC_HIP_ESTATE before any single E-step, after a batch, after a wide fast E-step that returned an error (ECONVERGE: its
 *     boundaries are not converged), after psmc_hip_select / a reload since that E-step, or for a segment that was not in its
 *     selection.
 *   - a wide fast factored E-step that kept checkpoints only ("wide_ckpt" = 1 while "wide_decode" was 0, or with
 *     "wide_decode_ckpt" = 1): with "wide_decode_ckpt" = 1 at the decoding call the same sweep, every block of eight positions
 *     recomputed forward from its checkpoint X_{8m} (in a tile's lowest block from the tile's start vector, or from a0 e(o_1)) with
 *     the stored 1/d -- the formulas, tolerances and state rules above, and the bits of decoding from the full table; the scales
 *     from one forward pass per tile.  With "wide_decode_ckpt" = 0: PSMC_HIP_ESTATE (the message names the checkpoints) until an
 *     E-step has kept the full table;
 * With "wide_decode" = 0 -- and beyond 256 states with "wide_fast" = 1 -- such a context decodes from the exact tables whatever
 * ran last (ESTATE when there are none).  psmc_hip_get_tables always reads the exact tables.
 * What it is worth beyond 256 states, on the 2.2 M-bin stress fixture (scripts/wide_fast_timing.py --decode --stress, one E-step plus
 * every decoding call over all segments, profiles/wide_fast_timing.txt): 0.69 s at 300 states against 19.2 s on the exact kernels,
 * 1.15 s at 1024 states against 193.8 s.  The E-step is the gain; of the calls themselves psmc_hip_scales (4 / 5 ms against a
 * 0.6 ms copy of the exact table) and, at 300 states, psmc_hip_decode (34 ms against 5 ms) are slower than their exact twins. */

/* ---- one E-step sharded over several GPUs of the node (replaces em.c:36-55 + the serial
 * hmm_add_expect of khmm.c:346-359 by per-device E-steps and ONE exchange per EM iteration).  One process; devices[]
 * lists the HIP devices (a device may appear twice: two shards on one GPU, for testing).  Segments are dealt to the
 * shards longest-first (LPT by length).  fast mode: RCCL all-reduce (sum, f64) of the n*n + 2n + 1 doubles each
 * device's reduction kernel left in HBM, over xGMI; exact mode: per-segment statistics gathered and added on the host
 * in the global input order -- bit-identical to the single-GPU result and to khmm.c.  librccl is opened on first use.
 * Options: every psmc_hip_set_option key (applied to all shards) and "rccl" (-1 auto: RCCL when the devices are
 * distinct and more than one shard holds segments, else the host adds the shards' vectors in shard order -- also when
 * librccl cannot be opened or refuses the communicator; 0 never; 1 always, e.g. a one-device group as a smoke test of
 * the RCCL path: a missing RCCL is then an error; 2 (tests) always, and the devices may repeat -- for a stand-in library
 * named by the environment variable PSMC_HIP_RCCL_LIB (tests/stub_rccl), which is loaded instead of librccl when set). */
typedef struct psmc_hip_group psmc_hip_group;
int  psmc_hip_group_create(psmc_hip_group **g, int n_states, int n_dev, const int *devices, int mode);
void psmc_hip_group_destroy(psmc_hip_group *g);
const char *psmc_hip_group_last_error(const psmc_hip_group *g);
int  psmc_hip_group_set_option(psmc_hip_group *g, const char *key, double value);
int  psmc_hip_group_load_segments(psmc_hip_group *g, int n_seg, const uint8_t *const *seq, const int32_t *L);
/* as psmc_hip_estep / psmc_hip_estep_factored, over all shards; chk has n_seg entries in input order */
int  psmc_hip_group_estep(psmc_hip_group *g, const double *a, const double *e, const double *a0, double *A, double *E,
                          double *A0, double *LL, double *chk);
int  psmc_hip_group_estep_factored(psmc_hip_group *g, const double *a, const double *e, const double *a0, double *sums,
                                   double *E, double *LL);
/* First contact with a multi-GPU node, callable before any segment is loaded: every listed device answers, the
 * exchange the E-steps will use comes up (RCCL communicator, or the host sum) and adds correctly in stream order (shard
 * s puts s + 1 into its vector with an asynchronous copy on its E-step stream, the reduction follows on the same stream,
 * every device must then hold n(n+1)/2).  out (may be NULL) = {shards, path as last_reduce below (1 RCCL, 2 host sum,
 * 0 single shard, 3 exact mode: nothing to exchange), communicator up (0/1), RCCL wanted but unusable (0/1; the reason
 * is then in psmc_hip_group_last_error although the call succeeds, auto mode falls back to the host sum)}.  A failure
 * names the step that failed.  bench.py --engine group calls this first. */
int  psmc_hip_group_selfcheck(psmc_hip_group *g, int out[4]);
/* shard_of_seg: n_seg entries (may be NULL); last_reduce: 0 none (one shard), 1 RCCL all-reduce, 2 host sum of the
 * shards' vectors, 3 ordered per-segment sum (exact mode) */
int  psmc_hip_group_info(psmc_hip_group *g, int *n_shards, int32_t *shard_of_seg, int *last_reduce);
/* the context and local index holding segment `seg` after a group E-step, for psmc_hip_get_tables / _decode /
 * _posterior / _post_counts / _scales (psmc_decode, aux.c:150-231) */
int  psmc_hip_group_route(psmc_hip_group *g, int seg, psmc_hip_ctx **ctx, int *local_seg);
/* psmc_hip_estep_factored with the result left in HBM: [SL|SU|DG|CL|CU | E | LL], 7n + 1 doubles, asynchronous on
 * `stream` like psmc_hip_estep_device */
int  psmc_hip_estep_factored_device(psmc_hip_ctx *ctx, const double *a, const double *e, const double *a0, void *d_stats,
                                    void *stream);

#ifdef __cplusplus
}
#endif
#endif
