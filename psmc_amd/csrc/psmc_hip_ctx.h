// psmc_hip_ctx.h -- the context behind the C-ABI of include/psmc_hip.h and the helpers its translation units share:
//   api.hip        context, options, segments, parameter staging, tables, exact mode, the table reader
//   api_fast.hip   fast mode: tile plan, sweep items, learning, the launch of one fast E-step and its entry points
//   api_wide_fast.hip  fast mode at 129..256 states ("wide_fast") and 257..1024 states ("wide_fast" = 2): plan, rounds and launch of the factored E-step; the full counts of that path ("wide_counts")
//   api_decode.hip psmc_hip_decode / _posterior / _post_counts / _scales from the exact, the fast or the wide fast tables (one wave per tile or 2..4)
//   api_viterbi.hip psmc_hip_viterbi: the Viterbi path of every segment (reads the observations only)
//   api_sample.hip psmc_hip_sample_paths: state paths drawn from the posterior, forward filtering and backward sampling (reads the observations only)
//   api_batch.hip  psmc_hip_estep_batch (bootstrap replicates): exact launch groups, fast per-replicate plans
//   api_probes.hip device self-test, microbenchmarks and probes (diagnostics)
// Everything is built with -ffp-contract=off: no host or device expression is ever fused.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>
#include "psmc_hip.h"
#include "psmc_hip_internal.h"
#include "wide_fast.h"

using namespace psmc;

#define HMM_TINY_H 1e-25

// psmc_hip_ctx::dec_kind: the tables the decoding entry points of a fast context (<= 128 states) would read (api_decode.hip)
constexpr int DEC_NONE = 0;   // no single E-step since the tables were last used otherwise (or it failed)
constexpr int DEC_FAST = 1;   // the fast tables X and bt (dense sweeps, or the structured ones with the unfused back half): estep_post_fast.hip
constexpr int DEC_EXACT = 2;  // the exact tables (65..128 states, a matrix without the PSMC form: fast mode ran the exact kernels)
constexpr int DEC_NO_BT = 3;  // the fused or factored back half: no backward table
constexpr int DEC_MERGED = 4; // the forward fix pass ("merge"): its X carries per-tile factors
constexpr int DEC_WIDE = 5;   // never stored, decode_source returns it: the tables of the wide fast path ("wide_decode"; estep_wide_post.hip: 129..256 states, 257..1024 with "wide_fast" = 2)
// psmc_hip_ctx::wd_kind: what the last wide fast E-step of the context left (set in api_wide_fast.hip, read by api_decode.hip decode_source)
constexpr int WD_NONE = 0;    // there was none, or a batch came after it
constexpr int WD_OK = 1;      // X, 1/d, entry and a converged bentry of every tile of its plan
constexpr int WD_FAILED = 2;  // it returned an error: bentry is not converged

struct psmc_hip_ctx;

// Device memory (BUF_DEVICE), pinned host memory (BUF_PINNED) or pinned host memory mapped into the device (BUF_MAPPED, `dev` its
// device view) of a context.  A buffer that owns its block frees it when it is reset, allocated again or destroyed; one that
// borrows another's block never frees.  Reads as the plain pointer.
enum BufKind { BUF_DEVICE, BUF_PINNED, BUF_MAPPED };
template <class T, BufKind K = BUF_DEVICE> struct Buf {
	T *p = nullptr, *dev = nullptr;
	size_t cap = 0; // elements (0 for a borrowed block)
	bool owned = false;
	Buf() = default;
	Buf(const Buf &) = delete;
	Buf &operator=(const Buf &) = delete;
	~Buf() { reset(); }
	operator T *() const { return p; }
	void reset()
	{
		if (p && owned) (void)(K == BUF_DEVICE ? hipFree(p) : hipHostFree(p));
		p = dev = nullptr; cap = 0; owned = false;
	}
	void borrow(T *q) { reset(); p = q; }
	hipError_t try_alloc(size_t n); // frees the old block first; n == 0 is one element; no error text, no poison fill
	int alloc(psmc_hip_ctx *c, size_t n); // try_alloc, PSMC_HIP_ENOMEM through fail(), the PSMC_HIP_POISON fill (defined below fail())
	int grow(psmc_hip_ctx *c, size_t n) { return p && n <= cap ? 0 : alloc(c, n); } // (an empty buffer gets its block even for n == 0)
};

// The options a replicate context of a fast batch inherits from its parent: api_batch.hip batch_child assigns this block in one
// statement (and then sets `chunk` and `tail` its own way).  An option that the replicates must see goes here; everything else is
// in psmc_hip_ctx itself.
struct psmc_hip_opts {
	int chunk = 0, warmup = 3072, max_rounds = 4096, rep_impl = -1, n_sub = 6, target_waves = 1536, overlap = 1;
	double warm_tol = 1e-12;
	int struct_opt = 1;        // "structured": 1 = use the O(N) sweeps when a[][] factors (auto), 0 = always dense
	bool struct_tiles_set = false; // the caller chose struct_tiles: no adaptation to small inputs
	int struct_tiles = 8192;   // "struct_tiles": tiles aimed at when the structured sweeps are used (4 per wave)
	int kc_sub = 4;            // "kc_sub": k_kcol2_struct cuts a tile's steps into this many ranges, one matrix (and one pair of waves) each; default: by the plan
	int kcol_prio = 2;         // "kcol_prio": wave priority of k_kcol2_struct
	int two_phase = -1;        // "two_phase": 2 = the fused back half runs as two launches and the tiles of the second list with an odd index start from
	                           // the exit vector of the tile above instead of speculating; 0 = every tile speculates; -1 = by the plan
	int merge1 = -1;           // "merge1": bulk forward sweep + backward warm-up pass in one grid (k_sweep_struct); -1 = by the plan (shard-sized inputs)
	int merge_order = -1;      // "merge_order": block order of that grid: 1 = forward blocks, then backward blocks; 0 = alternating (every XCD gets one
	                           // direction); -1 = by the plan: 1 while a tile is shorter than its warm-up (measured: 3.75 M bins 3.00 vs 3.25 ms, 7.5 M equal, 15 M 7.9 vs 7.6)
	int lanes8 = -1;           // "lanes8": 64 states, fused / factored plans: the bulk sweeps of phase 1 run eight tiles per wave (8 lanes x 8 states: a quarter
	                           // fewer vector instructions per tile-step, half the waves).  -1 = with the factored statistics of a genome-sized input only (more than one round of tiles) -- measured (round 4, genome):
	                           // factored 10.26 -> 9.91 ms; full counts 12.09 -> 12.73 (its forward sweep is paced by 15.6 GB of stores and half as many waves hide less)
	int gate = -1;             // "gate": order the dispatch of phase 1's grids walks -> bulk -> transfer matrices (estep_struct.hip k_gate); -1 = with coarse
	                           // items (measured: without them the bulk grid is the critical path and walks that land late, stacked on few SIMDs, slow fewer of its waves)
	int coarse = -1;           // "coarse": a bulk sweep item spans up to this many consecutive tiles of a segment: ONE speculative warm-up per item and
	                           // direction, the backward pass walks the item and leaves every tile's start vector (build_items); -1 = by the plan
	bool warm_shift_set = false, kc_sub_set = false;
	int kc_div = 16;           // "kc_div": at most n_tiles / kc_div tiles per direction get a transfer matrix (16 tile sweeps of work each)
	int kc_min = -1;           // "kc_min": runs of at least this many tiles get the transfer-matrix chain instead of a walk (0: never; -1: 4 / 5 with
	                           // 64 states (one round of tiles / two), 8 / 12 with 65..128 -- measured, build_items)
	int ckpt = 1;              // "ckpt": factored statistics recompute X from checkpoints every 8 positions instead of reading the table
	int fuse = 1;              // "fuse": backward sweep and counts in one kernel (estep_fused.hip): structured matrices, up to 64 states
	int fuse128 = 2;           // "fuse128": the same with 65..128 states: 2 = k_bwd_count8x_struct (sixteen tiles per work-group, one sweep per tile, operands
	                           // exchanged through LDS), 0 = unfused (1, round 3's kernel -- four waves redo the sweep of four tiles -- was removed in round 6)
	// Round 6: mis-speculation made cheap, then warm-ups sized per tile -- built, measured, and OFF: halving every warm-up at no
	// cost at all is worth 0.35 ms of 12.25 (profiles/r06_warmup_sensitivity.txt), and the three together cost more than that (profiles/r06_fix_pass_ab.txt).
	int merge = 0;             // "merge": the forward fix pass between the forward sweep and the back half (estep_struct.hip FwdCtl): a mis-speculated tile is rewritten
	                           // until it meets its stored trajectory, nothing is counted twice (0: verify afterwards, whole tiles and their groups of the counts again)
	int adapt = 0;             // "adapt": with "merge", every speculating tile's forward warm-up follows the mismatch its speculation left at the last E-step (0: "warmup" for all)
	int prev_start = 0;        // "prev_start": forward warm-ups start from the previous E-step's X at that position instead of the stationary vector
	int learn = 1;             // "learn": glue tiles that needed a repair to their neighbour for the following E-steps
	int warm_shift = 1;        // "warm_shift": before that, once, give such a tile a warm-up of warmup << warm_shift bins (0: glue at once)
	int group_cap = 131072;    // "group_cap": longest run of glued tiles, in bins
	int gap_tiles = 1;         // "gap_tiles": 0 = treat tiles of missing data like any other (rounds 1-4)
	int hom_tiles = 0;         // "hom_tiles": 1 = on (the rule: psmc_hip_ctx::hom)
	int hom_min = 0;           // "hom_min": bins; 0 = auto = warmup / 4
	int runs_late = 1;         // "runs_late": two-phase plan, 1 = run tiles go to the second launch of the fused back half
	int tail = 1;              // "tail": fused back half, 1 = the counts waves verify the backward boundaries and the reductions follow the counts
	                           // directly, list A's half beside list B (estep_fast.hip launch_fast); 0 = verify, compaction and reductions behind list B
	int exact_refwd = -1;      // "exact_refwd": exact batch, 64 states: 1 = no f table, the expect pass recomputes the forward sweep (twice the replicates
	                           // per group at +0.4 us per bin of the longest segment); 0 = tables for f and b; -1 = only when the tables of all
	                           // replicates do not fit one launch group (api_batch.hip batch_refwd)
};

// The streams and events of a root context; its batch children borrow them.  A base of psmc_hip_ctx: bases are destroyed after the
// members, so the buffers are freed first, then the events, then the streams.
struct psmc_hip_runtime {
	hipStream_t stream = nullptr, stream2 = nullptr, stream3 = nullptr, stream4 = nullptr, stream5 = nullptr;
	hipEvent_t ev[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	hipEvent_t evx[14] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	bool runtime_owned = true;
	psmc_hip_runtime() = default;
	psmc_hip_runtime(const psmc_hip_runtime &) = delete;
	psmc_hip_runtime &operator=(const psmc_hip_runtime &) = delete;
	void borrow_runtime(const psmc_hip_runtime &o)
	{
		stream = o.stream; stream2 = o.stream2; stream3 = o.stream3; stream4 = o.stream4; stream5 = o.stream5;
		for (int i = 0; i < 10; ++i) ev[i] = o.ev[i];
		for (int i = 0; i < 14; ++i) evx[i] = o.evx[i];
		runtime_owned = false;
	}
	~psmc_hip_runtime()
	{
		if (!runtime_owned) return;
		for (int i = 0; i < 10; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]);
		for (int i = 0; i < 14; ++i) if (evx[i]) (void)hipEventDestroy(evx[i]);
		if (stream4) (void)hipStreamDestroy(stream4);
		if (stream5) (void)hipStreamDestroy(stream5);
		if (stream2) (void)hipStreamDestroy(stream2);
		if (stream3) (void)hipStreamDestroy(stream3);
		if (stream) (void)hipStreamDestroy(stream);
	}
};

struct psmc_hip_ctx : psmc_hip_opts, psmc_hip_runtime {
	int n = 0, ns = 64, device = 0, mode = PSMC_HIP_MODE_EXACT; // ns: states padded to 64 or 128
	std::string err;
	// Options: those a batch replicate inherits are in psmc_hip_opts.  Every option below is per context and is NOT inherited -- the
	// wide_* and batch_* options, share_learn, warmup_set, vit_tile, samp_group, and phase1 / phase1_waves, although these two look
	// like plan options: a replicate runs with their defaults.
	bool use_struct = false, planned_struct = false;
	int last_fused = 0, last_ckpt = 0; // what the last fast E-step ran: EstepLaunch::fused / ckpt
	// what the last single E-step of a fast context left for the decoding entry points (api_decode.hip decode_source), and the table
	// serial it left it at: any later use of the tables (another E-step, a batch) makes it stale
	int dec_kind = 0; unsigned long long dec_serial = 0;
	bool want_factored = false; // this call asked for the factored statistics (psmc_hip_estep_factored)
	int two_phase_used = 2;    // what plan_fast chose about "two_phase"
	int merge1_used = 0;       // ... and about "merge1"
	Buf<int> d_gate;           // "gate": the words k_gate orders phase 1's grids by, then the head of the work queue below
	int phase1 = -1;           // "phase1": 1 = phase 1's bulk blocks (forward sweep, backward warm-up pass) from one work queue, longest first, pulled by a
	                           // persistent grid (estep_struct.hip k_phase1_queue); 0 = two launches on streams of their own; -1 = by the plan
	int phase1_waves = 2;      // "phase1_waves": waves per SIMD of that grid
	Buf<int> d_queue;          // the queue (build_items), n_queue entries
	int n_queue = 0;
	int coarse_used = 1, items_coarse = -1;
	int warm_shift_used = 1, kc_sub_used = 4;
	int n_wl_f = 0, n_wl_b = 0, n_kc = 0, n_chain_f = 0, n_chain_b = 0, n_singles_b = 0;
	Buf<double> d_Kcol;
	int count_group = 4;       // tiles per work-group of the fused back half, what the tile lists are padded to (build_items)
	Buf<int, BUF_MAPPED> h_mlen;     // [n_chunks]: blocks each merging repair rewrote / -1 ("merge", "adapt")
	Buf<double, BUF_MAPPED> h_mis;   // [2][n_chunks]: first-verify mismatch of every tile, forward | backward
	Buf<double> d_prevx, d_finv;     // [n_chunks][ns] gathered start vectors; [n_chunks] scale factors of the merging repairs
	std::vector<int> order_f;                        // head tiles of the bulk forward items in launch order (build_items): adapt_warmups looks at how well the rows of a wave still match
	int n_fix_f = 0;
	bool merge_used = false;                         // what the last E-step decided about "merge"; n_fix_f: tiles of its first fix launch
	Buf<Chunk, BUF_PINNED> h_chunks;                 // staging copy of the tiles (their warm-ups change between E-steps)
	bool prev_ok = false;                            // the X table holds a complete forward sweep of THIS plan ...
	unsigned long long prev_serial = 0, tab_serial = 0; // ... and nobody has used the tables since (tab_serial: on the root context, ensure_tables)
	const double *prev_f = nullptr; int prev_ckpt = 0;
	bool chunks_dirty = false; // a tile's warm-up changed: d_chunks is stale
	Buf<int> d_items;          // items_f | items_b | ritems_f | ritems_b, 2*n_chunks ints each
	Buf<int, BUF_MAPPED> h_ritems; // 2 * 2*n_chunks ints
	std::vector<uint8_t> glue_f, glue_b; // glue_f[b]: tile b continues the forward item of b-1; glue_b[b]: b continues b+1's backward item
	std::vector<uint8_t> gap;            // gap[b]: tile b is a FULL tile of missing data inside its segment (plan_fast: k_tile_class; "gap_tiles"): glued at once,
	                                     // free of "group_cap", one shared transfer matrix per direction (build_items)
	// "hom_tiles": runs without a heterozygous bin.  A HOM TILE is a full tile of k_tile_class 2 (all homozygous) or 3 (het-free: homozygous and
	// missing bins) that is neither the first nor the last tile of its segment -- what a gap tile is for missing data.  A QUALIFYING RUN is a
	// maximal sequence of consecutive tiles of one segment, each a hom tile or a gap tile, at least one of them a hom tile, whose hom tiles total at
	// least "hom_min" bins.  plan_fast glues every tile whose warm-up window overlaps a tile of a qualifying run (forward: [lo - wf, lo - 1];
	// backward: [hi + 1, hi + wb]) after the gap-tile rule, the flags OR-ed.  build_items: the all-homozygous tiles of qualifying runs share one
	// transfer matrix per direction as gap tiles do (a slot of their own, under the same T % 4 == 0), and those that share one cost nothing
	// towards the chain budget and count no bins towards "group_cap"; het-free mixes keep a matrix each and count in full.
	std::vector<uint8_t> hom;            // hom[b]: 0 = no hom tile, 1 = hom tile outside a qualifying run, 2 = het-free mix in a qualifying run, 3 = all homozygous in one
	int n_kuniq = 0;                     // transfer-matrix slots of the current item lists
	std::vector<int> flagged_f, flagged_b;
	bool items_dirty = true;
	int n_items_f = 0, n_items_b = 0;
	int n_sub_used = 6;
	// segments
	int n_seg = 0;
	std::vector<int32_t> L;
	std::vector<int64_t> off;
	int64_t total = 0; // padded bins
	Buf<uint8_t> d_obs; // borrowed: psmc_hip_load_segments_device (the caller's), a batch child and the exact twin (the parent's)
	Buf<int64_t> d_seg_off;
	Buf<int32_t> d_seg_len;
	// selection
	std::vector<int32_t> sel;      // as given
	std::vector<int32_t> work;     // unique selected ids
	std::vector<int32_t> sel2work; // sel[i] -> index into work
	std::vector<int32_t> mult;     // per work item
	Buf<int32_t> d_work;
	bool plan_dirty = true;
	// parameters (a batch child borrows its parent's)
	Buf<double, BUF_PINNED> h_par; Buf<double> d_par; // a | aeT(3) | e(3) | a0 | re(3)
	size_t par_len = 0;        // doubles in one parameter block: PAR_LEN up to 128 states, 2 S^2 + 4 S beyond (a | aT | e(3) | a0, estep_wide.hip)
	static constexpr size_t PAR_LEN = 2 * 16384 + 3 * 128 + 128 + 3 * 128 + 5 * 128 + 2 * 11 * 128; // ns=64: ... | re(3) | sp(5) (17152) | kcc; ns=128: a | aT | e(3) | a0 | re(3) | sp(5) | kcc
	static constexpr size_t RE128_OFF = 2 * 16384 + 3 * 128 + 128, SP128_OFF = RE128_OFF + 3 * 128, KCC128_OFF = SP128_OFF + 5 * 128;
	static constexpr size_t SP_OFF = 4 * 4096 + 192 + 64 + 192; // structured vectors P | R | qa | c | dd
	static constexpr size_t KCC_OFF = SP_OFF + 5 * 64;          // 64 states: constant tables of k_kcol2_struct, 2 x (2*64 + 9*64) doubles (the 128-state layout's space, unused here)
	// tables (a batch child borrows its parent's: ensure_tables)
	Buf<double> d_f, d_b, d_s, d_sb;
	int64_t tab_bins = 0; bool have_b = false;
	// exact outputs
	Buf<double> d_segA, d_segE, d_segA0, d_chk;
	int seg_cap = 0;
	std::vector<double> h_segA, h_segE, h_segA0, h_chk, h_s;
	// fast
	std::vector<Chunk> chunks;
	Buf<Chunk> d_chunks;
	int chunk_cap = 0, chunk_used = 0;
	Buf<double> d_entry, d_bentry, d_bexit, d_Cpart, d_Epart, d_LLpart; // (d_Cpart is sized per E-step: api_fast.hip enqueue_fast)
	Buf<int> d_dirty, d_cnt, d_touch;
	Buf<int, BUF_MAPPED> h_cnt;
	bool timing_two_launches = false; // the fused back half ran as two launches (lists A and B): evx[11] / evx[12] sit between them
	int n_long_f = 0, n_long_b = 0, n_mem_f = 0, n_mem_b = 0;
	int n_B_b = 0, n_list_a = 0, n_list_b = 0; // two-phase plan: trailing backward items that start from above; tile lists of the fused back half
	int items_two_phase = -1;  // what the current item lists were built for
	bool runs_in_b = false;    // two-phase plan: every tile of a glued run is in the second list of the fused back half (build_items)
	Buf<int> d_ftiles;         // [2 * (chunk_cap + 16)] tile lists A | B of the fused back half (bit 30: start from the tile above), then [chunk_cap]
	                           // who tests each backward boundary ("tail" = 1: TailVerify::cover, psmc_hip_internal.h)
	size_t vcover_off = 0;     // ... where that table starts in d_ftiles (ints)
	FastReport report = {0, 0, 0, 0, 1, 0, 0};
	Buf<double> d_stage, d_stats;
	Buf<unsigned long long> d_warm;
	double warm_err[2] = {0, 0};
	// timing of the last E-step (the streams and events: psmc_hip_runtime)
	double last_ms[7] = {0, 0, 0, 0, 0, 0, 0};
	bool timing_valid = false;
	// batch (psmc_hip_estep_batch)
	int64_t batch_bins = 0;            // "batch_bins": table bins per launch group of the exact batch (0 = from free memory)
	Buf<int32_t> d_bw_seg, d_bw_par; Buf<int64_t> d_bw_tab; size_t bw_cap = 0; // work list of a group
	Buf<double> d_bpar;                // [n_rep][par_len] parameter blocks of a batch call
	Buf<int> d_cu_mask;                // k_expect_exact_rf2: one word per compute unit (which role order its resident work-groups took), 4096 words
	Buf<double> d_lkp; std::vector<double> h_lkp; // hmm_lk's logged products of a launch's entries (k_lk_products)
	Buf<int64_t> d_lkoff;              // ... and where each entry's begin
	Buf<double> d_s_all;               // exact batch without the f table, several groups: the scale factors of ALL replicates (one forward pass)
	int batch_sort = 1;                // "batch_sort": the exact batch deals ENTRIES to its launches longest first (api_batch.hip); 0 = replicate-major order
	int batch_tailfill = 1;            // "batch_tailfill": the exact batch puts the shortest entries into the spare slots of the memory-bound launches when that saves a launch
	int batch_major = 1;               // "batch_major": blocks no longer than the dominant trunk length keep replicate order (replicates complete launch by launch)
	int batch_first = 0;               // "batch_first": the next batch calls' replicate 0 is replicate batch_first of the context (fast mode: which kept plan it uses)
	Buf<double> d_b2; int64_t b2_bins = 0, b2_alloc = 0; // exact batch without the f table: a second chunk of b table, allocated when memory became free later (api_batch.hip)
	int64_t reserved_cap = 0;          // ... and the per-launch capacity it sized the tables for
	int reserved_refwd = -1;           // what psmc_hip_reserve_batch_tables decided about the f table (-1: nothing reserved): the batches that follow keep it
	int cu_first = 0, cu_count = 0;    // psmc_hip_set_cu_range: the streams of this context are masked to these compute units (0: the whole device)
	int last_batch_groups = 0;
	bool tables_batch = false;         // the tables hold the slots of a batch group, not the segments at their own offsets
	// fast batch: one plan-holding child per replicate; children share the parent's streams, events, parameter
	// staging, observations and TABLES (they run one after the other)
	psmc_hip_ctx *x_twin = nullptr;    // fast batch: an exact-mode context over the same observations, made when a replicate's fast E-step does not converge (api_batch.hip batch_exact_once)
	int n_exact_fallbacks = 0;
	psmc_hip_ctx *parent = nullptr;
	std::vector<psmc_hip_ctx *> kids;
	// ... and what the replicates of one parent have LEARNED is shared through the parent (round 4): they tile every segment with the
	// same tile length share_T, so a tile is (segment, index) in all of them, and a replicate that plans starts from the glue flags and
	// warm-ups its predecessors needed (the slow regions belong to the data: the first E-step of replicate 2..R no longer repeats the
	// repair rounds of replicate 1).  Filled by learn_groups of the children, read by their plan_fast (api_fast.hip).
	int share_learn = 1;       // "share_learn": 0 = every replicate of a fast batch learns for itself (and tiles its own selection)
	int share_T = 0;
	std::vector<std::vector<uint8_t>> sh_glue_f, sh_glue_b;   // [segment][tile index]
	std::vector<std::vector<int32_t>> sh_wf, sh_wb;
	std::vector<int32_t> chunk_seg, chunk_idx;                // of every tile of the current plan
	// PSMC_HIP_DEBUG_TIMES: host seconds spent in the pieces of the fast E-steps of this context and its batch children since the last
	// report -- [0] replicate context creation, [1] select, [2] plan_fast (tiling + per-plan allocations), [3] build_items,
	// [4] launch_fast (kernels + verify / repair rounds, synchronous), [5] result read-back; and [6] repair rounds, [7] repaired tiles
	double dbg_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	// fast mode beyond 128 states (api_wide_fast.hip): "wide_fast" = 1 runs psmc_hip_estep_factored[_device] of a fast context with 129..256
	// states on the kernels of estep_wide_fast.hip, in tables of its own (the exact tables stay what the last exact E-step left);
	// "wide_fast" = 2: the same, and 257..1024 states on the same kernels with 2..4 waves per tile
	int wide_fast = 0;
	bool wf_ran = false;                 // the last fast E-step of this context was one of the wide path (fast_info, fast_diag)
	std::vector<Chunk> wf_chunks;        // its plan; rebuilt when plan_dirty
	Buf<Chunk> d_wf_chunks;
	int wf_cap = 0, wf_T = 0, wf_W = 0;  // tiles allocated; tile length and warm-up of the plan
	bool warmup_set = false;             // "warmup" was set: the wide path takes it instead of its own default (api_wide_fast.hip)
	Buf<double> d_wf_X, d_wf_inv; int64_t wf_bins = 0; // X [bins][padded width of the path: ns up to 256 states, 512 / 768 / 1024 beyond], 1/d_p [bins]
	Buf<double> d_wf_par; Buf<double, BUF_PINNED> h_wf_par;             // e0 | e1 | a0 | P | R | qa | c | dd
	Buf<double> d_wf_entry, d_wf_bentry, d_wf_bexit, d_wf_part, d_wf_ll;
	Buf<int> d_wf_dirty, d_wf_list;
	// "wide_ckpt" = 1: a wide fast E-step keeps X at every 8th position only (by absolute position: row (off >> 3) + (p >> 3) - 1 for
	// p % 8 == 0) and every tile's last row in d_wf_xhi; its accumulate sweep recomputes the rest.  "wide_decode" = 1 wins: the
	// decoding kernels read full rows.  wf_rows / wf_tab_iv: rows of d_wf_X and the interval it was sized for; wf_last_iv: the
	// interval of the last wide fast E-step (0: none ran) -- fast_info, psmc_hip_wide_table_info, decode_source
	int wide_ckpt = 0;
	Buf<double> d_wf_xhi; // [tiles][padded width]
	int64_t wf_rows = 0; int wf_tab_iv = 0, wf_last_iv = 0;
	// "wide_decode" = 1 (with "wide_fast"; beyond 256 states with "wide_fast" = 2): the decoding entry points of such a context read the
	// tables of the wide path when the last single E-step was one of its own.  wd_serial: the table serial at that E-step -- an exact E-step or a batch moves tab_serial on,
	// and the exact tables are the newer ones; wd_sel: the selection serial it ran with (psmc_hip_select moves sel_serial on)
	int wide_decode = 0;
	// "wide_decode_ckpt" = 1: a "wide_ckpt" E-step keeps checkpoints whatever "wide_decode" says, and the decoding entry points read
	// them (wf_last_iv == 8: the CKPT kernels of estep_wide_post.hip recompute the rows between them).  Read
	// by the E-step (the interval) and again by decode_source at every decoding call
	int wide_decode_ckpt = 0;
	int wd_kind = 0; unsigned long long wd_serial = 0, wd_sel = 0, sel_serial = 0;
	// "wide_batch" = 1: psmc_hip_estep_batch[_cb] of such a context, asked for sums only, runs every replicate's E-step on the wide fast
	// path -- on this context itself, one selection after the other: the path learns nothing, so no child contexts (api_batch.hip batch_wide)
	int wide_batch = 0;
	// "wide_counts" = 1: psmc_hip_estep of such a context (fast mode, a size "wide_fast" covers, "structured" on, a matrix of the PSMC
	// form) runs the factored wide E-step with the full X table and then the counts pass of estep_wide_counts.hip (api_wide_fast.hip
	// estep_counts_wide); the batch with "wide_batch" takes the wide path when A is asked for, too.  "wide_counts_slab": bins per
	// slab of that pass, 0 = auto.  wc_now: the E-step under way is one (interval 1 whatever "wide_ckpt" says, unless
	// "wide_counts_ckpt"); wc_ran: the last wide fast E-step was one (fast_info).  Device memory of the pass: one slab of V, the partial
	// matrices, a, A, the slab's ranges, and one int per tile.
	// "wide_counts_ckpt" = 1: a wide-counts E-step keeps checkpoints when "wide_ckpt" says so (and "wide_decode" without "wide_decode_ckpt"
	// does not forbid it); the counts pass follows wf_last_iv: at 8 k_wc_v CKPT recomputes the rows between the checkpoints and
	// writes the slab's X rows into d_wc_Xs (the V slab's size, allocated at the first such pass), which the GEMM reads
	int wide_counts = 0, wide_counts_slab = 0, wide_counts_ckpt = 0;
	Buf<double> d_wc_Xs;
	bool wc_now = false, wc_ran = false;
	Buf<double> d_wc_V, d_wc_P, d_wc_a, d_wc_out; // V: rows x width; P: doubles
	Buf<KRange> d_wc_kr; Buf<int32_t> d_wc_vrow;  // ranges; tiles
	// "wide_gap_tiles" = 1: plan_wide (api_wide_fast.hip) classifies the tiles of the wide plan with k_tile_class.  A GAP TILE is a full
	// tile (exactly T bins) of missing data only that is neither the first nor the last of its segment; a QUALIFYING RUN is a maximal
	// sequence of consecutive gap tiles of one segment that holds at least "wide_gap_min" bins (0 = auto: a quarter of the plan's
	// warm-up -- a shorter run leaves three quarters of a warm-up window as data, 12288 bins at the default, which
	// profiles/wide_fast_timing.txt measured as sufficient).  Glued forward: every gap tile of a qualifying run and every later tile of
	// the segment whose window lo - wf .. lo - 1 overlaps a tile of the run; backward: the mirror with hi + 1 .. hi + wb; never a tile
	// anchored in that direction.  Glued tiles do not speculate: the runs are crossed by the transfer-matrix chain of estep_wide_gap.hip.
	// wg_cls: 0, 1 = gap tile outside a qualifying run, 2 = gap tile of one; wg_glue: bit 0 forward, bit 1 backward, WG_FIRST_F / WG_FIRST_B
	// (wide_fast.h).  All empty / zero with the option off or without a qualifying run: then the E-step is the one without the option.
	int wide_gap_tiles = 0, wide_gap_min = 0;
	// "wide_hom_tiles" = 1, the same for runs of homozygosity.  k_tile_class answers 0 het, 1 all missing, 2 all homozygous, 3 het-free
	// mix.  A HOM TILE is a full tile (exactly T bins) of class 2 that is neither the first nor the last of its segment.  A CHAIN TILE is a
	// gap tile when "wide_gap_tiles" is on, or a hom tile when "wide_hom_tiles" is on; a RUN is a maximal sequence of consecutive chain
	// tiles of one segment, and it QUALIFIES when "wide_gap_tiles" is on and its gap tiles total at least "wide_gap_min" bins, or
	// "wide_hom_tiles" is on and its hom tiles total at least "wide_hom_min" bins (0 = auto for either: a quarter of the plan's warm-up).
	// With "wide_hom_tiles" = 0 that is the rule above.  Glue, levels, lists and chains do not look at what a tile holds: everything
	// above and below holds with "tile of a qualifying run" for "gap tile of a qualifying run".  A het-free tile with both kinds of bin
	// (class 3) is an ordinary data tile: it ends a run.  wg_cls gains 3 = hom tile outside a qualifying run, 4 = hom tile of one; the
	// chain applies the matrix of the tile's own kind (estep_wide_gap.hip: d_wg_Mh across class 4, d_wg_M across class 2).
	int wide_hom_tiles = 0, wide_hom_min = 0;
	// "wide_mix_tiles" = 1 (it has an effect only with "wide_hom_tiles" = 1): the class-3 tiles join the chain.  A MIX TILE is a full tile
	// (exactly T bins) of k_tile_class 3 -- no het, both symbol 0 and missing bins -- that is neither the first nor the last of its
	// segment.  Every mix tile of a qualifying run owns two matrices of n x S doubles (S the padded width), and "wide_mix_mb" (default
	// 2048, 1 .. 262144) caps their total: the mix tiles are ADMITTED in plan order for as long as the matrices of all admitted ones stay
	// within the cap (and they are no more than WG_MIX_MAX = 65535 tiles), and that happens before runs are formed.  An admitted mix tile is a chain tile beside gap and hom tiles; a mix
	// tile that is not admitted is an ordinary data tile and ends a run, as every mix tile does without the option.  A RUN is a maximal
	// sequence of consecutive chain tiles of one segment; the bins of its mix tiles count towards "wide_hom_min" like those of its hom
	// tiles.  Glue, chains, levels and walks are unchanged: they look only at which tiles belong to a qualifying run.  wg_cls gains
	// 5 = mix tile outside a qualifying run, or over the memory cap, and 6 = mix tile of a qualifying run; wg_mats gains bit 2.  The cap is
	// a condition, not a tuned number: at 1024 states a tile's two matrices are 16.8 MB, so the default holds about 120 tiles; at 200
	// states (S = 256) they are 0.8 MB and it holds about 2500.  With the option off, or without a class-3 chain tile in the input, plan,
	// launches and bits are those without it.
	int wide_mix_tiles = 0, wide_mix_mb = 2048;
	static constexpr int WG_MIX_MAX = 65535;
	std::vector<int32_t> wg_mix_slot, wg_mix_tiles; // [tiles] the slot of a class-6 tile's matrices, else -1; [slots] slot -> tile
	std::vector<int32_t> wg_mix_jobs; // 2 slot + dir for every matrix an E-step builds: F (dir 0) of a class-6 tile that a forward chain of the plan crosses, B (dir 1) where a backward chain does
	Buf<int> d_wg_mix_slot, d_wg_mix_tiles, d_wg_mix_jobs; // ... on the device (sized with d_wg_glue; jobs: twice that)
	Buf<double> d_wg_Mx; // [slots][2][n][padded width] every class-6 tile's F and B (written where wg_mix_jobs says), then [slots][2][ceil(T / 4)] their pilots' factors
	int wg_mx_T = 0, wg_mx_n = 0;   // the tile length and the slots d_wg_Mx was built for by the last wide fast E-step; 0: it built none (psmc_hip_wide_mix_matrix)
	std::vector<int32_t> wg_cls, wg_glue;
	// One direction of the plan's chains (d = 0 forward, 1 backward).  A chain starts behind the run's tiles that are anchored in its
	// direction (their speculation is exact) and ends with the start vector of the first tile behind the run, where one walk goes on
	// through the tiles glued behind it (`walk`).  A chain whose first vector comes out of the walk of the run before it in the segment
	// (two runs closer than a warm-up) is one LEVEL later: levels run one after the other, chains and sweeps of a level side by side.
	// In full, per direction and in sweep order: `first` is the run's first tile that is not anchored, the chain applies the matrix once
	// per tile from there to the run's last tile (`count` times) and `walk` is the tile behind the run.  A run that is anchored throughout
	// has no tile to cross: its chain has count 0 and stands on the first tile behind the run that is not anchored (first = walk), where only
	// the walk starts -- if that tile is glued in the direction, belongs to no qualifying run (then that run's chain starts there) and no
	// earlier chain's walk has been through it.  When every tile from the run to the segment's end is anchored there is no chain.  A walk
	// goes through the consecutive tiles behind its start that are glued in the direction and belong to no qualifying run.  A chain's
	// level is 0, or one more than the level of the chain before it when the tile before `first` is one that chain wrote or walked through.
	struct WgDir {
		std::vector<GapRun> runs;           // by level
		std::vector<int32_t> walk;          // [runs] the tile its walk starts on
		std::vector<int32_t> list;          // the tiles a level sweeps behind its chains (WG_OWN; the run's own tiles WG_SINGLE), by level
		std::vector<int32_t> run_off, list_off; // [levels + 1]
		std::vector<int32_t> spec;          // the tiles that speculate: everything else
	};
	WgDir wg[2];
	Buf<int> d_wg_glue, d_wg_list[2], d_wg_spec[2];
	Buf<GapRun> d_wg_runs[2], d_wg_again; // ... and the chains a repair round runs again
	Buf<double> d_wg_M; // [n][padded width] the transfer matrix of a full gap tile
	bool wg_m_valid = false;        // the last wide fast E-step built d_wg_M (psmc_hip_wide_gap_matrix, the diagnostic library)
	int wg_mats = 0;                // what the plan's qualifying runs hold: bit 0 gap tiles (d_wg_M), bit 1 hom tiles (d_wg_Mh, d_wg_cls), bit 2 mix tiles (d_wg_Mx, d_wg_mix_slot)
	Buf<double> d_wg_Mh; // [n][padded width] the matrix of a full hom tile on the pilot's scale, then the pilot's ceil(T / 4) factors
	int wg_mh_T = 0;                // the tile length d_wg_Mh was built for by the last wide fast E-step; 0: it built none (psmc_hip_wide_hom_matrix)
	Buf<int> d_wg_cls;              // [tiles] wg_cls on the device (sized with d_wg_glue)
	int wg_rechained[2] = {0, 0};   // chains the last wide fast E-step's repair rounds ran again, forward | backward (psmc_hip_wide_gap_rechained)
	int wg_cap = 0;
	// "vit_tile": bins per backtrace tile of psmc_hip_viterbi (api_viterbi.hip); results do not depend on it
	int vit_tile = 2048;
	// "samp_group": samples per sweep of psmc_hip_sample_paths (api_sample.hip); 0 = as many as the free device memory holds, at most 8
	int samp_group = 0;
};
// the padded width of the wide fast path's own tables (api_wide_fast.hip writes them, api_decode.hip reads them): c->ns (192 or 256)
// up to 256 states, beyond them the next multiple of 256 -- one wave of the tile per 256 states (c->ns stays what the wide exact
// kernels pad to, a multiple of 64: 320 at 300 states, where this is 512)
inline int wf_width(const psmc_hip_ctx *c) { return c->n <= 256 ? c->ns : 256 * ((c->n + 255) / 256); }
inline int wf_waves(const psmc_hip_ctx *c) { return c->n <= 256 ? 1 : (c->n + 255) / 256; }
inline double dbg_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline psmc_hip_ctx *dbg_root(psmc_hip_ctx *c) { return c->parent ? c->parent : c; }

inline int fail(psmc_hip_ctx *c, int code, const char *what, hipError_t e = hipSuccess)
{
	if (c) {
		c->err = what;
		if (e != hipSuccess) { c->err += ": "; c->err += hipGetErrorString(e); }
	}
	return code;
}
#define HIPCHK(c, call)                                                     \
	do {                                                                    \
		hipError_t e__ = (call);                                            \
		if (e__ != hipSuccess) return fail((c), PSMC_HIP_EDEVICE, #call, e__); \
	} while (0)

template <class T, BufKind K> hipError_t Buf<T, K>::try_alloc(size_t n)
{
	reset();
	if (n == 0) n = 1;
	hipError_t e = K == BUF_DEVICE ? hipMalloc((void **)&p, n * sizeof(T))
	                               : hipHostMalloc((void **)&p, n * sizeof(T), K == BUF_MAPPED ? hipHostMallocMapped : hipHostMallocDefault);
	if (e == hipSuccess && K == BUF_MAPPED && (e = hipHostGetDevicePointer((void **)&dev, p, 0)) != hipSuccess) (void)hipHostFree(p);
	if (e != hipSuccess) { p = dev = nullptr; return e; }
	cap = n; owned = true;
	return hipSuccess;
}
// PSMC_HIP_POISON=1 (tests): fresh device memory is usually zero, recycled memory is not -- fill every allocation with
// 0xFF bytes (NaN as double, -1 as int) so that anything that depends on memory nobody wrote shows up at once.
// PSMC_HIP_POISON=vary: a different finite garbage value per allocation (bytes 0x3B..0x42: doubles from 1e-23 to 1e5),
// so that two contexts with the same call history disagree if anything reads memory nobody wrote.  One rotation for the
// buffers of the contexts (Buf::alloc) and the per-call scratch (Scratch::get).  Without the variable: no call at all.
inline void poison_fill(void *p, size_t bytes)
{
	static const char *poison = getenv("PSMC_HIP_POISON");
	static std::atomic<int> poison_count{0};
	if (!poison) return;
	// the fill runs on the null stream, the kernels on non-blocking streams: finish it before anybody writes results there
	(void)hipMemset(p, strcmp(poison, "vary") == 0 ? 0x3B + (poison_count++ % 8) : 0xFF, bytes);
	(void)hipDeviceSynchronize();
}

template <class T, BufKind K> int Buf<T, K>::alloc(psmc_hip_ctx *c, size_t n)
{
	const hipError_t e = try_alloc(n);
	if (e != hipSuccess) return K == BUF_DEVICE ? fail(c, PSMC_HIP_ENOMEM, "hipMalloc", e) : fail(c, PSMC_HIP_ENOMEM, K == BUF_MAPPED ? "hipHostMalloc (mapped)" : "hipHostMalloc");
	if (K == BUF_DEVICE) poison_fill(p, cap * sizeof(T));
	return 0;
}

// Device scratch of one decoding, Viterbi or sampling call, freed when the call returns.  Plain hipMalloc and, unless
// PSMC_HIP_POISON is set (poison_fill: the block is filled, and the fill finished, before get() returns), nothing else: no fill
// and no device synchronise.  A failed get() returns null, leaves ok false and clears the runtime's last error; the gets after
// it still allocate (the caller checks ok, or the pointers, once).  ok never goes back to true: psmc_hip_sample_paths, which tries
// its map tables at a smaller size after a failure, looks at its pointers and not at ok.
struct Scratch {
	std::vector<void *> bufs;
	bool ok = true;
	Scratch() = default;
	Scratch(const Scratch &) = delete;
	Scratch &operator=(const Scratch &) = delete;
	~Scratch() { for (void *p : bufs) (void)hipFree(p); }
	template <class T> T *get(size_t n)
	{
		void *p = nullptr;
		if (hipMalloc(&p, sizeof(T) * (n ? n : 1)) != hipSuccess) { ok = false; (void)hipGetLastError(); return nullptr; }
		bufs.push_back(p);
		poison_fill(p, sizeof(T) * (n ? n : 1));
		return (T *)p;
	}
};

// ---- shared between the translation units (defined in the file named)
int  set_segments_common(psmc_hip_ctx *c, int n_seg, const int32_t *L);                                     // api.hip
bool fill_params(const psmc_hip_ctx *c, const double *a, const double *e, const double *a0, double *dst);   // api.hip
int  stage_params(psmc_hip_ctx *c, const double *a, const double *e, const double *a0, hipStream_t st);     // api.hip
int  ensure_tables(psmc_hip_ctx *c, bool need_b, int64_t want_bins = 0, bool need_f = true);                // api.hip
bool fused_counts(const psmc_hip_ctx *c);                                                                   // api.hip
bool kcol2_on(const psmc_hip_ctx *c);                                                                       // api.hip
void fill_common(psmc_hip_ctx *c, EstepLaunch &p, hipStream_t st, const double *par_base = nullptr);        // api.hip
void collect_timing(psmc_hip_ctx *c);                                                                       // api.hip
double host_lk(const double *s, int L);                                                                     // api.hip
int  ensure_seg_outputs(psmc_hip_ctx *c, int nw);                                                           // api.hip
int  estep_exact(psmc_hip_ctx *c, const double *a, const double *e, const double *a0, double *A, double *E, double *A0, double *LL, double *chk); // api.hip
int  ensure_fast_buffers(psmc_hip_ctx *c);                                                                  // api_fast.hip
int  auto_tile_len(const psmc_hip_ctx *c, int64_t bins, size_t n_work, bool structured);                    // api_fast.hip
int  enqueue_fast(psmc_hip_ctx *c, const double *a, const double *e, const double *a0, double *d_out, hipStream_t st); // api_fast.hip
int  read_warm(psmc_hip_ctx *c, hipStream_t st);                                                            // api_fast.hip
void unpack_factored(const double *h, int n, double *sums, double *E, double *LL);                          // api_fast.hip
bool factor_structure(int n, int S, const double *a, double *sp);                                         // api.hip
int  estep_wide_fast(psmc_hip_ctx *c, const double *a, const double *e, const double *a0, double *d_out, hipStream_t st); // api_wide_fast.hip
int  estep_factored_wide(psmc_hip_ctx *c, const double *a, const double *e, const double *a0, double *sums, double *E, double *LL); // api_wide_fast.hip
bool counts_go_wide(const psmc_hip_ctx *c, const double *a);                                                // api_wide_fast.hip
int  estep_counts_wide(psmc_hip_ctx *c, const double *a, const double *e, const double *a0, double *A, double *sums, double *E, double *A0, double *LL, double *chk); // api_wide_fast.hip
struct PathPlan { // api_viterbi.hip path_plan
	std::vector<VitSeg> segs;      // longest first
	std::vector<VitTile> tiles;    // the backtrace's, in load order of the segments (empty when no path is wanted)
	std::vector<int32_t> seg_tile; // [2][n_seg]: every segment's first tile | its number of tiles
	int64_t bins = 0;              // of all segments, unpadded: rows of a table, entries of a path
};
int  path_plan(psmc_hip_ctx *c, const char *who, bool want_path, PathPlan &pl);                             // api_viterbi.hip
std::vector<double> path_params(int n, int S, const double *a, const double *e, const double *a0, double (*f)(double), double pad, double miss); // api_viterbi.hip
int  estep_fast(psmc_hip_ctx *c, const double *a, const double *e, const double *a0, double *A, double *E, double *A0, double *LL, double *chk); // api_fast.hip
