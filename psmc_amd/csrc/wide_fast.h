// wide_fast.h -- what api_wide_fast.hip hands the kernels of estep_wide_fast.hip (fast mode, factored statistics: 129..256 states
// as one wave per tile, 257..1024 states as 2..4 waves per tile), of estep_wide_post.hip (decoding from the tables that E-step
// left) and of estep_wide_counts.hip (the full count matrix from those tables, "wide_counts").
#pragma once
#include <hip/hip_runtime.h>
#include "psmc_hip_internal.h"

namespace psmc {

enum { WF_FWD, WF_FWD_REPAIR, WF_BWARM, WF_ACC, WF_ACC_REPAIR, WF_VERIFY_F, WF_VERIFY_B, WF_FINISH,
       // "wide_gap_tiles" (a plan with qualifying runs of missing data): the sweeps over the tiles of WideLaunch::list only, and the
       // sweeps / repairs that may start from a tile's own start vector (list entries carry WG_OWN / WG_SINGLE)
       WF_FWD_LIST, WF_FWD_GAP, WF_BWARM_LIST, WF_ACC_LIST, WF_ACC_GAP };

// a list entry of WF_FWD_GAP / WF_ACC_GAP: the tile, and
constexpr int WG_OWN = 1 << 30;    // start from the tile's own entry / bentry (the transfer-matrix chain wrote it), not from the neighbour's exit vector
constexpr int WG_SINGLE = 1 << 29; // sweep this tile only: do not walk on
constexpr int WG_TILE = WG_SINGLE - 1;
// WideLaunch::glue[b]: bit 0 = glued forward, bit 1 = glued backward (psmc_hip_wide_plan_tiles), and
constexpr int WG_FIRST_F = 4;      // the first tile the forward chain of a qualifying run writes: no forward walk enters it
constexpr int WG_FIRST_B = 8;      // ... and the backward chain's (the run's highest chained tile): no backward walk enters it

struct WideLaunch {
	hipStream_t stream;
	int ns, n_states, n_tiles, chain; // ns: padded states, 192 or 256 (one wave per tile), 512, 768 or 1024 (waves = 2, 3, 4); chain: repairs walk on through glued runs
	int waves;                        // waves per tile: 1, or ns / 256 on the multi-wave path
	int ckpt;                         // positions per stored X row: 1 (X [bins][ns]), or 8 ("wide_ckpt": X [bins / 8][ns], the rows at p % 8 == 0 by absolute position, and xhi)
	double tol, tiny_total;
	const double *par;                // e0 | e1 | a0 | P | R | qa | c | dd, ns doubles each
	const uint8_t *obs;
	const Chunk *chunks;
	const int *list;                  // repair launches: the head tiles
	int *dirty, *cnt;                 // [n_tiles] verify flags; [2] failing tiles, forward | backward
	unsigned long long *warm;         // [2] largest mismatch of the last verify, forward | backward (bits of a double)
	double *X, *inv, *entry, *bentry, *bexit, *part, *LLpart, *stage, *out;
	double *xhi;                      // ckpt == 8: [n_tiles][ns] every tile's last row X_hi (what its neighbour's verify / repair and the LL read)
	const int *glue;                  // "wide_gap_tiles": [n_tiles] the plan's glue bits and WG_FIRST_F / WG_FIRST_B; null without a qualifying run
	int init;                         // WF_FWD_GAP / WF_ACC_GAP: 1 = the launch behind the chain at the start of an E-step (no verify flags yet; walks go through glued tiles)
};

int launch_wide_fast(const WideLaunch &w, int what, int n_list = 0); // estep_wide_fast.hip; -1: ns and waves do not go together, or ckpt is not 1 or 8 with xhi

// The transfer-matrix chain across qualifying runs of missing data ("wide_gap_tiles", estep_wide_gap.hip).  One chain per run and
// direction.  Forward: v = the exit vector of tile first - 1 (its last X row; ckpt == 8: xhi), entry[first] = v, then `count` times
// v <- v M (normalised), entry[first + i] = v.  Backward: v = bexit[first + 1], bentry[first] = v, then v <- M v, bentry[first - i] = v.
// "wide_hom_tiles": across a hom tile (class 4) the matrix is Mh -- forward v <- v Mh, backward v <- D Mh D^-1 v with D = diag(e0).
// "wide_mix_tiles": across a mix tile (class 6) the matrix is the tile's own -- forward v <- v F, backward v <- B v, no D scaling.
struct GapRun { int32_t first, count; };
enum { WG_MAT, WG_CHAIN_F, WG_CHAIN_B };

struct WideGap {
	hipStream_t stream;
	int ns, n_states, waves, ckpt;    // as WideLaunch
	int T;                            // WG_MAT: bins of a full tile -- M = (the forward step under the missing symbol)^T
	const double *par;                // as WideLaunch
	const Chunk *chunks;
	double *M;                        // [n_states][ns]: row k = the unit vector of state k swept T bins forward, unscaled
	int mats;                         // bit 0: the plan's qualifying runs hold gap tiles (M); bit 1: they hold hom tiles ("wide_hom_tiles": Mh, cls)
	double *Mh;                       // bit 1: [n_states][ns] the same under symbol 0 with the pilot's power-of-two factors, then the ceil(T / 4) factors
	const int *cls;                   // bit 1: [tiles of the plan] wg_cls -- a chain applies Mh across a tile of class 4, M across every other
	// bit 2 of mats ("wide_mix_tiles"): the qualifying runs hold mix tiles, het-free tiles with both symbol 0 and `N` (class 6).  Each owns
	// two matrices, F forward and B backward, swept bin by bin through the tile's own symbols (estep_wide_gap.hip):
	const uint8_t *obs;               // as WideLaunch
	int n_mix;                        // class-6 tiles of the plan, at most 65535 (a grid dimension)
	const int *mix_tiles;             // [n_mix] slot -> tile
	const int *mix_slot;              // [tiles of the plan] tile -> slot (read for class-6 tiles only)
	int n_jobs; const int *mix_jobs;  // WG_MAT: [n_jobs] 2 slot + dir -- the matrices to build: the directions in which a chain of the plan crosses the tile
	double *Mx;                       // [n_mix][2][n_states][ns] slot's F, then its B, each on its own pilot's scale (built where a job asks for it); then [n_mix][2][ceil(T / 4)] those pilots' factors
	const GapRun *runs; int n_runs;   // WG_CHAIN_*: the chains of this launch, one work-group each
	const double *X, *xhi, *bexit;    // where the chains start
	double *entry, *bentry;           // what they write
};

int launch_wide_gap(const WideGap &w, int what); // estep_wide_gap.hip; -1: ns and waves do not go together

// decoding of ONE segment: its tiles are t0 .. t0 + n_tiles - 1 of the plan; every output pointer is the segment's own buffer
enum { WP_PATH, WP_POST, WP_REC, WP_POST_REC, WP_COUNTS, WP_SCALES, WP_MEAN, WP_QUANT };

struct WidePost {
	hipStream_t stream;
	int what, ns, n_states, t0, n_tiles; // ns: the padded width of the tables, as WideLaunch
	int waves;                        // waves per tile of the E-step that wrote them: 1, or ns / 256
	int ckpt;                         // as WideLaunch: 1 (X holds every row), or 8 (the E-step kept checkpoints; "wide_decode_ckpt": the CKPT kernels recompute the rows between them)
	const double *xhi;                // ckpt == 8: [tiles of the plan][ns] every tile's last row X_hi (X_L of a segment's last tile)
	const double *par;                // as WideLaunch
	const uint8_t *obs;
	const Chunk *chunks;
	const double *X, *inv, *entry, *bentry;
	double *post, *recomb, *maxp, *s; // [L][n_states] | [L] | [L] | [L]
	int32_t *path;                    // [L]
	const int32_t *cnt1;              // WP_COUNTS: [min_l][n_cnt]
	int n_cnt, min_l;
	double *part, *cnt;               // [n_tiles][n_cnt][ns] per-tile partials; [n_states][n_cnt] running totals (in / out)
	const double *wts; int n_w;       // WP_MEAN: [n_w][ns] per-state weights, zeros beyond n_states; 1 <= n_w <= MEAN_COLS
	double *mean;                     // ... and [L][n_w] the posterior means (psmc_hip_post_mean)
	QuantQ q; int n_q;                // WP_QUANT: the thresholds q_j in [0, 1]; 1 <= n_q <= QUANT_COLS
	int32_t *qstate;                  // ... and [L][n_q] the states at those posterior quantiles (psmc_hip_post_quantile)
};

int launch_wide_post(const WidePost &w);         // estep_wide_post.hip; refuses as launch_wide_fast
int launch_wide_post_cnt_add(const WidePost &w); // estep_wide_post.hip: WP_COUNTS, the tiles' partials added in tile order, at every width

// the full count matrix ("wide_counts", estep_wide_counts.hip): per slab of whole tiles WC_V, then WC_GEMM; at the end WC_FINISH
enum { WC_V, WC_GEMM, WC_FINISH };

// rows of K the GEMM reads: `rows` consecutive positions of one tile, from row xrow of X and row vrow of the slab's V
struct KRange { int64_t xrow; int32_t vrow, rows; }; // (ckpt == 8: xrow is the row of the slab's Xs, and equals vrow)

struct WideCounts {
	hipStream_t stream;
	int ns, n_states, waves;          // as WideLaunch
	int t0, n_tiles;                  // WC_V: the slab's tiles t0 .. t0 + n_tiles - 1 of the plan
	const double *par;                // as WideLaunch
	const uint8_t *obs;
	const Chunk *chunks;
	int ckpt;                         // as WideLaunch: 1 (X holds every row), or 8 (the E-step kept checkpoints; "wide_counts_ckpt": k_wc_v CKPT recomputes the rows between them)
	const double *X, *bentry;         // the table the E-step left (ckpt == 1: every row) and its converged start vectors
	const double *inv, *entry;        // ckpt == 8: the stored scale factors [bins] and every tile's forward start vector [tiles][ns]
	double *Xs;                       // ckpt == 8: [rows of the largest slab][ns] the slab's X rows, row for row beside V (WC_V writes, WC_GEMM reads them)
	const int32_t *vrow;              // [tiles of the plan] the tile's first row in its slab's V
	double *V;                        // [rows of the largest slab][ns]
	const KRange *kr; int n_kr;       // WC_GEMM: the slab's ranges
	int n_split, first;               // partial matrices; first: this is the call's first slab (the partials start from zero)
	double *P;                        // [n_split][ns][ns]
	const double *a;                  // WC_FINISH: the transition matrix [n_states][n_states]
	double tiny_total;                // ... HMM_TINY x selected segments, added to every cell (as WideLaunch)
	double *out;                      // ... and A, [n_states][n_states]
};

int launch_wide_counts(const WideCounts &w, int what); // estep_wide_counts.hip; -1: ns and waves do not go together, or ckpt is not 1 or 8 with inv, entry and Xs

} // namespace psmc
