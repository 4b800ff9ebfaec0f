// wide_fast.h -- what api_wide_fast.hip hands the kernels of estep_wide_fast.hip (fast mode, factored statistics: 129..256 states
// as one wave per tile, 257..1024 states as 2..4 waves per tile), of estep_wide_post.hip (decoding from the tables that E-step
// left) and of estep_wide_counts.hip (the full count matrix from those tables, "wide_counts").
#pragma once
#include <hip/hip_runtime.h>
#include "psmc_hip_internal.h"

namespace psmc {

enum { WF_FWD, WF_FWD_REPAIR, WF_BWARM, WF_ACC, WF_ACC_REPAIR, WF_VERIFY_F, WF_VERIFY_B, WF_FINISH };

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
};

int launch_wide_fast(const WideLaunch &w, int what, int n_list = 0); // estep_wide_fast.hip; -1: ns and waves do not go together, or ckpt is not 1 or 8 with xhi

// decoding of ONE segment: its tiles are t0 .. t0 + n_tiles - 1 of the plan; every output pointer is the segment's own buffer
enum { WP_PATH, WP_POST, WP_REC, WP_POST_REC, WP_COUNTS, WP_SCALES };

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
