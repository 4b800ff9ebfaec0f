// api_wide_fast.hip -- fast mode beyond 128 states: the factored statistics of psmc_hip_estep_factored[_device] at 129..256
// states with the option "wide_fast" = 1 or 2 (kernels: estep_wide_fast.hip, one wave per tile) and at 257..1024 states with
// "wide_fast" = 2 (the same kernels at 2..4 waves per tile at the padded widths 512, 768 and 1024; plan, rounds and
// options are the same, only WideLaunch knows the width and the waves).  With "wide_decode" = 1 the decoding entry points read
// what such an E-step left (api_decode.hip; kernels: estep_wide_post.hip).  Everything else a context of that size does --
// psmc_hip_estep without "wide_counts", the batch without "wide_batch" (with it: api_batch.hip batch_wide calls estep_factored_wide once per replicate),
// psmc_hip_get_tables, decoding without "wide_decode" or after an exact E-step -- stays on the wide exact kernels, and this path does not touch their tables: it keeps its own X table (8 S bytes per bin) and scale factors.
// "wide_ckpt" = 1: X at every 8th position only (S bytes per bin) plus every tile's last row, the accumulate sweep recomputes the rest
// (estep_wide_fast.hip); "wide_decode" = 1 wins, because the full-table decoding kernels read every row -- unless "wide_decode_ckpt" = 1:
// then the table does not depend on "wide_decode", and decoding recomputes the rows between the checkpoints as the accumulate sweep
// does (the CKPT kernels of estep_wide_post.hip).  The table is sized anew when the interval
// changes between two E-steps, and what ran is recorded for fast_info, psmc_hip_wide_table_info and decode_source.
//
// "wide_counts" = 1: psmc_hip_estep of such a context (and, with "wide_batch", the batch asked for A) runs the factored E-step below with
// the full table (it wins over "wide_ckpt" for that E-step, as "wide_decode" does) and then the counts pass of estep_wide_counts.hip
// -- per slab of whole tiles a V pass and a split-K GEMM on the f64 matrix cores, at the end A = a . C (estep_counts_wide, below).
// "wide_counts_ckpt" = 1 lifts that as "wide_decode_ckpt" does for decoding: the counts E-step keeps checkpoints when "wide_ckpt" says
// so (and "wide_decode" does not forbid it), and the V pass recomputes the rows between them and writes the slab's X rows beside its V
// rows for the GEMM -- the same ranges, the same operands, the same bits.  The counts pass follows the interval the E-step kept.
//
// "wide_gap_tiles" = 1: runs of missing data are found when the plan is made (plan_wide_gaps; the rule: psmc_hip_ctx.h) and crossed by a
// transfer-matrix chain (estep_wide_gap.hip) instead of speculation and position-by-position repair.  With a qualifying run in the plan
// an E-step is, per direction: the speculative sweeps of the tiles that are not glued; the matrix of one full tile of missing data
// (once, forward); then level by level -- a run whose chain starts from what the walk of the run before it computes is one level
// later -- the chains of the level and ONE launch with the sweeps of the runs' tiles from the chain's vectors and one walk per run
// through the tiles glued behind it; then the verify / repair rounds as below.  A repair walk stops in front of a run's first
// chained tile; a run whose first chained tile heads a failing run is chained again for that round (one head tile in fast_diag).
// Off, or without a qualifying run: the plan and the launches below, nothing else.
// "wide_hom_tiles" = 1: the same for runs of homozygosity -- full tiles of symbol 0 only are chain tiles too, a run qualifies through its
// gap tiles ("wide_gap_min") or through its hom tiles ("wide_hom_min"), and across a hom tile the chain applies the matrix of a full
// tile of homozygous bins, built beside the other one (pilot, then rows: estep_wide_gap.hip).  Glue, levels, lists, rounds: unchanged.
// "wide_mix_tiles" = 1 (with "wide_hom_tiles"): het-free tiles that hold both symbol 0 and `N` are chain tiles too, as far as "wide_mix_mb"
// admits their matrices -- two per tile, the tile's own forward and backward map, each built where a chain of the plan crosses the tile
// in that direction, all of them by one pilot launch and one row launch per E-step beside the other two matrices, on the same stream.  Glue, levels, lists, rounds: unchanged.
//
// One E-step: forward sweep of every tile and backward warm-up of every tile; forward verify / repair rounds; the accumulate sweep
// of every tile; backward verify / repair rounds; LL and the fixed-order reduction.  A round copies the verify flags to the host,
// which launches one wave per HEAD of a failing run (a failing tile whose predecessor in the sweep direction passed).  With "learn"
// (default) the wave walks on through the tiles after its head for as long as their start vectors disagree with what it computes
// -- the run is glued for this E-step and repaired in one round; with "learn" = 0 every round rewrites the heads only.  The plan
// (tiles, warm-ups) is the same at every E-step, so the result depends only on the inputs of the call: bit-reproducible.
#include "psmc_hip_ctx.h"
#include "wide_fast.h"

static constexpr int WF_PAR = 8; // e0 | e1 | a0 | P | R | qa | c | dd (wide_fast.h)
static constexpr int WF_NACC = 7; // SL SU DG CL CU E0 E1 per tile

// rows of the X table over `bins` positions at one row per `iv` positions (iv = 8: the rows at p % 8 == 0, by absolute position)
static inline int64_t wide_table_rows(int64_t bins, int iv) { return (bins + iv - 1) / iv; }

// "wide_gap_tiles" / "wide_hom_tiles" / "wide_mix_tiles": runs of missing data and of homozygosity in the wide plan (the rule: psmc_hip_ctx.h).  One launch
// of k_tile_class (estep_struct.hip; 1 = missing data only, 2 = homozygous bins only, 3 = both: a mix tile, a chain tile with "wide_mix_tiles", else an ordinary data tile) over the plan's tiles,
// with d_wf_dirty borrowed as scratch; everything else is host work.  The result is a function
// of the selection, the data and the options, and lives with the plan.  Without a qualifying run nothing but wg_cls / wg_glue (for
// psmc_hip_wide_plan_tiles) is left, and the E-step is the one without the option.
static int plan_wide_gaps(psmc_hip_ctx *c, int T, int W)
{
	const std::vector<Chunk> &ch = c->wf_chunks;
	const int nc = (int)ch.size();
	std::vector<int> cls(nc, 0);
	if (launch_tile_class(c->stream, c->d_obs, c->d_wf_chunks, nc, c->d_wf_dirty) != 0) return fail(c, PSMC_HIP_EDEVICE, "k_tile_class", hipGetLastError());
	HIPCHK(c, hipMemcpyAsync(cls.data(), c->d_wf_dirty, sizeof(int) * nc, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemsetAsync(c->d_wf_dirty, 0, sizeof(int) * nc, c->stream)); // (borrowed as scratch: back to what an allocation holds)
	HIPCHK(c, hipStreamSynchronize(c->stream));
	std::vector<int32_t> &gc = c->wg_cls, &glue = c->wg_glue;
	gc.assign(nc, 0); glue.assign(nc, 0);
	auto same = [&](int x, int y) { return x >= 0 && y >= 0 && x < nc && y < nc && ch[x].off == ch[y].off; };
	// a chain tile: a FULL tile, not the first, not the last, of missing data only (gc 1) or, "wide_hom_tiles", of homozygous bins only (gc 3)
	// "wide_mix_tiles" (with "wide_hom_tiles"): such a tile of both symbols 0 and `N` (gc 5) is a chain tile too when its two matrices are
	// ADMITTED under "wide_mix_mb" -- in plan order, before runs are formed; a refused one ends a run as every mix tile does without the option
	const bool mix_on = c->wide_mix_tiles && c->wide_hom_tiles;
	const int64_t mix_bytes = (int64_t)2 * c->n * wf_width(c) * 8, mix_cap = (int64_t)c->wide_mix_mb * 1000000;
	int64_t mix_used = 0;
	int n_adm = 0; // (at most WG_MIX_MAX tiles are admitted whatever the cap says: the slots are numbered in 16 bits' worth of grid)
	std::vector<char> chain(nc, 0);
	for (int b = 0; b < nc; ++b) {
		const bool inner = ch[b].lo > 1 && ch[b].hi < ch[b].L && ch[b].hi - ch[b].lo + 1 == T;
		gc[b] = !inner ? 0 : (cls[b] == 1 && c->wide_gap_tiles ? 1 : (cls[b] == 2 && c->wide_hom_tiles ? 3 : (cls[b] == 3 && mix_on ? 5 : 0)));
		chain[b] = gc[b] == 1 || gc[b] == 3;
		if (gc[b] == 5 && mix_used + mix_bytes <= mix_cap && n_adm < psmc_hip_ctx::WG_MIX_MAX) { chain[b] = 1; mix_used += mix_bytes; ++n_adm; }
	}
	const int64_t need = c->wide_gap_min > 0 ? c->wide_gap_min : W / 4, need_hom = c->wide_hom_min > 0 ? c->wide_hom_min : W / 4;
	std::vector<std::pair<int, int>> runs; // first and last tile of every qualifying run
	std::vector<char> inrun(nc, 0);        // tile of a qualifying run
	c->wg_mats = 0;
	for (int b = 0; b < nc;) {
		if (!chain[b]) { ++b; continue; }
		int e = b;
		int64_t n_gap = 0, n_hom = 0, n_mix = 0; // (the bins of a mix tile count towards "wide_hom_min" like those of a hom tile)
		while (e < nc && same(b, e) && chain[e]) { if (gc[e] == 1) ++n_gap; else if (gc[e] == 3) ++n_hom; else ++n_mix; ++e; }
		if ((n_gap > 0 && n_gap * T >= need) || (n_hom + n_mix > 0 && (n_hom + n_mix) * T >= need_hom)) {
			runs.push_back({b, e - 1});
			for (int t = b; t < e; ++t) { inrun[t] = 1; ++gc[t]; } // 1 -> 2, 3 -> 4, 5 -> 6
			c->wg_mats |= (n_gap > 0 ? 1 : 0) | (n_hom > 0 ? 2 : 0) | (n_mix > 0 ? 4 : 0);
		}
		b = e;
	}
	if (runs.empty()) return 0;
	if (c->wg_mats & 4) { // the slots of the class-6 tiles' matrices, in plan order
		c->wg_mix_slot.assign(nc, -1);
		for (int b = 0; b < nc; ++b) if (gc[b] == 6) { c->wg_mix_slot[b] = (int32_t)c->wg_mix_tiles.size(); c->wg_mix_tiles.push_back(b); }
	}
	std::vector<int> inq(nc + 1, 0), first(nc, 0); // prefix sums of "tile of a qualifying run"; the segment's first tile
	for (int b = 0; b < nc; ++b) { inq[b + 1] = inq[b] + inrun[b]; first[b] = same(b - 1, b) ? first[b - 1] : b; }
	for (int b = 0; b < nc; ++b) { // the tile that holds position p of the segment is first + (p - 1) / T
		const Chunk &k = ch[b];
		if (!(k.flags & CHUNK_ANCHOR_F) && same(b - 1, b)) { // forward: positions lo - wf .. lo - 1, the tiles t0 .. b - 1
			const int t0 = first[b] + (int)((std::max<int64_t>(1, (int64_t)k.lo - k.wf) - 1) / T);
			if (inrun[b] || (k.wf > 0 && inq[b] - inq[t0] > 0)) glue[b] |= 1;
		}
		if (!(k.flags & CHUNK_ANCHOR_B) && same(b, b + 1)) { // backward: positions hi + 1 .. hi + wb, the tiles b + 1 .. t1
			const int t1 = first[b] + (int)((std::min<int64_t>(k.L, (int64_t)k.hi + k.wb) - 1) / T);
			if (inrun[b] || (k.wb > 0 && inq[t1 + 1] - inq[b + 1] > 0)) glue[b] |= 2;
		}
	}
	// the chains, one direction at a time, in sweep order
	struct Tmp { GapRun g; int walk, lev; };
	for (int d = 0; d < 2; ++d) {
		const int step = d ? -1 : 1, anchor = d ? CHUNK_ANCHOR_B : CHUNK_ANCHOR_F, bit = d ? 2 : 1;
		std::vector<char> late(nc, 0); // swept behind a chain: does not speculate
		std::vector<Tmp> tmp;
		int last_lev = 0;
		for (size_t i = 0; i < runs.size(); ++i) {
			const std::pair<int, int> &R = runs[d ? runs.size() - 1 - i : i];
			const int in = d ? R.second : R.first, out = d ? R.first : R.second; // the run's first and last tile in sweep order
			int f = in; // the first tile from `in` on that is not anchored in this direction: there the chain starts
			while (same(in, f) && (ch[f].flags & anchor)) f += step;
			if (!same(in, f)) continue; // anchored through to the segment's end: every speculation behind the run is exact
			Tmp t;
			const bool inside = d ? f >= out : f <= out;
			if (inside) { t.g = GapRun{f, std::abs(out - f) + 1}; t.walk = out + step; glue[f] |= d ? WG_FIRST_B : WG_FIRST_F; }
			else { // the whole run is anchored: no tile to cross, but the tiles glued behind it still hang on one walk from the last anchored tile's exit
				if (!(glue[f] & bit) || inrun[f] || late[f]) continue; // (a later run's tile: that run's chain starts there)
				t.g = GapRun{f, 0}; t.walk = f;
			}
			t.lev = late[f - step] ? last_lev + 1 : 0; // its first vector comes out of the walk before it
			last_lev = t.lev;
			for (int b = f; b != t.walk + step; b += step) late[b] = 1;
			for (int b = t.walk + step; same(f, b) && (glue[b] & bit) && !inrun[b]; b += step) late[b] = 1; // what the walk goes through at once
			tmp.push_back(t);
		}
		std::stable_sort(tmp.begin(), tmp.end(), [](const Tmp &x, const Tmp &y) { return x.lev < y.lev; });
		psmc_hip_ctx::WgDir &D = c->wg[d];
		for (size_t i = 0; i < tmp.size(); ++i) {
			const Tmp &t = tmp[i];
			if (i == 0 || t.lev != tmp[i - 1].lev) { D.run_off.push_back((int32_t)D.runs.size()); D.list_off.push_back((int32_t)D.list.size()); }
			D.runs.push_back(t.g); D.walk.push_back(t.walk);
			for (int j = 0; j < t.g.count; ++j) D.list.push_back((t.g.first + step * j) | WG_OWN | WG_SINGLE);
			D.list.push_back(t.walk | WG_OWN);
		}
		D.run_off.push_back((int32_t)D.runs.size()); D.list_off.push_back((int32_t)D.list.size());
		for (int b = 0; b < nc; ++b) if (!late[b]) D.spec.push_back(b);
	}
	if (c->wg[0].runs.empty() && c->wg[1].runs.empty()) return 0;
	// the matrices to build: a class-6 tile's F where a forward chain crosses it, its B where a backward chain does (a tile anchored in
	// a direction is not crossed in it, and a run whose chain was dropped above is not crossed at all)
	if (c->wg_mats & 4)
		for (int d = 0; d < 2; ++d)
			for (const GapRun &r : c->wg[d].runs)
				for (int j = 0; j < r.count; ++j) {
					const int t = r.first + (d ? -j : j);
					if (gc[t] == 6) c->wg_mix_jobs.push_back(2 * c->wg_mix_slot[t] + d);
				}
	int rc;
	if (nc > c->wg_cap) {
		c->wg_cap = 0;
		if ((rc = c->d_wg_glue.alloc(c, (size_t)nc))) return rc;
		for (int d = 0; d < 2; ++d) // (a run has at least one tile, a walk one more: no list is longer than the plan)
			if ((rc = c->d_wg_list[d].alloc(c, (size_t)nc)) || (rc = c->d_wg_spec[d].alloc(c, (size_t)nc)) || (rc = c->d_wg_runs[d].alloc(c, (size_t)nc))) return rc;
		if ((rc = c->d_wg_again.alloc(c, (size_t)nc)) || (rc = c->d_wg_cls.alloc(c, (size_t)nc))) return rc;
		if ((rc = c->d_wg_mix_slot.alloc(c, (size_t)nc)) || (rc = c->d_wg_mix_tiles.alloc(c, (size_t)nc)) || (rc = c->d_wg_mix_jobs.alloc(c, (size_t)2 * nc))) return rc;
		c->wg_cap = nc;
	}
	HIPCHK(c, hipMemcpy(c->d_wg_glue, glue.data(), sizeof(int32_t) * nc, hipMemcpyHostToDevice));
	HIPCHK(c, hipMemcpy(c->d_wg_cls, gc.data(), sizeof(int32_t) * nc, hipMemcpyHostToDevice));
	if (c->wg_mats & 4) {
		HIPCHK(c, hipMemcpy(c->d_wg_mix_slot, c->wg_mix_slot.data(), sizeof(int32_t) * nc, hipMemcpyHostToDevice));
		HIPCHK(c, hipMemcpy(c->d_wg_mix_tiles, c->wg_mix_tiles.data(), sizeof(int32_t) * c->wg_mix_tiles.size(), hipMemcpyHostToDevice));
		if (!c->wg_mix_jobs.empty()) HIPCHK(c, hipMemcpy(c->d_wg_mix_jobs, c->wg_mix_jobs.data(), sizeof(int32_t) * c->wg_mix_jobs.size(), hipMemcpyHostToDevice));
	}
	for (int d = 0; d < 2; ++d) {
		const psmc_hip_ctx::WgDir &D = c->wg[d];
		if (!D.list.empty()) HIPCHK(c, hipMemcpy(c->d_wg_list[d], D.list.data(), sizeof(int32_t) * D.list.size(), hipMemcpyHostToDevice));
		if (!D.spec.empty()) HIPCHK(c, hipMemcpy(c->d_wg_spec[d], D.spec.data(), sizeof(int32_t) * D.spec.size(), hipMemcpyHostToDevice));
		if (!D.runs.empty()) HIPCHK(c, hipMemcpy(c->d_wg_runs[d], D.runs.data(), sizeof(GapRun) * D.runs.size(), hipMemcpyHostToDevice));
	}
	return 0;
}

// Tiles of T bins (option "chunk", else about WF_TILES tiles: four waves per SIMD of an MI355X -- the forward sweep fits four at
// up to 110 VGPRs; the accumulate sweep, at 154 / 206 VGPRs, fits three (192 states) or two (256) and runs the tiles in two generations), every one speculating "warmup" bins in both directions -- by default WF_WARMUP, not the 3072 of
// the paths up to 128 states.  On the 30 M-bin benchmark genome at 200 and 256 states a warm-up of 3072 or 6144 bins leaves a few
// tiles whose start vector is wrong outright (mismatch ~1), and the repair that follows walks on for a whole segment: 2.4-2.9 s
// per E-step; 8192: 0.2-0.5 s; 12288 or 16384: 0.16 s (profiles/wide_fast_timing.txt).  The extra warm-up costs a few ms.
static int plan_wide(psmc_hip_ctx *c)
{
	constexpr int64_t WF_TILES = 4096;
	constexpr int WF_WARMUP = 16384;
	int64_t bins = 0;
	for (int32_t s : c->work) bins += c->L[s];
	int T = c->chunk;
	if (T <= 0) T = (int)std::max<int64_t>(256, ((bins + WF_TILES - 1) / WF_TILES + 63) & ~(int64_t)63);
	const int W = c->warmup_set ? c->warmup : WF_WARMUP;
	c->wf_chunks.clear();
	for (size_t w = 0; w < c->work.size(); ++w) {
		const int32_t s = c->work[w];
		for (int32_t lo = 1; lo <= c->L[s]; lo += T) {
			Chunk ch;
			ch.off = c->off[s]; ch.L = c->L[s]; ch.lo = lo; ch.hi = std::min(c->L[s], lo + T - 1); ch.mult = c->mult[w];
			ch.flags = 0; ch.wf = ch.wb = W;
			if (ch.lo - W <= 1) ch.flags |= CHUNK_ANCHOR_F;
			if ((int64_t)ch.hi + W + 1 >= ch.L) ch.flags |= CHUNK_ANCHOR_B;
			if (ch.hi == ch.L) ch.flags |= CHUNK_LAST;
			c->wf_chunks.push_back(ch);
		}
	}
	const int nc = (int)c->wf_chunks.size(), S = wf_width(c);
	int rc;
	if (nc > c->wf_cap) {
		if ((rc = c->d_wf_chunks.alloc(c, (size_t)nc))) return rc;
		if ((rc = c->d_wf_entry.alloc(c, (size_t)nc * S))) return rc;
		if ((rc = c->d_wf_bentry.alloc(c, (size_t)nc * S))) return rc;
		if ((rc = c->d_wf_bexit.alloc(c, (size_t)(nc + 1) * S))) return rc;
		if ((rc = c->d_wf_part.alloc(c, (size_t)nc * WF_NACC * S))) return rc;
		if ((rc = c->d_wf_ll.alloc(c, (size_t)nc))) return rc;
		if ((rc = c->d_wf_dirty.alloc(c, (size_t)nc))) return rc;
		if ((rc = c->d_wf_list.alloc(c, (size_t)nc))) return rc;
		c->wf_cap = nc;
	}
	HIPCHK(c, hipMemcpy(c->d_wf_chunks, c->wf_chunks.data(), sizeof(Chunk) * nc, hipMemcpyHostToDevice));
	c->wf_T = T; c->wf_W = W;
	c->wg_cls.clear(); c->wg_glue.clear();
	for (auto &d : c->wg) { d.runs.clear(); d.walk.clear(); d.list.clear(); d.run_off.clear(); d.list_off.clear(); d.spec.clear(); }
	c->wg_mats = 0; c->wg_mix_slot.clear(); c->wg_mix_tiles.clear(); c->wg_mix_jobs.clear();
	c->wg_mx_T = c->wg_mx_n = 0; // (what psmc_hip_wide_mix_matrix reads beside the plan's slots: an E-step under this plan sets them again)
	if ((c->wide_gap_tiles || c->wide_hom_tiles) && nc > 0 && (rc = plan_wide_gaps(c, T, W))) return rc;
	c->plan_dirty = false;
	return 0;
}

// verify / repair rounds of one direction; returns 0, or PSMC_HIP_ECONVERGE after max_rounds repair rounds
// (g: the plan has qualifying runs of missing data, "wide_gap_tiles" -- what their chains are launched with; else null)
static int wide_rounds(psmc_hip_ctx *c, WideLaunch &w, bool bwd, int &rounds, int &tiles, WideGap *g = nullptr)
{
	const int nc = w.n_tiles;
	std::vector<int> dirty(nc), heads, again;
	std::vector<char> own;
	std::vector<GapRun> chains;
	int n_again = 0;
	rounds = tiles = 0;
	for (;;) {
		HIPCHK(c, hipMemsetAsync(w.cnt + (bwd ? 1 : 0), 0, sizeof(int), w.stream));
		HIPCHK(c, hipMemsetAsync(w.warm + (bwd ? 1 : 0), 0, sizeof(unsigned long long), w.stream));
		if (launch_wide_fast(w, bwd ? WF_VERIFY_B : WF_VERIFY_F)) return fail(c, PSMC_HIP_EDEVICE, "k_wf_verify", hipGetLastError());
		int bad = 0;
		HIPCHK(c, hipMemcpyAsync(&bad, w.cnt + (bwd ? 1 : 0), sizeof(int), hipMemcpyDeviceToHost, w.stream));
		HIPCHK(c, hipMemcpyAsync(dirty.data(), w.dirty, sizeof(int) * nc, hipMemcpyDeviceToHost, w.stream));
		HIPCHK(c, hipStreamSynchronize(w.stream));
		if (bad == 0) return 0;
		if (rounds >= c->max_rounds) return PSMC_HIP_ECONVERGE;
		heads.clear();
		auto follows = [&](int b) {
			const int nb = bwd ? b + 1 : b - 1; // the neighbour it starts from
			return nb >= 0 && nb < nc && c->wf_chunks[nb].off == c->wf_chunks[b].off && dirty[nb];
		};
		if (g) {
			// "wide_gap_tiles": a qualifying run whose first chained tile heads a failing run is chained again from the exit vector its
			// neighbour holds now -- the chain, then its tiles' sweeps and its walk in the repair launch below (WG_OWN) -- instead of being walked
			// position by position.  Its tiles count as failing for everybody else (no walk enters them, no head starts from them); the run is one head.
			const psmc_hip_ctx::WgDir &D = c->wg[bwd ? 1 : 0];
			const int step = bwd ? -1 : 1;
			again.clear(); own.assign(nc, 0);
			for (size_t i = 0; i < D.runs.size(); ++i) if (dirty[D.runs[i].first] && !follows(D.runs[i].first)) again.push_back((int)i);
			for (int i : again) {
				for (int j = 0; j < D.runs[i].count; ++j) own[D.runs[i].first + step * j] = 1;
				own[D.walk[i]] = 2;
			}
			for (int b = 0; b < nc; ++b) if (own[b]) dirty[b] = 1;
			n_again = 0;
			if (!again.empty()) {
				chains.clear();
				for (int i : again) chains.push_back(D.runs[i]);
				HIPCHK(c, hipMemcpyAsync(w.dirty, dirty.data(), sizeof(int) * nc, hipMemcpyHostToDevice, w.stream));
				HIPCHK(c, hipMemcpyAsync(c->d_wg_again, chains.data(), sizeof(GapRun) * chains.size(), hipMemcpyHostToDevice, w.stream));
				g->runs = c->d_wg_again; g->n_runs = (int)chains.size();
				if (launch_wide_gap(*g, bwd ? WG_CHAIN_B : WG_CHAIN_F)) return fail(c, PSMC_HIP_EDEVICE, "k_wf_gapchain", hipGetLastError());
				n_again = (int)again.size();
				c->wg_rechained[bwd ? 1 : 0] += n_again;
			}
			for (int b = 0; b < nc; ++b) {
				if (own[b]) heads.push_back(b | WG_OWN | (own[b] == 1 ? WG_SINGLE : 0));
				else if (dirty[b] && !follows(b)) heads.push_back(b);
			}
			int n_own = 0;
			for (int b = 0; b < nc; ++b) n_own += own[b] != 0;
			HIPCHK(c, hipMemcpyAsync(c->d_wf_list, heads.data(), sizeof(int) * heads.size(), hipMemcpyHostToDevice, w.stream));
			w.list = c->d_wf_list; w.init = 0;
			if (launch_wide_fast(w, bwd ? WF_ACC_GAP : WF_FWD_GAP, (int)heads.size()))
				return fail(c, PSMC_HIP_EDEVICE, "wide repair", hipGetLastError());
			HIPCHK(c, hipStreamSynchronize(w.stream)); // (heads, dirty and chains live on the host)
			++rounds; tiles += (int)heads.size() - n_own + n_again;
			continue;
		}
		for (int b = 0; b < nc; ++b) if (dirty[b] && !follows(b)) heads.push_back(b);
		HIPCHK(c, hipMemcpyAsync(c->d_wf_list, heads.data(), sizeof(int) * heads.size(), hipMemcpyHostToDevice, w.stream));
		w.list = c->d_wf_list;
		if (launch_wide_fast(w, bwd ? WF_ACC_REPAIR : WF_FWD_REPAIR, (int)heads.size()))
			return fail(c, PSMC_HIP_EDEVICE, "wide repair", hipGetLastError());
		HIPCHK(c, hipStreamSynchronize(w.stream)); // (heads lives on the host)
		++rounds; tiles += (int)heads.size();
	}
}

int estep_wide_fast(psmc_hip_ctx *c, const double *a, const double *e, const double *a0, double *d_out, hipStream_t ust)
{
	char msg[320];
	if (c->n > 256 && c->wide_fast < 2) {
		snprintf(msg, sizeof msg, "estep_factored: the wide fast path (\"wide_fast\") covers 129..256 states; %d states run on the exact kernels only (psmc_hip_estep)", c->n);
		return fail(c, PSMC_HIP_ENOTSUP, msg);
	}
	if (c->n_seg < 1) return fail(c, PSMC_HIP_ESTATE, "estep_factored: no segments loaded");
	HIPCHK(c, hipSetDevice(c->device));
	// this is the context's last single E-step from now on; until it has succeeded there is nothing to decode (api_decode.hip decode_source)
	c->wd_kind = WD_FAILED; c->wd_serial = c->tab_serial; c->wd_sel = c->sel_serial;
	const int n = c->n, S = wf_width(c);
	std::vector<double> sp((size_t)5 * n);
	if (!c->struct_opt) // as up to 128 states: the factored statistics come from the structured sweeps only
		return fail(c, PSMC_HIP_ENOTSUP, "estep_factored: the factored statistics need the structured sweeps (option \"structured\" is 0)");
	if (!factor_structure(n, n, a, sp.data()))
		return fail(c, PSMC_HIP_ENOTSUP, "estep_factored: the wide fast path needs a transition matrix of the PSMC form (two rank-1 triangles, core.c:112-122)");
	int rc;
	if ((rc = ensure_fast_buffers(c))) return rc;
	if (!c->h_wf_par && (rc = c->h_wf_par.alloc(c, (size_t)WF_PAR * S))) return rc;
	if (!c->d_wf_par && (rc = c->d_wf_par.alloc(c, (size_t)WF_PAR * S))) return rc;
	if ((c->plan_dirty || c->wf_chunks.empty()) && (rc = plan_wide(c))) return rc;
	const int64_t bins = c->total + 128;
	// "wide_ckpt": one X row per 8 positions -- unless "wide_decode" is on without "wide_decode_ckpt": the full-table decoding kernels
	// read every row, so that E-step keeps them; and so does a wide-counts E-step ("wide_counts": the GEMM reads every row of the
	// table) -- unless "wide_counts_ckpt" is on: then the counts pass recomputes the rows between the checkpoints slab by slab
	const int iv = c->wide_ckpt && (!c->wc_now || c->wide_counts_ckpt) && (!c->wide_decode || c->wide_decode_ckpt) ? 8 : 1;
	const int nt = (int)c->wf_chunks.size();
	c->wf_last_iv = 0;
	if (c->wf_bins < bins || c->wf_tab_iv != iv) { // the X table: 8 S bytes per bin (61 GB at 256 states and 30 M bins; 8 KB per bin at S = 1024), with "wide_ckpt" S bytes per bin; sized anew when the interval changes, whether it grows or shrinks
		const int64_t rows = wide_table_rows(bins, iv);
		c->wf_bins = 0; c->wf_rows = 0; c->wf_tab_iv = 0;
		if ((rc = c->d_wf_X.alloc(c, (size_t)rows * S))) {
			snprintf(msg, sizeof msg, "estep_factored: no device memory for the X table of the wide fast path: %lld bytes (%lld bins x %d padded states x 8%s)",
			         (long long)rows * S * 8, (long long)bins, S, iv == 8 ? " / 8: \"wide_ckpt\"" : "");
			return fail(c, PSMC_HIP_ENOMEM, msg);
		}
		if ((rc = c->d_wf_inv.alloc(c, (size_t)bins))) return rc;
		c->wf_bins = bins; c->wf_rows = rows; c->wf_tab_iv = iv;
	}
	if (iv == 8 && (rc = c->d_wf_xhi.grow(c, (size_t)nt * S))) return rc; // every tile's last row X_hi
	HIPCHK(c, hipStreamSynchronize(c->stream)); // the previous upload out of the pinned staging block
	double *hp = c->h_wf_par;
	memset(hp, 0, sizeof(double) * WF_PAR * S); // padded states: zero emission and matrix entries
	for (int k = 0; k < n; ++k) { hp[k] = e[k]; hp[S + k] = e[n + k]; hp[2 * S + k] = a0[k]; }
	for (int v = 0; v < 5; ++v)
		for (int k = 0; k < n; ++k) hp[(size_t)(3 + v) * S + k] = sp[(size_t)v * n + k];
	hipStream_t st = c->stream;
	if (ust && ust != st) { HIPCHK(c, hipEventRecord(c->evx[0], ust)); HIPCHK(c, hipStreamWaitEvent(st, c->evx[0], 0)); }
	HIPCHK(c, hipEventRecord(c->ev[0], st));
	HIPCHK(c, hipMemcpyAsync(c->d_wf_par, hp, sizeof(double) * WF_PAR * S, hipMemcpyHostToDevice, st));
	WideLaunch w;
	memset(&w, 0, sizeof(w));
	w.stream = st; w.ns = S; w.n_states = n; w.n_tiles = (int)c->wf_chunks.size(); w.chain = c->learn ? 1 : 0;
	w.waves = wf_waves(c); w.ckpt = iv; w.xhi = iv == 8 ? c->d_wf_xhi : nullptr;
	w.tol = c->warm_tol; w.tiny_total = (double)c->sel.size() * HMM_TINY_H;
	w.par = c->d_wf_par; w.obs = c->d_obs; w.chunks = c->d_wf_chunks; w.list = c->d_wf_list; w.dirty = c->d_wf_dirty;
	w.cnt = c->d_cnt; w.warm = c->d_warm;
	w.X = c->d_wf_X; w.inv = c->d_wf_inv; w.entry = c->d_wf_entry; w.bentry = c->d_wf_bentry; w.bexit = c->d_wf_bexit;
	w.part = c->d_wf_part; w.LLpart = c->d_wf_ll; w.stage = c->d_stage; w.out = d_out;
	c->report = FastReport{0, 0, 0, 0, 0, 0, 2};
	c->wf_ran = true; c->wc_ran = false; c->last_fused = 3; c->wf_last_iv = iv;
	c->wg_m_valid = false; c->wg_mh_T = 0; c->wg_mx_T = c->wg_mx_n = 0; c->wg_rechained[0] = c->wg_rechained[1] = 0;
	// "wide_gap_tiles" with a qualifying run in the plan: the tiles glued at plan time do not speculate.  Per direction: the sweeps of
	// the others; the transfer matrix (once); then level by level the chains across the runs and ONE launch with the sweeps of the runs'
	// tiles from the chain's vectors and the walks behind the runs (no work-group of it reads what another one of it writes).
	const bool gaps = !c->wg[0].runs.empty() || !c->wg[1].runs.empty();
	WideGap g;
	memset(&g, 0, sizeof(g));
	if (gaps) {
		if ((c->wg_mats & 1) && (rc = c->d_wg_M.grow(c, (size_t)n * S))) return rc;
		const size_t mh = (size_t)n * S + (size_t)(c->wf_T + 3) / 4; // M_h, then the pilot's factors
		if ((c->wg_mats & 2) && c->d_wg_Mh.grow(c, mh)) {
			snprintf(msg, sizeof msg, "estep_factored: no device memory for the matrix of a homozygous tile (\"wide_hom_tiles\"): %lld bytes (%d states x %d padded states x 8, and %d scale factors)",
			         (long long)mh * 8, n, S, (c->wf_T + 3) / 4);
			return fail(c, PSMC_HIP_ENOMEM, msg);
		}
		const int n_mix = (int)c->wg_mix_tiles.size();
		const size_t mx = (size_t)2 * n_mix * ((size_t)n * S + (size_t)(c->wf_T + 3) / 4); // every class-6 tile's F and B, then their pilots' factors
		if ((c->wg_mats & 4) && c->d_wg_Mx.grow(c, mx)) {
			snprintf(msg, sizeof msg, "estep_factored: no device memory for the matrices of the mix tiles (\"wide_mix_tiles\"): %lld bytes (%d tiles x 2 x %d states x %d padded states x 8, and their scale factors); \"wide_mix_mb\" caps them",
			         (long long)mx * 8, n_mix, n, S);
			return fail(c, PSMC_HIP_ENOMEM, msg);
		}
		g.mats = c->wg_mats; g.Mh = c->d_wg_Mh; g.cls = c->d_wg_cls;
		g.obs = c->d_obs; g.n_mix = n_mix; g.mix_tiles = c->d_wg_mix_tiles; g.mix_slot = c->d_wg_mix_slot; g.Mx = c->d_wg_Mx;
		g.n_jobs = (int)c->wg_mix_jobs.size(); g.mix_jobs = c->d_wg_mix_jobs;
		g.stream = st; g.ns = S; g.n_states = n; g.waves = w.waves; g.ckpt = iv; g.T = c->wf_T; g.par = c->d_wf_par; g.chunks = c->d_wf_chunks;
		g.M = c->d_wg_M; g.X = c->d_wf_X; g.xhi = w.xhi; g.bexit = c->d_wf_bexit; g.entry = c->d_wf_entry; g.bentry = c->d_wf_bentry;
		w.glue = c->d_wg_glue;
	}
	auto gap_levels = [&](int d) -> int { // the chains of direction d and what hangs on them
		const psmc_hip_ctx::WgDir &D = c->wg[d];
		for (size_t l = 0; l + 1 < D.run_off.size(); ++l) {
			g.runs = c->d_wg_runs[d] + D.run_off[l]; g.n_runs = D.run_off[l + 1] - D.run_off[l];
			if (launch_wide_gap(g, d ? WG_CHAIN_B : WG_CHAIN_F)) return -1;
			w.list = c->d_wg_list[d] + D.list_off[l]; w.init = 1;
			if (launch_wide_fast(w, d ? WF_ACC_GAP : WF_FWD_GAP, D.list_off[l + 1] - D.list_off[l])) return -1;
		}
		w.list = c->d_wf_list; w.init = 0;
		return 0;
	};
	if (!gaps) {
		if (launch_wide_fast(w, WF_FWD) || launch_wide_fast(w, WF_BWARM)) return fail(c, PSMC_HIP_EDEVICE, "wide sweeps", hipGetLastError());
	} else {
		w.list = c->d_wg_spec[0];
		if (launch_wide_fast(w, WF_FWD_LIST, (int)c->wg[0].spec.size())) return fail(c, PSMC_HIP_EDEVICE, "wide sweeps", hipGetLastError());
		w.list = c->d_wg_spec[1];
		if (launch_wide_fast(w, WF_BWARM_LIST, (int)c->wg[1].spec.size())) return fail(c, PSMC_HIP_EDEVICE, "wide sweeps", hipGetLastError());
		if (launch_wide_gap(g, WG_MAT) || gap_levels(0)) return fail(c, PSMC_HIP_EDEVICE, "wide gap chains (forward)", hipGetLastError());
		c->wg_m_valid = (c->wg_mats & 1) != 0;
		if (c->wg_mats & 2) c->wg_mh_T = c->wf_T;
		if (c->wg_mats & 4) { c->wg_mx_T = c->wf_T; c->wg_mx_n = (int)c->wg_mix_tiles.size(); }
	}
	int r = 0, t = 0;
	rc = wide_rounds(c, w, false, r, t, gaps ? &g : nullptr);
	c->report.fwd_rounds = r; c->report.fwd_tiles = t;
	if (rc == PSMC_HIP_ECONVERGE) return fail(c, rc, "fast mode (wide_fast): forward tile boundaries did not converge within max_rounds");
	if (rc) return rc;
	if (!gaps) {
		if (launch_wide_fast(w, WF_ACC)) return fail(c, PSMC_HIP_EDEVICE, "k_wf_acc", hipGetLastError());
	} else {
		w.list = c->d_wg_spec[1];
		if (launch_wide_fast(w, WF_ACC_LIST, (int)c->wg[1].spec.size()) || gap_levels(1)) return fail(c, PSMC_HIP_EDEVICE, "wide gap chains (backward)", hipGetLastError());
	}
	rc = wide_rounds(c, w, true, r, t, gaps ? &g : nullptr);
	c->report.bwd_rounds = r; c->report.bwd_tiles = t;
	if (rc == PSMC_HIP_ECONVERGE) return fail(c, rc, "fast mode (wide_fast): backward tile boundaries did not converge within max_rounds");
	if (rc) return rc;
	if (launch_wide_fast(w, WF_FINISH)) return fail(c, PSMC_HIP_EDEVICE, "k_wf_ll / k_wf_reduce", hipGetLastError());
	HIPCHK(c, hipEventRecord(c->ev[4], st));
	if (ust && ust != st) { HIPCHK(c, hipEventRecord(c->evx[1], st)); HIPCHK(c, hipStreamWaitEvent(ust, c->evx[1], 0)); }
	c->report.converged = 1;
	c->wd_kind = WD_OK;
	return 0;
}

int estep_factored_wide(psmc_hip_ctx *c, const double *a, const double *e, const double *a0, double *sums, double *E, double *LL)
{
	int rc = ensure_fast_buffers(c);
	if (rc) return rc;
	if ((rc = estep_wide_fast(c, a, e, a0, c->d_stats, c->stream))) return rc;
	const int n = c->n;
	std::vector<double> h((size_t)7 * n + 1);
	HIPCHK(c, hipMemcpyAsync(h.data(), c->d_stats, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	float ms = 0.0f;
	c->timing_valid = hipEventElapsedTime(&ms, c->ev[0], c->ev[4]) == hipSuccess;
	if (!c->timing_valid) (void)hipGetLastError();
	for (double &v : c->last_ms) v = 0.0;
	c->last_ms[0] = ms;
	unpack_factored(h.data(), n, sums, E, LL);
	return PSMC_HIP_OK;
}

// ---------------------------------------------------------------- "wide_counts": the full count matrix (estep_wide_counts.hip)
// does psmc_hip_estep with this matrix run on the wide fast path?  (everything else: the wide exact kernels, as without the option)
bool counts_go_wide(const psmc_hip_ctx *c, const double *a)
{
	if (!c->wide_counts || c->mode != PSMC_HIP_MODE_FAST || c->ns <= 128 || !c->wide_fast || (c->n > 256 && c->wide_fast < 2) || !c->struct_opt) return false;
	std::vector<double> sp((size_t)5 * c->n);
	return factor_structure(c->n, c->n, a, sp.data());
}

// The plan of the counts pass, from the tile plan and "wide_counts_slab" alone -- `xs`: the GEMM reads X from the slab's own X rows
// ("wide_counts_ckpt" after a checkpointed E-step), so a range's xrow is its vrow; slabs, ranges, their order and n_split do not depend on it.  A tile owns the transitions of its positions
// lo .. min(hi, L - 1) -- none when it holds only position L.  Slabs are runs of whole tiles in plan order with at most `slab` rows
// (a tile longer than that is a slab of its own); auto: 2^29 / S rows, a V slab of 4 GB -- the V pass of a slab is one sweep of
// a tile's length whatever the number of its tiles (up to the ~3000 waves the device holds), so few tiles per slab serialise it: on the
// 30 M-bin genome at 200 states (tiles of 7360 bins) slabs of 2^26 / S rows, 35 tiles each, made the pass 734 ms, of which the GEMM
// needs about 160.  The GEMM's K is cut into ranges of at
// most WC_KC rows that never cross a tile's end; split s of a slab takes an equal share of its ranges.  n_split: about 2048 waves
// with the (S / 64)^2 blocks of C -- 64 MB of partials at every width -- and no more than the largest slab has ranges.
struct CountsPlan {
	std::vector<int32_t> vrow;        // [tiles] first V row of the tile in its slab
	std::vector<KRange> kr;           // every slab's ranges, slab after slab
	std::vector<int> slab_t0, slab_kr; // [slabs + 1] first tile / first range of every slab
	int64_t max_rows = 0; int max_kr = 0, n_split = 1;
};
static constexpr int WC_KC = 256;

static void plan_counts(const psmc_hip_ctx *c, int S, bool xs, CountsPlan &pl)
{
	const int nt = (int)c->wf_chunks.size();
	const int64_t slab = c->wide_counts_slab > 0 ? c->wide_counts_slab : std::max<int64_t>(1, ((int64_t)1 << 29) / S);
	pl.vrow.assign(nt, 0);
	pl.slab_t0.assign(1, 0); pl.slab_kr.assign(1, 0);
	int64_t rows = 0;
	for (int b = 0; b < nt; ++b) {
		const Chunk &ch = c->wf_chunks[b];
		const int own = std::max(0, std::min(ch.hi, ch.L - 1) - ch.lo + 1);
		if (rows > 0 && rows + own > slab) { // the slab is full: this tile opens the next one
			pl.slab_t0.push_back(b); pl.slab_kr.push_back((int)pl.kr.size());
			rows = 0;
		}
		pl.vrow[b] = (int32_t)rows;
		for (int r = 0; r < own; r += WC_KC) pl.kr.push_back(KRange{xs ? rows + r : ch.off + ch.lo - 1 + r, (int32_t)(rows + r), std::min(WC_KC, own - r)});
		rows += own;
		pl.max_rows = std::max(pl.max_rows, rows);
	}
	pl.slab_t0.push_back(nt); pl.slab_kr.push_back((int)pl.kr.size());
	for (size_t i = 0; i + 1 < pl.slab_kr.size(); ++i) pl.max_kr = std::max(pl.max_kr, pl.slab_kr[i + 1] - pl.slab_kr[i]);
	pl.n_split = std::max(1, std::min(2048 / ((S / 64) * (S / 64)), pl.max_kr));
}

// One wide-counts E-step: the factored wide E-step with the full table, or with checkpoints ("wide_ckpt" + "wide_counts_ckpt") (its bits: E, LL and the factored statistics), then per slab
// the V pass and the GEMM, then the finish -- all on the context's stream.  Device memory the pass adds, whatever the number of
// bins: the V slab (at most 8 S max(slab, longest tile) bytes; auto: 4 GB), the partials (n_split S^2 doubles, at most 64 MB),
// a and A (n^2 doubles each), one slab's ranges (16 bytes per 256 rows) -- and four bytes per tile of the plan.  After a checkpointed
// E-step (wf_last_iv == 8) one X slab of the V slab's size beside it, allocated at the first such pass.
int estep_counts_wide(psmc_hip_ctx *c, const double *a, const double *e, const double *a0, double *A, double *sums, double *E, double *A0,
                      double *LL, double *chk)
{
	int rc = ensure_fast_buffers(c);
	if (rc) return rc;
	c->wc_now = true;
	rc = estep_wide_fast(c, a, e, a0, c->d_stats, c->stream);
	c->wc_now = false;
	if (rc) return rc;
	c->wd_kind = WD_FAILED; // until the counts are through (an error below leaves nothing to decode, as one in the E-step)
	const int n = c->n, S = wf_width(c);
	char msg[320];
	CountsPlan pl;
	const bool ck = c->wf_last_iv == 8; // the interval the E-step above actually kept
	plan_counts(c, S, ck, pl);
	const int nt = (int)c->wf_chunks.size(), n_slabs = (int)pl.slab_t0.size() - 1;
	auto grow = [&](auto &buf, size_t want, const char *what) -> int {
		if (buf.grow(c, want) == 0) return 0;
		snprintf(msg, sizeof msg, "estep: no device memory for %s of the wide counts pass: %lld bytes (\"wide_counts_slab\" bounds the slab)",
		         what, (long long)(want * sizeof(*buf.p)));
		return fail(c, PSMC_HIP_ENOMEM, msg);
	};
	if ((rc = grow(c->d_wc_V, (size_t)std::max<int64_t>(pl.max_rows, 1) * S, "the V slab"))) return rc;
	if (ck && (rc = grow(c->d_wc_Xs, (size_t)std::max<int64_t>(pl.max_rows, 1) * S, "the X slab (\"wide_counts_ckpt\")"))) return rc;
	if ((rc = grow(c->d_wc_P, (size_t)pl.n_split * S * S, "the partial matrices"))) return rc;
	if ((rc = grow(c->d_wc_kr, (size_t)std::max(pl.max_kr, 1), "the K ranges"))) return rc;
	if ((rc = grow(c->d_wc_vrow, (size_t)nt, "the tiles' rows"))) return rc;
	if (!c->d_wc_a && ((rc = c->d_wc_a.alloc(c, (size_t)n * n)) || (rc = c->d_wc_out.alloc(c, (size_t)n * n)))) return rc;
	hipStream_t st = c->stream;
	HIPCHK(c, hipMemcpyAsync(c->d_wc_a, a, sizeof(double) * n * n, hipMemcpyHostToDevice, st));
	HIPCHK(c, hipMemcpyAsync(c->d_wc_vrow, pl.vrow.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice, st));
	WideCounts w;
	memset(&w, 0, sizeof(w));
	w.stream = st; w.ns = S; w.n_states = n; w.waves = wf_waves(c);
	w.par = c->d_wf_par; w.obs = c->d_obs; w.chunks = c->d_wf_chunks; w.X = c->d_wf_X; w.bentry = c->d_wf_bentry;
	w.ckpt = ck ? 8 : 1; w.inv = c->d_wf_inv; w.entry = c->d_wf_entry; w.Xs = ck ? c->d_wc_Xs : nullptr;
	w.vrow = c->d_wc_vrow; w.V = c->d_wc_V; w.kr = c->d_wc_kr; w.n_split = pl.n_split; w.P = c->d_wc_P;
	w.a = c->d_wc_a; w.out = c->d_wc_out; w.tiny_total = (double)c->sel.size() * HMM_TINY_H;
	bool first = true;
	for (int i = 0; i < n_slabs; ++i) { // (pl lives on the host until the stream is through: the synchronize below)
		w.t0 = pl.slab_t0[i]; w.n_tiles = pl.slab_t0[i + 1] - w.t0; w.n_kr = pl.slab_kr[i + 1] - pl.slab_kr[i]; w.first = first ? 1 : 0;
		if (w.n_kr == 0) continue; // tiles without a transition only
		HIPCHK(c, hipMemcpyAsync(c->d_wc_kr, pl.kr.data() + pl.slab_kr[i], sizeof(KRange) * w.n_kr, hipMemcpyHostToDevice, st));
		if (launch_wide_counts(w, WC_V) || launch_wide_counts(w, WC_GEMM)) {
			const hipError_t err = hipGetLastError();
			(void)hipStreamSynchronize(st); // (the copies out of pl)
			return fail(c, PSMC_HIP_EDEVICE, "wide counts: k_wc_v / k_wc_gemm", err);
		}
		first = false;
	}
	if (first) w.n_split = 0; // no transition at all: no partial was written, and none is read
	if (launch_wide_counts(w, WC_FINISH)) return fail(c, PSMC_HIP_EDEVICE, "k_wc_finish", hipGetLastError());
	HIPCHK(c, hipEventRecord(c->ev[5], st));
	std::vector<double> h((size_t)7 * n + 1), hA(A ? (size_t)n * n : 0);
	HIPCHK(c, hipMemcpyAsync(h.data(), c->d_stats, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
	if (A) HIPCHK(c, hipMemcpyAsync(hA.data(), c->d_wc_out, sizeof(double) * hA.size(), hipMemcpyDeviceToHost, st));
	HIPCHK(c, hipStreamSynchronize(st));
	float ms = 0.0f, ms_c = 0.0f; // last_ms: [0] the whole E-step, [1] the factored part, [3] the counts pass (psmc_hip_last_timing: total, chains, expect)
	c->timing_valid = hipEventElapsedTime(&ms, c->ev[0], c->ev[5]) == hipSuccess && hipEventElapsedTime(&ms_c, c->ev[4], c->ev[5]) == hipSuccess;
	if (!c->timing_valid) (void)hipGetLastError();
	for (double &v : c->last_ms) v = 0.0;
	c->last_ms[0] = ms; c->last_ms[1] = ms - ms_c; c->last_ms[3] = ms_c;
	unpack_factored(h.data(), n, sums, E, LL);
	if (A) memcpy(A, hA.data(), sizeof(double) * hA.size());
	if (A0) memset(A0, 0, sizeof(double) * n); // as every fast-mode E-step (api_fast.hip estep_fast)
	if (chk) for (size_t i = 0; i < c->sel.size(); ++i) chk[i] = 1.0;
	c->wc_ran = true;
	c->wd_kind = WD_OK;
	return PSMC_HIP_OK;
}

// rows of X held for the wide fast path (the table, and with "wide_ckpt" the tiles' last rows beside it), their width, the interval
// of the last wide fast E-step, bytes
extern "C" int psmc_hip_wide_table_info(psmc_hip_ctx *c, int64_t out[4])
{
	if (!c || !out) return PSMC_HIP_EINVAL;
	const int64_t rows = c->wf_rows + (int64_t)(c->d_wf_xhi.cap / (size_t)wf_width(c));
	out[0] = rows; out[1] = rows ? wf_width(c) : 0; out[2] = c->wf_last_iv; out[3] = rows * out[1] * 8;
	return PSMC_HIP_OK;
}
