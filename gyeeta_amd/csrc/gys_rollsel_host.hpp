// gys_rollsel_host.hpp -- host side of the filtered, grouped roll-ups (kernels: gys_rollsel.hpp).  Included once by gys_engine.hip behind
// gys_svcquery_host.hpp and gys_rollup_host.hpp: the filter goes through q_fill_filter, the members through rollup_run / hll_union_launch /
// hist_union_rows as those of the fixed roll-ups.
#pragma once

#define GYS_RS_ROWS_EAGER 65536u // up to this many possible rows (512 KB) the rows travel with the totals, before it is known how many there are

extern "C" {

int gys_set_service_groups(gys_ctx *c, const uint64_t *glob_ids, const uint32_t *groups, uint32_t n)
try {
	GYS_ENTER(c);
	if (!c || (n && (!glob_ids || !groups))) return GYS_ERR_INVAL;
	std::vector<uint32_t> slots(n);
	for (uint32_t i = 0; i < n; ++i) { // everything is checked before anything is applied
		auto it = c->gid_map_h.find(glob_ids[i]);
		if (it == c->gid_map_h.end()) {
			set_err("gys_set_service_groups: unknown glob_id %016llx (entry %u); nothing was changed", (unsigned long long)glob_ids[i], i);
			return GYS_ERR_INVAL;
		}
		if (groups[i] != GYS_NO_GROUP && groups[i] >= c->cfg.max_services) {
			set_err("gys_set_service_groups: group %u of entry %u is not below max_services (%u)", groups[i], i, c->cfg.max_services);
			return GYS_ERR_INVAL;
		}
		slots[i] = it->second;
	}
	if (!c->svc_label.p) {
		const int rc = c->svc_label.alloc(c->cfg.max_services, false);
		if (rc) return rc;
		if (hipMemsetAsync(c->svc_label, 0xFF, c->svc_label.cap * 4, c->stream) != hipSuccess) {
			c->svc_label.release();
			set_err("gys_set_service_groups: could not clear the label array");
			return GYS_ERR_HIP;
		}
	}
	if (!n) return GYS_OK;
	// an id named twice keeps the later group: every entry of a slot carries the group of the slot's LAST entry, so the order of the device's
	// stores does not matter
	uint32_t dom = c->label_domain;
	std::vector<uint32_t> fin(groups, groups + n);
	{
		std::unordered_map<uint32_t, uint32_t> last; // slot -> its last entry
		last.reserve(n);
		for (uint32_t i = 0; i < n; ++i) last[slots[i]] = i;
		if (last.size() != n)
			for (uint32_t i = 0; i < n; ++i) fin[i] = groups[last[slots[i]]];
	}
	for (uint32_t i = 0; i < n; ++i)
		if (fin[i] != GYS_NO_GROUP) dom = std::max(dom, fin[i] + 1u);
	DevBuf<uint32_t> d_slots, d_groups;
	int rc = d_slots.upload(slots, c->stream);
	if (rc == GYS_OK) rc = d_groups.upload(fin, c->stream);
	if (rc) return rc;
	hipLaunchKernelGGL(k_rollsel_labels, dim3((uint32_t)std::min<uint64_t>(((uint64_t)n + 255u) / 256u, (uint64_t)c->ncu * 8)), dim3(256), 0, c->stream, d_slots.p, d_groups.p, n,
			   c->svc_label);
	const hipError_t e = hipGetLastError();
	const hipError_t es = hipStreamSynchronize(c->stream); // the lists are freed at scope exit
	HIPCHK(e);
	HIPCHK(es);
	c->label_domain = dom; // (only once the device holds the labels)
	return GYS_OK;
} GYS_CATCH_ALL

} // extern "C"

// the selection half of the filtered roll-ups: the filter's services grouped into rows (rows / *nrows are the caller's), their members in
// c->rs_members.p, the chunk lists in c->rs_chunks.p (*pnchunks chunks) and the rows' chunk ranges in c->rs_gchunks.p (*pnr rows, 0: nothing to do)
static int rollsel_select(gys_ctx *c, const gys_svc_filter *f, uint32_t flags, int group_by, gys_rollup_row *rows, uint32_t maxrows, uint32_t *nrows, uint32_t *pnr,
			  uint32_t *pnchunks)
{
	*pnr = *pnchunks = 0;
	const uint32_t nh = (uint32_t)c->hosts.size(), ncl = (uint32_t)c->cluster_names.size();
	const uint32_t ndomain = group_by == GYS_GROUP_NONE ? 1u : group_by == GYS_GROUP_HOST ? nh : group_by == GYS_GROUP_CLUSTER ? ncl : (c->svc_label ? c->label_domain : 0u);
	int rc;
	RollSelP p{};
	if ((rc = q_fill_filter(c, f, p)) != GYS_OK) return rc; // (a bad filter is refused whatever is registered)
	if (!c->nsvc || !ndomain) return GYS_OK; // (no service, or no label was ever set: no group has a member)
	uint32_t nscan_tiles;
	uint32_t tot[RS_TOT_WORDS];
	{
		ProfScope ps(c, "rollsel");
		p.any_state = flags & GYS_RF_ANY_STATE ? 1u : 0u;
		p.group_by = (uint32_t)group_by;
		p.host_cluster = c->host_cluster;
		p.labels = c->svc_label;
		p.ndomain = ndomain;
		p.ntiles = (p.nitems + GYS_RS_TILE - 1u) / GYS_RS_TILE;
		nscan_tiles = (ndomain + GYS_RS_SCAN_TILE - 1u) / GYS_RS_SCAN_TILE;
		const uint32_t rowcap = std::min(maxrows, ndomain);
		if ((rc = c->rs_item_group.grow(p.nitems, c->stream)) != GYS_OK) return rc;
		if ((rc = c->rs_counts.grow((uint64_t)ndomain + 4u, c->stream)) != GYS_OK) return rc;
		if ((rc = c->rs_members.grow(p.nitems, c->stream)) != GYS_OK) return rc;
		if ((rc = c->rs_tiles.grow(3ull * nscan_tiles, c->stream)) != GYS_OK) return rc;
		if ((rc = c->rs_tot.grow(RS_TOT_WORDS, c->stream)) != GYS_OK) return rc;
		if ((rc = c->rs_rows.grow(rowcap, c->stream)) != GYS_OK) return rc;
		if ((rc = c->rs_rowoff.grow(rowcap, c->stream)) != GYS_OK) return rc;
		p.item_group = c->rs_item_group.p;
		p.counts = c->rs_counts.p;
		p.tot = c->rs_tot.p;
		p.members = c->rs_members.p;
		HIPCHK(hipMemsetAsync(c->rs_counts.p, 0, (size_t)ndomain * 4, c->stream));
		const uint32_t grid = std::max(1u, std::min<uint32_t>(p.ntiles, (uint32_t)c->ncu * 8));
		hipLaunchKernelGGL(k_rollsel_count, dim3(grid), dim3(GYS_RS_THREADS), 0, c->stream, p);
		RollScanP sp{};
		sp.counts = c->rs_counts.p;
		sp.ndomain = ndomain;
		sp.ntiles = nscan_tiles;
		sp.per = GYS_RB_CHUNK_SERVICES;
		sp.maxrows = maxrows;
		sp.tiles = c->rs_tiles.p;
		sp.tot = c->rs_tot.p;
		sp.rows = c->rs_rows.p;
		sp.rowoff = c->rs_rowoff.p;
		const uint32_t sgrid = std::min<uint32_t>(nscan_tiles, (uint32_t)c->ncu * 8);
		for (uint32_t phase = 0; phase < 3u; ++phase) {
			sp.phase = phase;
			hipLaunchKernelGGL(k_rollsel_scan, dim3(phase == 1u ? 1u : sgrid), dim3(GYS_RS_THREADS), 0, c->stream, sp);
		}
		HIPCHK(hipGetLastError());
		// the one read inside the call: the totals and the rows together (every row there can be, while that is a small copy; a caller who
		// asks for more than GYS_RS_ROWS_EAGER rows pays a second small read of the rows there are).  Nothing after it waits for the host.
		const bool eager = rowcap <= GYS_RS_ROWS_EAGER;
		std::vector<gys_rollup_row> hrows(eager ? rowcap : 0u);
		HIPCHK(hipMemcpyAsync(tot, c->rs_tot.p, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
		if (eager && rowcap) HIPCHK(hipMemcpyAsync(hrows.data(), c->rs_rows.p, (size_t)rowcap * sizeof(gys_rollup_row), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
		*nrows = tot[RS_TOT_ROWS];
		const uint32_t nr = std::min(tot[RS_TOT_ROWS], maxrows);
		if (!nr) return GYS_OK;
		if (eager) {
			memcpy(rows, hrows.data(), (size_t)nr * sizeof(gys_rollup_row));
		} else {
			HIPCHK(hipMemcpyAsync(rows, c->rs_rows.p, (size_t)nr * sizeof(gys_rollup_row), hipMemcpyDeviceToHost, c->stream));
			HIPCHK(hipStreamSynchronize(c->stream)); // (rows is the caller's: valid on return)
		}
		if ((rc = c->rs_chunks.grow(tot[RS_TOT_CHUNKS], c->stream)) != GYS_OK) return rc;
		if ((rc = c->rs_gchunks.grow(nr, c->stream)) != GYS_OK) return rc;
		hipLaunchKernelGGL(k_rollsel_scatter, dim3(grid), dim3(GYS_RS_THREADS), 0, c->stream, p);
		RollChunksP cp{};
		cp.rows = c->rs_rows.p;
		cp.rowoff = c->rs_rowoff.p;
		cp.tot = c->rs_tot.p;
		cp.maxrows = maxrows;
		cp.per = GYS_RB_CHUNK_SERVICES;
		cp.chunks = c->rs_chunks.p;
		cp.gchunks = c->rs_gchunks.p;
		hipLaunchKernelGGL(k_rollsel_chunks, dim3(std::min<uint32_t>((nr + 3u) / 4u, (uint32_t)c->ncu * 8)), dim3(GYS_RS_THREADS), 0, c->stream, cp);
		HIPCHK(hipGetLastError());
	}
	*pnr = std::min(tot[RS_TOT_ROWS], maxrows);
	*pnchunks = tot[RS_TOT_CHUNKS];
	return GYS_OK;
}

extern "C" {

int gys_rollup_filtered_dev(gys_ctx *c, const gys_svc_filter *f, uint32_t flags, int group_by, int hll_level, uint64_t tusec, gys_rollup_row *rows, uint32_t maxrows,
			    uint32_t *nrows, gys_tdigest_slab *d_slabs, uint8_t *d_regs, double *d_est)
try {
	GYS_ENTER(c);
	if (!c || !f || !rows || !nrows || (flags & ~GYS_RF_ANY_STATE) || group_by < GYS_GROUP_NONE || group_by > GYS_GROUP_LABEL || (!d_slabs && !d_regs && !d_est) ||
	    hll_level < -1 || hll_level >= GYS_NLEVELS || !HLL_ALIGNED(d_regs)) {
		set_err("gys_rollup_filtered_dev: null filter / rows / nrows / outputs, d_regs not 16-byte aligned, unknown flags, group_by or hll_level");
		return GYS_ERR_INVAL;
	}
	*nrows = 0;
	if (d_slabs) TDIGEST_CHECK();
	const bool want_hll = d_regs || d_est;
	if (want_hll) {
		HLL_CHECK();
		if (hll_level >= 0 && !c->hl_lvl) {
			set_err("distinct-count levels are off (gys_config.svc_hll_levels = 0)");
			return GYS_ERR_STATE;
		}
	}
	uint32_t nr, nchunks;
	int rc = rollsel_select(c, f, flags, group_by, rows, maxrows, nrows, &nr, &nchunks);
	if (rc != GYS_OK || !nr) return rc;
	if (d_slabs) {
		ProfScope ps(c, "rollsel_digests");
		if ((rc = rollup_run(c, 0, c->rs_chunks.p, nchunks, c->rs_members.p, nr, nullptr, d_slabs)) != GYS_OK) return rc;
	}
	if (want_hll) {
		const uint8_t *src = c->svc_hll;
		if (hll_level >= 0) {
			if ((rc = hll_level_files(c, hll_level, tusec)) != GYS_OK) return rc;
			src = c->hl_view.p;
		}
		uint8_t *parts = nullptr, *groupfiles = nullptr;
		if ((rc = hll_scratch(c, nchunks, 0, d_regs ? 0 : nr, &parts, nullptr, &groupfiles)) != GYS_OK) return rc;
		uint8_t *out = d_regs ? d_regs : groupfiles;
		const uint32_t hp = c->cfg.svc_hll_p;
		ProfScope ps(c, "rollsel_hll"); // the members' files -> one file per chunk -> one per row, then the estimates
		hll_union_launch(c, HllUnionP{src, parts, c->rs_chunks.p, c->rs_members.p, nchunks, 0u, 0u, hp});
		hll_union_launch(c, HllUnionP{parts, out, c->rs_gchunks.p, nullptr, nr, 0u, 0u, hp});
		if (d_est) hll_estimate_launch(c, out, nr, d_est);
		HIPCHK(hipGetLastError());
	}
	return GYS_OK;
} GYS_CATCH_ALL

// the argument rules the filtered group-histogram calls share
#define HIST_FILTERED_ARGS_OK(f, rows, nrows, out, flags, group_by) \
	((f) && (rows) && (nrows) && (out) && !((flags) & ~GYS_RF_ANY_STATE) && (group_by) >= GYS_GROUP_NONE && (group_by) <= GYS_GROUP_LABEL)

// the members' records `src` of a selection (rollsel_select: nr rows, nchunks chunks) -> one record per chunk -> one per row (d_recs)
static int hist_rollup_selected(gys_ctx *c, const HistMemberSrc &src, uint32_t nr, uint32_t nchunks, gys_hist_rec *d_recs)
{
	gys_hist_rec *parts = nullptr;
	const int rc = hist_union_scratch(c, nchunks, 0, &parts, nullptr);
	if (rc) return rc;
	return hist_union_rows(c, src, c->rs_chunks.p, nchunks, c->rs_members.p, c->rs_gchunks.p, nr, parts, d_recs);
}

int gys_hist_rollup_filtered_dev(gys_ctx *c, const gys_svc_filter *f, uint32_t flags, int group_by, int level, uint64_t tusec, gys_rollup_row *rows, uint32_t maxrows,
				 uint32_t *nrows, gys_hist_rec *d_recs)
try {
	GYS_ENTER(c);
	if (!c || !HIST_FILTERED_ARGS_OK(f, rows, nrows, d_recs, flags, group_by) || level < 0 || level >= GYS_NLEVELS) {
		set_err("gys_hist_rollup_filtered_dev: null filter / rows / nrows / d_recs, unknown flags or group_by, or a level outside 0 .. %d", GYS_NLEVELS - 1);
		return GYS_ERR_INVAL;
	}
	*nrows = 0;
	LEVELS_CHECK();
	LEVEL0_CHECK(level);
	uint32_t nr, nchunks;
	const int rc = rollsel_select(c, f, flags, group_by, rows, maxrows, nrows, &nr, &nchunks);
	if (rc != GYS_OK || !nr) return rc;
	return hist_rollup_selected(c, hist_src_level(level, tusec), nr, nchunks, d_recs);
} GYS_CATCH_ALL

int gys_hist_rollup_period_filtered_dev(gys_ctx *c, const gys_svc_filter *f, uint32_t flags, int group_by, int64_t starttime, int64_t endtime, uint64_t tusec,
					gys_rollup_row *rows, uint32_t maxrows, uint32_t *nrows, gys_hist_rec *d_recs, int *level_used)
try {
	GYS_ENTER(c);
	if (!c || !HIST_FILTERED_ARGS_OK(f, rows, nrows, d_recs, flags, group_by)) {
		set_err("gys_hist_rollup_period_filtered_dev: null filter / rows / nrows / d_recs, unknown flags or group_by");
		return GYS_ERR_INVAL;
	}
	*nrows = 0;
	LEVELS_CHECK();
	LevelPeriodP plan;
	period_plan(c, starttime, endtime + 1, tusec, plan, level_used);
	uint32_t nr, nchunks;
	const int rc = rollsel_select(c, f, flags, group_by, rows, maxrows, nrows, &nr, &nchunks);
	if (rc != GYS_OK || !nr) return rc;
	return hist_rollup_selected(c, hist_src_period(&plan), nr, nchunks, d_recs);
} GYS_CATCH_ALL

int gys_svc_hist_rollup_filtered_dev(gys_ctx *c, const gys_svc_filter *f, uint32_t flags, int group_by, int which, gys_rollup_row *rows, uint32_t maxrows, uint32_t *nrows,
				     gys_hist_rec *d_recs)
try {
	GYS_ENTER(c);
	if (!c || !HIST_FILTERED_ARGS_OK(f, rows, nrows, d_recs, flags, group_by) || which < 0 || which > 1) {
		set_err("gys_svc_hist_rollup_filtered_dev: null filter / rows / nrows / d_recs, unknown flags or group_by, or which outside 0 .. 1");
		return GYS_ERR_INVAL;
	}
	*nrows = 0;
	LEVELS_CHECK();
	uint32_t nr, nchunks;
	const int rc = rollsel_select(c, f, flags, group_by, rows, maxrows, nrows, &nr, &nchunks);
	if (rc != GYS_OK || !nr) return rc;
	return hist_rollup_selected(c, hist_src_plain(which ? c->act_hist : c->qps_hist), nr, nchunks, d_recs);
} GYS_CATCH_ALL

int gys_day_stats_rollup_filtered_dev(gys_ctx *c, const gys_svc_filter *f, uint32_t flags, int group_by, uint64_t tusec, gys_rollup_row *rows, uint32_t maxrows,
				      uint32_t *nrows, gys_listener_day_stats *d_out)
try {
	GYS_ENTER(c);
	if (!c || !HIST_FILTERED_ARGS_OK(f, rows, nrows, d_out, flags, group_by)) {
		set_err("gys_day_stats_rollup_filtered_dev: null filter / rows / nrows / d_out, unknown flags or group_by");
		return GYS_ERR_INVAL;
	}
	*nrows = 0;
	LEVELS_CHECK();
	uint32_t nr, nchunks;
	const int rc = rollsel_select(c, f, flags, group_by, rows, maxrows, nrows, &nr, &nchunks);
	if (rc != GYS_OK || !nr) return rc;
	// one selection, three families over it; glob_id = the row's group (the device's copy of the rows)
	return day_stats_groups(c, nr, std::max<size_t>(nchunks, 1), c->rs_rows.p, d_out, [&](int fam, gys_hist_rec *recs) {
		return hist_rollup_selected(c, fam == 0 ? hist_src_level(2, tusec) : hist_src_plain(fam == 1 ? c->qps_hist : c->act_hist), nr, nchunks, recs);
	});
} GYS_CATCH_ALL

} // extern "C"
