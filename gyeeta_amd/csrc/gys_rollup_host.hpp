// gys_rollup_host.hpp -- host side of the three roll-up families over the fixed scopes (host / cluster / this rank): the digests
// (kernels: gys_rollup.hpp), the distinct counts (gys_hllroll.hpp) and the group histograms of the levels (gys_histroll.hpp).  Included once
// by gys_engine.hip, ahead of gys_rollsel_host.hpp (the filtered roll-ups run their own member lists through rollup_run / hll_union_launch /
// hist_union_rows).  The member lists come from the cached groupings of the engine (ensure_host_groups / ensure_cluster_groups).
#pragma once

extern "C" {

// what the fixed scopes share: the scope's number of groups, the cached lists it needs, and the partial slots a two-stage union takes
// (a file / record per chunk of the host lists, of the cluster lists, or of the contiguous host results of the rank's union)
static int rollup_scope(gys_ctx *c, int scope, uint32_t *ngroups, uint32_t *nparts)
{
	const uint32_t nh = (uint32_t)c->hosts.size();
	*ngroups = scope == GYS_ROLLUP_HOST ? nh : (scope == GYS_ROLLUP_CLUSTER ? (uint32_t)c->cluster_names.size() : 1u);
	*nparts = 0;
	if (!*ngroups) return GYS_OK;
	int rc = ensure_host_groups(c);
	if (rc == GYS_OK && scope == GYS_ROLLUP_CLUSTER) rc = ensure_cluster_groups(c);
	if (rc) return rc;
	*nparts = std::max(std::max(c->host_groups.nchunks, scope == GYS_ROLLUP_CLUSTER ? c->cluster_groups.nchunks : 0u), (nh + GYS_RB_CHUNK_SERVICES - 1) / GYS_RB_CHUNK_SERVICES);
	return GYS_OK;
}

// ------------------------------------------------------------------------------------------------ roll-up digests
// bins of `ngroups` groups <- the members the chunks name; slabs out.  d_chunks / d_members: DEVICE arrays.
static int rollup_run(gys_ctx *c, int kind, const RollupChunk *d_chunks, uint32_t nchunks, const uint32_t *d_members, uint32_t ngroups,
		      const gys_tdigest_slab *d_in, gys_tdigest_slab *d_out)
{
	if (!ngroups) return GYS_OK;
	const int rcg = c->rb_bins.grow((size_t)ngroups * GYS_RB_STRIDE, c->stream);
	if (rcg) return rcg;
	RollupP rp{};
	rp.d = digest_params(c);
	rp.chunks = d_chunks;
	rp.nchunks = nchunks;
	rp.members = d_members;
	rp.kind = kind;
	rp.in = d_in;
	rp.bins = c->rb_bins.p;
	rp.out = d_out;
	rp.ngroups = ngroups;
	{
		ProfScope ps(c, kind == 0 ? "rollup_services" : "rollup_slabs");
		const size_t words = (size_t)ngroups * (GYS_RB_HDR + 1u);
		hipLaunchKernelGGL(k_rollup_init, dim3((uint32_t)std::min<size_t>((words + 255) / 256, (size_t)c->ncu * 16)), dim3(256), 0, c->stream, c->rb_bins.p, ngroups);
		if (nchunks) hipLaunchKernelGGL(k_rollup_accum, dim3(std::min<uint32_t>(nchunks, (uint32_t)c->ncu * 16)), dim3(GYS_RB_NT), 0, c->stream, rp);
		hipLaunchKernelGGL(k_rollup_mark, dim3(std::min<uint32_t>(ngroups, (uint32_t)c->ncu * 8)), dim3(256), 0, c->stream, rp);
		if (nchunks) hipLaunchKernelGGL(k_rollup_refine, dim3(std::min<uint32_t>(nchunks, (uint32_t)c->ncu * 16)), dim3(GYS_RB_NT), 0, c->stream, rp);
		hipLaunchKernelGGL(k_rollup_cluster, dim3(std::min<uint32_t>(ngroups, (uint32_t)c->ncu * 8)), dim3(256), 0, c->stream, rp);
	}
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

// groups of slabs (kind 1): g's members are indices into d_in; the chunk lists are cut and travel with the call
static int rollup_slabs(gys_ctx *c, const GroupLists &g, const gys_tdigest_slab *d_in, gys_tdigest_slab *d_out)
{
	if (!g.ngroups()) return GYS_OK;
	std::vector<RollupChunk> chunks;
	rollup_chunks(g.off, GYS_RB_CHUNK_SLABS, chunks);
	DevBuf<RollupChunk> d_chunks;
	DevBuf<uint32_t> d_mem;
	int rc = d_chunks.upload(chunks, c->stream);
	if (rc == GYS_OK) rc = d_mem.upload(g.members, c->stream);
	if (rc == GYS_OK) rc = rollup_run(c, 1, d_chunks.p, (uint32_t)chunks.size(), d_mem.p, g.ngroups(), d_in, d_out);
	HIPCHK(hipStreamSynchronize(c->stream)); // the lists are freed at scope exit
	return rc;
}

int gys_tdigest_rollup_dev(gys_ctx *c, int scope, gys_tdigest_slab *d_out)
try {
	GYS_ENTER(c);
	if (!c || !d_out || scope < GYS_ROLLUP_HOST || scope > GYS_ROLLUP_GLOBAL) return GYS_ERR_INVAL;
	TDIGEST_CHECK();
	const uint32_t nh = (uint32_t)c->hosts.size();
	if (!nh) {
		if (scope == GYS_ROLLUP_GLOBAL) HIPCHK(hipMemsetAsync(d_out, 0, sizeof(gys_tdigest_slab), c->stream));
		return GYS_OK;
	}
	uint32_t ngroups, nparts;
	int rc = rollup_scope(c, scope, &ngroups, &nparts);
	if (rc) return rc;
	const DeviceGroups &hg = c->host_groups;
	if (scope == GYS_ROLLUP_HOST) return rollup_run(c, 0, hg.chunks.p, hg.nchunks, hg.members.p, nh, nullptr, d_out);
	DevBuf<gys_tdigest_slab> d_hosts; // the hosts' slabs, then those of their groups
	if ((rc = d_hosts.grow(nh, c->stream)) != GYS_OK) return rc;
	rc = rollup_run(c, 0, hg.chunks.p, hg.nchunks, hg.members.p, nh, nullptr, d_hosts.p);
	GroupLists all;
	if (scope == GYS_ROLLUP_GLOBAL) all = groups_single(nh); // one group: every host slab
	if (rc == GYS_OK) rc = rollup_slabs(c, scope == GYS_ROLLUP_GLOBAL ? all : c->cluster_groups.h, d_hosts.p, d_out);
	HIPCHK(hipStreamSynchronize(c->stream)); // d_hosts is freed at scope exit
	return rc;
} GYS_CATCH_ALL

int gys_tdigest_merge_slabs_dev(gys_ctx *c, const gys_tdigest_slab *d_in, uint32_t n, gys_tdigest_slab *d_out)
try {
	GYS_ENTER(c);
	if (!c || !d_in || !d_out || n == 0) return GYS_ERR_INVAL;
	return rollup_slabs(c, groups_single(n), d_in, d_out);
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ distinct counts (gys_hllroll.hpp)
// the scratch buffer: [partial files: one per chunk][host files][group files], each part 256-byte aligned.  Grows, never shrinks; its
// size follows from the registered services / hosts / clusters (chunks <= services / 1024 + hosts), not from how often it is asked for.
static int hll_scratch(gys_ctx *c, size_t nparts, size_t nhostfiles, size_t ngroupfiles, uint8_t **parts, uint8_t **hostfiles, uint8_t **groupfiles)
{
	const size_t m = (size_t)1 << c->cfg.svc_hll_p;
	const size_t a = align_up(std::max<size_t>(nparts, 1) * m, 256), b = align_up(nhostfiles * m, 256), g = align_up(ngroupfiles * m, 256);
	const int rc = c->hl_buf.grow(a + b + g, c->stream);
	if (rc) return rc;
	*parts = c->hl_buf.p;
	if (hostfiles) *hostfiles = c->hl_buf.p + a;
	if (groupfiles) *groupfiles = c->hl_buf.p + a + b;
	return GYS_OK;
}

static void hll_union_launch(gys_ctx *c, const HllUnionP &q)
{
	if (q.nchunks) hipLaunchKernelGGL(k_hll_union, dim3(std::min<uint32_t>(q.nchunks, (uint32_t)c->ncu * 8)), dim3(GYS_HLL_NT), 0, c->stream, q);
}
// dst[0] = union of the n contiguous files at src: chunks of GYS_RB_CHUNK_SERVICES files into `parts`, then the chunks' files
static void hll_union_contiguous(gys_ctx *c, const uint8_t *src, uint32_t n, uint8_t *parts, uint8_t *dst)
{
	const uint32_t p = c->cfg.svc_hll_p, nch = (n + GYS_RB_CHUNK_SERVICES - 1) / GYS_RB_CHUNK_SERVICES;
	if (nch <= 1) {
		hll_union_launch(c, HllUnionP{src, dst, nullptr, nullptr, 1u, n, std::max(n, 1u), p});
		return;
	}
	hll_union_launch(c, HllUnionP{src, parts, nullptr, nullptr, nch, n, GYS_RB_CHUNK_SERVICES, p});
	hll_union_launch(c, HllUnionP{parts, dst, nullptr, nullptr, 1u, nch, nch, p});
}

// host / cluster / rank files and estimates of the services' files at src ([nsvc] files: the open registers, or a level's files)
static int hll_rollup_src(gys_ctx *c, const uint8_t *src, int scope, uint8_t *d_regs, double *d_est)
{
	const uint32_t p = c->cfg.svc_hll_p, nh = (uint32_t)c->hosts.size();
	const size_t m = (size_t)1 << p;
	uint32_t ngroups, nparts;
	int rc = rollup_scope(c, scope, &ngroups, &nparts);
	if (rc || !ngroups) return rc;
	const DeviceGroups &hg = c->host_groups, &cg = c->cluster_groups;
	uint8_t *parts = nullptr, *hostfiles = nullptr, *groupfiles = nullptr;
	rc = hll_scratch(c, nparts, scope == GYS_ROLLUP_HOST && d_regs ? 0 : nh, scope == GYS_ROLLUP_HOST || d_regs ? 0 : ngroups, &parts, &hostfiles, &groupfiles);
	if (rc) return rc;
	if (scope == GYS_ROLLUP_HOST && d_regs) hostfiles = d_regs;
	uint8_t *out = scope == GYS_ROLLUP_HOST ? hostfiles : (d_regs ? d_regs : groupfiles);
	{
		ProfScope ps(c, "hll_rollup_hosts"); // the services' files -> one file per chunk -> one per host
		hll_union_launch(c, HllUnionP{src, parts, hg.chunks.p, hg.members.p, hg.nchunks, 0u, 0u, p});
		hll_union_launch(c, HllUnionP{parts, hostfiles, hg.gchunks.p, nullptr, nh, 0u, 0u, p});
	}
	if (scope != GYS_ROLLUP_HOST) {
		ProfScope ps(c, "hll_union_files");
		if (scope == GYS_ROLLUP_GLOBAL) {
			if (nh) hll_union_contiguous(c, hostfiles, nh, parts, out);
			else HIPCHK(hipMemsetAsync(out, 0, m, c->stream));
		} else {
			hll_union_launch(c, HllUnionP{hostfiles, parts, cg.chunks.p, cg.members.p, cg.nchunks, 0u, 0u, p});
			hll_union_launch(c, HllUnionP{parts, out, cg.gchunks.p, nullptr, ngroups, 0u, 0u, p});
		}
	}
	if (d_est) {
		ProfScope ps(c, "hll_estimate_groups");
		hll_estimate_launch(c, out, ngroups, d_est);
	}
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

int gys_hll_rollup_dev(gys_ctx *c, int scope, uint8_t *d_regs, double *d_est)
try {
	GYS_ENTER(c);
	if (!c || (!d_regs && !d_est) || scope < GYS_ROLLUP_HOST || scope > GYS_ROLLUP_GLOBAL || !HLL_ALIGNED(d_regs)) {
		set_err("gys_hll_rollup_dev: null outputs, an output that is not 16-byte aligned or an unknown scope");
		return GYS_ERR_INVAL;
	}
	HLL_CHECK();
	return hll_rollup_src(c, c->svc_hll, scope, d_regs, d_est);
} GYS_CATCH_ALL

int gys_hll_merge_files_dev(gys_ctx *c, const uint8_t *d_in, uint32_t n, uint8_t *d_out, double *d_est)
try {
	GYS_ENTER(c);
	if (!c || !d_in || (!d_out && !d_est) || n == 0 || !HLL_ALIGNED(d_in) || !HLL_ALIGNED(d_out)) {
		set_err("gys_hll_merge_files_dev: null pointers, a pointer that is not 16-byte aligned or n = 0");
		return GYS_ERR_INVAL;
	}
	HLL_CHECK();
	uint8_t *parts = nullptr, *groupfiles = nullptr;
	const int rc = hll_scratch(c, (n + GYS_RB_CHUNK_SERVICES - 1) / GYS_RB_CHUNK_SERVICES, 0, d_out ? 0 : 1, &parts, nullptr, &groupfiles);
	if (rc) return rc;
	uint8_t *out = d_out ? d_out : groupfiles;
	{
		ProfScope ps(c, "hll_union_files");
		hll_union_contiguous(c, d_in, n, parts, out);
	}
	if (d_est) hll_estimate_launch(c, out, 1u, d_est);
	HIPCHK(hipGetLastError());
	return GYS_OK;
} GYS_CATCH_ALL

// the level's files of every service once into c->hl_view (nsvc files; grows, never shrinks): the roll-ups of the open window then run on them
static int hll_level_files(gys_ctx *c, int level, uint64_t tusec)
{
	const int rc = c->hl_view.grow(std::max<size_t>((size_t)c->nsvc << c->cfg.svc_hll_p, 16), c->stream);
	if (rc) return rc;
	ProfScope ps(c, "hll_level_files");
	return hll_level_view(c, level, tusec, 0u, c->nsvc, c->hl_view.p, nullptr);
}

int gys_hll_rollup_level_dev(gys_ctx *c, int scope, int level, uint64_t tusec, uint8_t *d_regs, double *d_est)
try {
	GYS_ENTER(c);
	if (!c || (!d_regs && !d_est) || scope < GYS_ROLLUP_HOST || scope > GYS_ROLLUP_GLOBAL || !HLL_ALIGNED(d_regs)) {
		set_err("gys_hll_rollup_level_dev: null outputs, an output that is not 16-byte aligned or an unknown scope");
		return GYS_ERR_INVAL;
	}
	HLL_LEVEL_CHECK(level);
	const int rc = hll_level_files(c, level, tusec);
	if (rc) return rc;
	return hll_rollup_src(c, c->hl_view.p, scope, d_regs, d_est);
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ group histograms of the levels (gys_histroll.hpp)
// the scratch buffer: [partial records: one per chunk][host records].  Grows, never shrinks (chunks <= services / 1024 + groups).
static int hist_union_scratch(gys_ctx *c, size_t nparts, size_t nhostrecs, gys_hist_rec **parts, gys_hist_rec **hostrecs)
{
	const size_t a = std::max<size_t>(nparts, 1);
	const int rc = c->hr_buf.grow(a + nhostrecs, c->stream);
	if (rc) return rc;
	*parts = c->hr_buf.p;
	if (hostrecs) *hostrecs = c->hr_buf.p + a;
	return GYS_OK;
}

static void hist_union_launch(gys_ctx *c, const HistUnionP &q)
{
	if (q.nchunks) hipLaunchKernelGGL(k_hist_level_union, dim3(std::min<uint32_t>(q.nchunks, (uint32_t)c->ncu * 8)), dim3(GYS_HR_NT), 0, c->stream, q);
}

// where the members' records of a group histogram come from: a level at tusec, a planned period, or a per-service array as it stands
// (the QPS / active-connection histograms).  One descriptor, so that the fixed scopes and the filtered selection share one path per family.
struct HistMemberSrc {
	enum Kind { LEVEL, PERIOD, PLAIN } kind;
	int level;                 // LEVEL
	uint64_t tusec;            // LEVEL
	const LevelPeriodP *plan;  // PERIOD: period_plan()'s result
	const gys_hist_rec *recs;  // PLAIN: [nsvc]
};
static HistMemberSrc hist_src_level(int level, uint64_t tusec) { return HistMemberSrc{HistMemberSrc::LEVEL, level, tusec, nullptr, nullptr}; }
static HistMemberSrc hist_src_period(const LevelPeriodP *plan) { return HistMemberSrc{HistMemberSrc::PERIOD, 0, 0, plan, nullptr}; }
static HistMemberSrc hist_src_plain(const gys_hist_rec *recs) { return HistMemberSrc{HistMemberSrc::PLAIN, 0, 0, nullptr, recs}; }

// the sources of `level` at tusec for every service, exactly as level_view() reads them:
// tq = max(tusec / 10^6, the last close) -- never the open window
static void hist_union_level(gys_ctx *c, int level, uint64_t tusec, HistUnionP &q)
{
	int64_t tq = (int64_t)(tusec / 1000000ull);
	if (tq < c->lvl_t_last) tq = c->lvl_t_last;
	q = HistUnionP{};
	q.v.win = c->hist_win;
	q.v.all = c->hist_all;
	q.v.meta = c->cfg.enable_tdigest ? c->td_meta : nullptr;
	q.v.epoch_open = c->epoch + (c->prepared ? 1u : 0u);
	level_source(c, level, tq, &q.v.mode, &q.v.sub);
	q.v.last_tag = c->cfg.enable_tdigest ? c->lvl_last_tag : nullptr;
	q.v.last_epoch = c->lvl_last_epoch;
}

// the members' records -> one record per chunk (parts) -> one per row (d_rows).  Levels and periods: the fold of the buffered values first
// (the members' open windows, as level_view() / level_period() fold the slots they read)
static int hist_union_rows(gys_ctx *c, const HistMemberSrc &src, const RollupChunk *d_chunks, uint32_t nchunks, const uint32_t *d_members, const RollupChunk *d_gchunks,
			   uint32_t nrows, gys_hist_rec *parts, gys_hist_rec *d_rows)
{
	if (src.kind != HistMemberSrc::PLAIN) {
		const int rcf = fold_range(c, 0, c->nsvc);
		if (rcf) return rcf;
	}
	ProfScope ps(c, "hist_rollup_union");
	if (src.kind == HistMemberSrc::PERIOD) {
		HistPeriodUnionP q{};
		q.v = *src.plan;
		q.dst = parts;
		q.chunks = d_chunks;
		q.members = d_members;
		q.nchunks = nchunks;
		if (nchunks) hipLaunchKernelGGL(k_hist_period_union, dim3(std::min<uint32_t>(nchunks, (uint32_t)c->ncu * 8)), dim3(GYS_HR_NT), 0, c->stream, q);
	} else {
		HistUnionP q{};
		if (src.kind == HistMemberSrc::LEVEL) {
			hist_union_level(c, src.level, src.tusec, q);
		} else {
			q.plain = 1;
			q.src = src.recs;
		}
		q.dst = parts;
		q.chunks = d_chunks;
		q.members = d_members;
		q.nchunks = nchunks;
		hist_union_launch(c, q);
	}
	HistUnionP g{};
	g.plain = 1;
	g.src = parts;
	g.dst = d_rows;
	g.chunks = d_gchunks;
	g.nchunks = nrows;
	hist_union_launch(c, g);
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

// one record per host slot / registered cluster / one of the members' records `src` into d_out (DEVICE): the fixed scopes of every family
static int hist_rollup_scope(gys_ctx *c, int scope, const HistMemberSrc &src, gys_hist_rec *d_out)
{
	const uint32_t nh = (uint32_t)c->hosts.size();
	uint32_t ngroups, nparts;
	int rc = rollup_scope(c, scope, &ngroups, &nparts);
	if (rc || !ngroups) return rc;
	const DeviceGroups &hg = c->host_groups, &cg = c->cluster_groups;
	gys_hist_rec *parts = nullptr, *hostrecs = nullptr;
	if ((rc = hist_union_scratch(c, nparts, scope == GYS_ROLLUP_HOST ? 0 : nh, &parts, &hostrecs)) != GYS_OK) return rc;
	if (scope == GYS_ROLLUP_HOST) hostrecs = d_out;
	if ((rc = hist_union_rows(c, src, hg.chunks.p, hg.nchunks, hg.members.p, hg.gchunks.p, nh, parts, hostrecs)) != GYS_OK) return rc;
	if (scope == GYS_ROLLUP_HOST) return GYS_OK;
	ProfScope ps(c, "hist_rollup_groups"); // host records -> cluster records / the rank's record (plain)
	HistUnionP g{};
	g.plain = 1;
	g.src = hostrecs;
	g.dst = parts;
	if (scope == GYS_ROLLUP_CLUSTER) {
		g.chunks = cg.chunks.p;
		g.members = cg.members.p;
		g.nchunks = cg.nchunks;
	} else { // equal chunks of the contiguous host records (no host: one empty chunk)
		g.n = nh;
		g.per = GYS_RB_CHUNK_SERVICES;
		g.nchunks = std::max(1u, (nh + GYS_RB_CHUNK_SERVICES - 1) / GYS_RB_CHUNK_SERVICES);
	}
	hist_union_launch(c, g);
	HistUnionP f{};
	f.plain = 1;
	f.src = parts;
	f.dst = d_out;
	if (scope == GYS_ROLLUP_CLUSTER) {
		f.chunks = cg.gchunks.p;
		f.nchunks = ngroups;
	} else {
		f.n = g.nchunks;
		f.per = std::max(g.nchunks, 1u);
		f.nchunks = 1u;
	}
	hist_union_launch(c, f);
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

#define HIST_SCOPE_OK(scope) ((scope) >= GYS_ROLLUP_HOST && (scope) <= GYS_ROLLUP_GLOBAL)

int gys_hist_rollup_level_dev(gys_ctx *c, int scope, int level, uint64_t tusec, gys_hist_rec *d_out)
try {
	GYS_ENTER(c);
	if (!c || !d_out || !HIST_SCOPE_OK(scope) || level < 0 || level >= GYS_NLEVELS) {
		set_err("gys_hist_rollup_level_dev: null output, an unknown scope or a level outside 0 .. %d", GYS_NLEVELS - 1);
		return GYS_ERR_INVAL;
	}
	LEVELS_CHECK();
	LEVEL0_CHECK(level);
	return hist_rollup_scope(c, scope, hist_src_level(level, tusec), d_out);
} GYS_CATCH_ALL

// the group record of the seconds [starttime, endtime] at tusec: the plan of gys_export_hist_period once, the members through k_hist_period_union
int gys_hist_rollup_period_dev(gys_ctx *c, int scope, int64_t starttime, int64_t endtime, uint64_t tusec, gys_hist_rec *d_out, int *level_used)
try {
	GYS_ENTER(c);
	if (!c || !d_out || !HIST_SCOPE_OK(scope)) {
		set_err("gys_hist_rollup_period_dev: null output or an unknown scope");
		return GYS_ERR_INVAL;
	}
	LEVELS_CHECK();
	LevelPeriodP plan;
	period_plan(c, starttime, endtime + 1, tusec, plan, level_used);
	return hist_rollup_scope(c, scope, hist_src_period(&plan), d_out);
} GYS_CATCH_ALL

int gys_svc_hist_rollup_dev(gys_ctx *c, int scope, int which, gys_hist_rec *d_out)
try {
	GYS_ENTER(c);
	if (!c || !d_out || !HIST_SCOPE_OK(scope) || which < 0 || which > 1) {
		set_err("gys_svc_hist_rollup_dev: null output, an unknown scope or which outside 0 .. 1");
		return GYS_ERR_INVAL;
	}
	LEVELS_CHECK();
	return hist_rollup_scope(c, scope, hist_src_plain(which ? c->act_hist : c->qps_hist), d_out);
} GYS_CATCH_ALL

// the day statistics of ngroups groups: their 5-day response records, QPS records and active-connection records into three record arrays of
// the scratch buffer (behind the `used` records a roll-up itself takes), then k_day_stats' rule on them.  `one` runs one family into its array.
static int day_stats_groups(gys_ctx *c, uint32_t ngroups, size_t used, const gys_rollup_row *d_rows, gys_listener_day_stats *d_out,
			    const std::function<int(int, gys_hist_rec *)> &one)
{
	// (grown to its full size before the first pointer into it is taken: a later grow would move the records)
	int rc = c->hr_buf.grow(used + 3ull * ngroups, c->stream);
	if (rc) return rc;
	for (int fam = 0; fam < 3; ++fam)
		if ((rc = one(fam, c->hr_buf.p + used + (size_t)fam * ngroups)) != GYS_OK) return rc;
	ProfScope ps(c, "day_stats_groups");
	const gys_hist_rec *r = c->hr_buf.p + used;
	hipLaunchKernelGGL(k_day_stats_groups, dim3((ngroups + 255) / 256), dim3(256), 0, c->stream, r, r + ngroups, r + 2ull * ngroups, d_rows, ngroups, d_out);
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

int gys_day_stats_rollup_dev(gys_ctx *c, int scope, uint64_t tusec, gys_listener_day_stats *d_out)
try {
	GYS_ENTER(c);
	if (!c || !d_out || !HIST_SCOPE_OK(scope)) {
		set_err("gys_day_stats_rollup_dev: null output or an unknown scope");
		return GYS_ERR_INVAL;
	}
	LEVELS_CHECK();
	uint32_t ngroups, nparts;
	const int rc = rollup_scope(c, scope, &ngroups, &nparts);
	if (rc || !ngroups) return rc;
	const size_t used = std::max<size_t>(nparts, 1) + (size_t)c->hosts.size(); // what hist_rollup_scope takes of the scratch buffer
	return day_stats_groups(c, ngroups, used, nullptr, d_out, [&](int fam, gys_hist_rec *recs) {
		return hist_rollup_scope(c, scope, fam == 0 ? hist_src_level(2, tusec) : hist_src_plain(fam == 1 ? c->qps_hist : c->act_hist), recs);
	});
} GYS_CATCH_ALL

} // extern "C"
