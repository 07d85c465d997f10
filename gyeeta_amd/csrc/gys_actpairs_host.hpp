// gys_actpairs_host.hpp -- host side of the live (listener, client task group) rows (kernels and layout: gys_actpairs.hpp; definition:
// "Live active-connection rows" in include/gysketch.h).  Included once by gys_engine.hip in front of gys_json.hpp (gys_json_activeconn
// reads the rows through actp_list_host).
//
// Room: the host keeps an UPPER BOUND of the occupied entries of the buffer in use -- every call adds its row count.  A call that could
// take the bound past half of the entries first reads the exact count back (8 bytes); if that still does not leave room, and a window has
// closed since the last rebuild (entries only die at a close), the live entries are re-inserted into the other buffer and counted.  With
// live keys + the call's new keys <= actconn_pair_cap <= entries / 2 the call then finds room for every row.
#pragma once

namespace {

#define ACTP_CHECK()                                                                         \
	if (!c->ap_entries) {                                                                \
		set_err("the active-connection row table is off (gys_config.actconn_pair_cap = 0)"); \
		return GYS_ERR_STATE;                                                        \
	}

ActPairTbl actp_view(const gys_ctx *c, uint32_t b) { return ActPairTbl{c->ap_key[b].p, c->ap_ent[b].p, c->ap_entries - 1u}; }

uint32_t actp_scan_grid(const gys_ctx *c) { return std::max(1u, (uint32_t)std::min<uint64_t>(((uint64_t)c->ap_entries + 255u) / 256u, (uint64_t)c->ncu * 8)); }

int actp_read_ctr(gys_ctx *c, unsigned long long out[APC_NUM])
{
	HIPCHK(hipMemcpyAsync(out, c->ap_ctr.p, APC_NUM * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
}

// the live entries move to the other buffer; the bound becomes their number
int actp_rebuild(gys_ctx *c)
{
	const uint32_t from = c->ap_cur, to = c->ap_cur ^ 1u;
	HIPCHK(hipMemsetAsync(c->ap_key[to].p, 0xFF, (uint64_t)c->ap_entries * sizeof(ActPairKey), c->stream));
	HIPCHK(hipMemsetAsync(c->ap_ent[to].p, 0, (uint64_t)c->ap_entries * sizeof(ActPairEnt), c->stream));
	HIPCHK(hipMemsetAsync(c->ap_ctr.p + APC_OCCUPIED, 0, sizeof(unsigned long long), c->stream));
	hipLaunchKernelGGL(k_actp_rebuild, dim3(actp_scan_grid(c)), dim3(256), 0, c->stream, actp_view(c, from), actp_view(c, to), c->epoch, c->ap_ctr.p);
	HIPCHK(hipGetLastError());
	c->ap_cur = to;
	c->ap_rebuilds++;
	unsigned long long ctr[APC_NUM];
	const int rc = actp_read_ctr(c, ctr);
	if (rc) return rc;
	c->ap_occ_bound = ctr[APC_OCCUPIED];
	return GYS_OK;
}

// the rows of one gys_ingest_active_conns[_dev] call into the table (run_actconn; enq_mu or the exclusive call lock is held)
int actp_ingest(gys_ctx *c, const uint8_t *d_batch, uint32_t n)
{
	const uint64_t half = c->ap_entries / 2u;
	if (c->ap_occ_bound + n > half) {
		unsigned long long ctr[APC_NUM];
		int rc = actp_read_ctr(c, ctr);
		if (rc) return rc;
		c->ap_occ_bound = ctr[APC_OCCUPIED];
		if (c->ap_occ_bound + n > half && c->ap_occ_bound && c->ap_rebuild_epoch != c->epoch) {
			if ((rc = actp_rebuild(c)) != GYS_OK) return rc;
			c->ap_rebuild_epoch = c->epoch;
		}
	}
	ActPairP p{};
	p.batch = d_batch;
	p.n = n;
	p.t = actp_view(c, c->ap_cur);
	p.epoch = c->epoch;
	p.ctr = c->ap_ctr.p;
	if (n <= GYS_ACTP_FUSED_MAX) { // a partha's report: one launch
		hipLaunchKernelGGL(k_actp_all, dim3(1), dim3(GYS_ACTP_FUSED_MAX), 0, c->stream, p);
	} else {
		const int rc = c->ap_row_ent.grow(n, c->stream);
		if (rc) return rc;
		p.row_ent = c->ap_row_ent.p;
		const dim3 grid((n + 255u) / 256u);
		hipLaunchKernelGGL(k_actp_find, grid, dim3(256), 0, c->stream, p);
		hipLaunchKernelGGL(k_actp_keep, grid, dim3(256), 0, c->stream, p);
		hipLaunchKernelGGL(k_actp_add, grid, dim3(256), 0, c->stream, p);
	}
	HIPCHK(hipGetLastError());
	c->ap_occ_bound = std::min<uint64_t>(c->ap_occ_bound + n, c->ap_entries);
	return GYS_OK;
}

// a caller's selection, checked; NULL = everything
int actp_sel(const gys_actconn_sel *sel, gys_actconn_sel &s)
{
	s = gys_actconn_sel{};
	s.struct_size = (uint32_t)sizeof(gys_actconn_sel);
	if (!sel) return GYS_OK;
	const uint32_t known = GYS_ACS_BY_LISTENER | GYS_ACS_BY_CLIENT | GYS_ACS_BY_HOST | GYS_ACS_KIND_LOCAL | GYS_ACS_KIND_REMOTE;
	if (sel->struct_size != sizeof(gys_actconn_sel) || (sel->flags & ~known)) {
		set_err("bad selection (struct_size %u, expected %zu; flags %#x)", sel->struct_size, sizeof(gys_actconn_sel), sel->flags);
		return GYS_ERR_INVAL;
	}
	s = *sel;
	return GYS_OK;
}

// the matches into d_out[0 .. cap), their number into *nmatch (synchronous: one read of the count)
int actp_list_run(gys_ctx *c, const gys_actconn_sel &s, gys_actconn_row *d_out, uint32_t cap, uint32_t *nmatch)
{
	HIPCHK(hipMemsetAsync(c->ap_ctr.p + APC_MATCH, 0, sizeof(unsigned long long), c->stream));
	ActPairListP p{};
	p.t = actp_view(c, c->ap_cur);
	p.epoch = c->epoch;
	p.gid = c->gid_tbl;
	p.svc_host = c->svc_host;
	p.nsvc = c->nsvc;
	p.sel = s;
	p.out = d_out;
	p.cap = d_out ? cap : 0u;
	p.count = c->ap_ctr.p + APC_MATCH;
	{
		ProfScope ps(c, "actconn_list");
		hipLaunchKernelGGL(k_actp_list, dim3(actp_scan_grid(c)), dim3(256), 0, c->stream, p);
		HIPCHK(hipGetLastError());
	}
	unsigned long long cnt = 0;
	HIPCHK(hipMemcpyAsync(&cnt, c->ap_ctr.p + APC_MATCH, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	*nmatch = (uint32_t)cnt;
	return GYS_OK;
}

// the matches on the host in (listener id, client id, kind) order; more than cap: GYS_ERR_NOMEM with *nmatch set and `rows` empty
int actp_list_host(gys_ctx *c, const gys_actconn_sel &s, uint32_t cap, std::vector<gys_actconn_row> &rows, uint32_t *nmatch)
{
	rows.clear();
	const uint32_t dcap = std::min(cap, c->ap_entries);
	int rc = c->ap_rows.grow(std::max(dcap, 1u), c->stream);
	if (rc) return rc;
	if ((rc = actp_list_run(c, s, c->ap_rows.p, dcap, nmatch)) != GYS_OK) return rc;
	if (*nmatch > cap) {
		set_err("%u rows match, room for %u", *nmatch, cap);
		return GYS_ERR_NOMEM;
	}
	rows.resize(*nmatch);
	if (*nmatch) {
		HIPCHK(hipMemcpyAsync(rows.data(), c->ap_rows.p, (uint64_t)*nmatch * sizeof(gys_actconn_row), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
	}
	std::sort(rows.begin(), rows.end(), [](const gys_actconn_row &a, const gys_actconn_row &b) {
		if (a.listener_glob_id != b.listener_glob_id) return a.listener_glob_id < b.listener_glob_id;
		if (a.cli_aggr_task_id != b.cli_aggr_task_id) return a.cli_aggr_task_id < b.cli_aggr_task_id;
		return a.kind < b.kind;
	});
	return GYS_OK;
}

static_assert(sizeof(gys_actconn_row) == 128 && sizeof(gys_actconn_sel) == 40 && sizeof(ActPairKey) == 24 && sizeof(ActPairEnt) == 104, "table layouts");

} // namespace

extern "C" {

int gys_actconn_list_dev(gys_ctx *c, const gys_actconn_sel *sel, gys_actconn_row *d_out, uint32_t cap, uint32_t *nmatch)
try {
	GYS_ENTER(c);
	if (nmatch) *nmatch = 0;
	if (!c || !nmatch || (cap && !d_out)) return GYS_ERR_INVAL;
	ACTP_CHECK();
	gys_actconn_sel s;
	const int rc = actp_sel(sel, s);
	if (rc) return rc;
	return actp_list_run(c, s, d_out, cap, nmatch);
} GYS_CATCH_ALL

int gys_actconn_list(gys_ctx *c, const gys_actconn_sel *sel, gys_actconn_row *out, uint32_t cap, uint32_t *nout, uint32_t *nmatch)
try {
	GYS_ENTER(c);
	if (nout) *nout = 0;
	if (nmatch) *nmatch = 0;
	if (!c || !nout || !nmatch || (cap && !out)) return GYS_ERR_INVAL;
	ACTP_CHECK();
	gys_actconn_sel s;
	int rc = actp_sel(sel, s);
	if (rc) return rc;
	std::vector<gys_actconn_row> rows;
	if ((rc = actp_list_host(c, s, cap, rows, nmatch)) != GYS_OK) return rc;
	if (!rows.empty()) memcpy(out, rows.data(), rows.size() * sizeof(gys_actconn_row));
	*nout = (uint32_t)rows.size();
	return GYS_OK;
} GYS_CATCH_ALL

int gys_actconn_svc_stats_dev(gys_ctx *c, double *d_out)
try {
	GYS_ENTER(c);
	if (!c || (!d_out && c->nsvc)) return GYS_ERR_INVAL;
	ACTP_CHECK();
	const uint64_t n = (uint64_t)c->nsvc * 4u;
	if (!n) return GYS_OK;
	const int rc = c->ap_acc.grow(n, c->stream);
	if (rc) return rc;
	HIPCHK(hipMemsetAsync(c->ap_acc.p, 0, n * sizeof(unsigned long long), c->stream));
	ProfScope ps(c, "actconn_svc_stats");
	hipLaunchKernelGGL(k_actp_svc_accum, dim3(actp_scan_grid(c)), dim3(256), 0, c->stream, actp_view(c, c->ap_cur), c->epoch, c->gid_tbl, c->nsvc, c->ap_acc.p);
	hipLaunchKernelGGL(k_actp_svc_convert, dim3(std::max(1u, (uint32_t)std::min<uint64_t>((n + 255u) / 256u, (uint64_t)c->ncu * 8))), dim3(256), 0, c->stream, c->ap_acc.p, n,
			   d_out);
	HIPCHK(hipGetLastError());
	return GYS_OK;
} GYS_CATCH_ALL

int gys_actconn_table_stats(gys_ctx *c, gys_actconn_tblstats *out)
try {
	GYS_ENTER(c);
	if (!c || !out) return GYS_ERR_INVAL;
	ACTP_CHECK();
	gys_actconn_sel s;
	(void)actp_sel(nullptr, s);
	uint32_t live = 0;
	int rc = actp_list_run(c, s, nullptr, 0u, &live);
	if (rc) return rc;
	unsigned long long ctr[APC_NUM];
	if ((rc = actp_read_ctr(c, ctr)) != GYS_OK) return rc;
	out->entries = c->ap_entries;
	out->occupied = ctr[APC_OCCUPIED];
	out->live_keys = live;
	out->rows_dropped = ctr[APC_DROPPED];
	out->rows_bad_key = ctr[APC_BADKEY];
	out->rebuilds = c->ap_rebuilds;
	return GYS_OK;
} GYS_CATCH_ALL

} // extern "C"
