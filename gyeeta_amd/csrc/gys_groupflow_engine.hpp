// gys_groupflow_engine.hpp -- engine side of the group flow map (kernels: gys_groupflow.hpp; definition: "Group flow map" in
// include/gysketch.h).  Included once by gys_engine.hip behind gys_svccomp_engine.hpp (dep_ensure_tasks, dep_edge_params, dep_edges_run,
// dep_levels_run, dep_collect).
//
// A call COUNTS the service edges first (k_dep_edges with cap 0, one read), sizes the keyed table from that count -- a power of two
// >= 2 x min(edges, domain^2), never from the row count -- and then runs a fixed list of launches: the first-of-group flags over the
// task -> services list, the accumulation, the walk of the keyed table.  The counter words are read once behind them; the host form
// walks the keyed table a second time to write the rows it has counted.  Nothing is cached between calls, no engine state is modified,
// and every buffer is scratch of the context that only grows (nothing is allocated before the first call).
#pragma once

namespace {

struct GfMap {
	uint32_t ndomain = 0;
	uint64_t edges = 0; // the count pass
	uint32_t tcap = 0;  // entries of the keyed table; 0: the map is empty, no kernel ran
};

int gf_check_group_by(int group_by)
{
	if (group_by == GYS_GROUP_HOST || group_by == GYS_GROUP_CLUSTER || group_by == GYS_GROUP_LABEL) return GYS_OK;
	set_err("group flow map: group_by %d (GYS_GROUP_HOST, _CLUSTER or _LABEL)", group_by);
	return GYS_ERR_INVAL;
}

uint32_t gf_domain(const gys_ctx *c, int group_by)
{
	return group_by == GYS_GROUP_HOST ? (uint32_t)c->hosts.size() : group_by == GYS_GROUP_CLUSTER ? (uint32_t)c->cluster_names.size() : (c->svc_label.p ? c->label_domain : 0u);
}

int gf_sel(const gys_group_edge_sel *sel, GfRowsP &rp)
{
	rp.sel_flags = 0u;
	rp.src_group = rp.dst_group = GYS_NO_GROUP;
	if (!sel) return GYS_OK;
	if (sel->struct_size != sizeof(gys_group_edge_sel) || (sel->flags & ~(uint32_t)(GYS_GES_BY_SRC | GYS_GES_BY_DST | GYS_GES_NO_SELF))) {
		set_err("bad selection (struct_size %u, expected %zu; flags %#x)", sel->struct_size, sizeof(gys_group_edge_sel), sel->flags);
		return GYS_ERR_INVAL;
	}
	rp.sel_flags = sel->flags;
	rp.src_group = sel->src_group;
	rp.dst_group = sel->dst_group;
	return GYS_OK;
}

uint32_t gf_grid(const gys_ctx *c, uint64_t n) { return std::max(1u, (uint32_t)std::min<uint64_t>((n + 255u) / 256u, (uint64_t)c->ncu * 8)); }

// the keyed table of the map in c->gf_keys / c->gf_acc; the counter words are cleared first and are NOT read here
int gf_build(gys_ctx *c, int group_by, GfMap &m)
{
	int rc = dep_ensure_tasks(c);
	if (rc) return rc;
	if (!c->gf_ctr.p && (rc = c->gf_ctr.alloc(GFC_NUM)) != GYS_OK) return rc;
	m.ndomain = gf_domain(c, group_by);
	m.tcap = 0;
	m.edges = 0;
	if (!c->nsvc) return GYS_OK;
	DepEdgeP dp{};
	dep_edge_params(c, dp);
	(void)dep_sel(c, nullptr, dp);
	if ((rc = dep_edges_run<false>(c, dp, nullptr, 0u, &m.edges)) != GYS_OK) return rc;
	if (!m.edges || !m.ndomain) return GYS_OK; // (no label was ever set: every edge has an end in no group)
	const uint64_t want = std::min<uint64_t>(m.edges, (uint64_t)m.ndomain * m.ndomain);
	if (want > (1ull << 30)) {
		set_err("group flow map: up to %llu group edges: too many for the keyed table", (unsigned long long)want);
		return GYS_ERR_NOMEM;
	}
	uint32_t tcap = 256u;
	while (tcap < 2u * want) tcap <<= 1;
	const uint32_t nmem = c->dep_tasks.nbound();
	uint32_t hcap = 256u;
	while (hcap < 2u * (uint64_t)nmem) hcap <<= 1;
	if ((rc = c->gf_keys.grow(tcap, c->stream)) != GYS_OK || (rc = c->gf_acc.grow((uint64_t)tcap * GYS_GF_ACC, c->stream)) != GYS_OK ||
	    (rc = c->gf_first.grow(nmem, c->stream)) != GYS_OK || (rc = c->gf_hkey.grow(hcap, c->stream)) != GYS_OK || (rc = c->gf_hmin.grow(hcap, c->stream)) != GYS_OK)
		return rc;
	HIPCHK(hipMemsetAsync(c->gf_ctr.p, 0, GFC_NUM * sizeof(unsigned long long), c->stream));
	HIPCHK(hipMemsetAsync(c->gf_keys.p, 0xFF, (size_t)tcap * sizeof(unsigned long long), c->stream));
	HIPCHK(hipMemsetAsync(c->gf_acc.p, 0, (size_t)tcap * GYS_GF_ACC * sizeof(unsigned long long), c->stream));
	GfGroupP g{};
	g.group_by = (uint32_t)group_by;
	g.ndomain = m.ndomain;
	g.svc_host = c->svc_host;
	g.host_cluster = c->host_cluster;
	g.labels = c->svc_label;
	g.nsvc = c->nsvc;
	if (nmem) {
		ProfScope ps(c, "gf_first");
		HIPCHK(hipMemsetAsync(c->gf_hkey.p, 0xFF, (size_t)hcap * sizeof(unsigned long long), c->stream));
		HIPCHK(hipMemsetAsync(c->gf_hmin.p, 0xFF, (size_t)hcap * sizeof(uint32_t), c->stream));
		GfFirstP fp{};
		fp.g = g;
		fp.task_off = c->dep_task_off.p;
		fp.task_slot = c->dep_task_slot.p;
		fp.ntask = c->dep_tasks.ntasks();
		fp.nmem = nmem;
		fp.hkey = c->gf_hkey.p;
		fp.hmin = c->gf_hmin.p;
		fp.hmask = hcap - 1u;
		fp.first = c->gf_first.p;
		fp.ctr = c->gf_ctr.p;
		hipLaunchKernelGGL(k_gf_first_min, dim3(gf_grid(c, nmem)), dim3(256), 0, c->stream, fp);
		hipLaunchKernelGGL(k_gf_first_flag, dim3(gf_grid(c, nmem)), dim3(256), 0, c->stream, c->gf_first.p, (const uint32_t *)c->gf_hmin.p, hcap - 1u, nmem);
		HIPCHK(hipGetLastError());
	}
	{
		ProfScope ps(c, "gf_accum");
		GfAccP ap{};
		ap.d = dp;
		ap.g = g;
		ap.first = c->gf_first.p;
		ap.keys = c->gf_keys.p;
		ap.acc = c->gf_acc.p;
		ap.mask = tcap - 1u;
		ap.ctr = c->gf_ctr.p;
		hipLaunchKernelGGL(k_gf_accum, dim3(actp_scan_grid(c)), dim3(256), 0, c->stream, ap);
		HIPCHK(hipGetLastError());
	}
	m.tcap = tcap;
	return GYS_OK;
}

// one walk of the keyed table: rows under the selection into out[0 .. cap), the pairs with gu != gv into pairs[0 .. pcap)
int gf_rows_run(gys_ctx *c, const GfMap &m, GfRowsP rp, gys_group_edge *out, uint32_t cap, uint2 *pairs, uint32_t pcap)
{
	if (!m.tcap) return GYS_OK;
	HIPCHK(hipMemsetAsync(c->gf_ctr.p + GFC_GROUP_EDGES, 0, (GFC_NUM - GFC_GROUP_EDGES) * sizeof(unsigned long long), c->stream));
	rp.keys = c->gf_keys.p;
	rp.acc = c->gf_acc.p;
	rp.mask = m.tcap - 1u;
	rp.out = out;
	rp.cap = out ? cap : 0u;
	rp.pairs = pairs;
	rp.pcap = pairs ? pcap : 0u;
	rp.ctr = c->gf_ctr.p;
	ProfScope ps(c, "gf_rows");
	hipLaunchKernelGGL(k_gf_rows, dim3(gf_grid(c, m.tcap)), dim3(256), 0, c->stream, rp);
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

// the one read of the counter words; a probe loop that reached its cap, or a second count of the edges that differs from the first, is
// an error of the library, not of the caller
int gf_read_ctr(gys_ctx *c, const GfMap &m, unsigned long long ctr[GFC_NUM], gys_group_flow_stats *stats)
{
	memset(ctr, 0, GFC_NUM * sizeof(unsigned long long));
	if (m.tcap) {
		HIPCHK(hipMemcpyAsync(ctr, c->gf_ctr.p, GFC_NUM * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
		if (ctr[GFC_ERR]) {
			set_err("group flow map: %llu keys found no place in a table (%u entries); the map is not valid", ctr[GFC_ERR], m.tcap);
			return GYS_ERR_INTERNAL;
		}
		if (ctr[GFC_EDGES] != m.edges) {
			set_err("the edge count moved between the passes (%llu, %llu)", (unsigned long long)m.edges, ctr[GFC_EDGES]);
			return GYS_ERR_INTERNAL;
		}
	} else {
		ctr[GFC_EDGES] = ctr[GFC_NOGROUP] = m.edges;
	}
	if (stats) {
		stats->edges = ctr[GFC_EDGES];
		stats->edges_no_group = ctr[GFC_NOGROUP];
		stats->group_edges = ctr[GFC_GROUP_EDGES];
		stats->self_group_edges = ctr[GFC_SELF];
	}
	return GYS_OK;
}

// hops[] of every group of the domain into d_hops (m.ndomain > 0 words) from the root groups
int gf_traverse(gys_ctx *c, int group_by, GfMap &m, const uint32_t *root_groups, uint32_t nroots, uint32_t dir, uint32_t max_hops, uint32_t *d_hops)
{
	std::vector<uint32_t> roots;
	for (uint32_t i = 0; i < nroots; ++i)
		if (root_groups[i] < m.ndomain) roots.push_back(root_groups[i]);
	std::sort(roots.begin(), roots.end());
	roots.erase(std::unique(roots.begin(), roots.end()), roots.end());
	int rc;
	if ((rc = c->dep_roots.upload(roots, c->stream)) != GYS_OK) return rc;
	hipLaunchKernelGGL(k_dep_seed, dim3(gf_grid(c, m.ndomain)), dim3(256), 0, c->stream, d_hops, m.ndomain, (const uint32_t *)c->dep_roots.p, (uint32_t)roots.size());
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(c->stream)); // (roots is a local)
	if (roots.empty() || !m.tcap) return GYS_OK;
	// the pair array: at most one pair per occupied key, and the table is at most half full
	const uint32_t pcap = m.tcap / 2u;
	if ((rc = c->gf_pairs.grow(pcap, c->stream)) != GYS_OK) return rc;
	GfRowsP rp{};
	(void)gf_sel(nullptr, rp);
	if ((rc = gf_rows_run(c, m, rp, nullptr, 0u, c->gf_pairs.p, pcap)) != GYS_OK) return rc;
	unsigned long long ctr[GFC_NUM];
	if ((rc = gf_read_ctr(c, m, ctr, nullptr)) != GYS_OK) return rc;
	if (ctr[GFC_NPAIRS] > pcap) {
		set_err("group flow map: %llu pairs, room for %u", ctr[GFC_NPAIRS], pcap);
		return GYS_ERR_INTERNAL;
	}
	if (!ctr[GFC_NPAIRS]) return GYS_OK;
	return dep_levels_run(c, (const uint2 *)c->gf_pairs.p, ctr[GFC_NPAIRS], d_hops, m.ndomain, dir, max_hops);
}

static_assert(sizeof(gys_group_edge) == 64 && sizeof(gys_group_edge_sel) == 16 && sizeof(gys_group_flow_stats) == 32, "group flow layouts");

} // namespace

extern "C" {

int gys_group_edges_dev(gys_ctx *c, int group_by, const gys_group_edge_sel *sel, gys_group_edge *d_out, uint32_t cap, uint32_t *nmatch, gys_group_flow_stats *stats)
try {
	GYS_ENTER(c);
	if (nmatch) *nmatch = 0;
	if (stats) memset(stats, 0, sizeof(*stats));
	if (!c || !nmatch || (cap && !d_out)) return GYS_ERR_INVAL;
	ACTP_CHECK();
	int rc;
	GfRowsP rp{};
	if ((rc = gf_check_group_by(group_by)) != GYS_OK || (rc = gf_sel(sel, rp)) != GYS_OK) return rc;
	GfMap m;
	if ((rc = gf_build(c, group_by, m)) != GYS_OK) return rc;
	if ((rc = gf_rows_run(c, m, rp, d_out, cap, nullptr, 0u)) != GYS_OK) return rc;
	unsigned long long ctr[GFC_NUM];
	if ((rc = gf_read_ctr(c, m, ctr, stats)) != GYS_OK) return rc;
	*nmatch = (uint32_t)ctr[GFC_NMATCH];
	return GYS_OK;
} GYS_CATCH_ALL

int gys_group_edges(gys_ctx *c, int group_by, const gys_group_edge_sel *sel, gys_group_edge *out, uint32_t cap, uint32_t *nout, uint32_t *nmatch,
		    gys_group_flow_stats *stats)
try {
	GYS_ENTER(c);
	if (nout) *nout = 0;
	if (nmatch) *nmatch = 0;
	if (stats) memset(stats, 0, sizeof(*stats));
	if (!c || !nout || !nmatch || (cap && !out)) return GYS_ERR_INVAL;
	ACTP_CHECK();
	int rc;
	GfRowsP rp{};
	if ((rc = gf_check_group_by(group_by)) != GYS_OK || (rc = gf_sel(sel, rp)) != GYS_OK) return rc;
	GfMap m;
	if ((rc = gf_build(c, group_by, m)) != GYS_OK) return rc;
	if ((rc = gf_rows_run(c, m, rp, nullptr, 0u, nullptr, 0u)) != GYS_OK) return rc;
	unsigned long long ctr[GFC_NUM];
	if ((rc = gf_read_ctr(c, m, ctr, stats)) != GYS_OK) return rc;
	const uint32_t nm = (uint32_t)ctr[GFC_NMATCH];
	*nmatch = nm;
	if (nm > cap) {
		set_err("%u group edges match, room for %u", nm, cap);
		return GYS_ERR_NOMEM;
	}
	if (!nm) return GYS_OK;
	// the rows: the keyed table stands as it is, it is walked again
	if ((rc = c->gf_rows.grow(nm, c->stream)) != GYS_OK) return rc;
	if ((rc = gf_rows_run(c, m, rp, c->gf_rows.p, nm, nullptr, 0u)) != GYS_OK) return rc;
	std::vector<gys_group_edge> rows(nm);
	HIPCHK(hipMemcpyAsync(rows.data(), c->gf_rows.p, (size_t)nm * sizeof(gys_group_edge), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	std::sort(rows.begin(), rows.end(), [](const gys_group_edge &a, const gys_group_edge &b) { return a.src_group != b.src_group ? a.src_group < b.src_group : a.dst_group < b.dst_group; });
	memcpy(out, rows.data(), (size_t)nm * sizeof(gys_group_edge));
	*nout = nm;
	return GYS_OK;
} GYS_CATCH_ALL

int gys_group_deps_dev(gys_ctx *c, int group_by, const uint32_t *root_groups, uint32_t nroots, uint32_t dir, uint32_t max_hops, uint32_t *d_hops, uint32_t *ndomain,
		       uint32_t *nreached)
try {
	GYS_ENTER(c);
	if (ndomain) *ndomain = 0;
	if (nreached) *nreached = 0;
	if (!c || dir < 1u || dir > 3u || !d_hops || !nreached || (!root_groups && nroots)) return GYS_ERR_INVAL;
	ACTP_CHECK();
	int rc;
	if ((rc = gf_check_group_by(group_by)) != GYS_OK) return rc;
	GfMap m;
	if ((rc = gf_build(c, group_by, m)) != GYS_OK) return rc;
	if (ndomain) *ndomain = m.ndomain;
	if (!m.ndomain) return GYS_OK;
	if ((rc = gf_traverse(c, group_by, m, root_groups, nroots, dir, max_hops, d_hops)) != GYS_OK) return rc;
	return dep_collect(c, d_hops, m.ndomain, nullptr, 0u, nreached);
} GYS_CATCH_ALL

int gys_group_deps(gys_ctx *c, int group_by, const uint32_t *root_groups, uint32_t nroots, uint32_t dir, uint32_t max_hops, uint32_t *groups, uint32_t *hops, uint32_t cap,
		   uint32_t *nout, uint32_t *nreached)
try {
	GYS_ENTER(c);
	if (nout) *nout = 0;
	if (nreached) *nreached = 0;
	if (!c || dir < 1u || dir > 3u || !nout || !nreached || (!root_groups && nroots) || (cap && (!groups || !hops))) return GYS_ERR_INVAL;
	ACTP_CHECK();
	int rc;
	if ((rc = gf_check_group_by(group_by)) != GYS_OK) return rc;
	GfMap m;
	if ((rc = gf_build(c, group_by, m)) != GYS_OK) return rc;
	if (!m.ndomain) return GYS_OK;
	if ((rc = c->gf_hops.grow(m.ndomain, c->stream)) != GYS_OK) return rc;
	if ((rc = gf_traverse(c, group_by, m, root_groups, nroots, dir, max_hops, c->gf_hops.p)) != GYS_OK) return rc;
	const uint32_t dcap = std::min(cap, m.ndomain);
	if ((rc = c->dep_hits.grow(std::max(dcap, 1u), c->stream)) != GYS_OK) return rc;
	if ((rc = dep_collect(c, c->gf_hops.p, m.ndomain, c->dep_hits.p, dcap, nreached)) != GYS_OK) return rc;
	if (*nreached > cap) {
		set_err("%u groups reached, room for %u", *nreached, cap);
		return GYS_ERR_NOMEM;
	}
	std::vector<uint2> hits(*nreached);
	if (*nreached) {
		HIPCHK(hipMemcpyAsync(hits.data(), c->dep_hits.p, (uint64_t)*nreached * sizeof(uint2), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
	}
	std::sort(hits.begin(), hits.end(), [](const uint2 &a, const uint2 &b) { return a.y != b.y ? a.y < b.y : a.x < b.x; });
	for (uint32_t i = 0; i < *nreached; ++i) {
		groups[i] = hits[i].x;
		hops[i] = hits[i].y;
	}
	*nout = *nreached;
	return GYS_OK;
} GYS_CATCH_ALL

} // extern "C"
