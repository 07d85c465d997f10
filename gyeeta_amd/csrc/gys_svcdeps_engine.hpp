// gys_svcdeps_engine.hpp -- engine side of the service dependency graph (kernels: gys_svcdeps.hpp; the task -> services list:
// gys_svcdeps_host.hpp; definition: "Service dependency graph" in include/gysketch.h).  Included once by gys_engine.hip behind
// gys_actpairs_host.hpp (ACTP_CHECK, actp_view, actp_scan_grid).
//
// The bindings are host state (gys_ctx::svc_task_h).  gys_ctx::task_gen counts every call that can change the task -> services list
// (gys_set_listener_tasks, a delete, a registration); the first graph call after such a change rebuilds the list and uploads it.
//
// Scratch: a graph call COUNTS its edges first (k_dep_edges with cap 0: the same walk, nothing written), grows the pair / row buffer to
// that count and walks again to write them -- the table cannot change between the two passes (one stream, the call holds the context).
// The edge count is not bounded by the row count (a task group may own many listeners), so nothing is sized from the table.
#pragma once

namespace {

int dep_ensure_tasks(gys_ctx *c)
{
	if (!c->dep_ctr.p) {
		const int rc = c->dep_ctr.alloc(DPC_NUM);
		if (rc) return rc;
	}
	if (c->dep_tasks_gen == c->task_gen) return GYS_OK;
	c->svc_task_h.resize(c->nsvc, 0ull);
	HIPCHK(hipStreamSynchronize(c->stream)); // (an upload in flight may still read the old lists)
	c->dep_tasks = task_lists_build(c->svc_task_h.data(), c->svc_host_h.data(), GYS_NOSLOT, c->nsvc);
	if ((uint64_t)c->dep_tasks.longest() * 64u > 0xFFFFFFFFull) {
		set_err("a task group bound to %u listeners: too many for the edge pass", c->dep_tasks.longest());
		return GYS_ERR_NOMEM;
	}
	int rc;
	if ((rc = c->dep_task_id.upload(c->dep_tasks.ids, c->stream)) != GYS_OK || (rc = c->dep_task_off.upload(c->dep_tasks.off, c->stream)) != GYS_OK ||
	    (rc = c->dep_task_slot.upload(c->dep_tasks.slots, c->stream)) != GYS_OK)
		return rc;
	c->dep_tasks_gen = c->task_gen;
	return GYS_OK;
}

// a caller's selection, checked and resolved to slots; NULL = everything
int dep_sel(gys_ctx *c, const gys_svc_edge_sel *sel, DepEdgeP &p)
{
	p.sel_flags = 0u;
	p.src_slot = p.dst_slot = GYS_NOSLOT;
	p.src_task = 0ull;
	if (!sel) return GYS_OK;
	if (sel->struct_size != sizeof(gys_svc_edge_sel) || (sel->flags & ~(uint32_t)(GYS_SES_BY_SRC | GYS_SES_BY_DST))) {
		set_err("bad selection (struct_size %u, expected %zu; flags %#x)", sel->struct_size, sizeof(gys_svc_edge_sel), sel->flags);
		return GYS_ERR_INVAL;
	}
	p.sel_flags = sel->flags;
	if (sel->flags & GYS_SES_BY_SRC) {
		auto it = c->gid_map_h.find(sel->src_glob_id);
		if (it != c->gid_map_h.end()) {
			p.src_slot = it->second;
			p.src_task = c->svc_task_h[it->second];
		}
	}
	if (sel->flags & GYS_SES_BY_DST) {
		auto it = c->gid_map_h.find(sel->dst_glob_id);
		if (it != c->gid_map_h.end()) p.dst_slot = it->second;
	}
	return GYS_OK;
}

void dep_edge_params(gys_ctx *c, DepEdgeP &p)
{
	p.t = actp_view(c, c->ap_cur);
	p.epoch = c->epoch;
	p.gid = c->gid_tbl;
	p.task_id = c->dep_task_id.p;
	p.task_off = c->dep_task_off.p;
	p.task_slot = c->dep_task_slot.p;
	p.ntask = c->dep_tasks.ntasks();
	p.nsvc = c->nsvc;
	p.svc_gid = c->svc_gid;
	p.ctr = c->dep_ctr.p;
}

// one walk of the table: the edges into out[0 .. cap) (pairs or rows), their number into *nedges; with ctr_out the DPC_* words as well
template <bool FULL>
int dep_edges_run(gys_ctx *c, DepEdgeP p, void *out, uint32_t cap, uint64_t *nedges, unsigned long long *ctr_out = nullptr)
{
	HIPCHK(hipMemsetAsync(c->dep_ctr.p, 0, DPC_NUM * sizeof(unsigned long long), c->stream));
	p.out = out;
	p.cap = out ? cap : 0u;
	p.stats = ctr_out ? 1u : 0u;
	{
		ProfScope ps(c, "dep_edges");
		hipLaunchKernelGGL(k_dep_edges<FULL>, dim3(actp_scan_grid(c)), dim3(256), 0, c->stream, p);
		HIPCHK(hipGetLastError());
	}
	unsigned long long ctr[DPC_NUM];
	HIPCHK(hipMemcpyAsync(ctr, c->dep_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	*nedges = ctr[DPC_EDGES];
	if (ctr_out) memcpy(ctr_out, ctr, sizeof(ctr));
	if (*nedges > 0xFFFFFFFFull) {
		set_err("%llu edges: more than a 32-bit count holds", ctr[DPC_EDGES]);
		return GYS_ERR_NOMEM;
	}
	return GYS_OK;
}

// the levels of the search over `ne` pairs of indices below `n` (slots; the group flow map searches its group pairs over the domain), a few
// per read of the "changed" word; a level that claims nothing ends the search (at most n - 1 levels claim)
int dep_levels_run(gys_ctx *c, const uint2 *pairs, uint64_t ne, uint32_t *d_hops, uint32_t n, uint32_t dir, uint32_t max_hops)
{
	const uint32_t last = max_hops ? std::min(max_hops, n) : n;
	const uint32_t egrid = std::max(1u, (uint32_t)std::min<uint64_t>((ne + 255u) / 256u, (uint64_t)c->ncu * 8));
	ProfScope ps(c, "dep_levels");
	for (uint32_t level = 0; level < last;) {
		HIPCHK(hipMemsetAsync(c->dep_ctr.p + DPC_CHANGED, 0, sizeof(unsigned long long), c->stream));
		const uint32_t upto = std::min(last, level + 4u);
		for (; level < upto; ++level)
			hipLaunchKernelGGL(k_dep_level, dim3(egrid), dim3(256), 0, c->stream, pairs, ne, d_hops, n, level, dir, c->dep_ctr.p + DPC_CHANGED);
		HIPCHK(hipGetLastError());
		unsigned long long changed = 0;
		HIPCHK(hipMemcpyAsync(&changed, c->dep_ctr.p + DPC_CHANGED, sizeof(changed), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
		if (!changed) break;
	}
	return GYS_OK;
}

// the reached slots of c->dep_hops / d_hops from the roots; *nreached = their number
int dep_traverse(gys_ctx *c, const uint64_t *root_ids, uint32_t nroots, uint32_t dir, uint32_t max_hops, uint32_t *d_hops, uint32_t *nreached)
{
	int rc = dep_ensure_tasks(c);
	if (rc) return rc;
	*nreached = 0;
	if (!c->nsvc) return GYS_OK;
	// the roots: known ids, as distinct slots in ascending order
	std::vector<uint32_t> roots;
	for (uint32_t i = 0; i < nroots; ++i) {
		auto it = c->gid_map_h.find(root_ids[i]);
		if (it != c->gid_map_h.end()) roots.push_back(it->second);
	}
	std::sort(roots.begin(), roots.end());
	roots.erase(std::unique(roots.begin(), roots.end()), roots.end());
	if ((rc = c->dep_roots.upload(roots, c->stream)) != GYS_OK) return rc;
	const uint32_t sgrid = std::max(1u, (uint32_t)std::min<uint64_t>(((uint64_t)c->nsvc + 255u) / 256u, (uint64_t)c->ncu * 8));
	hipLaunchKernelGGL(k_dep_seed, dim3(sgrid), dim3(256), 0, c->stream, d_hops, c->nsvc, (const uint32_t *)c->dep_roots.p, (uint32_t)roots.size());
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(c->stream)); // (roots is a local)
	if (roots.empty()) return GYS_OK;
	// the pair array: count, grow, write
	DepEdgeP p{};
	dep_edge_params(c, p);
	(void)dep_sel(c, nullptr, p);
	uint64_t ne = 0, ne2 = 0;
	if ((rc = dep_edges_run<false>(c, p, nullptr, 0u, &ne)) != GYS_OK) return rc;
	if (ne) {
		if ((rc = c->dep_pairs.grow(ne, c->stream)) != GYS_OK) return rc;
		if ((rc = dep_edges_run<false>(c, p, c->dep_pairs.p, (uint32_t)ne, &ne2)) != GYS_OK) return rc;
		if (ne2 != ne) {
			set_err("the edge count moved between the passes (%llu, %llu)", (unsigned long long)ne, (unsigned long long)ne2);
			return GYS_ERR_INTERNAL;
		}
		if ((rc = dep_levels_run(c, (const uint2 *)c->dep_pairs.p, ne, d_hops, c->nsvc, dir, max_hops)) != GYS_OK) return rc;
	}
	return GYS_OK;
}

// the reached of the `n` words of d_hops: counted, and with d_hits compacted into it (room for `cap`)
int dep_collect(gys_ctx *c, const uint32_t *d_hops, uint32_t n, uint2 *d_hits, uint32_t cap, uint32_t *nreached)
{
	*nreached = 0;
	if (!n) return GYS_OK;
	HIPCHK(hipMemsetAsync(c->dep_ctr.p + DPC_REACHED, 0, sizeof(unsigned long long), c->stream));
	const uint32_t sgrid = std::max(1u, (uint32_t)std::min<uint64_t>(((uint64_t)n + 255u) / 256u, (uint64_t)c->ncu * 8));
	hipLaunchKernelGGL(k_dep_collect, dim3(sgrid), dim3(256), 0, c->stream, d_hops, n, d_hits, d_hits ? cap : 0u, c->dep_ctr.p + DPC_REACHED);
	HIPCHK(hipGetLastError());
	unsigned long long cnt = 0;
	HIPCHK(hipMemcpyAsync(&cnt, c->dep_ctr.p + DPC_REACHED, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	*nreached = (uint32_t)cnt;
	return GYS_OK;
}

static_assert(sizeof(gys_svc_edge) == 64 && sizeof(gys_svc_edge_sel) == 24 && sizeof(gys_svcgraph_stats_t) == 48, "graph layouts");

} // namespace

extern "C" {

int gys_set_listener_tasks(gys_ctx *c, const uint64_t *glob_ids, const uint64_t *aggr_task_ids, uint32_t n)
try {
	GYS_ENTER(c);
	if (!c || ((!glob_ids || !aggr_task_ids) && n)) return GYS_ERR_INVAL;
	ACTP_CHECK();
	std::vector<uint32_t> slots(n);
	for (uint32_t i = 0; i < n; ++i) {
		auto it = c->gid_map_h.find(glob_ids[i]);
		if (it == c->gid_map_h.end()) {
			set_err("gys_set_listener_tasks: unknown glob_id %016llx (entry %u); nothing was changed", (unsigned long long)glob_ids[i], i);
			return GYS_ERR_INVAL;
		}
		slots[i] = it->second;
	}
	c->svc_task_h.resize(c->nsvc, 0ull);
	for (uint32_t i = 0; i < n; ++i) c->svc_task_h[slots[i]] = aggr_task_ids[i];
	c->task_gen++;
	return GYS_OK;
} GYS_CATCH_ALL

int gys_svc_edges_dev(gys_ctx *c, const gys_svc_edge_sel *sel, gys_svc_edge *d_out, uint32_t cap, uint32_t *nmatch)
try {
	GYS_ENTER(c);
	if (nmatch) *nmatch = 0;
	if (!c || !nmatch || (cap && !d_out)) return GYS_ERR_INVAL;
	ACTP_CHECK();
	int rc = dep_ensure_tasks(c);
	if (rc) return rc;
	DepEdgeP p{};
	dep_edge_params(c, p);
	if ((rc = dep_sel(c, sel, p)) != GYS_OK) return rc;
	uint64_t ne = 0;
	if ((rc = dep_edges_run<true>(c, p, d_out, cap, &ne)) != GYS_OK) return rc;
	*nmatch = (uint32_t)ne;
	return GYS_OK;
} GYS_CATCH_ALL

int gys_svc_edges(gys_ctx *c, const gys_svc_edge_sel *sel, gys_svc_edge *out, uint32_t cap, uint32_t *nout, uint32_t *nmatch)
try {
	GYS_ENTER(c);
	if (nout) *nout = 0;
	if (nmatch) *nmatch = 0;
	if (!c || !nout || !nmatch || (cap && !out)) return GYS_ERR_INVAL;
	ACTP_CHECK();
	int rc = dep_ensure_tasks(c);
	if (rc) return rc;
	DepEdgeP p{};
	dep_edge_params(c, p);
	if ((rc = dep_sel(c, sel, p)) != GYS_OK) return rc;
	uint64_t ne = 0, ne2 = 0;
	if ((rc = dep_edges_run<true>(c, p, nullptr, 0u, &ne)) != GYS_OK) return rc;
	*nmatch = (uint32_t)ne;
	if (ne > cap) {
		set_err("%u edges match, room for %u", *nmatch, cap);
		return GYS_ERR_NOMEM;
	}
	if (!ne) return GYS_OK;
	if ((rc = c->dep_rows.grow(ne, c->stream)) != GYS_OK) return rc;
	if ((rc = dep_edges_run<true>(c, p, c->dep_rows.p, (uint32_t)ne, &ne2)) != GYS_OK) return rc;
	if (ne2 != ne) {
		set_err("the edge count moved between the passes (%llu, %llu)", (unsigned long long)ne, (unsigned long long)ne2);
		return GYS_ERR_INTERNAL;
	}
	std::vector<gys_svc_edge> rows(ne);
	HIPCHK(hipMemcpyAsync(rows.data(), c->dep_rows.p, ne * sizeof(gys_svc_edge), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	std::sort(rows.begin(), rows.end(), [](const gys_svc_edge &a, const gys_svc_edge &b) {
		if (a.src_slot != b.src_slot) return a.src_slot < b.src_slot;
		if (a.dst_slot != b.dst_slot) return a.dst_slot < b.dst_slot;
		return a.kind < b.kind;
	});
	memcpy(out, rows.data(), ne * sizeof(gys_svc_edge));
	*nout = (uint32_t)ne;
	return GYS_OK;
} GYS_CATCH_ALL

int gys_svcgraph_stats(gys_ctx *c, gys_svcgraph_stats_t *out)
try {
	GYS_ENTER(c);
	if (!c || !out) return GYS_ERR_INVAL;
	ACTP_CHECK();
	int rc = dep_ensure_tasks(c);
	if (rc) return rc;
	DepEdgeP p{};
	dep_edge_params(c, p);
	(void)dep_sel(c, nullptr, p);
	uint64_t ne = 0;
	unsigned long long ctr[DPC_NUM];
	if ((rc = dep_edges_run<false>(c, p, nullptr, 0u, &ne, ctr)) != GYS_OK) return rc;
	out->live_rows = ctr[DPC_LIVE];
	out->rows_no_listener = ctr[DPC_NOLISTENER];
	out->rows_no_client = ctr[DPC_NOCLIENT];
	out->edges = ne;
	out->bound_services = c->dep_tasks.nbound();
	out->bound_tasks = c->dep_tasks.ntasks();
	return GYS_OK;
} GYS_CATCH_ALL

int gys_svc_deps_dev(gys_ctx *c, const uint64_t *root_ids, uint32_t nroots, uint32_t dir, uint32_t max_hops, uint32_t *d_hops, uint32_t *nreached)
try {
	GYS_ENTER(c);
	if (nreached) *nreached = 0;
	if (!c || dir < 1u || dir > 3u || !d_hops || !nreached || (!root_ids && nroots)) return GYS_ERR_INVAL;
	ACTP_CHECK();
	const int rc = dep_traverse(c, root_ids, nroots, dir, max_hops, d_hops, nreached);
	if (rc) return rc;
	return dep_collect(c, d_hops, c->nsvc, nullptr, 0u, nreached);
} GYS_CATCH_ALL

int gys_svc_deps(gys_ctx *c, const uint64_t *root_ids, uint32_t nroots, uint32_t dir, uint32_t max_hops, uint64_t *glob_ids, uint32_t *hops, uint32_t cap,
		 uint32_t *nout, uint32_t *nreached)
try {
	GYS_ENTER(c);
	if (nout) *nout = 0;
	if (nreached) *nreached = 0;
	if (!c || dir < 1u || dir > 3u || !nout || !nreached || (!root_ids && nroots) || (cap && (!glob_ids || !hops))) return GYS_ERR_INVAL;
	ACTP_CHECK();
	if (!c->nsvc) return GYS_OK;
	int rc = c->dep_hops.grow(c->nsvc, c->stream);
	if (rc) return rc;
	if ((rc = dep_traverse(c, root_ids, nroots, dir, max_hops, c->dep_hops.p, nreached)) != GYS_OK) return rc;
	const uint32_t dcap = std::min(cap, c->nsvc);
	if ((rc = c->dep_hits.grow(std::max(dcap, 1u), c->stream)) != GYS_OK) return rc;
	if ((rc = dep_collect(c, c->dep_hops.p, c->nsvc, c->dep_hits.p, dcap, nreached)) != GYS_OK) return rc;
	if (*nreached > cap) {
		set_err("%u services reached, room for %u", *nreached, cap);
		return GYS_ERR_NOMEM;
	}
	std::vector<uint2> hits(*nreached);
	if (*nreached) {
		HIPCHK(hipMemcpyAsync(hits.data(), c->dep_hits.p, (uint64_t)*nreached * sizeof(uint2), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream));
	}
	std::sort(hits.begin(), hits.end(), [](const uint2 &a, const uint2 &b) { return a.y != b.y ? a.y < b.y : a.x < b.x; });
	for (uint32_t i = 0; i < *nreached; ++i) {
		glob_ids[i] = c->svc_gid_h[hits[i].x];
		hops[i] = hits[i].y;
	}
	*nout = *nreached;
	return GYS_OK;
} GYS_CATCH_ALL

} // extern "C"
