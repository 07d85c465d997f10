// gys_svccomp_engine.hpp -- engine side of the service components (kernels: gys_svccomp.hpp; definition: "Service components" in
// include/gysketch.h).  Included once by gys_engine.hip behind gys_svcdeps_engine.hpp (dep_ensure_tasks, dep_edge_params, dep_edges_run).
//
// A call builds the pair array as the traversal does (count, grow, write: two walks of the table, a read of the count behind each), then
// runs a FIXED list of launches -- init, hook, flatten; sizes and roots where figures are asked for; the third walk of the table for the
// sums -- and reads the counter words once behind them.  Nothing loops on a device result: the launches and reads of a call do not
// depend on the graph.
#pragma once

namespace {

uint32_t cc_slot_grid(const gys_ctx *c) { return std::max(1u, (uint32_t)std::min<uint64_t>(((uint64_t)c->nsvc + 255u) / 256u, (uint64_t)c->ncu * 8)); }

// comp[] of every slot below nsvc into d_comp (nsvc > 0); the counter words are cleared first and are NOT read here
int cc_partition(gys_ctx *c, uint32_t *d_comp)
{
	int rc = dep_ensure_tasks(c);
	if (rc) return rc;
	if (!c->cc_ctr.p && (rc = c->cc_ctr.alloc(CCC_NUM)) != GYS_OK) return rc;
	if ((rc = c->cc_parent.grow(c->nsvc, c->stream)) != GYS_OK) return rc;
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
	}
	HIPCHK(hipMemsetAsync(c->cc_ctr.p, 0, CCC_NUM * sizeof(unsigned long long), c->stream));
	const uint32_t sgrid = cc_slot_grid(c);
	{
		ProfScope ps(c, "cc_hook"); // (with the init in front of it)
		hipLaunchKernelGGL(k_cc_init, dim3(sgrid), dim3(256), 0, c->stream, c->cc_parent.p, (const uint32_t *)c->svc_host, c->nsvc);
		if (ne) {
			const uint32_t egrid = std::max(1u, (uint32_t)std::min<uint64_t>((ne + 255u) / 256u, (uint64_t)c->ncu * 8));
			hipLaunchKernelGGL(k_cc_hook, dim3(egrid), dim3(256), 0, c->stream, (const uint2 *)c->dep_pairs.p, ne, c->cc_parent.p, c->nsvc, c->cc_ctr.p + CCC_CAPPED);
		}
		HIPCHK(hipGetLastError());
	}
	{
		ProfScope ps(c, "cc_flatten");
		hipLaunchKernelGGL(k_cc_flatten, dim3(sgrid), dim3(256), 0, c->stream, c->cc_parent.p, d_comp, c->nsvc, c->cc_ctr.p + CCC_CAPPED);
		HIPCHK(hipGetLastError());
	}
	return GYS_OK;
}

// the sizes of the components of d_comp into c->cc_size; the counts into the counter words; with `list` the components with
// >= min_services members into c->cc_list / c->cc_index
int cc_figures(gys_ctx *c, const uint32_t *d_comp, uint32_t min_services, bool list)
{
	int rc;
	if ((rc = c->cc_size.grow(c->nsvc, c->stream)) != GYS_OK) return rc;
	if (list && ((rc = c->cc_list.grow(c->nsvc, c->stream)) != GYS_OK || (rc = c->cc_index.grow(c->nsvc, c->stream)) != GYS_OK)) return rc;
	ProfScope ps(c, "cc_figures");
	HIPCHK(hipMemsetAsync(c->cc_size.p, 0, (size_t)c->nsvc * 4, c->stream));
	const uint32_t sgrid = cc_slot_grid(c);
	hipLaunchKernelGGL(k_cc_sizes, dim3(sgrid), dim3(256), 0, c->stream, d_comp, c->cc_size.p, c->nsvc);
	CcRootsP rp{};
	rp.comp = d_comp;
	rp.size = c->cc_size.p;
	rp.nsvc = c->nsvc;
	rp.min_services = min_services;
	rp.list = list ? c->cc_list.p : nullptr;
	rp.index = list ? c->cc_index.p : nullptr;
	rp.ctr = c->cc_ctr.p;
	hipLaunchKernelGGL(k_cc_roots, dim3(sgrid), dim3(256), 0, c->stream, rp);
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

// the one read of the counter words; a loop that reached its cap is an error of the library, not of the caller
int cc_read_ctr(gys_ctx *c, unsigned long long ctr[CCC_NUM])
{
	HIPCHK(hipMemcpyAsync(ctr, c->cc_ctr.p, CCC_NUM * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (ctr[CCC_CAPPED]) {
		set_err("service components: %llu union-find walks reached their step limit (%u slots); the partition is not valid", ctr[CCC_CAPPED], c->nsvc);
		return GYS_ERR_INTERNAL;
	}
	return GYS_OK;
}

static_assert(sizeof(gys_svc_component) == 64, "component layout");

} // namespace

extern "C" {

int gys_svc_components_dev(gys_ctx *c, uint32_t *d_comp, uint32_t *ncomp, uint32_t *nlinked)
try {
	GYS_ENTER(c);
	if (ncomp) *ncomp = 0;
	if (nlinked) *nlinked = 0;
	if (!c || !d_comp) return GYS_ERR_INVAL;
	ACTP_CHECK();
	if (!c->nsvc) return GYS_OK;
	int rc = cc_partition(c, d_comp);
	if (rc) return rc;
	if ((ncomp || nlinked) && (rc = cc_figures(c, d_comp, 0u, false)) != GYS_OK) return rc;
	unsigned long long ctr[CCC_NUM];
	if ((rc = cc_read_ctr(c, ctr)) != GYS_OK) return rc;
	if (ncomp) *ncomp = (uint32_t)ctr[CCC_NCOMP];
	if (nlinked) *nlinked = (uint32_t)ctr[CCC_NLINKED];
	return GYS_OK;
} GYS_CATCH_ALL

int gys_svc_components(gys_ctx *c, uint32_t min_services, gys_svc_component *out, uint32_t cap, uint32_t *nout, uint32_t *nmatch, uint32_t *ncomp)
try {
	GYS_ENTER(c);
	if (nout) *nout = 0;
	if (nmatch) *nmatch = 0;
	if (ncomp) *ncomp = 0;
	if (!c || !nout || !nmatch || (cap && !out)) return GYS_ERR_INVAL;
	ACTP_CHECK();
	if (!c->nsvc) return GYS_OK;
	int rc = c->cc_comp.grow(c->nsvc, c->stream);
	if (rc) return rc;
	if ((rc = cc_partition(c, c->cc_comp.p)) != GYS_OK) return rc;
	if ((rc = cc_figures(c, c->cc_comp.p, min_services, true)) != GYS_OK) return rc;
	unsigned long long ctr[CCC_NUM];
	if ((rc = cc_read_ctr(c, ctr)) != GYS_OK) return rc;
	const uint32_t nm = (uint32_t)ctr[CCC_NMATCH];
	*nmatch = nm;
	if (ncomp) *ncomp = (uint32_t)ctr[CCC_NCOMP];
	if (ctr[CCC_CURSOR] != ctr[CCC_NMATCH] || nm > c->nsvc) {
		set_err("service components: %llu components listed, %llu counted", ctr[CCC_CURSOR], ctr[CCC_NMATCH]);
		return GYS_ERR_INTERNAL;
	}
	if (nm > cap) {
		set_err("%u components match, room for %u", nm, cap);
		return GYS_ERR_NOMEM;
	}
	if (!nm) return GYS_OK;
	// the sums of the listed components: the third walk of the table
	if ((rc = c->cc_acc.grow((uint64_t)nm * GYS_CC_ACC, c->stream)) != GYS_OK) return rc;
	HIPCHK(hipMemsetAsync(c->cc_acc.p, 0, (size_t)nm * GYS_CC_ACC * sizeof(unsigned long long), c->stream));
	{
		ProfScope ps(c, "cc_rows");
		DepEdgeP p{};
		dep_edge_params(c, p);
		(void)dep_sel(c, nullptr, p);
		hipLaunchKernelGGL(k_cc_rows, dim3(actp_scan_grid(c)), dim3(256), 0, c->stream, p, (const uint32_t *)c->cc_comp.p, (const uint32_t *)c->cc_index.p, nm, c->cc_acc.p);
		HIPCHK(hipGetLastError());
	}
	std::vector<uint2> list(nm);
	std::vector<unsigned long long> acc((size_t)nm * GYS_CC_ACC);
	HIPCHK(hipMemcpyAsync(list.data(), c->cc_list.p, (size_t)nm * sizeof(uint2), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(acc.data(), c->cc_acc.p, acc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	std::vector<gys_svc_component> rows(nm);
	for (uint32_t i = 0; i < nm; ++i) { // (acc is indexed by the place in the list)
		gys_svc_component &r = rows[i];
		const unsigned long long *a = &acc[(size_t)i * GYS_CC_ACC];
		r.root_slot = list[i].x;
		r.nservices = list[i].y;
		r.root_glob_id = c->svc_gid_h[list[i].x];
		r.nrows = a[0];
		r.nedges = a[1];
		r.active_conns = a[2];
		r.bytes_sent = a[3];
		r.bytes_received = a[4];
		r.reserved = 0;
	}
	std::sort(rows.begin(), rows.end(), [](const gys_svc_component &a, const gys_svc_component &b) {
		return a.nservices != b.nservices ? a.nservices > b.nservices : a.root_slot < b.root_slot;
	});
	memcpy(out, rows.data(), (size_t)nm * sizeof(gys_svc_component));
	*nout = nm;
	return GYS_OK;
} GYS_CATCH_ALL

int gys_label_service_components(gys_ctx *c, uint32_t min_services, uint32_t *ngroups)
try {
	GYS_ENTER(c);
	if (ngroups) *ngroups = 0;
	if (!c) return GYS_ERR_INVAL;
	ACTP_CHECK();
	int rc;
	if (!c->svc_label.p) { // (as gys_set_service_groups when no label was ever set)
		if ((rc = c->svc_label.alloc(c->cfg.max_services, false)) != GYS_OK) return rc;
		if (hipMemsetAsync(c->svc_label, 0xFF, c->svc_label.cap * 4, c->stream) != hipSuccess) {
			c->svc_label.release();
			set_err("gys_label_service_components: could not clear the label array");
			return GYS_ERR_HIP;
		}
	}
	if (!c->nsvc) return GYS_OK;
	if ((rc = c->cc_comp.grow(c->nsvc, c->stream)) != GYS_OK) return rc;
	if ((rc = cc_partition(c, c->cc_comp.p)) != GYS_OK) return rc;
	if ((rc = cc_figures(c, c->cc_comp.p, min_services, false)) != GYS_OK) return rc;
	unsigned long long ctr[CCC_NUM];
	if ((rc = cc_read_ctr(c, ctr)) != GYS_OK) return rc; // (before the labels: a partition that is not valid labels nothing)
	hipLaunchKernelGGL(k_cc_labels, dim3(cc_slot_grid(c)), dim3(256), 0, c->stream, (const uint32_t *)c->cc_comp.p, (const uint32_t *)c->cc_size.p, c->nsvc, min_services,
			   c->svc_label.p);
	HIPCHK(hipGetLastError());
	c->label_domain = std::max(c->label_domain, c->nsvc); // (the roll-ups follow in stream order; a root slot is below nsvc <= max_services)
	if (ngroups) *ngroups = (uint32_t)ctr[CCC_NMATCH];
	return GYS_OK;
} GYS_CATCH_ALL

} // extern "C"
