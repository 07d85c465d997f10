// gys_svcresol_engine.hpp -- engine side of the issue resolution (kernels: gys_svcresol.hpp; definition: "Issue resolution" in
// include/gysketch.h).  Included once by gys_engine.hip behind gys_groupflow_engine.hpp (dep_ensure_tasks, dep_edge_params,
// dep_edges_run, cc_slot_grid).
//
// A call builds the pair array as the traversal does (count, grow, write: two walks of the table, a read of the count behind each), then
// runs a FIXED list of launches -- seed, a level pass over the pairs and a settle pass over the slots per tier, finish -- and reads the
// counter words once behind them.  Nothing loops on a device result.  The host form compacts the rows it has counted with one more
// launch and copies them.  Every buffer is scratch of the context that only grows (nothing is allocated before the first call).
#pragma once

namespace {

int ri_check(const void *d_out, uint32_t max_tiers)
{
	if (max_tiers > GYS_RESOL_MAX_TIERS) {
		set_err("issue resolution: max_tiers %u (0 = %u, or 1 .. %u)", max_tiers, GYS_RESOL_MAX_TIERS, GYS_RESOL_MAX_TIERS);
		return GYS_ERR_INVAL;
	}
	if ((uintptr_t)d_out & 15u) {
		set_err("issue resolution: the record array is not 16-byte aligned");
		return GYS_ERR_INVAL;
	}
	return GYS_OK;
}

// RECORD of every slot below nsvc (> 0) into d_out, the impact column into d_impact (may be nullptr); the counter words and the edge
// count into ctr / *nedges: the one read
int ri_resolve(gys_ctx *c, const gys_listener_decision *d_dec, uint32_t max_tiers, gys_svc_resol *d_out, double *d_impact, unsigned long long ctr[RSC_NUM], uint64_t *nedges)
{
	int rc = dep_ensure_tasks(c);
	if (rc) return rc;
	if (!c->ri_ctr.p && (rc = c->ri_ctr.alloc(RSC_NUM)) != GYS_OK) return rc;
	if ((rc = c->ri_word.grow(c->nsvc, c->stream)) != GYS_OK || (rc = c->ri_best.grow(c->nsvc, c->stream)) != GYS_OK || (rc = c->ri_nres.grow(c->nsvc, c->stream)) != GYS_OK) return rc;
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
	*nedges = ne;
	HIPCHK(hipMemsetAsync(c->ri_ctr.p, 0, RSC_NUM * sizeof(unsigned long long), c->stream));
	const uint32_t sgrid = cc_slot_grid(c);
	{
		ProfScope ps(c, "resol_seed");
		ResolSeedP sp{};
		sp.svc_state = c->svc_state;
		sp.svc_host = c->svc_host;
		sp.svc_gid = c->svc_gid;
		sp.dec = d_dec;
		sp.nsvc = c->nsvc;
		sp.epoch = c->epoch;
		sp.word = c->ri_word.p;
		sp.best = c->ri_best.p;
		sp.nres = c->ri_nres.p;
		hipLaunchKernelGGL(k_resol_seed, dim3(sgrid), dim3(256), 0, c->stream, sp);
		HIPCHK(hipGetLastError());
	}
	if (ne) { // (without an edge nothing is attributed: the seed's words stand)
		const uint32_t tiers = max_tiers ? max_tiers : GYS_RESOL_MAX_TIERS;
		const uint32_t egrid = std::max(1u, (uint32_t)std::min<uint64_t>((ne + 255u) / 256u, (uint64_t)c->ncu * 8));
		for (uint32_t level = 0; level < tiers; ++level) {
			{
				ProfScope ps(c, "resol_level");
				hipLaunchKernelGGL(k_resol_level, dim3(egrid), dim3(256), 0, c->stream, (const uint2 *)c->dep_pairs.p, ne, (const uint32_t *)c->ri_word.p, c->ri_best.p, c->nsvc, level);
			}
			{
				ProfScope ps(c, "resol_settle");
				hipLaunchKernelGGL(k_resol_settle, dim3(sgrid), dim3(256), 0, c->stream, c->ri_word.p, (const unsigned long long *)c->ri_best.p, c->ri_nres.p, c->nsvc, level);
			}
		}
		HIPCHK(hipGetLastError());
	}
	{
		ProfScope ps(c, "resol_finish");
		ResolFinP fp{};
		fp.word = c->ri_word.p;
		fp.best = c->ri_best.p;
		fp.nres = c->ri_nres.p;
		fp.nsvc = c->nsvc;
		fp.out = d_out;
		fp.impact = d_impact;
		fp.ctr = c->ri_ctr.p;
		hipLaunchKernelGGL(k_resol_finish, dim3(std::min(sgrid, (uint32_t)c->ncu * 4u)), dim3(256), 0, c->stream, fp); // (fewer workgroups: fewer adds to the 13 counter words)
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipMemcpyAsync(ctr, c->ri_ctr.p, RSC_NUM * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
}

void ri_stats(const unsigned long long ctr[RSC_NUM], uint64_t nedges, gys_svc_resol_stats *st)
{
	if (!st) return;
	st->with_state = ctr[RSC_WITH_STATE];
	st->sources = ctr[RSC_SOURCES];
	st->resolved = ctr[RSC_RESOLVED];
	st->unresolved = ctr[RSC_UNRESOLVED];
	st->carriers = ctr[RSC_CARRIERS];
	st->edges = nedges;
	for (uint32_t t = 0; t < GYS_RESOL_MAX_TIERS; ++t) st->resolved_at_tier[t] = ctr[RSC_TIER0 + t];
}

static_assert(sizeof(gys_svc_resol) == 16 && sizeof(gys_svc_resol_row) == 48 && sizeof(gys_svc_resol_stats) == 112, "issue resolution layouts");

} // namespace

extern "C" {

int gys_svc_resolve_issues_dev(gys_ctx *c, const gys_listener_decision *d_dec, uint32_t max_tiers, gys_svc_resol *d_out, double *d_impact, gys_svc_resol_stats *stats)
try {
	GYS_ENTER(c);
	if (stats) memset(stats, 0, sizeof(*stats));
	if (!c || !d_out) return GYS_ERR_INVAL;
	int rc = ri_check(d_out, max_tiers);
	if (rc) return rc;
	ACTP_CHECK();
	if (!c->nsvc) return GYS_OK;
	unsigned long long ctr[RSC_NUM];
	uint64_t ne = 0;
	if ((rc = ri_resolve(c, d_dec, max_tiers, d_out, d_impact, ctr, &ne)) != GYS_OK) return rc;
	ri_stats(ctr, ne, stats);
	return GYS_OK;
} GYS_CATCH_ALL

int gys_svc_resolve_issues(gys_ctx *c, const gys_listener_decision *d_dec, uint32_t max_tiers, uint32_t role_mask, gys_svc_resol_row *out, uint32_t cap, uint32_t *nout,
			   uint32_t *nmatch, gys_svc_resol_stats *stats)
try {
	GYS_ENTER(c);
	if (nout) *nout = 0;
	if (nmatch) *nmatch = 0;
	if (stats) memset(stats, 0, sizeof(*stats));
	if (!c || !nout || !nmatch || (cap && !out)) return GYS_ERR_INVAL;
	if (role_mask & ~0x1Fu) {
		set_err("issue resolution: role_mask %#x (bits 0 .. 4)", role_mask);
		return GYS_ERR_INVAL;
	}
	int rc = ri_check(nullptr, max_tiers);
	if (rc) return rc;
	ACTP_CHECK();
	if (!c->nsvc) return GYS_OK;
	if (!role_mask) role_mask = 0x1Eu;
	if ((rc = c->ri_rec.grow(c->nsvc, c->stream)) != GYS_OK) return rc;
	unsigned long long ctr[RSC_NUM];
	uint64_t ne = 0;
	if ((rc = ri_resolve(c, d_dec, max_tiers, c->ri_rec.p, nullptr, ctr, &ne)) != GYS_OK) return rc;
	ri_stats(ctr, ne, stats);
	// the matches from the role counts: every slot below nsvc has one role
	const uint64_t per_role[5] = {c->nsvc - (ctr[RSC_SOURCES] + ctr[RSC_RESOLVED] + ctr[RSC_CARRIERS] + ctr[RSC_UNRESOLVED]), ctr[RSC_SOURCES], ctr[RSC_RESOLVED], ctr[RSC_CARRIERS],
				      ctr[RSC_UNRESOLVED]};
	uint64_t nm64 = 0;
	for (uint32_t r = 0; r < 5; ++r)
		if ((role_mask >> r) & 1u) nm64 += per_role[r];
	if (nm64 > c->nsvc) {
		set_err("issue resolution: %llu rows counted for %u slots", (unsigned long long)nm64, c->nsvc);
		return GYS_ERR_INTERNAL;
	}
	const uint32_t nm = (uint32_t)nm64;
	*nmatch = nm;
	if (nm > cap) {
		set_err("%u services match, room for %u", nm, cap);
		return GYS_ERR_NOMEM;
	}
	if (!nm) return GYS_OK;
	if ((rc = c->ri_rows.grow(nm, c->stream)) != GYS_OK) return rc;
	HIPCHK(hipMemsetAsync(c->ri_ctr.p + RSC_CURSOR, 0, sizeof(unsigned long long), c->stream));
	{
		ProfScope ps(c, "resol_rows");
		ResolRowsP rp{};
		rp.rec = c->ri_rec.p;
		rp.svc_gid = c->svc_gid;
		rp.svc_host = c->svc_host;
		rp.nsvc = c->nsvc;
		rp.role_mask = role_mask;
		rp.out = c->ri_rows.p;
		rp.cap = nm;
		rp.cursor = c->ri_ctr.p + RSC_CURSOR;
		hipLaunchKernelGGL(k_resol_rows, dim3(cc_slot_grid(c)), dim3(256), 0, c->stream, rp);
		HIPCHK(hipGetLastError());
	}
	std::vector<gys_svc_resol_row> rows(nm);
	unsigned long long listed = 0;
	HIPCHK(hipMemcpyAsync(rows.data(), c->ri_rows.p, (size_t)nm * sizeof(gys_svc_resol_row), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(&listed, c->ri_ctr.p + RSC_CURSOR, sizeof(listed), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (listed != nm) {
		set_err("issue resolution: %llu rows listed, %u counted", listed, nm);
		return GYS_ERR_INTERNAL;
	}
	std::sort(rows.begin(), rows.end(), [](const gys_svc_resol_row &a, const gys_svc_resol_row &b) { return a.slot < b.slot; });
	memcpy(out, rows.data(), (size_t)nm * sizeof(gys_svc_resol_row));
	*nout = nm;
	return GYS_OK;
} GYS_CATCH_ALL

} // extern "C"
