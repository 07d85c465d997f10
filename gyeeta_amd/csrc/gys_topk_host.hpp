// gys_topk_host.hpp -- host side of the rankings on sketch results (kernels: gys_topk.hpp, k_td_slab_quantiles in gys_tdrank.hpp).  Included once
// by gys_engine.hip behind gys_svcquery_host.hpp (the q_misc layout, the selection rounds) and gys_rollsel_host.hpp (rollsel_select).
#pragma once

namespace {

// q_misc words behind the svcstate scan's (QM_*): the tie list's cursor and the tie rounds' prefix (u64, 8-byte aligned)
constexpr uint32_t TKM_NTIE = QM_WORDS, TKM_TPREFIX = QM_WORDS + 2, TKM_WORDS = QM_WORDS + 4;
static_assert(TKM_TPREFIX % 2 == 0, "the tie prefix is a 64-bit word");
static_assert(sizeof(gys_topk_entry) == 24 && sizeof(TopkEntry) == 24 && sizeof(gys_top_service) == 32, "entry layouts");

// `rounds` rounds of k_svc_hist / k_svc_pick on sp's keys
void topk_rounds(gys_ctx *c, SvcSelectP sp, uint32_t nkeys_max, const uint32_t *shifts, const uint32_t *widths, uint32_t rounds)
{
	const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)nkeys_max + 256u * 16u - 1) / (256u * 16u), (uint64_t)c->ncu * 4);
	for (uint32_t r = 0; r < rounds; ++r) {
		sp.shift = shifts[r];
		sp.bits = widths[r];
		hipLaunchKernelGGL(k_svc_hist, dim3(std::max(1u, grid)), dim3(256), 0, c->stream, sp);
		hipLaunchKernelGGL(k_svc_pick, dim3(1), dim3(256), 0, c->stream, sp);
	}
}

// workgroups of k_topk_keys for nrows rows: a tile of 1024 rows each, grid-stride beyond four workgroups per CU
uint32_t topk_keys_grid(const gys_ctx *c, uint32_t nrows)
{
	const uint32_t tile = GYS_SVCQ_THREADS * GYS_SVCQ_PER_THREAD;
	return std::max(1u, (uint32_t)std::min<uint64_t>(((uint64_t)nrows + tile - 1) / tile, (uint64_t)c->ncu * 4));
}

// the top-k of a device column ("Top-k" in gysketch.h): the entries in their order in `out`, the number of eligible rows in *neligible
int topk_run(gys_ctx *c, const double *d_col, uint32_t stride, uint32_t nrows, const uint32_t *d_rows, const uint64_t *d_weight, uint64_t min_weight, int order, uint32_t k,
	     std::vector<gys_topk_entry> &out, uint64_t *neligible)
{
	out.clear();
	*neligible = 0;
	if (!nrows) return GYS_OK;
	int rc;
	if ((rc = c->q_cand_key.grow(nrows, c->stream)) != GYS_OK) return rc;
	if ((rc = c->q_cand_slot.grow(nrows, c->stream)) != GYS_OK) return rc;
	if ((rc = c->q_misc.grow(TKM_WORDS, c->stream)) != GYS_OK) return rc;
	HIPCHK(hipMemsetAsync(c->q_misc.p, 0, TKM_WORDS * 4, c->stream));
	uint32_t ncand = 0;
	{
		ProfScope ps(c, "topk_keys");
		TopkKeysP p{};
		p.col = (const unsigned long long *)d_col;
		p.stride = stride;
		p.nrows = nrows;
		p.rows = d_rows;
		p.weight = (const unsigned long long *)d_weight;
		p.min_weight = min_weight;
		p.smallest = order == GYS_TOPK_SMALLEST ? 1u : 0u;
		p.cand_key = c->q_cand_key.p;
		p.cand_row = c->q_cand_slot.p;
		p.cursor = c->q_misc.p + QM_CURSOR;
		hipLaunchKernelGGL(k_topk_keys, dim3(topk_keys_grid(c, nrows)), dim3(GYS_SVCQ_THREADS), 0, c->stream, p);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipMemcpyAsync(&ncand, c->q_misc.p + QM_CURSOR, 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	*neligible = ncand;
	const uint32_t ntake = std::min(ncand, k);
	if (!ntake) return GYS_OK;
	const bool select = ncand > k;
	if ((rc = c->q_out_rows.grow((uint64_t)ntake * sizeof(TopkEntry), c->stream)) != GYS_OK) return rc;
	if (select) {
		if ((rc = c->q_tie_key.grow(ncand, c->stream)) != GYS_OK) return rc;
		ProfScope ps(c, "topk_rounds");
		// the k-th largest key T, 11 bits per round; `want` of the rows with key T are still to be taken ...
		SvcSelectP sp{};
		sp.cand_key = c->q_cand_key.p;
		sp.ncand = c->q_misc.p + QM_CURSOR;
		sp.hist = c->q_misc.p + QM_HIST;
		sp.prefix = (unsigned long long *)(c->q_misc.p + QM_PREFIX);
		sp.want = c->q_misc.p + QM_WANT;
		HIPCHK(hipMemcpyAsync(c->q_misc.p + QM_WANT, &k, 4, hipMemcpyHostToDevice, c->stream)); // (k is the caller's frame: synchronised below)
		static const uint32_t shifts[GYS_SVCQ_ROUNDS] = {53, 42, 31, 20, 9, 0}, widths[GYS_SVCQ_ROUNDS] = {11, 11, 11, 11, 11, 9};
		topk_rounds(c, sp, ncand, shifts, widths, GYS_SVCQ_ROUNDS);
		// ... the ones with the lowest row numbers: the `want` largest of 0xFFFFFFFF - row among them, three rounds over 32 bits
		TopkTiesP tp{};
		tp.cand_key = c->q_cand_key.p;
		tp.cand_row = c->q_cand_slot.p;
		tp.ncand = c->q_misc.p + QM_CURSOR;
		tp.threshold = sp.prefix;
		tp.tie_key = c->q_tie_key.p;
		tp.ntie = c->q_misc.p + TKM_NTIE;
		const uint32_t tgrid = (uint32_t)std::min<uint64_t>(((uint64_t)ncand + 255u) / 256u, (uint64_t)c->ncu * 8);
		hipLaunchKernelGGL(k_topk_ties, dim3(std::max(1u, tgrid)), dim3(256), 0, c->stream, tp);
		sp.cand_key = c->q_tie_key.p;
		sp.ncand = c->q_misc.p + TKM_NTIE;
		sp.prefix = (unsigned long long *)(c->q_misc.p + TKM_TPREFIX);
		static const uint32_t tshifts[3] = {21, 10, 0}, twidths[3] = {11, 11, 10};
		topk_rounds(c, sp, ncand, tshifts, twidths, 3u);
		HIPCHK(hipGetLastError());
	}
	uint32_t nout = 0;
	{
		ProfScope ps(c, "topk_gather");
		TopkGatherP gp{};
		gp.col = (const unsigned long long *)d_col;
		gp.stride = stride;
		gp.weight = (const unsigned long long *)d_weight;
		gp.cand_key = c->q_cand_key.p;
		gp.cand_row = c->q_cand_slot.p;
		gp.ncand = c->q_misc.p + QM_CURSOR;
		gp.threshold = select ? (const unsigned long long *)(c->q_misc.p + QM_PREFIX) : nullptr;
		gp.tie_threshold = (const unsigned long long *)(c->q_misc.p + TKM_TPREFIX);
		gp.maxout = ntake;
		gp.out_count = c->q_misc.p + QM_OUT;
		gp.out = (TopkEntry *)c->q_out_rows.p;
		const uint32_t ggrid = (uint32_t)std::min<uint64_t>(((uint64_t)ncand + 255u) / 256u, (uint64_t)c->ncu * 8);
		hipLaunchKernelGGL(k_topk_gather, dim3(std::max(1u, ggrid)), dim3(256), 0, c->stream, gp);
		HIPCHK(hipGetLastError());
	}
	ProfScope ps(c, "topk_read");
	HIPCHK(hipMemcpyAsync(&nout, c->q_misc.p + QM_OUT, 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (nout != ntake) {
		set_err("top-k: selected %u rows, expected %u", nout, ntake);
		return GYS_ERR_INTERNAL;
	}
	std::vector<gys_topk_entry> raw(nout);
	HIPCHK(hipMemcpyAsync(raw.data(), c->q_out_rows.p, (uint64_t)nout * sizeof(gys_topk_entry), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	// the definition's total order: larger key first, then the lower row
	const uint32_t smallest = order == GYS_TOPK_SMALLEST ? 1u : 0u;
	std::vector<std::pair<unsigned long long, uint32_t>> ord(nout); // {key, index}
	for (uint32_t i = 0; i < nout; ++i) {
		unsigned long long bits;
		memcpy(&bits, &raw[i].value, 8);
		ord[i] = {topk_key(bits, smallest), i};
	}
	std::sort(ord.begin(), ord.end(), [&](const std::pair<unsigned long long, uint32_t> &a, const std::pair<unsigned long long, uint32_t> &b) {
		return a.first != b.first ? a.first > b.first : raw[a.second].row < raw[b.second].row;
	});
	out.resize(nout);
	for (uint32_t i = 0; i < nout; ++i) out[i] = raw[ord[i].second];
	return GYS_OK;
}

} // namespace

extern "C" {

int gys_tdigest_slab_quantiles_dev(gys_ctx *c, const gys_tdigest_slab *d_slabs, uint32_t nslabs, const double *q, uint32_t nq, double *d_out)
try {
	GYS_ENTER(c);
	if (!c || !d_slabs || !q || !d_out) return GYS_ERR_INVAL;
	if (nq == 0 || nq > GYS_TR_MAXT) {
		set_err("gys_tdigest_slab_quantiles_dev: 1 .. %u quantiles per call", (unsigned)GYS_TR_MAXT);
		return GYS_ERR_INVAL;
	}
	if (!nslabs) return GYS_OK;
	TdSlabQP p{};
	p.in = d_slabs;
	p.n = nslabs;
	p.nq = nq;
	for (uint32_t i = 0; i < nq; ++i) p.q[i] = q[i];
	p.out = d_out;
	ProfScope ps(c, "slab_quantiles");
	hipLaunchKernelGGL(k_td_slab_quantiles, dim3(std::max(1u, std::min<uint32_t>((nslabs + 3u) / 4u, (uint32_t)c->ncu * 16u))), dim3(GYS_TR_NT), 0, c->stream, p);
	HIPCHK(hipGetLastError());
	return GYS_OK;
} GYS_CATCH_ALL

int gys_topk_dev(gys_ctx *c, const double *d_col, uint32_t stride, uint32_t nrows, const uint32_t *d_rows, const uint64_t *d_weight, uint64_t min_weight, int order,
		 uint32_t k, gys_topk_entry *out, uint32_t *nout, uint64_t *neligible)
try {
	GYS_ENTER(c);
	if (nout) *nout = 0;
	if (neligible) *neligible = 0;
	if (!c || !d_col || !stride || !nout || (order != GYS_TOPK_LARGEST && order != GYS_TOPK_SMALLEST) || (k && !out)) {
		set_err("gys_topk_dev: null column / nout, stride 0, unknown order, or k > 0 without out");
		return GYS_ERR_INVAL;
	}
	std::vector<gys_topk_entry> got;
	uint64_t nel = 0;
	const int rc = topk_run(c, d_col, stride, nrows, d_rows, d_weight, min_weight, order, k, got, &nel);
	if (rc) return rc;
	if (!got.empty()) memcpy(out, got.data(), got.size() * sizeof(gys_topk_entry));
	*nout = (uint32_t)got.size();
	if (neligible) *neligible = nel;
	return GYS_OK;
} GYS_CATCH_ALL

int gys_top_services(gys_ctx *c, int metric, double param, int level, uint64_t tusec, const gys_svc_filter *f, uint32_t flags, uint64_t min_total, int order, uint32_t k,
		     gys_top_service *out, uint32_t *nout, uint64_t *neligible)
try {
	GYS_ENTER(c);
	if (nout) *nout = 0;
	if (neligible) *neligible = 0;
	const bool distinct = metric == GYS_TOP_DISTINCT;
	if (!c || !nout || metric < GYS_TOP_QUANTILE || metric > GYS_TOP_DISTINCT || (order != GYS_TOPK_LARGEST && order != GYS_TOPK_SMALLEST) || (flags & ~GYS_RF_ANY_STATE) ||
	    (k && !out) || (distinct && (level < -1 || level >= GYS_NLEVELS))) {
		set_err("gys_top_services: null nout, unknown metric, order, level or flags, or k > 0 without out");
		return GYS_ERR_INVAL;
	}
	if (distinct) {
		HLL_CHECK();
		if (level >= 0 && !c->hl_lvl) {
			set_err("distinct-count levels are off (gys_config.svc_hll_levels = 0)");
			return GYS_ERR_STATE;
		}
	} else {
		TDIGEST_CHECK();
	}
	// the candidates: the filter's members (those of gys_rollup_filtered_dev with GYS_GROUP_NONE), or every slot -- a free one is never eligible
	const uint32_t *d_rows = nullptr;
	uint32_t nrows = c->nsvc;
	if (f) {
		gys_rollup_row row{};
		uint32_t ngroups = 0, nr = 0, nchunks = 0;
		const int rc = rollsel_select(c, f, flags, GYS_GROUP_NONE, &row, 1u, &ngroups, &nr, &nchunks);
		if (rc) return rc;
		d_rows = c->rs_members.p;
		nrows = nr ? row.nmembers : 0u;
	}
	if (!nrows) return GYS_OK;
	const uint32_t nsvc = c->nsvc;
	int rc;
	if ((rc = c->top_col.grow(nsvc, c->stream)) != GYS_OK || (rc = c->top_weight.grow(nsvc, c->stream)) != GYS_OK) return rc;
	if (metric != GYS_TOP_DISTINCT && (rc = c->top_below.grow(nsvc, c->stream)) != GYS_OK) return rc;
	// the metric column: the scans themselves
	const int64_t x = metric == GYS_TOP_QUANTILE ? 0 : (int64_t)param;
	if (metric == GYS_TOP_QUANTILE) rc = gys_scan_quantiles_dev(c, &param, 1u, c->top_col.p);
	else if (distinct) rc = level < 0 ? gys_scan_distinct_dev(c, c->top_col.p) : gys_scan_distinct_level_dev(c, level, tusec, c->top_col.p);
	if (rc) return rc;
	if (!distinct && (rc = td_ranks_launch(c, nullptr, 0u, nsvc, &x, 1u, c->top_below.p, (uint64_t *)c->top_weight.p)) != GYS_OK) return rc; // (the totals; below(x))
	if (metric != GYS_TOP_QUANTILE) {
		TopMetricP mp{};
		mp.metric = metric;
		mp.nsvc = nsvc;
		mp.below = c->top_below.p;
		mp.svc_host = c->svc_host;
		mp.col = c->top_col.p;
		mp.weight = c->top_weight.p;
		ProfScope ps(c, "top_metric");
		hipLaunchKernelGGL(k_top_metric, dim3(std::max(1u, std::min<uint32_t>((nsvc + 255u) / 256u, (uint32_t)c->ncu * 8u))), dim3(256), 0, c->stream, mp);
		HIPCHK(hipGetLastError());
	}
	std::vector<gys_topk_entry> got;
	uint64_t nel = 0;
	rc = topk_run(c, c->top_col.p, 1u, nrows, d_rows, (const uint64_t *)c->top_weight.p, distinct ? 1ull : std::max<uint64_t>(min_total, 1ull), order, k, got, &nel);
	if (rc) return rc;
	for (size_t i = 0; i < got.size(); ++i) {
		gys_top_service &o = out[i];
		o.slot = got[i].row;
		o.glob_id = c->svc_gid_h[o.slot];
		o.host_slot = c->svc_host_h[o.slot];
		o.value = got[i].value;
		o.total = distinct ? 0ull : got[i].weight;
	}
	*nout = (uint32_t)got.size();
	if (neligible) *neligible = nel;
	return GYS_OK;
} GYS_CATCH_ALL

} // extern "C"
