// TEST INFRASTRUCTURE (CPU): the LOGIC of the ranking kernels under the CPU stand-in of the device model, compared BIT FOR BIT with plain
// loops of the definitions written here:
//   * gyeeta_amd/csrc/gys_topk.hpp (k_topk_keys, k_topk_ties, k_topk_gather) with the selection rounds k_svc_hist / k_svc_pick of
//     gys_svcquery.hpp, in the sequence gys_topk_dev runs them: "Top-k" in include/gysketch.h.  Rows 1, 2, 255, 256, 257, 1 023, 1 025, 4 095,
//     4 096, 4 097; k = 0, 1, nrows - 1, nrows, nrows + 3; both orders; columns of distinct doubles, all equal, two values with the cut inside
//     the lower one's ties, values that differ in the last round's nine bits only, +-0.0 / +-inf / denormals / negatives / NaNs, the integers
//     0 .. 49; a stride of 3; a shuffled subset of rows against the same subset sorted; weights with a threshold; grids that need
//     grid-striding; lists pre-filled with garbage.
//   * k_td_slab_quantiles (gys_tdrank.hpp) against the loop of gys_tdigest_slab_quantiles: 1, 3, 4, 5 and 257 slabs, 1, 3 and 16 quantiles,
//     an empty slab, one cluster, only cluster 199, gaps, equal neighbouring means, counts above 2^32, q = -0.5, 0, 1, 1.5 and a q whose
//     target weight falls exactly on a cluster centre.
// Build + run: tests/test_kernel_logic_topk_cpu.py (plain and with -fsanitize=address; there `brief`: without the sizes 4 095 and 4 096 and the
// larger stride / subset / weight table).
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../../gyeeta_amd/csrc/gys_svcquery.hpp"
#include "../../../gyeeta_amd/csrc/gys_tdrank.hpp"
#include "../../../gyeeta_amd/csrc/gys_topk.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <limits>
#include <random>

using namespace gys;

namespace {
int fails = 0;
#define CHECK(c, ...)                                               \
	do {                                                        \
		if (!(c)) {                                         \
			if (fails++ < 20) {                         \
				printf("FAIL %s:%d: ", __FILE__, __LINE__); \
				printf(__VA_ARGS__);                \
				printf("\n");                       \
			}                                           \
		}                                                   \
	} while (0)

uint64_t bits_of(double v)
{
	uint64_t b;
	memcpy(&b, &v, 8);
	return b;
}
double from_bits(uint64_t b)
{
	double v;
	memcpy(&v, &b, 8);
	return v;
}

// ---------------------------------------------------------------------------------------------------- the definition ("Top-k")
struct Want {
	std::vector<TopkEntry> rows;
	uint64_t neligible;
};

Want topk_def(const std::vector<double> &col, uint32_t stride, std::vector<uint32_t> cand, const std::vector<uint64_t> *weight, uint64_t min_weight, int order, uint32_t k)
{
	std::vector<uint32_t> el;
	for (uint32_t r : cand) {
		const double v = col[(size_t)r * stride];
		if (v != v) continue;
		if (weight && (*weight)[r] < min_weight) continue;
		el.push_back(r);
	}
	std::sort(el.begin(), el.end(), [&](uint32_t a, uint32_t b) {
		const double x = col[(size_t)a * stride], y = col[(size_t)b * stride]; // (real-number comparison: -0.0 == +0.0)
		if (x != y) return order == TOPK_LARGEST ? x > y : x < y;
		return a < b;
	});
	Want w;
	w.neligible = el.size();
	for (size_t i = 0; i < el.size() && i < k; ++i) w.rows.push_back(TopkEntry{el[i], 0u, bits_of(col[(size_t)el[i] * stride]), weight ? (*weight)[el[i]] : 0ull});
	return w;
}

// ---------------------------------------------------------------------------------------------------- the kernels, in gys_topk_dev's sequence
struct Got {
	std::vector<TopkEntry> rows;
	uint64_t neligible;
	bool ok;
};

Got topk_dev(const std::vector<double> &col, uint32_t stride, uint32_t nrows, const std::vector<uint32_t> *rows, const std::vector<uint64_t> *weight, uint64_t min_weight,
	     int order, uint32_t k, uint32_t kgrid, uint32_t hgrid)
{
	Got g{{}, 0, true};
	// (exact sizes on the heap: AddressSanitizer sees a write past a list)
	std::vector<unsigned long long> cand_key(nrows, 0xEEEEEEEEEEEEEEEEull), tie_key;
	std::vector<uint32_t> cand_row(nrows, 0xEEEEEEEEu), hist(GYS_SVCQ_RADIX, 0);
	uint32_t cursor = 0, want = k, ntie = 0, nout = 0;
	unsigned long long prefix = 0, tprefix = 0;
	TopkKeysP p{};
	p.col = (const unsigned long long *)col.data();
	p.stride = stride;
	p.nrows = nrows;
	p.rows = rows ? rows->data() : nullptr;
	p.weight = weight ? (const unsigned long long *)weight->data() : nullptr;
	p.min_weight = min_weight;
	p.smallest = order == TOPK_SMALLEST;
	p.cand_key = cand_key.data();
	p.cand_row = cand_row.data();
	p.cursor = &cursor;
	kemu::launch(kgrid, GYS_SVCQ_THREADS, 0, [&] { k_topk_keys(p); });
	g.neligible = cursor;
	CHECK(cursor <= nrows, "more candidates (%u) than rows (%u)", cursor, nrows);
	const uint32_t ncand = cursor, ntake = std::min(ncand, k);
	if (!ntake) return g;
	const bool select = ncand > k;
	if (select) {
		SvcSelectP sp{};
		sp.cand_key = cand_key.data();
		sp.ncand = &cursor;
		sp.hist = hist.data();
		sp.prefix = &prefix;
		sp.want = &want;
		static const uint32_t shifts[GYS_SVCQ_ROUNDS] = {53, 42, 31, 20, 9, 0}, widths[GYS_SVCQ_ROUNDS] = {11, 11, 11, 11, 11, 9};
		for (uint32_t r = 0; r < GYS_SVCQ_ROUNDS; ++r) {
			sp.shift = shifts[r];
			sp.bits = widths[r];
			kemu::launch(hgrid, 256, 0, [&] { k_svc_hist(sp); });
			kemu::launch(1, 256, 0, [&] { k_svc_pick(sp); });
		}
		tie_key.assign(ncand, 0xEEEEEEEEEEEEEEEEull);
		TopkTiesP tp{};
		tp.cand_key = cand_key.data();
		tp.cand_row = cand_row.data();
		tp.ncand = &cursor;
		tp.threshold = &prefix;
		tp.tie_key = tie_key.data();
		tp.ntie = &ntie;
		kemu::launch(hgrid, 256, 0, [&] { k_topk_ties(tp); });
		CHECK(ntie >= want && want >= 1u, "%u ties, %u of them wanted", ntie, want);
		sp.cand_key = tie_key.data();
		sp.ncand = &ntie;
		sp.prefix = &tprefix;
		static const uint32_t tshifts[3] = {21, 10, 0}, twidths[3] = {11, 11, 10};
		for (uint32_t r = 0; r < 3u; ++r) {
			sp.shift = tshifts[r];
			sp.bits = twidths[r];
			kemu::launch(hgrid, 256, 0, [&] { k_svc_hist(sp); });
			kemu::launch(1, 256, 0, [&] { k_svc_pick(sp); });
		}
	}
	std::vector<TopkEntry> out(ntake);
	memset(out.data(), 0xEE, out.size() * sizeof(TopkEntry));
	TopkGatherP gp{};
	gp.col = p.col;
	gp.stride = stride;
	gp.weight = p.weight;
	gp.cand_key = cand_key.data();
	gp.cand_row = cand_row.data();
	gp.ncand = &cursor;
	gp.threshold = select ? &prefix : nullptr;
	gp.tie_threshold = &tprefix;
	gp.maxout = ntake;
	gp.out_count = &nout;
	gp.out = out.data();
	kemu::launch(hgrid, 256, 0, [&] { k_topk_gather(gp); });
	if (nout != ntake) {
		g.ok = false;
		CHECK(false, "selected %u rows, expected %u", nout, ntake);
		return g;
	}
	std::sort(out.begin(), out.end(), [&](const TopkEntry &a, const TopkEntry &b) {
		const unsigned long long ka = topk_key(a.vbits, p.smallest), kb = topk_key(b.vbits, p.smallest);
		return ka != kb ? ka > kb : a.row < b.row;
	});
	g.rows = out;
	return g;
}

void compare(const char *what, uint32_t nrows, uint32_t k, int order, const Got &g, const Want &w)
{
	if (!g.ok) return;
	CHECK(g.neligible == w.neligible, "%s n %u k %u order %d: %llu eligible, want %llu", what, nrows, k, order, (unsigned long long)g.neligible, (unsigned long long)w.neligible);
	CHECK(g.rows.size() == w.rows.size(), "%s n %u k %u order %d: %zu entries, want %zu", what, nrows, k, order, g.rows.size(), w.rows.size());
	for (size_t i = 0; i < g.rows.size() && i < w.rows.size(); ++i) {
		const TopkEntry &a = g.rows[i], &b = w.rows[i];
		if (a.row != b.row || a.vbits != b.vbits || a.weight != b.weight || a.reserved != 0u) {
			CHECK(false, "%s n %u k %u order %d: entry %zu is row %u (%.17g, weight %llu), want row %u (%.17g, weight %llu)", what, nrows, k, order, i, a.row,
			      from_bits(a.vbits), a.weight, b.row, from_bits(b.vbits), b.weight);
			break;
		}
	}
}

enum { COL_DISTINCT, COL_EQUAL, COL_TWO, COL_LASTBITS, COL_SPECIAL, COL_INTS, NCOLS };
const char *COLNAME[NCOLS] = {"distinct", "equal", "two-values", "last-nine-bits", "specials", "ints-0-49"};

std::vector<double> make_col(std::mt19937_64 &rng, int kind, uint32_t n)
{
	std::vector<double> c(n);
	const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity(), den = std::numeric_limits<double>::denorm_min();
	std::vector<uint32_t> perm(n);
	for (uint32_t i = 0; i < n; ++i) perm[i] = i;
	std::shuffle(perm.begin(), perm.end(), rng);
	for (uint32_t i = 0; i < n; ++i) {
		switch (kind) {
		case COL_DISTINCT: c[i] = ((double)perm[i] - (double)(n / 2)) * 1.25 + 0.125; break;
		case COL_EQUAL: c[i] = 42.5; break;
		case COL_TWO: c[i] = perm[i] % 3u == 0 ? 7.0 : 3.0; break;
		case COL_LASTBITS: c[i] = from_bits(bits_of(1.0) + perm[i] % 512u); break;
		case COL_SPECIAL: {
			static const double sp[] = {0.0, -0.0, inf, -inf, den, -den, 4.0 * den, -1.5, 1.5, -1e300, 1e300, nan, -nan, 0.0, -0.0, 2.0};
			c[i] = sp[rng() % 16u];
			break;
		}
		default: c[i] = (double)(rng() % 50u); break;
		}
	}
	return c;
}

const uint32_t SIZES[] = {1, 2, 255, 256, 257, 1023, 1025, 4095, 4096, 4097};

// brief: without the sizes 4 095 and 4 096 (4 097 stays) -- the run under AddressSanitizer, where a thread costs several times as much
void test_topk(std::mt19937_64 &rng, bool brief)
{
	unsigned long long cases = 0, tie_cuts = 0;
	for (uint32_t n : SIZES)
		for (int kind = 0; kind < NCOLS; ++kind) {
			if (brief && (n == 4095u || n == 4096u)) continue;
			const std::vector<double> col = make_col(rng, kind, n);
			std::vector<uint32_t> all(n);
			for (uint32_t i = 0; i < n; ++i) all[i] = i;
			uint32_t ks[6] = {0u, 1u, n - 1u, n, n + 3u, 0u};
			uint32_t nk = 5;
			if (kind == COL_TWO) { // the cut inside the lower value's ties (LARGEST: the 3.0s; SMALLEST: the 7.0s)
				uint32_t n7 = 0;
				for (double v : col) n7 += v == 7.0;
				ks[nk++] = n7 + (n - n7) / 2u; // (for SMALLEST it lies inside either run: both are tie runs)
			}
			for (uint32_t i = 0; i < nk; ++i) {
				const uint32_t k = ks[i];
				const int order = (int)((i + kind + (n & 1u)) & 1u); // (both orders for every column kind and every place of k across the sizes)
				const uint32_t tiles = (n + 1023u) / 1024u, kgrid = std::max(1u, i % 2u ? tiles : (tiles + 1u) / 2u), hgrid = 1u + (i + kind) % 3u;
				const Want w = topk_def(col, 1u, all, nullptr, 0, order, k);
				compare(COLNAME[kind], n, k, order, topk_dev(col, 1u, n, nullptr, nullptr, 0, order, k, kgrid, hgrid), w);
				++cases;
				if (k && k < w.neligible && w.rows.size() == k) { // was the k-th value shared with a row left out?
					const double last = from_bits(w.rows.back().vbits);
					uint32_t same = 0, taken = 0;
					for (double v : col) same += v == last;
					for (const TopkEntry &e : w.rows) taken += from_bits(e.vbits) == last;
					tie_cuts += taken < same;
				}
			}
		}
	CHECK(tie_cuts >= 30ull, "the cut fell inside a run of ties in %llu of %llu cases only", tie_cuts, cases);
	// ---- a stride of 3 (column 1 of an n x 3 array), a shuffled 60 % subset of the rows against the same subset sorted, weights with a threshold
	for (uint32_t n : {257u, 4097u}) {
		if (brief && n == 4097u) continue;
		std::vector<double> arr((size_t)n * 3u);
		for (auto &v : arr) v = (double)(rng() % 97u) - 48.0;
		std::vector<double> col1(arr.begin() + 1, arr.end()); // (element r * 3 of col1 = arr[r][1])
		std::vector<uint32_t> all(n), sub;
		for (uint32_t i = 0; i < n; ++i) all[i] = i;
		for (uint32_t i = 0; i < n; ++i)
			if (rng() % 10u < 6u) sub.push_back(i);
		std::vector<uint32_t> shuf = sub;
		std::shuffle(shuf.begin(), shuf.end(), rng);
		std::vector<uint64_t> weight(n);
		for (auto &x : weight) x = rng() % 1000u;
		for (int order = 0; order < 2; ++order)
			for (uint32_t k : {1u, 33u, (uint32_t)sub.size() - 1u, n + 3u}) {
				compare("stride 3", n, k, order, topk_dev(col1, 3u, n, nullptr, nullptr, 0, order, k, 2u, 2u), topk_def(col1, 3u, all, nullptr, 0, order, k));
				const Got a = topk_dev(col1, 3u, (uint32_t)sub.size(), &shuf, nullptr, 0, order, k, 1u, 3u), b = topk_dev(col1, 3u, (uint32_t)sub.size(), &sub, nullptr, 0, order, k, 3u, 1u);
				const Want w = topk_def(col1, 3u, sub, nullptr, 0, order, k);
				compare("subset shuffled", n, k, order, a, w);
				compare("subset sorted", n, k, order, b, w);
				compare("weights", n, k, order, topk_dev(col1, 3u, n, nullptr, &weight, 500u, order, k, 2u, 2u), topk_def(col1, 3u, all, &weight, 500u, order, k));
				compare("weights on a subset", n, k, order, topk_dev(col1, 3u, (uint32_t)shuf.size(), &shuf, &weight, 500u, order, k, 2u, 2u),
					topk_def(col1, 3u, sub, &weight, 500u, order, k));
			}
	}
	printf("top-k: %llu table cases, the cut inside a run of ties in %llu\n", cases, tie_cuts);
}

// ---------------------------------------------------------------------------------------------------- slab quantiles
// gys_tdigest_slab_quantiles' loop (gys_engine.hip)
double slab_quantile_def(const gys_tdigest_slab &s, double q)
{
	uint64_t N = 0;
	for (int k = 0; k < (int)GYS_TD_NB; ++k) N += s.cnt[k];
	double r = 0.0;
	if (N) {
		double qq = q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q);
		const double t = qq * (double)N;
		double wbefore = 0.0, prev_c = 0.0, prev_mean = 0.0;
		bool have_prev = false, done = false;
		for (int k = 0; k < (int)GYS_TD_NB && !done; ++k) {
			if (!s.cnt[k]) continue;
			const double mean = (double)s.sum[k] / (double)s.cnt[k];
			const double cc = wbefore + (double)s.cnt[k] * 0.5;
			if (t < cc) {
				if (!have_prev) {
					const double lo = (double)s.vmin;
					r = cc <= 0.0 ? mean : lo + (mean - lo) * (t / cc);
				} else {
					r = prev_mean + (mean - prev_mean) * ((t - prev_c) / (cc - prev_c));
				}
				done = true;
				break;
			}
			wbefore += (double)s.cnt[k];
			prev_c = cc;
			prev_mean = mean;
			have_prev = true;
		}
		if (!done) {
			const double hi = (double)s.vmax, span = (double)N - prev_c;
			r = span <= 0.0 ? hi : prev_mean + (hi - prev_mean) * ((t - prev_c) / span);
		}
		r = floor(r + 0.5);
	}
	return r;
}

gys_tdigest_slab make_slab(std::mt19937_64 &rng, uint32_t style)
{
	gys_tdigest_slab s;
	memset(&s, 0, sizeof(s));
	std::vector<uint32_t> idx;
	switch (style % 8u) {
	case 0: break; // empty
	case 1: idx = {(uint32_t)(rng() % GYS_TD_NB)}; break;
	case 2: idx = {199u}; break;
	case 3:
	case 4: for (uint32_t k = 0; k < GYS_TD_NB; ++k) idx.push_back(k); break; // all 200 (4: equal neighbouring means)
	case 5: for (uint32_t k = 0; k < GYS_TD_NB; ++k) if (rng() % 3u == 0) idx.push_back(k); break; // gaps
	case 6: idx = {63u, 64u, 127u, 128u, 191u, 192u, 199u}; break; // the lanes' row borders
	default: for (uint32_t k = 0; k < GYS_TD_NB; k += 2u) idx.push_back(k); break; // counts above 2^32
	}
	if (idx.empty()) {
		s.vmin = 12345; // (an empty slab's extremes are not valid and must not show)
		s.vmax = -7;
		return s;
	}
	int64_t b = (int64_t)(rng() % 5000u);
	for (size_t i = 0; i < idx.size(); ++i) {
		const uint64_t cn = style % 8u == 7u && i % 3u == 1u ? (1ull << 32) + rng() % (1ull << 34) : 1u + rng() % (i % 5 == 0 ? 3u : 5000u);
		const uint64_t rem = style % 8u == 4u ? 0u : rng() % cn;
		if (style % 8u != 4u || i % 3u == 0) b += (int64_t)(rng() % 900u) + 1;
		s.cnt[idx[i]] = cn;
		s.sum[idx[i]] = b * (int64_t)cn + (int64_t)rem;
		if (i == 0) s.vmin = b - (int64_t)(rng() % 40u);
		s.vmax = b + 1 + (int64_t)(rng() % 40u);
		if (rem) ++b;
	}
	return s;
}

void test_slab_quantiles(std::mt19937_64 &rng)
{
	unsigned long long exact_centres = 0, total = 0;
	for (uint32_t ns : {1u, 3u, 4u, 5u, 257u})
		for (uint32_t nq : {1u, 3u, 16u}) {
			std::vector<gys_tdigest_slab> slabs(ns);
			for (uint32_t i = 0; i < ns; ++i) slabs[i] = make_slab(rng, ns == 1u ? nq : i + nq);
			// quantiles: the ends and beyond, a q whose target weight is exactly a centre of the focus slab (an even count: q N = W + cnt / 2 in doubles), others
			TdSlabQP p{};
			const gys_tdigest_slab &f = slabs[(ns * 7u + nq) % ns];
			uint64_t N = 0, W = 0;
			double qc = 0.5;
			for (uint32_t k = 0; k < GYS_TD_NB; ++k) N += f.cnt[k];
			for (uint32_t k = 0; k < GYS_TD_NB && N; ++k) {
				if (f.cnt[k] && f.cnt[k] % 2u == 0 && N < (1ull << 40)) {
					const double cand = ((double)W + (double)f.cnt[k] * 0.5) / (double)N;
					if (cand * (double)N == (double)W + (double)f.cnt[k] * 0.5) {
						qc = cand;
						++exact_centres;
						if (rng() % 4u == 0) break;
					}
				}
				W += f.cnt[k];
			}
			const double cands[16] = {qc, -0.5, 0.0, 1.0, 1.5, 0.5, 0.99, 0.25, 1e-9, 1.0 - 1e-12, 0.95, 0.75, 0.001, 0.999999, 0.1, 0.9};
			for (uint32_t t = 0; t < nq; ++t) p.q[t] = nq == 1u ? cands[(ns + t) % 5u] : cands[t];
			std::vector<double> out((size_t)(ns + 1u) * nq);
			memset(out.data(), 0xEE, out.size() * sizeof(double)); // (no pre-zeroed output needed)
			p.in = slabs.data();
			p.n = ns;
			p.nq = nq;
			p.out = out.data();
			for (uint32_t grid : {1u, 2u, 70u}) {
				if (ns < 257u && grid == 70u) continue;
				kemu::launch(grid, GYS_TR_NT, 0, [=] { k_td_slab_quantiles(p); });
				for (uint32_t i = 0; i < ns; ++i)
					for (uint32_t t = 0; t < nq; ++t) {
						const double want = slab_quantile_def(slabs[i], p.q[t]), got = out[(size_t)i * nq + t];
						++total;
						CHECK(memcmp(&want, &got, 8) == 0, "slab quantiles: %u slabs nq %u grid %u: slab %u q %.17g: %.17g, the host loop gives %.17g", ns, nq, grid, i, p.q[t],
						      got, want);
					}
				const uint8_t *tail = (const uint8_t *)&out[(size_t)ns * nq];
				for (uint32_t i = 0; i < 8u * nq; ++i) CHECK(tail[i] == 0xEE, "slab quantiles: wrote past the output");
			}
		}
	CHECK(exact_centres >= 5ull, "a target weight fell exactly on a centre in %llu cases only", exact_centres);
	printf("slab quantiles: %llu entries, %llu quantiles exactly on a centre\n", total, exact_centres);
}
} // namespace

int main(int argc, char **argv)
{
	if (!kemu::can_run(GYS_SVCQ_THREADS)) {
		printf("kemu: this process cannot have 256 threads\n");
		return 77;
	}
	std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
	test_slab_quantiles(rng);
	test_topk(rng, argc > 2 && !strcmp(argv[2], "brief"));
	if (fails) {
		printf("kemu topk: %d failures\n", fails);
		return 1;
	}
	printf("kemu topk ok\n");
	return 0;
}
