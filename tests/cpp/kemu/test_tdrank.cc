// TEST INFRASTRUCTURE (CPU): the LOGIC of the rank kernel k_td_ranks (gyeeta_amd/csrc/gys_tdrank.hpp) under the CPU stand-in of the device
// model, on synthetic digests, compared BIT FOR BIT with a plain loop of the definition ("Ranks" in include/gysketch.h) written here:
//   * service members: buffers of 0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257 and td_pend_cap values, a buffer stride that is a multiple of 4
//     (16-byte loads) and one that is not; 0, 1, 2 and 200 non-empty clusters, gaps of empty clusters, equal neighbouring means, members with
//     buffered values only and without anything; td_minmax as a partial fold leaves it (widened by a prefix of the buffer only);
//   * slab members with counts above 2^32 and thresholds whose product with a count needs 128 bits;
//   * 1, 15, 16 and 17 members and the whole world, several grid sizes, a range that does not start at member 0;
//   * thresholds below the minimum, on it, on a cluster mean, between means, on the maximum, above it, negative, above 2^26, INT64_MIN / MAX;
//     1, 3, 7 and 16 thresholds a call (every instantiation of the kernel);
//   * outputs pre-filled with garbage (nothing needs zeroing), nothing written past them.
// Build + run: tests/test_kernel_logic_tdrank_cpu.py.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../../gyeeta_amd/csrc/gys_tdrank.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
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

struct Digest {
	int64_t sum[GYS_TD_NB];
	uint64_t cnt[GYS_TD_NB];
	int64_t vmin, vmax;      // of the clustered values
	std::vector<int32_t> P;  // buffered values (services)
};

// how often each branch of the definition was taken: main() refuses a run that missed one
enum { B_EMPTY, B_BELOW, B_ABOVE, B_FIRST, B_LAST, B_BETWEEN, B_WIDE, B_N };
unsigned long long branches[B_N];

// ---- the definition, step by step (include/gysketch.h, "Ranks")
double below_def(const Digest &d, int64_t x, uint64_t *total)
{
	uint64_t nb = 0, N = 0;
	for (int32_t v : d.P) nb += (int64_t)v <= x; // 1.
	for (uint32_t k = 0; k < GYS_TD_NB; ++k) N += d.cnt[k]; // 2.
	*total = N + d.P.size();
	if (N == 0) {
		branches[B_EMPTY]++;
		return (double)nb;
	}
	int64_t lo = d.vmin, hi = d.vmax; // 3.
	for (int32_t v : d.P) {
		lo = std::min<int64_t>(lo, v);
		hi = std::max<int64_t>(hi, v);
	}
	double r;
	if (x < lo) {
		branches[B_BELOW]++;
		r = 0.0;
	} else if (x >= hi) {
		branches[B_ABOVE]++;
		r = (double)N;
	} else { // 4.
		int j = -1, n = -1, f = -1;
		for (int k = 0; k < (int)GYS_TD_NB; ++k)
			if (d.cnt[k]) {
				if (f < 0) f = k;
				if ((__int128)d.sum[k] - (__int128)(d.cnt[k] / 2) <= (__int128)x * (__int128)d.cnt[k]) j = k;
				if ((__int128)x * (__int128)d.cnt[k] != (__int128)(int64_t)((uint64_t)x * d.cnt[k])) branches[B_WIDE]++; // (64 bits would not do)
			}
		for (int k = j + 1; j >= 0 && k < (int)GYS_TD_NB; ++k)
			if (d.cnt[k]) {
				n = k;
				break;
			}
		auto W = [&](int k) {
			uint64_t w = 0;
			for (int i = 0; i < k; ++i) w += d.cnt[i];
			return w;
		};
		auto c = [&](int k) { return (double)W(k) + (double)d.cnt[k] * 0.5; };
		auto m = [&](int k) { return (double)d.sum[k] / (double)d.cnt[k]; };
		branches[j < 0 ? B_FIRST : (n < 0 ? B_LAST : B_BETWEEN)]++;
		const double y = (double)x + 0.5;
		if (j < 0) r = c(f) * ((y - ((double)lo - 0.5)) / (m(f) - ((double)lo - 0.5)));
		else if (n < 0) r = c(j) + ((double)N - c(j)) * ((y - m(j)) / (((double)hi + 0.5) - m(j)));
		else r = c(j) + (c(n) - c(j)) * ((y - m(j)) / (m(n) - m(j)));
	}
	return r + (double)nb; // 5.
}

// clusters at the indices `idx` (ascending) with non-decreasing means from `base` up; `wide`: counts above 2^32
void fill_clusters(std::mt19937_64 &rng, Digest &d, const std::vector<uint32_t> &idx, int64_t base, bool equal_means, bool wide)
{
	memset(d.sum, 0, sizeof(d.sum));
	memset(d.cnt, 0, sizeof(d.cnt));
	d.vmin = INT32_MAX;
	d.vmax = INT32_MIN;
	if (idx.empty()) return;
	int64_t b = base, first_floor = 0, last_ceil = 0;
	for (size_t i = 0; i < idx.size(); ++i) {
		const uint64_t cn = wide && i % 3 == 1 ? (1ull << 32) + rng() % (1ull << 34) : 1u + rng() % (i % 5 == 0 ? 3u : 5000u);
		uint64_t rem = (i % 4 == 2 || equal_means) ? 0u : rng() % cn; // (integer means among them: a threshold can sit on one)
		if (!equal_means || i % 3 == 0) b += (int64_t)(rng() % (i % 7 == 3 ? 1u : 900u)) + (i % 7 == 3 ? 0 : 1); // (i % 7 == 3: the same mean as the last, too)
		if (i % 7 == 3) rem = 0;
		d.cnt[idx[i]] = cn;
		d.sum[idx[i]] = b * (int64_t)cn + (int64_t)rem;
		if (i == 0) first_floor = b;
		last_ceil = b + (rem != 0);
		if (rem) ++b; // the next mean is no smaller
	}
	d.vmin = first_floor - (int64_t)(rng() % 3u == 0 ? 0u : rng() % 50u);
	d.vmax = last_ceil + (int64_t)(rng() % 3u == 0 ? 0u : rng() % 50u);
}

std::vector<uint32_t> pick_idx(std::mt19937_64 &rng, int style)
{
	std::vector<uint32_t> idx;
	switch (style) {
	case 0: break;                                   // no cluster
	case 1: idx = {(uint32_t)(rng() % GYS_TD_NB)}; break;
	case 2: idx = {(uint32_t)(rng() % 100u), 100u + (uint32_t)(rng() % 100u)}; break;
	case 3:
	case 4: for (uint32_t k = 0; k < GYS_TD_NB; ++k) idx.push_back(k); break; // all 200 (4: equal neighbouring means)
	case 5: for (uint32_t k = 0; k < GYS_TD_NB; ++k) if (rng() % 3u == 0) idx.push_back(k); break; // gaps
	default: idx = {63u, 64u, 127u, 128u, 191u, 192u, 199u}; break; // the lanes' row borders
	}
	return idx;
}

const uint32_t NPENDS[] = {0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 896};
const uint32_t PEND_CAP = 896, NSTYLE = 7;

struct World {
	uint32_t nsvc, pcap;
	std::vector<Digest> dg;
	std::vector<int64_t> td_sum;
	std::vector<uint32_t> td_cnt, td_pend;
	std::vector<TdMeta> meta;
	std::vector<int2> mm;
	DigestP params()
	{
		DigestP p{};
		p.td_sum = td_sum.data();
		p.td_cnt = td_cnt.data();
		p.td_meta = meta.data();
		p.td_minmax = mm.data();
		p.td_pend = td_pend.data();
		p.pcap = pcap;
		p.nsvc = nsvc;
		p.pend_cap = PEND_CAP;
		return p;
	}
};

World make_world(std::mt19937_64 &rng, uint32_t pcap)
{
	World w;
	w.pcap = pcap;
	w.nsvc = (uint32_t)(sizeof(NPENDS) / sizeof(NPENDS[0])) * NSTYLE;
	w.dg.resize(w.nsvc);
	w.td_sum.assign((size_t)w.nsvc * GYS_TD_NB, 0);
	w.td_cnt.assign((size_t)w.nsvc * GYS_TD_NB, 0);
	w.td_pend.assign((size_t)w.nsvc * pcap, 0xEEEEEEEEu); // (what lies behind a buffer's fill must not count)
	w.meta.resize(w.nsvc);
	w.mm.resize(w.nsvc);
	for (uint32_t s = 0; s < w.nsvc; ++s) {
		Digest &d = w.dg[s];
		const uint32_t npend = NPENDS[s % 12u], style = (s / 12u + s) % NSTYLE;
		const int64_t base = s % 5 == 0 ? 0 : (int64_t)(rng() % 20000u);
		fill_clusters(rng, d, pick_idx(rng, (int)style), base, style == 4, false);
		for (uint32_t k = 0; k < GYS_TD_NB; ++k) {
			w.td_sum[(size_t)s * GYS_TD_NB + k] = d.sum[k];
			w.td_cnt[(size_t)s * GYS_TD_NB + k] = (uint32_t)d.cnt[k];
		}
		// buffered values around the clusters' range, some below the minimum and above the maximum, some large (26 bits)
		const int64_t span = d.vmax >= d.vmin ? d.vmax - d.vmin + 40 : 5000;
		const int64_t from = d.vmax >= d.vmin ? std::max<int64_t>(0, d.vmin - 20) : base;
		for (uint32_t i = 0; i < npend; ++i) {
			int64_t v = rng() % 50u == 0 ? (int64_t)(rng() % (1u << 26)) : from + (int64_t)(rng() % (uint64_t)span);
			d.P.push_back((int32_t)std::min<int64_t>(v, (1 << 26) - 1));
			w.td_pend[(size_t)s * pcap + i] = ((uint32_t)d.P.back() << GYS_ROW_BITS) | (uint32_t)(rng() & GYS_ROW_MASK);
		}
		memset(&w.meta[s], 0, sizeof(TdMeta));
		w.meta[s].npend = npend;
		w.meta[s].nh = (uint16_t)(npend ? rng() % (npend + 1u) : 0u); // folded so far: td_minmax covers the clusters and words [0, nh) only
		int32_t mn = (int32_t)d.vmin, mx = (int32_t)d.vmax;
		for (uint32_t i = 0; i < w.meta[s].nh; ++i) {
			mn = std::min(mn, d.P[i]);
			mx = std::max(mx, d.P[i]);
		}
		w.mm[s] = make_int2(mn, mx);
	}
	return w;
}

// thresholds around member `focus`: every place of the definition, then far ones
std::vector<int64_t> thresholds_for(std::mt19937_64 &rng, const Digest &d, uint32_t nt)
{
	std::vector<int64_t> c;
	int64_t lo = d.vmin, hi = d.vmax;
	for (int32_t v : d.P) {
		lo = std::min<int64_t>(lo, v);
		hi = std::max<int64_t>(hi, v);
	}
	if (lo > hi) lo = hi = 100;
	c.push_back(lo - 1);
	c.push_back(lo);
	c.push_back(hi);
	c.push_back(hi + 1);
	std::vector<int64_t> means;
	for (uint32_t k = 0; k < GYS_TD_NB; ++k)
		if (d.cnt[k]) means.push_back(d.sum[k] / (int64_t)d.cnt[k]); // (the mean itself where it is an integer, else just below it)
	if (!means.empty()) {
		c.push_back(means[rng() % means.size()]);
		c.push_back(means[rng() % means.size()] + 1);
		c.push_back(means.front());
		c.push_back(means.front() - 1);
		c.push_back(means.back());
		c.push_back(means.back() + 1);
		c.push_back((means.front() + means.back()) / 2);
	}
	c.push_back(-5);
	c.push_back((1ll << 26) + 12345);
	c.push_back(INT64_MIN);
	c.push_back(INT64_MAX);
	c.push_back(0);
	c.push_back(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)));
	c.push_back(1ll << 40);
	std::shuffle(c.begin(), c.end(), rng);
	c.resize(std::max<size_t>(c.size(), nt), 7);
	// the first nt; with a single threshold rotate through the candidates by the draw above
	return std::vector<int64_t>(c.begin(), c.begin() + nt);
}

template <int KIND>
void launch(const TdRankP &q, uint32_t grid)
{
	if (KIND == 1) kemu::launch(grid, GYS_TR_NT, 0, [=] { k_td_ranks<1, 1u>(q); });
	else if (q.nt <= 2u) kemu::launch(grid, GYS_TR_NT, 0, [=] { k_td_ranks<0, 1u>(q); });
	else if (q.nt <= 4u) kemu::launch(grid, GYS_TR_NT, 0, [=] { k_td_ranks<0, 2u>(q); });
	else if (q.nt <= 8u) kemu::launch(grid, GYS_TR_NT, 0, [=] { k_td_ranks<0, 4u>(q); });
	else kemu::launch(grid, GYS_TR_NT, 0, [=] { k_td_ranks<0, 8u>(q); });
}

// members [first, first + n) of `dg` through the kernel against the definition
template <int KIND>
void run_case(const char *what, TdRankP q, const std::vector<Digest> &dg, uint32_t first, uint32_t n, const std::vector<int64_t> &thr, uint32_t grid, bool with_total)
{
	const uint32_t nt = (uint32_t)thr.size();
	std::vector<double> below((size_t)(n + 1) * nt);
	std::vector<unsigned long long> total(n + 1);
	memset(below.data(), 0xEE, below.size() * sizeof(double)); // (no pre-zeroed output needed)
	memset(total.data(), 0xEE, total.size() * sizeof(unsigned long long));
	q.first = first;
	q.n = n;
	q.nt = nt;
	for (uint32_t t = 0; t < nt; ++t) q.thr[t] = thr[t];
	q.below = below.data();
	q.total = with_total ? total.data() : nullptr;
	launch<KIND>(q, grid);
	for (uint32_t i = 0; i < n; ++i) {
		uint64_t want_total = 0;
		for (uint32_t t = 0; t < nt; ++t) {
			const double want = below_def(dg[first + i], thr[t], &want_total), got = below[(size_t)i * nt + t];
			CHECK(memcmp(&want, &got, 8) == 0, "%s grid %u members [%u, +%u) nt %u: member %u threshold %lld: %.17g, the definition gives %.17g", what, grid, first, n,
			      nt, first + i, (long long)thr[t], got, want);
		}
		if (with_total) CHECK(total[i] == want_total, "%s grid %u: total of member %u: %llu, want %llu", what, grid, first + i, total[i], (unsigned long long)want_total);
	}
	const uint8_t *tb = (const uint8_t *)&below[(size_t)n * nt], *tt = (const uint8_t *)&total[n];
	for (uint32_t i = 0; i < 8u * nt; ++i) CHECK(tb[i] == 0xEE, "%s grid %u: wrote past below[]", what, grid);
	for (uint32_t i = 0; i < 8u; ++i) CHECK(tt[i] == 0xEE, "%s grid %u: wrote past total[]", what, grid);
	if (!with_total)
		for (uint32_t i = 0; i < n; ++i) CHECK(total[i] == 0xEEEEEEEEEEEEEEEEull, "%s: total[] written though it was not asked for", what);
}

void test_services(std::mt19937_64 &rng, uint32_t pcap)
{
	World w = make_world(rng, pcap);
	TdRankP q{};
	q.d = w.params();
	char what[64];
	snprintf(what, sizeof(what), "services pcap %u", pcap);
	const uint32_t grids[] = {1u, 3u, 7u, 32u}, nts[] = {1u, 3u, 7u, 16u};
	for (uint32_t i = 0; i < 4u; ++i) { // the whole world
		const uint32_t focus = (uint32_t)(rng() % w.nsvc);
		run_case<0>(what, q, w.dg, 0u, w.nsvc, thresholds_for(rng, w.dg[focus], nts[i]), grids[(i + pcap) % 4u], i != 1u);
	}
	for (uint32_t n : {1u, 15u, 16u, 17u}) // a few members, from anywhere
		for (uint32_t grid : {1u, 2u, 5u}) {
			const uint32_t first = (uint32_t)(rng() % (w.nsvc - n + 1u));
			run_case<0>(what, q, w.dg, first, n, thresholds_for(rng, w.dg[first + (uint32_t)(rng() % n)], grid == 2u ? 16u : (grid == 1u ? 1u : 3u)), grid, true);
		}
	// every member at the thresholds made for it, one at a time (as gys_query_ranks runs the kernel)
	for (uint32_t s = 0; s < w.nsvc; s += 5u) run_case<0>(what, q, w.dg, s, 1u, thresholds_for(rng, w.dg[s], 16u), 1u, true);
}

void test_slabs(std::mt19937_64 &rng)
{
	const uint32_t ns = 21;
	std::vector<Digest> dg(ns);
	std::vector<gys_tdigest_slab> slabs(ns);
	for (uint32_t s = 0; s < ns; ++s) {
		fill_clusters(rng, dg[s], pick_idx(rng, (int)(s % NSTYLE)), s % 4 == 0 ? 0 : (int64_t)(rng() % 100000u), s % NSTYLE == 4, s % 2 == 1);
		if (s == 20) { // heavy clusters at small means, light ones far above: for a threshold in between, x * cnt passes 64 bits
			Digest &d = dg[s];
			memset(d.sum, 0, sizeof(d.sum));
			memset(d.cnt, 0, sizeof(d.cnt));
			for (uint32_t k = 0; k < 10u; ++k) {
				d.cnt[3u * k] = (1ull << 33) + k;
				d.sum[3u * k] = (int64_t)d.cnt[3u * k] * (1000 + k) + (int64_t)(rng() % 1000u);
				d.cnt[100u + 7u * k] = 1u + k;
				d.sum[100u + 7u * k] = (int64_t)d.cnt[100u + 7u * k] * ((1ll << 36) + ((int64_t)k << 30)) + (int64_t)(rng() % (1u + k));
			}
			d.vmin = 900;
			d.vmax = 1ll << 37;
		}
		for (uint32_t k = 0; k < GYS_TD_NB; ++k) {
			slabs[s].sum[k] = dg[s].sum[k];
			slabs[s].cnt[k] = dg[s].cnt[k];
		}
		slabs[s].vmin = dg[s].vmin;
		slabs[s].vmax = dg[s].vmax;
		if (dg[s].vmin > dg[s].vmax) slabs[s].vmin = slabs[s].vmax = 0; // (an empty slab's extremes are not valid)
	}
	TdRankP q{};
	q.in = slabs.data();
	for (uint32_t nt : {1u, 16u})
		for (uint32_t grid : {1u, 4u, 9u})
			for (uint32_t focus : {1u, 3u, 20u}) run_case<1>("slabs", q, dg, 0u, ns, thresholds_for(rng, dg[focus], nt), grid, grid != 4u);
	for (uint32_t n : {1u, 15u, 16u, 17u}) run_case<1>("slabs", q, dg, ns - n, n, thresholds_for(rng, dg[20], 16u), 2u, true);
}
} // namespace

int main(int argc, char **argv)
{
	if (!kemu::can_run(GYS_TR_NT)) {
		printf("kemu: this process cannot have 256 threads\n");
		return 77;
	}
	std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
	test_services(rng, 960u); // 16-byte loads
	test_services(rng, 963u); // dword loads
	test_slabs(rng);
	for (int b = 0; b < B_N; ++b) CHECK(branches[b] >= 20ull, "branch %d of the definition was taken %llu times only", b, branches[b]);
	printf("branches: empty %llu below %llu above %llu first %llu last %llu between %llu wide-product %llu\n", branches[0], branches[1], branches[2], branches[3],
	       branches[4], branches[5], branches[6]);
	if (fails) {
		printf("kemu tdrank: %d failures\n", fails);
		return 1;
	}
	printf("kemu tdrank ok\n");
	return 0;
}
