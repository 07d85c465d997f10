// TEST INFRASTRUCTURE (CPU): k_digest_bins (gyeeta_amd/csrc/gys_kernels.hpp) at the bounds that decide what a ROUND of 256 values has to test, and at
// the shapes of the large-value list, ONE workgroup walking the whole list of entries back to back under the CPU stand-in of the device model,
// against the oracle (gyo_td_merge_values, the record fold written out below as in test_bins_edges.cc).
//   Rounds: a thread's k-th value is element tid + 256 k, and the kernel decides per round whether it lies wholly below, wholly above or across
// each of nh (folded part), nwin0 = max(nh, nw) (the current window starts), ent.nbuf (buffer / staged run) and m (the end).  Each of the four is put
// at 0, 1, 255, 256, 257, 511, 512, 513, the last round's first element, the last element and one past it while the others sit on round
// boundaries; once all four fall into one round; with and without a staged run; with nothing folded (the scan folds the one-value bins) and
// with a folded part (it does not).
//   Large values: 0, 1, 3, 4, 5, 255, 256, 257, 512, 513, 1 023, 1 024 of them and one more than the list holds (the hand-over); all of them in one
// cell (one repeated value; all distinct); one value in every one of the 640 cells; the first and last value of a cell and 1 000 000; old clusters
// whose thresholds lie in an occupied cell, in an empty cell between two occupied ones and exactly on a large value; an entry with large values
// directly behind one with none.
// Build + run: tests/test_merge_kernel_rounds_cpu.py (-DKEMU_BINS_VPT=4 / 8 / 64; once more with -fsanitize=address,undefined).
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../../gyeeta_amd/csrc/gys_kernels.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>

#include "../../../oracle/gy_oracle.h"

#ifndef KEMU_BINS_NT
#define KEMU_BINS_NT 256
#endif

using namespace gys;

namespace {

struct Key {
	gyo_tdigest d;             // oracle digest before the merge
	std::vector<int32_t> vals; // buffered (then run) values, in buffer order
	std::vector<uint32_t> rows;
	uint32_t nbuf, mrun, nh, nw, win_epoch, hw_epoch;
	gyo_hist all0, win0; // records before
	uint32_t bm0[GYS_BM_WORDS];
	int32_t mn0, mx0;
};

int fails = 0;
#define CHECK(c, ...)                                  \
	do {                                           \
		if (!(c)) {                            \
			if (fails++ < 20) {            \
				printf("FAIL %s:%d: ", __FILE__, __LINE__); \
				printf(__VA_ARGS__);   \
				printf("\n");          \
			}                              \
		}                                      \
	} while (0)

int32_t draw(std::mt19937 &rng, double mu, double sigma)
{
	std::lognormal_distribution<double> ln(mu, sigma);
	double v = std::floor(ln(rng));
	if (v > 1000000.0) v = 1000000.0;
	return (int32_t)v;
}

int32_t draw_big(std::mt19937 &rng) // a value >= 1024: every octave of the cells, the edges of the value domain among them
{
	static const int32_t edges[] = {1024, 1087, 1088, 999999, 1000000, 1025, 2047, 2048, 65535, 65536, 524288, 983040};
	const uint32_t r = (uint32_t)rng();
	if (r % 4u == 0u) return edges[(r >> 8) % (sizeof(edges) / sizeof(edges[0]))];
	const uint32_t msb = 10u + (r >> 4) % 10u;
	const uint32_t v = (1u << msb) | ((r >> 10) & ((1u << msb) - 1u));
	return (int32_t)std::min(v, 1000000u);
}


struct Spec {
	const char *what;
	std::vector<int32_t> vals; // buffered (then run) values, in buffer order
	std::vector<int32_t> hist; // the key's history: merged and folded before (-> old clusters)
	uint32_t nbuf, nh, nw;
};

std::vector<int32_t> mixed(std::mt19937 &rng, uint32_t m) // ~ 1 in 16 values large (fewer in a streamed merge: the list holds 1 024), the rest below 1 024 with repeats
{
	std::vector<int32_t> v(m);
	const uint32_t den = std::max(16u, m / 40u);
	for (auto &x : v) x = (rng() % den == 0u) ? draw_big(rng) : std::min(draw(rng, 4.0, 1.3), 1023);
	return v;
}

std::vector<int32_t> history(std::mt19937 &rng, int old, uint32_t n)
{
	std::vector<int32_t> h(old ? n : 0u);
	for (auto &v : h) v = old == 2 ? draw(rng, 6.9, 1.6) : std::min(draw(rng, 3.0, 1.2), 1023);
	return h;
}

uint32_t cell_lo(uint32_t cell) // first value of cell `cell` (0 .. 639) and its width
{
	const uint32_t msb = 10u + cell / 64u;
	return (1u << msb) | ((cell % 64u) << (msb - 6u));
}

} // namespace

int main(int argc, char **argv)
{
	const uint32_t NT = 256;
	if (!kemu::can_run(NT)) {
		printf("kemu: this process cannot have %u threads\n", NT);
		return 77;
	}
#ifndef KEMU_BINS_VPT
#define KEMU_BINS_VPT 8
#endif
	const uint32_t CAP = (uint32_t)KEMU_BINS_VPT * NT;
	const uint32_t pcap = CAP + 64u;
	std::mt19937 rng(argc > 1 ? (unsigned)atoi(argv[1]) : 1913u);
	std::vector<Spec> specs;
	uint32_t serial = 0;
	auto add_bounds = [&](const char *what, uint32_t nh, uint32_t nw, uint32_t nbuf, uint32_t m) {
		CHECK(nh <= nbuf && nw <= nbuf && nbuf <= m && m <= CAP, "spec %s: nh %u nw %u nbuf %u m %u", what, nh, nw, nbuf, m);
		const int old = (int)(serial++ % 3u);
		specs.push_back(Spec{what, mixed(rng, m), history(rng, old, 2500u + 37u * serial), nbuf, nh, nw});
	};
	auto up = [](uint32_t x) { return (x + 255u) & ~255u; };
	const uint32_t pos[] = {0u, 1u, 255u, 256u, 257u, 511u, 512u, 513u, CAP - 256u, CAP - 1u, CAP};
	for (uint32_t x : pos) {
		for (uint32_t f = 0; f < 2u; ++f) { // f: a folded part of one value (the scan then does not fold the one-value bins)
			// m = x: no run (the buffer ends there too), and a run from the round boundary below
			if (f <= x) add_bounds("m", f, 0, x, x);
			if (x >= 2u) add_bounds("m, run", f, 0, (x - 1u) & ~255u ? (x - 1u) & ~255u : 1u, x);
			// ent.nbuf = x, the run ends on a round boundary
			if (x < CAP && f <= x) add_bounds("nbuf, run", f, 0, x, std::min(CAP, std::max(256u, up(x + 1u))));
			// the window starts at x, buffer and run end on round boundaries
			const uint32_t nb = std::min(CAP, std::max(256u, up(x)));
			add_bounds("nw", f, x, nb, nb);
			if (nb + 256u <= CAP) add_bounds("nw, run", f, x, nb, nb + 256u);
			else if (nb >= 256u + x && nb > 256u) add_bounds("nw, run", f, x, nb - 256u, nb);
		}
		// the folded part ends at x, the window starts on the round boundary above it
		const uint32_t nb = std::min(CAP, std::max(256u, up(x)));
		add_bounds("nh", x, std::min(nb, up(x)), nb, nb);
		if (nb + 256u <= CAP) add_bounds("nh, run", x, std::min(nb, up(x)), nb, nb + 256u);
		else if (nb >= 256u + up(x) && nb > 256u) add_bounds("nh, run", x, up(x), nb - 256u, nb);
	}
	add_bounds("all four in one round, run", 260, 300, 400, 500);
	add_bounds("all four in one round", 260, 300, 500, 500);
	add_bounds("three in one round, nothing folded", 0, 300, 400, 500);

	// ---- the large-value list
	auto add_big = [&](const char *what, std::vector<int32_t> v, std::vector<int32_t> h) {
		if (v.size() > CAP) return; // (a merge of this instance cannot hold it)
		std::shuffle(v.begin(), v.end(), rng);
		const uint32_t m = (uint32_t)v.size();
		specs.push_back(Spec{what, std::move(v), std::move(h), m, 0u, 0u});
	};
	auto smalls = [&](std::vector<int32_t> v, uint32_t n) {
		for (uint32_t i = 0; i < n && v.size() < CAP; ++i) v.push_back((int32_t)(rng() % 1024u));
		return v;
	};
	for (uint32_t nbig : {0u, 1u, 3u, 4u, 5u, 255u, 256u, 257u, 512u, 513u, 1023u, 1024u, GYS_MB_BIG_CAP + 1u}) {
		std::vector<int32_t> v;
		for (uint32_t i = 0; i < nbig; ++i) v.push_back(draw_big(rng));
		add_big("nbig", smalls(v, 150), history(rng, nbig % 2u ? 2 : 0, 4000u));
		if (nbig == 0u) add_big("nbig 1 behind nbig 0", smalls({5000}, 150), history(rng, 2, 4000u)); // (directly behind an entry without large values)
	}
	add_big("one cell, one value", smalls(std::vector<int32_t>(300, 5000), 50), history(rng, 2, 4000u));
	{
		std::vector<int32_t> v;
		for (int i = 0; i < 600; ++i) v.push_back(65536 + i); // the cell [65536, 66560)
		add_big("one cell, all distinct", smalls(v, 50), history(rng, 2, 4000u));
	}
	{
		std::vector<int32_t> v; // one value in every cell (the kernel's value domain: below 2^20)
		for (uint32_t c = 0; c < 640u; ++c) {
			const uint32_t lo = cell_lo(c), w = 1u << (4u + c / 64u);
			v.push_back((int32_t)(lo + (uint32_t)rng() % w));
		}
		add_big("every cell once", smalls(v, 100), history(rng, 2, 4000u));
		add_big("no large value behind every cell", smalls({}, 300), history(rng, 2, 4000u));
	}
	{
		std::vector<int32_t> v;
		for (uint32_t c : {0u, 1u, 63u, 64u, 200u, 377u, 634u}) {
			const uint32_t lo = cell_lo(c), w = 1u << (4u + c / 64u);
			for (int r = 0; r < 3; ++r) {
				v.push_back((int32_t)lo);
				v.push_back((int32_t)(lo + w - 1u));
			}
		}
		for (int r = 0; r < 3; ++r) v.push_back(1000000);
		v.push_back(999999);
		add_big("first and last value of a cell, 1 000 000", smalls(v, 100), history(rng, 2, 4000u));
	}
	{
		// pure old clusters at 5003 (its cell [4992, 5056) holds new values), 5100 (its cell [5056, 5120) holds none, the cells on both sides do) and
		// 9000 (a new value itself)
		std::vector<int32_t> h;
		for (int32_t x : {5003, 5100, 9000}) h.insert(h.end(), 800, x);
		std::vector<int32_t> v{5000, 5010, 5002, 5003, 5004, 5055, 4992, 5130, 5150, 5120, 9000, 9000, 9000, 8999, 9001, 8960, 9023};
		add_big("old thresholds in / between / on", smalls(v, 120), h);
		add_big("old thresholds in / between / on, twice", smalls(v, 40), h);
	}

	const uint32_t S = (uint32_t)specs.size();
	std::vector<Key> keys(S);
	std::vector<int64_t> td_sum((size_t)S * GYS_TD_NB, 0);
	std::vector<uint32_t> td_cnt((size_t)S * GYS_TD_NB, 0), td_pend((size_t)S * pcap, 0xDEADBEEFu), td_cur(S, 0), staged((size_t)S * 256u + CAP, 0), bitmap((size_t)S * GYS_BM_WORDS, 0);
	std::vector<TdMeta> meta(S);
	std::vector<int2> minmax(S);
	std::vector<gys_hist_rec> hist_all(S), hist_win(S);
	std::vector<MergeEnt> list(S), slow(S + 1);
	std::vector<bool> handed(S, false);
	uint32_t count = S, slow_count = 0, staged_used = 0, want_slow = 0;

	for (uint32_t s = 0; s < S; ++s) {
		Key &k = keys[s];
		const Spec &sp = specs[s];
		gyo_td_init(&k.d);
		gyo_hist_init(&k.all0, GYO_RESP_TIME_HASH);
		gyo_hist_init(&k.win0, GYO_RESP_TIME_HASH);
		memset(k.bm0, 0, sizeof(k.bm0));
		k.mn0 = INT32_MAX;
		k.mx0 = INT32_MIN;
		if (!sp.hist.empty()) {
			for (int32_t v : sp.hist) {
				gyo_hist_add(&k.all0, v);
				k.mn0 = std::min(k.mn0, v);
				k.mx0 = std::max(k.mx0, v);
			}
			gyo_td_merge_values(&k.d, sp.hist.data(), sp.hist.size());
		}
		if (!strncmp(sp.what, "old thresholds", 14)) {
			for (int64_t want : {5003, 5100, 9000}) {
				bool pure = false;
				for (int j = 0; j < GYO_TD_NB; ++j) pure = pure || (k.d.cnt[j] && k.d.sum[j] == want * (int64_t)k.d.cnt[j]);
				CHECK(pure, "spec: no old cluster with threshold %lld", (long long)want);
			}
		}
		k.vals = sp.vals;
		std::vector<int32_t> &v = k.vals;
		uint32_t nbig = 0;
		for (int32_t x : v) nbig += x >= (int32_t)GYS_MB_EXACT ? 1u : 0u;
		const uint32_t m = (uint32_t)v.size();
		CHECK(m <= CAP, "spec: key %u holds %u values", s, m);
		handed[s] = nbig > GYS_MB_BIG_CAP;
		want_slow += handed[s] ? 1u : 0u;
		k.nbuf = sp.nbuf;
		k.mrun = m - k.nbuf;
		k.nh = sp.nh;
		k.nw = sp.nw;
		k.rows.resize(m);
		for (uint32_t i = 0; i < m; ++i) k.rows[i] = (uint32_t)(rng() & (s % 3 == 0 ? 31u : 63u));
		k.win_epoch = 7;
		k.hw_epoch = s % 2 ? 7u : 5u;
		for (uint32_t i = 0; i < k.nh; ++i) {
			gyo_hist_add(&k.all0, k.vals[i]);
			k.mn0 = std::min(k.mn0, k.vals[i]);
			k.mx0 = std::max(k.mx0, k.vals[i]);
			if (i >= k.nw && k.hw_epoch == k.win_epoch) {
				const uint32_t b = gyo_hist_add(&k.win0, k.vals[i]);
				k.bm0[k.rows[i] >> 1] |= (1u << b) << ((k.rows[i] & 1u) * 16u);
			}
		}
		if (k.hw_epoch != k.win_epoch) {
			gyo_hist_add(&k.win0, 123);
			k.bm0[3] = 0x00010002u;
			k.bm0[21] = 0x00400001u;
		}
		for (int j = 0; j < GYO_TD_NB; ++j) {
			td_sum[(size_t)s * GYS_TD_NB + j] = k.d.sum[j];
			td_cnt[(size_t)s * GYS_TD_NB + j] = k.d.cnt[j];
		}
		for (uint32_t i = 0; i < k.nbuf; ++i) td_pend[(size_t)s * pcap + i] = ((uint32_t)k.vals[i] << GYS_ROW_BITS) | k.rows[i];
		uint32_t off_end = 0;
		if (k.mrun) {
			for (uint32_t i = 0; i < k.mrun; ++i) staged[staged_used + i] = ((uint32_t)k.vals[k.nbuf + i] << GYS_ROW_BITS) | k.rows[k.nbuf + i];
			staged_used += k.mrun;
			off_end = staged_used;
		}
		meta[s].npend = k.nbuf;
		meta[s].nh = (uint16_t)k.nh;
		meta[s].nw = (uint16_t)k.nw;
		meta[s].win_epoch = k.win_epoch;
		meta[s].hw_epoch = k.hw_epoch;
		td_cur[s] = k.nbuf;
		minmax[s] = make_int2(k.mn0, k.mx0);
		for (int b = 0; b < 15; ++b) {
			hist_all[s].stats[b].count = k.all0.stats[b].count;
			hist_all[s].stats[b].sum = k.all0.stats[b].sum;
			hist_win[s].stats[b].count = k.win0.stats[b].count;
			hist_win[s].stats[b].sum = k.win0.stats[b].sum;
		}
		hist_all[s].total_count = k.all0.total_count;
		hist_all[s].max_val_seen = k.all0.total_count ? k.all0.max_val_seen : INT64_MIN;
		hist_win[s].total_count = k.win0.total_count;
		hist_win[s].max_val_seen = k.win0.total_count ? k.win0.max_val_seen : INT64_MIN;
		memcpy(&bitmap[(size_t)s * GYS_BM_WORDS], k.bm0, sizeof(k.bm0));
		list[s] = MergeEnt{s, k.nbuf, k.mrun, off_end};
	}

	MergeBP q{};
	q.d.td_sum = td_sum.data();
	q.d.td_cnt = td_cnt.data();
	q.d.td_meta = meta.data();
	q.d.td_minmax = minmax.data();
	q.d.td_pend = td_pend.data();
	q.d.td_cur = td_cur.data();
	q.d.pcap = pcap;
	q.d.pend_cap = CAP - 128u;
	q.d.nsvc = S;
	q.d.staged = staged.data();
	q.d.hist_win = hist_win.data();
	q.d.hist_all = hist_all.data();
	q.d.bitmap = bitmap.data();
	q.list = list.data();
	q.count = &count;
	q.slow_list = slow.data();
	q.slow_count = &slow_count;

	kemu::launch(1, NT, 0, [&] { k_digest_bins<false, KEMU_BINS_VPT>(q); }); // ONE workgroup: the entries back to back

	CHECK(slow_count == want_slow, "hand-over list: %u entries, want %u", slow_count, want_slow);
	for (uint32_t i = 0; i < slow_count && i < S; ++i) CHECK(slow[i].slot < S && handed[slow[i].slot], "key %u was handed over", slow[i].slot);
	printf("%u entries, merges of up to %u values; %u keys handed over\n", S, CAP, want_slow);
	for (uint32_t s = 0; s < S; ++s) {
		const Key &k = keys[s];
		const uint32_t m = k.nbuf + k.mrun;
		if (handed[s] || m == 0) { // untouched
			bool same = meta[s].npend == k.nbuf && meta[s].nh == k.nh && meta[s].nw == k.nw && meta[s].hw_epoch == k.hw_epoch && td_cur[s] == k.nbuf;
			for (int j = 0; j < GYO_TD_NB; ++j) same = same && td_sum[(size_t)s * GYS_TD_NB + j] == k.d.sum[j] && td_cnt[(size_t)s * GYS_TD_NB + j] == k.d.cnt[j];
			same = same && hist_all[s].total_count == k.all0.total_count && minmax[s].x == k.mn0 && minmax[s].y == k.mx0;
			CHECK(same, "key %u (%s) was modified", s, m ? "handed over" : "nothing buffered");
			continue;
		}
		gyo_tdigest d = k.d;
		gyo_td_merge_values(&d, k.vals.data(), m);
		for (int j = 0; j < GYO_TD_NB; ++j)
			CHECK(td_sum[(size_t)s * GYS_TD_NB + j] == d.sum[j] && td_cnt[(size_t)s * GYS_TD_NB + j] == d.cnt[j], "key %u (m %u) cluster %d: got {%lld, %u} want {%lld, %u}", s, m,
			      j, (long long)td_sum[(size_t)s * GYS_TD_NB + j], td_cnt[(size_t)s * GYS_TD_NB + j], (long long)d.sum[j], d.cnt[j]);
		// records: every not yet folded value into the all-time record; the values of window win_epoch into the window record (rolled first
		// when it belonged to an older window) and into the CONN_BITMAP rows
		gyo_hist all = k.all0, win = k.win0;
		uint32_t bm[GYS_BM_WORDS];
		memcpy(bm, k.bm0, sizeof(bm));
		int32_t mn = k.mn0, mx = k.mx0;
		const uint32_t nwin0 = std::max(k.nh, k.nw);
		const bool any_win = m > nwin0, roll = k.hw_epoch != k.win_epoch;
		if (any_win && roll) {
			gyo_hist_init(&win, GYO_RESP_TIME_HASH);
			memset(bm, 0, sizeof(bm));
		}
		for (uint32_t i = k.nh; i < m; ++i) {
			gyo_hist_add(&all, k.vals[i]);
			mn = std::min(mn, k.vals[i]);
			mx = std::max(mx, k.vals[i]);
			if (i >= nwin0) {
				const uint32_t b = gyo_hist_add(&win, k.vals[i]);
				bm[k.rows[i] >> 1] |= (1u << b) << ((k.rows[i] & 1u) * 16u);
			}
		}
		for (int b = 0; b < 15; ++b) {
			CHECK(hist_all[s].stats[b].count == all.stats[b].count && hist_all[s].stats[b].sum == all.stats[b].sum, "key %u all-time bucket %d: {%llu, %lld} want {%llu, %lld}", s, b,
			      (unsigned long long)hist_all[s].stats[b].count, (long long)hist_all[s].stats[b].sum, (unsigned long long)all.stats[b].count, (long long)all.stats[b].sum);
			CHECK(hist_win[s].stats[b].count == win.stats[b].count && hist_win[s].stats[b].sum == win.stats[b].sum, "key %u window bucket %d: {%llu, %lld} want {%llu, %lld}", s, b,
			      (unsigned long long)hist_win[s].stats[b].count, (long long)hist_win[s].stats[b].sum, (unsigned long long)win.stats[b].count, (long long)win.stats[b].sum);
		}
		CHECK(hist_all[s].total_count == all.total_count, "key %u all-time total %llu want %llu", s, (unsigned long long)hist_all[s].total_count, (unsigned long long)all.total_count);
		if (all.total_count) CHECK(hist_all[s].max_val_seen == all.max_val_seen, "key %u all-time max %lld want %lld", s, (long long)hist_all[s].max_val_seen, (long long)all.max_val_seen);
		CHECK(hist_win[s].total_count == win.total_count, "key %u window total %llu want %llu", s, (unsigned long long)hist_win[s].total_count, (unsigned long long)win.total_count);
		if (any_win) CHECK(hist_win[s].max_val_seen == win.max_val_seen, "key %u window max %lld want %lld", s, (long long)hist_win[s].max_val_seen, (long long)win.max_val_seen);
		for (int g = 0; g < (int)GYS_BM_WORDS; ++g) CHECK(bitmap[(size_t)s * GYS_BM_WORDS + g] == bm[g], "key %u bitmap word %d: %08x want %08x", s, g, bitmap[(size_t)s * GYS_BM_WORDS + g], bm[g]);
		CHECK(minmax[s].x == mn && minmax[s].y == mx, "key %u min/max {%d, %d} want {%d, %d}", s, minmax[s].x, minmax[s].y, mn, mx);
		// the buffer is drained; the window bookkeeping moves on
		CHECK(meta[s].npend == 0 && meta[s].nh == 0 && meta[s].nw == 0 && meta[s].win_epoch == k.win_epoch && meta[s].hw_epoch == (any_win ? k.win_epoch : k.hw_epoch) && td_cur[s] == 0,
		      "key %u meta {%u, %u, %u, %u, %u} cur %u", s, meta[s].npend, meta[s].nh, meta[s].nw, meta[s].win_epoch, meta[s].hw_epoch, td_cur[s]);
	}
	if (fails) {
		printf("%d checks failed\n", fails);
		return 1;
	}
	printf("kemu bins rounds ok (one workgroup, %u entries, merges of up to %u values)\n", S, CAP);
	return 0;
}
