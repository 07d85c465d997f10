// TEST INFRASTRUCTURE (CPU): the several-workgroup t-digest path for large keys (gys_huge.hpp: k_huge_plan / k_huge_clear / k_huge_count,
// the two tiers of k_huge_merge, the one-workgroup fallback k_digest_huge) at the inputs that steer it, under the CPU stand-in of the
// device model -- the table of tests/test_gpu_huge_edges.py (run lengths around a chunk and a sweep of the vector loop, runs at every
// residue from a 16-byte boundary, runs of equal values on either side of bin 16 383 | 16 384, tail counts around the two tiers'
// capacities, tail values split between buffer and run, every route in one batch, several pool rounds, a full and an overflowing
// global tail list).  Every case is one batch of one host through k_resp_host (+ its spill pass), the merges it queues and the
// large-key kernels; after it the path's own list lengths (large entries, entries handed to tier B, entries handed to the fallback)
// must be the ones the table states, and every key's digest, buffered values, records, CONN_BITMAP rows and min / max must equal the
// oracle's sequential engine fed the same bytes.  Also built with -fsanitize=address (tests/test_kernel_logic_huge_edges_cpu.py): the
// run area, the bin pool, the tail list and the lists are heap arrays of exactly the engine's sizes.
// Usage: test_huge_edges SEED PART, PART = lengths | values | tails | routes | taillist (the parts run side by side).
// Differences from the engine: the buffer holds 960 words (td_pend_cap 896), there is no streamed size class (a key of 4 097 .. 16 384
// values would take this path too; the table has none), runs are always exact (no predicted runs), workgroups run one after the other.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../../gyeeta_amd/csrc/gys_huge.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <string>

#include "../../../oracle/gy_oracle.h"

extern "C" {
struct gyo_engine;
gyo_engine *gyo_engine_new(uint32_t max_services, int enable_td);
void gyo_engine_free(gyo_engine *e);
int gyo_engine_register(gyo_engine *e, uint32_t host_slot, uint64_t glob_id, uint32_t netns, uint16_t port);
void gyo_engine_resp_batch(gyo_engine *e, const uint8_t *ev24, uint64_t n, const uint32_t *seg_host, const uint64_t *seg_first, uint32_t nsegs);
const gyo_hist_serial *gyo_engine_hist(const gyo_engine *e);
const uint16_t *gyo_engine_bitmap(const gyo_engine *e);
void gyo_engine_window_clear(gyo_engine *e, int clear_hist);
const gyo_td_buffered *gyo_engine_td(const gyo_engine *e, uint32_t slot);
const uint64_t *gyo_engine_counters(const gyo_engine *e);
}

#ifndef KEMU_TAIL_CAP
#define KEMU_TAIL_CAP GYS_HB_TAIL_CAP
#endif

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
uint16_t bswap(uint16_t v) { return (uint16_t)((v >> 8) | (v << 8)); }

using Vals = std::vector<uint32_t>;
struct Case {
	std::string name;
	std::vector<std::pair<uint32_t, Vals>> keys; // service, its latencies in this batch
	bool close_before = false;                   // a window closes before the batch
	uint32_t maxent = 0;                         // pool entries (0: room for every service -- one round)
	int huge = -1, tier_b = -1, fallback = -1;   // expected list lengths (-1: not looked at)
	int tail_values = -1;                        // expected fill of the global tail list
};

std::mt19937 rng;
constexpr uint32_t BINS = GYS_HB_BINS, CHUNK = GYS_HB_CHUNK, TA = GYS_HB_TAIL_A, TB = GYS_HB_TAIL_LDS, LARGE = BINS + 1u, SWEEP = 1024u * GYS_HB_VEC * 4u;

Vals low(uint32_t n) // below GYS_HB_BINS: a lognormal body and both edge bins
{
	std::lognormal_distribution<double> ln(4.0, 1.6);
	Vals v(n);
	for (auto &x : v) x = (uint32_t)std::min(std::floor(ln(rng)), (double)(BINS - 1u));
	if (n > 0) v[0] = 0;
	if (n > 1) v[1] = BINS - 1u;
	return v;
}
Vals tail(uint32_t n) // at or above GYS_HB_BINS: a third from a narrow range just above the last bin (ties), the rest up to 10^6, both ends
{
	Vals v(n);
	for (auto &x : v) x = rng() % 3u == 0 ? BINS + rng() % (1u + n / 8u) : BINS + rng() % (1000001u - BINS);
	if (n > 0) v[0] = 1000000u;
	if (n > 1) v[1] = BINS;
	return v;
}
Vals cat(Vals a, const Vals &b)
{
	a.insert(a.end(), b.begin(), b.end());
	return a;
}
void route(Case &c, uint32_t T) // one large key with T tail values, by the rule in the source
{
	c.huge = 1;
	c.tier_b = T > TA ? 1 : 0;
	c.fallback = T > TB ? 1 : 0;
	c.tail_values = (int)T;
}
} // namespace

int main(int argc, char **argv)
{
	setvbuf(stdout, nullptr, _IOLBF, 0); // (a failed route check is on record even if a later kernel then runs off its arrays)
	if (!kemu::can_run(1024u)) {
		printf("kemu: this process cannot have 1024 threads\n");
		return 77;
	}
	rng.seed(argc > 1 ? (unsigned)atoi(argv[1]) : 4100u);
	const std::string part = argc > 2 ? argv[2] : "routes";
	constexpr uint32_t TPT = 16, T = GYS_RESP_THREADS(TPT), TILE = TPT * T;
	const uint32_t tail_cap = KEMU_TAIL_CAP, NK = tail_cap / TB; // keys of TB tail values that fill the global tail list exactly
	const uint32_t nsvc = std::max(16u, NK + 1u), pcap = GYS_TD_PEND_CAP + 64u;

	// ---- the table
	std::vector<Case> cases;
	if (part == "lengths") {
		// T = 0, empty buffer: the smallest large key, one chunk, a second chunk of 1 .. 7 values, of one and of two sweeps give or take, a third chunk
		std::vector<uint32_t> lens = {LARGE, CHUNK, CHUNK + 1, CHUNK + 3, CHUNK + 4, CHUNK + 5, CHUNK + 7, 2 * CHUNK + 3};
		for (uint32_t k = 1; k <= 2; ++k)
			for (int d : {-1, 0, 1, 7}) lens.push_back(CHUNK + k * SWEEP + (uint32_t)d);
		for (size_t i = 0; i < lens.size(); ++i) {
			Case c;
			c.name = "run of " + std::to_string(lens[i]);
			c.keys.push_back({(uint32_t)(i % 6), low(lens[i])});
			route(c, 0);
			cases.push_back(c);
		}
		// three large keys of lengths = 1 resp. 3 (mod 4): the bump cursor starts at 0 in every batch, so their runs start at residues {0, 1, 2} resp. {0, 3, 2}
		for (uint32_t mod4 : {1u, 3u}) {
			Case c;
			c.name = "three runs of lengths = " + std::to_string(mod4) + " (mod 4)";
			const uint32_t l3[3] = {LARGE + mod4 - 1u, CHUNK + 4u + mod4, LARGE + 4u + mod4 - 1u};
			for (uint32_t s = 0; s < 3; ++s) c.keys.push_back({6u + s, cat(low(l3[s] - 40u * (s + 1)), tail(40u * (s + 1)))});
			c.huge = 3, c.tier_b = 0, c.fallback = 0, c.tail_values = 240;
			cases.push_back(c);
		}
	} else if (part == "values") {
		auto asc = [](uint32_t m) {
			Vals v(m);
			for (uint32_t i = 0; i < m; ++i) v[i] = std::min(i, 1000000u);
			return v;
		};
		std::vector<std::pair<std::string, Vals>> vc = {
			{"all 16383", Vals(LARGE, BINS - 1u)},
			{"all 16384", Vals(LARGE, BINS)},
			{"all 0", Vals(LARGE, 0u)},
			{"all 1000000", Vals(LARGE, 1000000u)},
			{"ascending, T in tier A", asc(BINS + 416u)},
			{"ascending, T in tier B", asc(20000u)},
			{"ascending, clipped to 10^6", asc(1000003u)},
			{"half 16383, half 16384", cat(Vals(8193u, BINS - 1u), Vals(8193u, BINS))},
			{"equal tail values in tier A", cat(low(LARGE - 400u), Vals(400u, BINS))},
			{"equal tail values in tier B", cat(low(LARGE - 5000u), Vals(5000u, BINS))},
			{"two equal tail values, the rest 16383", cat(Vals(LARGE, BINS - 1u), Vals(2u, BINS + 7u))},
		};
		for (size_t i = 0; i < vc.size(); ++i) {
			Case c;
			c.name = vc[i].first;
			c.keys.push_back({(uint32_t)(i % 8), vc[i].second});
			route(c, (uint32_t)std::count_if(vc[i].second.begin(), vc[i].second.end(), [](uint32_t v) { return v >= BINS; }));
			cases.push_back(c);
		}
	} else if (part == "tails") {
		// T tail values and L others, twice in a row on a fresh key: into an empty digest, then into one with clusters above 16 384
		const uint32_t tc[12][2] = {{0, LARGE}, {1, LARGE - 1}, {TA - 1, LARGE - TA + 1}, {TA, LARGE - TA}, {TA + 1, LARGE - TA - 1}, {1023, LARGE - 1023}, {1024, LARGE - 1024},
					    {1025, LARGE - 1025}, {TB - 1, 2}, {TB, 1}, {TB + 1, 1}, {LARGE, 0}};
		for (uint32_t k = 0; k < 12; ++k)
			for (int rep = 0; rep < 2; ++rep) {
				Case c;
				c.name = "T = " + std::to_string(tc[k][0]) + ", L = " + std::to_string(tc[k][1]) + (rep ? " (again)" : "");
				c.keys.push_back({k, cat(low(tc[k][1]), tail(tc[k][0]))});
				c.keys.push_back({12u, low(50)});
				route(c, tc[k][0]);
				cases.push_back(c);
			}
	} else if (part == "routes") {
		// 300 tail values wait in the buffer, a run brings 212 (512: tier A) resp. 213 (513: tier B) more; then the same with a window close in between
		for (uint32_t w = 0; w < 2; ++w) {
			Case pre;
			pre.name = "300 buffered tail values";
			pre.keys = {{4 * w, tail(300)}, {4 * w + 1, tail(300)}, {4 * w + 2, low(300)}};
			pre.huge = 0;
			cases.push_back(pre);
			for (uint32_t k = 0; k < 2; ++k) {
				const uint32_t t = TA - 300u + k;
				Case c;
				c.name = "buffer 300 + run " + std::to_string(t) + (w ? ", window closed in between" : "");
				c.keys = {{4 * w + k, cat(low(LARGE - t), tail(t))}, {4 * w + 2, low(10)}};
				c.close_before = w == 1 && k == 0;
				route(c, 300u + t);
				c.tail_values = (int)t; // (the list holds the run's share)
				cases.push_back(c);
			}
		}
		// the tail values all wait in the buffer (two batches of 300 and 212 resp. 213 stay buffered), the run brings none: the buffered words' own bound
		for (uint32_t step = 0; step < 2; ++step) {
			Case pre;
			pre.name = "buffered tail values, part " + std::to_string(step);
			pre.keys = {{14, tail(step ? TA - 300u : 300u)}, {15, tail(step ? TA - 300u + 1u : 300u)}};
			pre.huge = 0;
			cases.push_back(pre);
		}
		for (uint32_t k = 0; k < 2; ++k) {
			Case c;
			c.name = "buffer " + std::to_string(TA + k) + " + run 0";
			c.keys = {{14 + k, low(LARGE)}};
			route(c, TA + k);
			c.tail_values = 0;
			cases.push_back(c);
		}
		for (int rep = 0; rep < 2; ++rep) { // every route in one batch, next to a key that spills without being large and one that only appends
			Case c;
			c.name = "mixed batch";
			c.keys = {{8, low(LARGE + 2)}, {9, cat(low(LARGE), tail(1))}, {10, cat(low(17000), tail(600))}, {11, cat(low(9), tail(TB + 1))}, {12, low(pcap + 38)}, {13, low(100)}};
			c.huge = 4, c.tier_b = 2, c.fallback = 1, c.tail_values = 1 + 600 + (int)TB + 1;
			cases.push_back(c);
		}
		for (int rep = 0; rep < 2; ++rep) { // a pool of two entries, five large keys: three rounds
			Case c;
			c.name = "pool rounds";
			for (uint32_t s = 0; s < 4; ++s) c.keys.push_back({s, cat(low(LARGE + 3 * s), tail(5 * s))});
			c.keys.push_back({4, cat(low(LARGE), tail(600))});
			c.keys.push_back({5, low(70)});
			c.maxent = 2;
			c.huge = 5, c.fallback = 0;
			cases.push_back(c);
		}
	} else if (part == "taillist") {
		// NK keys of GYS_HB_TAIL_LDS tail values fill the list to its last place (nothing lost: all go through tier B); one tail value more
		// in the round and every entry takes the fallback
		Case c;
		c.name = "tail list full";
		for (uint32_t s = 0; s < NK; ++s) c.keys.push_back({s, cat(low(1), tail(TB))});
		c.huge = (int)NK, c.tier_b = (int)NK, c.fallback = 0, c.tail_values = (int)tail_cap;
		cases.push_back(c);
		c.name = "tail list lost";
		c.keys.push_back({NK, cat(low(BINS), tail(1))});
		c.huge = (int)NK + 1, c.tier_b = 0, c.fallback = (int)NK + 1, c.tail_values = (int)tail_cap + 1;
		cases.push_back(c);
	} else {
		printf("unknown part %s\n", part.c_str());
		return 2;
	}

	// ---- registration: one host, nsvc services
	gyo_engine *orc = gyo_engine_new(nsvc + 8, 1);
	gyo_engine *orcw = gyo_engine_new(nsvc + 8, 0); // the same stream with the records cleared at every window roll: what hist_win / CONN_BITMAP must show
	uint32_t cap = 1;
	while (cap < 2 * nsvc) cap <<= 1;
	std::vector<HostDesc> hdesc(1, HostDesc{0u, cap - 1, nsvc, 0u});
	std::vector<uint64_t> htbl(cap, GYS_HOST_TBL_EMPTY);
	std::vector<uint32_t> hlst, svc_host(nsvc, 0);
	const uint32_t netns = 0xF0000000u;
	for (uint32_t s = 0; s < nsvc; ++s) {
		const uint16_t port = (uint16_t)(1024 + s);
		gyo_engine_register(orc, 0, 0x100000ull + s, netns, port);
		gyo_engine_register(orcw, 0, 0x100000ull + s, netns, port);
		const uint64_t key48 = ((uint64_t)netns << 16) | port;
		uint32_t at = host_tbl_slot(host_tbl_hash(key48), cap - 1);
		while (htbl[at] != GYS_HOST_TBL_EMPTY) at = (at + 1) & (cap - 1);
		htbl[at] = (key48 << 16) | s;
		hlst.push_back(s);
	}

	// ---- engine state (the pools have the engine's sizes: a bin array per entry, a tail list of GYS_HB_TAIL_CAP places)
	std::vector<int64_t> td_sum((size_t)nsvc * GYS_TD_NB, 0);
	std::vector<uint32_t> td_cnt((size_t)nsvc * GYS_TD_NB, 0), td_pend((size_t)nsvc * pcap, 0), td_cur(nsvc + 64, 0), td_run(nsvc, 0), staged(1u << 21, 0), bitmap((size_t)nsvc * GYS_BM_WORDS, 0),
		hll32(1u << GYS_HLL_P, 0), resp_win(nsvc, 0), host_spill(1, 0), counts(FIN_NWORDS, 0);
	std::vector<TdMeta> meta(nsvc, TdMeta{0, 0, 0, 0, 0});
	std::vector<int2> minmax(nsvc, make_int2(INT32_MAX, INT32_MIN));
	std::vector<gys_hist_rec> hist_all(nsvc), hist_win(nsvc);
	for (auto *hv : {&hist_all, &hist_win})
		for (auto &r : *hv) {
			memset(&r, 0, sizeof(r));
			r.max_val_seen = INT64_MIN;
		}
	std::vector<MergeEnt> list0(nsvc + 1), list1(nsvc + 1), list2(nsvc + 1), listh(nsvc + 1), slow(nsvc + 1), fb(nsvc + 1);
	std::vector<uint64_t> counters(CTR_NUM, 0);
	std::vector<unsigned long long> ghist(32, 0);
	long long gmax = INT64_MIN;
	std::vector<uint32_t> scratch(GYS_HUGE_BINS, 0);
	std::vector<unsigned long long> tail_list(tail_cap);
	uint32_t residues = 0; // bit r: a large key's run started r words behind a 16-byte boundary

	uint32_t stamp = 0, epoch = 1;
	for (const Case &cs : cases) {
		if (cs.close_before) {
			++epoch;
			gyo_engine_window_clear(orc, 0);
			gyo_engine_window_clear(orcw, 1);
			std::fill(hll32.begin(), hll32.end(), 0u);
		}
		// ---- the batch: the keys' events shuffled together
		std::vector<std::pair<uint32_t, uint32_t>> sv;
		for (auto &k : cs.keys)
			for (uint32_t v : k.second) sv.push_back({k.first, v});
		std::shuffle(sv.begin(), sv.end(), rng);
		const uint64_t n = sv.size();
		std::vector<uint64_t> ev64(n * 3);
		for (uint64_t i = 0; i < n; ++i) {
			uint32_t w[6];
			w[0] = 0x0A000000u | (rng() & 0xFFFFFFu);
			w[1] = 0x0B000000u | (rng() & 0xFFFFu);
			w[2] = netns;
			const uint16_t sport = (uint16_t)(1024 + sv[i].first), dport = (uint16_t)(20000 + (rng() % 3000));
			w[3] = (uint32_t)bswap(sport) | ((uint32_t)bswap(dport) << 16);
			const uint32_t lrcv = rng();
			w[4] = lrcv + sv[i].second;
			w[5] = lrcv;
			memcpy(&ev64[i * 3], w, 24);
		}
		const uint32_t seg_host = 0;
		const uint64_t seg_first = 0;
		gyo_engine_resp_batch(orc, (const uint8_t *)ev64.data(), n, &seg_host, &seg_first, 1);
		gyo_engine_resp_batch(orcw, (const uint8_t *)ev64.data(), n, &seg_host, &seg_first, 1);

		// ---- event pass, spill pass
		std::fill(counts.begin(), counts.begin() + FIN_BATCH_CLEARED, 0u); // (what the engine clears per batch; the other words are k_huge_plan's)
		gys_resp_seg seg{0u, 0u, 0u};
		FinP fin{};
		fin.td_cur = td_cur.data();
		fin.td_meta = meta.data();
		fin.nsvc = nsvc;
		fin.pcap = pcap;
		fin.pend_cap = GYS_TD_PEND_CAP;
		fin.merge_fast = GYS_TDIGEST_MERGE_FAST;
		fin.epoch = epoch;
		fin.resp_win = resp_win.data();
		fin.list[FIN_CLASS0] = list0.data();
		fin.list[FIN_CLASS1] = list1.data();
		fin.list[FIN_CLASS2] = list2.data();
		fin.list[FIN_HUGE] = listh.data();
		fin.counts = counts.data();
		fin.td_run = td_run.data();
		fin.svc_host = svc_host.data();
		fin.host_spill = host_spill.data();
		fin.spill_stamp = ++stamp;
		fin.counters = counters.data();
		fin.staged_cap = (uint32_t)staged.size();
		RespHostP hp{};
		hp.ev = ev64.data();
		hp.n = n;
		hp.segs = &seg;
		hp.nsegs = 1;
		hp.hdesc = hdesc.data();
		hp.htbl = htbl.data();
		hp.hlst = hlst.data();
		hp.hll32 = hll32.data();
		hp.td_cur = td_cur.data();
		hp.td_pend = td_pend.data();
		hp.pcap = pcap;
		hp.td_run = td_run.data();
		hp.staged = staged.data();
		hp.host_spill = host_spill.data();
		hp.spill_stamp = stamp;
		hp.counters = counters.data();
		hp.ghist = ghist.data();
		hp.gmax = &gmax;
		hp.lds_tbl_entries = cap;
		hp.lds_key_entries = (nsvc + 1u) & ~1u;
		hp.fin = fin;
		const size_t dyn = resp_host_lds_bytes(cap, hp.lds_key_entries, TILE);
		kemu::launch(1, T, dyn, [&] { k_resp_host<TPT, false, false, false>(hp); });
		CHECK(counts[FIN_RUN_ALLOC] <= staged.size(), "run area too small");
		if (host_spill[0] == stamp) kemu::launch(1, T, dyn, [&] { k_resp_host<TPT, true, true, false>(hp); });

		// ---- the queued merges (launches whose list is empty are left out: an empty launch only costs threads here)
		MergeBP q{};
		q.d.td_sum = td_sum.data();
		q.d.td_cnt = td_cnt.data();
		q.d.td_meta = meta.data();
		q.d.td_minmax = minmax.data();
		q.d.td_pend = td_pend.data();
		q.d.td_cur = td_cur.data();
		q.d.pcap = pcap;
		q.d.pend_cap = GYS_TD_PEND_CAP;
		q.d.nsvc = nsvc;
		q.d.staged = staged.data();
		q.d.hist_win = hist_win.data();
		q.d.hist_all = hist_all.data();
		q.d.bitmap = bitmap.data();
		q.list = list0.data();
		q.count = &counts[FIN_CLASS0];
		q.slow_list = slow.data();
		q.slow_count = &counts[FIN_SLOW];
		std::vector<uint32_t> merged;
		for (uint32_t i = 0; i < counts[FIN_CLASS0]; ++i) merged.push_back(list0[i].slot);
		for (uint32_t i = 0; i < counts[FIN_CLASS1]; ++i) merged.push_back(list1[i].slot);
		for (uint32_t i = 0; i < counts[FIN_HUGE]; ++i) merged.push_back(listh[i].slot);
		if (counts[FIN_CLASS0]) kemu::launch(1, 256, 0, [&] { k_digest_bins<false>(q); });
		CHECK(counts[FIN_SLOW] == 0, "hand-over list not empty");
		if (counts[FIN_CLASS1]) {
			MergeP mp{};
			mp.d = q.d;
			mp.list = list1.data();
			mp.count = &counts[FIN_CLASS1];
			kemu::launch(1, 256, 0, [&] { k_digest_merge<GYS_MERGE_CLASS1, 256u>(mp); });
		}
		const uint32_t nhuge = counts[FIN_HUGE];
		if (cs.huge >= 0) CHECK((int)nhuge == cs.huge, "%s: %u large entries, want %d", cs.name.c_str(), nhuge, cs.huge);
		if (nhuge) {
			const uint32_t maxent = cs.maxent ? cs.maxent : nsvc;
			std::vector<uint32_t> hbins((size_t)maxent * GYS_HB_BINS), hbm((size_t)maxent * GYS_BM_WORDS), chunk_off(maxent + 1), tb(maxent);
			std::vector<unsigned long long> hacc((size_t)maxent * GYS_HB_ACC);
			for (uint32_t i = 0; i < nhuge; ++i) residues |= 1u << (((uintptr_t)(staged.data() + (listh[i].off_end - listh[i].mrun)) >> 2) & 3u);
			Huge2P hq{};
			hq.d = q.d;
			hq.list = listh.data();
			hq.count = &counts[FIN_HUGE];
			hq.bins = hbins.data();
			hq.acc = hacc.data();
			hq.bm = hbm.data();
			hq.chunk_off = chunk_off.data();
			hq.tail = tail_list.data();
			hq.tail_count = &counts[FIN_HUGE_TAIL];
			hq.tail_cap = tail_cap;
			hq.maxent = maxent;
			hq.fb_list = fb.data();
			hq.fb_count = &counts[FIN_HUGE_FB];
			hq.nent_used = &counts[FIN_HUGE_NENT];
			hq.tb_list = tb.data();
			hq.tb_count = &counts[FIN_HUGE_TB];
			for (uint32_t first = 0; first < nhuge; first += maxent) {
				hq.first = first;
				kemu::launch(1, 1024, 0, [&] { k_huge_plan(hq); });
				kemu::launch(1, 256, 0, [&] { k_huge_clear(hq); });
				kemu::launch(2, 1024, GYS_HB_BINS * 4, [&] { k_huge_count(hq); }); // (two workgroups: a long run's chunks are shared out)
				kemu::launch(1, 512, (GYS_HB_BINS + GYS_HB_TAIL_A) * 4, [&] { k_huge_merge<512, GYS_HB_TAIL_A, false>(hq); });
				if (counts[FIN_HUGE_TB]) kemu::launch(1, 1024, (GYS_HB_BINS + GYS_HB_TAIL_LDS) * 4, [&] { k_huge_merge<1024, GYS_HB_TAIL_LDS, true>(hq); });
			}
			if (cs.tier_b >= 0) CHECK((int)counts[FIN_HUGE_TB] == cs.tier_b, "%s: %u entries handed to tier B, want %d", cs.name.c_str(), counts[FIN_HUGE_TB], cs.tier_b);
			if (cs.fallback >= 0) CHECK((int)counts[FIN_HUGE_FB] == cs.fallback, "%s: %u entries handed to the fallback, want %d", cs.name.c_str(), counts[FIN_HUGE_FB], cs.fallback);
			if (cs.tail_values >= 0) CHECK((int)counts[FIN_HUGE_TAIL] == cs.tail_values, "%s: tail list fill %u, want %d", cs.name.c_str(), counts[FIN_HUGE_TAIL], cs.tail_values);
			if (counts[FIN_HUGE_FB]) {
				HugeP hf{};
				hf.d = q.d;
				hf.huge_list = fb.data();
				hf.huge_count = &counts[FIN_HUGE_FB];
				hf.scratch = scratch.data();
				kemu::launch(1, 256, 0, [&] { k_digest_huge(hf); });
			}
		}

		// ---- compare with the oracle
		const char *nm = cs.name.c_str();
		const uint64_t *oc = gyo_engine_counters(orc);
		CHECK(counters[CTR_RESP_EVENTS] == oc[0] && counters[CTR_RESP_DROP_RANGE] == oc[1] && counters[CTR_RESP_DROP_NOLISTENER] == oc[2], "%s: counters", nm);
		const gyo_hist_serial *oh = gyo_engine_hist(orc);
		for (uint32_t s = 0; s < nsvc; ++s) {
			const gyo_td_buffered *ot = gyo_engine_td(orc, s);
			CHECK(meta[s].npend == ot->npend && td_cur[s] == ot->npend, "%s: key %u buffered %u (cur %08x) want %u", nm, s, meta[s].npend, td_cur[s], ot->npend);
			if (meta[s].npend == ot->npend) {
				std::vector<int32_t> a(ot->npend), b(ot->pend, ot->pend + ot->npend);
				for (uint32_t i = 0; i < ot->npend; ++i) a[i] = (int32_t)(td_pend[(size_t)s * pcap + i] >> GYS_ROW_BITS);
				std::sort(a.begin(), a.end());
				std::sort(b.begin(), b.end());
				CHECK(a == b, "%s: key %u: buffered values differ", nm, s);
			}
			for (int j = 0; j < GYS_TD_NB; ++j)
				CHECK(td_sum[(size_t)s * GYS_TD_NB + j] == ot->d.sum[j] && td_cnt[(size_t)s * GYS_TD_NB + j] == ot->d.cnt[j], "%s: key %u cluster %d: {%lld, %u} want {%lld, %u}", nm, s, j,
				      (long long)td_sum[(size_t)s * GYS_TD_NB + j], td_cnt[(size_t)s * GYS_TD_NB + j], (long long)ot->d.sum[j], ot->d.cnt[j]);
		}
		for (uint32_t s : merged) { // (a key that was just merged has everything folded: its records are complete)
			for (int b = 0; b < 15; ++b)
				CHECK(hist_all[s].stats[b].count == oh[(size_t)s * 16 + b].count && hist_all[s].stats[b].sum == oh[(size_t)s * 16 + b].sum, "%s: key %u all-time bucket %d: {%llu, %lld} want {%llu, %lld}", nm,
				      s, b, (unsigned long long)hist_all[s].stats[b].count, (long long)hist_all[s].stats[b].sum, (unsigned long long)oh[(size_t)s * 16 + b].count, (long long)oh[(size_t)s * 16 + b].sum);
			CHECK(hist_all[s].total_count == oh[(size_t)s * 16 + 15].count && hist_all[s].max_val_seen == oh[(size_t)s * 16 + 15].sum, "%s: key %u all-time total / max", nm, s);
			const gyo_hist_serial *ow = gyo_engine_hist(orcw) + (size_t)s * 16;
			const uint16_t *ob = gyo_engine_bitmap(orcw) + (size_t)s * 64;
			const bool cur = meta[s].hw_epoch == epoch;
			for (int b = 0; b < 15; ++b) {
				const unsigned long long gc = cur ? hist_win[s].stats[b].count : 0ull;
				const long long gs = cur ? hist_win[s].stats[b].sum : 0ll;
				CHECK(gc == ow[b].count && gs == ow[b].sum, "%s: key %u window bucket %d: {%llu, %lld} want {%llu, %lld}", nm, s, b, gc, gs, (unsigned long long)ow[b].count, (long long)ow[b].sum);
			}
			CHECK((cur ? hist_win[s].total_count : 0ull) == ow[15].count && (cur ? hist_win[s].max_val_seen : INT64_MIN) == ow[15].sum, "%s: key %u window total / max", nm, s);
			for (int g = 0; g < (int)GYS_BM_WORDS; ++g) {
				const uint32_t want = (uint32_t)ob[2 * g] | ((uint32_t)ob[2 * g + 1] << 16);
				CHECK((cur ? bitmap[(size_t)s * GYS_BM_WORDS + g] : 0u) == want, "%s: key %u CONN_BITMAP rows %d, %d: %08x want %08x", nm, s, 2 * g, 2 * g + 1, cur ? bitmap[(size_t)s * GYS_BM_WORDS + g] : 0u, want);
			}
			const gyo_td_buffered *ot = gyo_engine_td(orc, s);
			CHECK(minmax[s].x == ot->d.vmin && minmax[s].y == ot->d.vmax, "%s: key %u min/max {%d, %d} want {%d, %d}", nm, s, minmax[s].x, minmax[s].y, ot->d.vmin, ot->d.vmax);
		}
	}
	if (part == "lengths") CHECK(residues == 15u, "run residues reached: mask %x, want all four", residues);
	gyo_engine_free(orc);
	gyo_engine_free(orcw);
	if (fails) {
		printf("%d checks failed\n", fails);
		return 1;
	}
	printf("kemu huge edges ok (%s: %zu batches, run residues reached: mask %x)\n", part.c_str(), cases.size(), residues);
	return 0;
}
