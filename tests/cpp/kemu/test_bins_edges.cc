// TEST INFRASTRUCTURE (CPU): k_digest_bins (gyeeta_amd/csrc/gys_kernels.hpp) at the edges of its phases, ONE workgroup walking the whole list
// (every barrier of an entry is followed by the next entry's clears and loads: the loop-carried order of the write-back), under the CPU
// stand-in of the device model and against the oracle (gyo_td_merge_values, the record fold written out below as in test_bins.cc):
//   - the list of non-empty one-value bins that the bin scan writes: 0, 1, 256, 257 and 1 024 entries;
//   - 512 / 513 large values (the compact list / the plain form), more than the large-value list holds (hand-over);
//   - the values 0, 1023, 1024, 1087, 1088, 999 999, 1 000 000; keys without old clusters and with old clusters on both sides of 1024;
//   - part of the buffer folded / of an earlier window, a run in `staged`, the 64-bit-weight hand-over, an entry with m == 0 between two others.
// First of all mb_bin (the float-conversion form) against the bit formula written out here, for every value below 2^20.
// Build + run: tests/test_merge_kernel_edges_cpu.py (-DKEMU_BINS_VPT=4 / 8 / 64; once more with -fsanitize=address,undefined).
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

// what the key is there for
enum Shape {
	ALL_BIG_512,   // no one-value bin holds a value; 512 large values: the compact side of the choice, the list's room exactly used
	ONE_BIN,       // one non-empty one-value bin
	BINS_256,      // 256 non-empty one-value bins: the list is exactly one round of the workgroup
	BINS_257,      // 257: one bin in the second round
	BINS_1024,     // every one-value bin holds a value (0 and 1023 among them): the list is full
	BIG_513,       // 513 large values: the plain side of the choice
	BIG_OVER,      // more large values than the list holds: handed over (instances whose merges can hold that many)
	EDGE_VALUES,   // 0, 1023, 1024, 1087, 1088, 999 999, 1 000 000, each several times, and random ones between
	FOLDED_PART,   // nh > 0 and nw > 0
	STAGED_RUN,    // a third of the values arrive through a run in `staged`
	WEIGHT_64,     // total weight beyond 2^31: handed over
	EMPTY,         // m == 0: nothing to do, between two ordinary entries
	RANDOM,
};
struct Spec {
	Shape shape;
	int old; // 0: no old clusters, 1: old clusters below 1024 only, 2: old clusters with thresholds on both sides of 1024
};

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
	// ---- mb_bin against the formula it replaced
	for (uint32_t v = 0; v < (1u << 20); ++v) {
		uint32_t want = v;
		if (v >= 1024u) {
			const uint32_t msb = 31u - (uint32_t)__builtin_clz(v);
			want = 1024u + (msb - 10u) * 64u + ((v >> (msb - 6u)) & 63u);
		}
		CHECK(mb_bin(v) == want && mb_bin_clz(v) == want, "mb_bin(%u) = %u / %u, want %u", v, mb_bin(v), mb_bin_clz(v), want);
		CHECK(want < GYS_MB_BINS, "bin %u of value %u", want, v);
	}
	printf("mb_bin: every value below 2^20\n");

	const uint32_t CAP = (uint32_t)KEMU_BINS_VPT * NT;
	const uint32_t pcap = CAP + 64u;
	std::mt19937 rng(argc > 1 ? (unsigned)atoi(argv[1]) : 4711u);
	std::vector<Spec> specs;
	for (int old = 0; old < 3; ++old) {
		for (Shape sh : {ALL_BIG_512, ONE_BIN, BINS_256, EMPTY, BINS_257, BINS_1024, BIG_513, EDGE_VALUES, FOLDED_PART, STAGED_RUN, RANDOM}) specs.push_back(Spec{sh, old});
		specs.push_back(Spec{BIG_OVER, old});
	}
	specs.insert(specs.begin() + 5, Spec{WEIGHT_64, 1});
	specs.push_back(Spec{ONE_BIN, 2}); // (an ordinary entry behind the last hand-over)
	const uint32_t S = (uint32_t)specs.size();
	std::vector<Key> keys(S);
	std::vector<int64_t> td_sum((size_t)S * GYS_TD_NB, 0);
	std::vector<uint32_t> td_cnt((size_t)S * GYS_TD_NB, 0), td_pend((size_t)S * pcap, 0xDEADBEEFu), td_cur(S, 0), staged(1u << 18, 0), bitmap((size_t)S * GYS_BM_WORDS, 0);
	std::vector<TdMeta> meta(S);
	std::vector<int2> minmax(S);
	std::vector<gys_hist_rec> hist_all(S), hist_win(S);
	std::vector<MergeEnt> list(S), slow(S + 1);
	std::vector<bool> handed(S, false);
	uint32_t count = S, slow_count = 0, staged_used = 0, want_slow = 0;

	for (uint32_t s = 0; s < S; ++s) {
		Key &k = keys[s];
		const Spec sp = specs[s];
		gyo_td_init(&k.d);
		gyo_hist_init(&k.all0, GYO_RESP_TIME_HASH);
		gyo_hist_init(&k.win0, GYO_RESP_TIME_HASH);
		memset(k.bm0, 0, sizeof(k.bm0));
		k.mn0 = INT32_MAX;
		k.mx0 = INT32_MIN;
		if (sp.shape == WEIGHT_64) {
			for (int j = 0; j < GYO_TD_NB; ++j) {
				k.d.cnt[j] = 17000000u;
				k.d.sum[j] = (int64_t)k.d.cnt[j] * (10 + j);
			}
			k.d.vmin = 10;
			k.d.vmax = 10 + GYO_TD_NB;
		} else if (sp.old) { // the key's history: merged and folded values -> old clusters (old == 2: about half of them above 1024)
			std::vector<int32_t> old(3000u + 511u * s);
			for (auto &v : old) {
				v = sp.old == 2 ? draw(rng, 6.9, 1.6) : std::min(draw(rng, 3.0, 1.2), 1023);
				gyo_hist_add(&k.all0, v);
				k.mn0 = std::min(k.mn0, v);
				k.mx0 = std::max(k.mx0, v);
			}
			gyo_td_merge_values(&k.d, old.data(), old.size());
		}
		// the values of the merge
		std::vector<int32_t> &v = k.vals;
		auto small = [&] { return (int32_t)(rng() % 1024u); };
		switch (sp.shape) {
		case ALL_BIG_512: for (int i = 0; i < 512; ++i) v.push_back(draw_big(rng)); break;
		case ONE_BIN: v.assign(300, 37); break;
		case BINS_256: for (int i = 0; i < 400; ++i) v.push_back(i < 256 ? 4 * i : 4 * (int)(rng() % 256u)); break; // (0 among them)
		case BINS_257: for (int i = 0; i < 300; ++i) v.push_back(i < 257 ? 3 * i + 200 : 3 * (int)(rng() % 257u) + 200); break;
		case BINS_1024: for (int i = 0; i < 1024; ++i) v.push_back((i * 389) % 1024); break; // (a permutation: every bin once)
		case BIG_513: for (int i = 0; i < 713; ++i) v.push_back(i % 3 == 1 && i / 3 < 200 ? small() : draw_big(rng)); break; // exactly 513 large values, 200 small ones
		case BIG_OVER: if (CAP >= 2048u) for (uint32_t i = 0; i < GYS_MB_BIG_CAP + 1u + 60u; ++i) v.push_back(i < GYS_MB_BIG_CAP + 1u ? draw_big(rng) : small()); else v.assign(50, 5); break;
		case EDGE_VALUES: {
			static const int32_t e[] = {0, 1023, 1024, 1087, 1088, 999999, 1000000};
			for (int i = 0; i < 600; ++i) v.push_back(i < 70 ? e[i % 7] : (i % 3 ? small() : draw_big(rng)));
			break;
		}
		case FOLDED_PART:
		case STAGED_RUN:
		case RANDOM: {
			const uint32_t m = sp.shape == RANDOM ? CAP : (uint32_t)(rng() % (CAP - 100u)) + 50u;
			for (uint32_t i = 0; i < m; ++i) v.push_back(draw(rng, 3.0 + 1.3 * sp.old, 1.5));
			break;
		}
		case WEIGHT_64: v.assign(100, 15); break;
		case EMPTY: break;
		}
		std::shuffle(v.begin(), v.end(), rng);
		uint32_t nbig = 0;
		for (int32_t x : v) nbig += x >= (int32_t)GYS_MB_EXACT ? 1u : 0u;
		if (sp.shape == ALL_BIG_512) CHECK(nbig == 512u && v.size() == 512u, "spec: %u large values", nbig);
		if (sp.shape == BIG_513) CHECK(nbig == 513u, "spec: %u large values", nbig);
		const uint32_t m = (uint32_t)v.size();
		CHECK(m <= CAP, "spec: key %u holds %u values", s, m);
		handed[s] = sp.shape == WEIGHT_64 || nbig > GYS_MB_BIG_CAP;
		want_slow += handed[s] ? 1u : 0u;
		k.mrun = sp.shape == STAGED_RUN ? m / 3u : 0u;
		k.nbuf = m - k.mrun;
		k.rows.resize(m);
		for (uint32_t i = 0; i < m; ++i) k.rows[i] = (uint32_t)(rng() & (s % 3 == 0 ? 31u : 63u));
		k.win_epoch = 7;
		k.nh = sp.shape == FOLDED_PART ? k.nbuf / 2u : 0u;
		k.nw = sp.shape == FOLDED_PART ? (sp.old == 1 ? k.nbuf / 4u : 2u * k.nbuf / 3u) : 0u; // (nw below and above nh)
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
	// the thresholds of an `old == 2` key lie on both sides of 1024
	for (uint32_t s = 0; s < S; ++s)
		if (specs[s].old == 2 && specs[s].shape != WEIGHT_64) {
			uint32_t lo = 0, hi = 0;
			for (int j = 0; j < GYO_TD_NB; ++j)
				if (keys[s].d.cnt[j]) (keys[s].d.sum[j] / (int64_t)keys[s].d.cnt[j] < 1024 ? lo : hi)++;
			CHECK(lo >= 4u && hi >= 4u, "spec: key %u has %u / %u old clusters below / above 1024", s, lo, hi);
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
	printf("kemu bins edges ok (one workgroup, %u entries, merges of up to %u values)\n", S, CAP);
	return 0;
}
