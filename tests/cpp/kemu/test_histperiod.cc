// TEST INFRASTRUCTURE (CPU): the LOGIC of the group-period kernel k_hist_period_union (gyeeta_amd/csrc/gys_histroll.hpp) under the CPU stand-in
// of the device model, on synthetic cumulative / window / boundary-snapshot / last-window / first-close records with their td_meta and tags:
//   * all four period modes (0 ring level, 1 empty, 2 the last-window record, 3 since start), each with lazily folded records (meta: some
//     services' open window partly folded) and with eagerly kept ones (no meta);
//   * mode 0 with nrb = 1, 2 and 10 overlapping ring buckets, all whole and partly covered, the last boundary a snapshot or the cumulative
//     record now; the ring buckets hold counts of 1 .. 9 and the scales are 0.3 .. 0.9, so the per-member truncation bites; mode 3 with
//     services that closed no window yet, that lie wholly inside the interval, partly, and outside it;
//   * chunks of 1, 15, 16, 17, 1023 and 1024 members, a group of three chunks (2100 members), an empty group, shuffled member lists with
//     repeats, several grid sizes, outputs pre-filled with garbage (no pre-zeroed output needed);
//   * expected: every chunk's partial record and every row's record equal a plain loop of period_pair_load / period_pair_value per member
//     (total_count = the sum of the member's 15 counts) followed by gyo_hist_merge, byte for byte; total_count of every result = the sum of its
//     counts; k_level_period, run on the same arrays, stores exactly the per-member records of that loop; and for the partly covered cases the
//     shortcut "scale the group's summed ring buckets" gives a different record (the test can tell the rule from the shortcut).
// Build + run: tests/test_kernel_logic_histperiod_cpu.py.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../../gyeeta_amd/csrc/gys_rollup.hpp"
#include "../../../gyeeta_amd/csrc/gys_histroll.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "../../../oracle/gy_oracle.h"

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

static_assert(sizeof(gys_hist_rec) == 256, "a record is 16 pairs of 16 bytes");
typedef std::vector<gys_hist_rec> Recs;
typedef unsigned long long u64;

gys_hist_rec empty_rec()
{
	gys_hist_rec r;
	memset(&r, 0, sizeof(r));
	((u64 *)&r)[31] = (u64)INT64_MIN;
	return r;
}

// a ring bucket's worth of adds: counts of 1 .. 9 (0 in some buckets), sums of count x a latency
gys_hist_rec delta_rec(std::mt19937_64 &rng)
{
	gys_hist_rec r;
	memset(&r, 0, sizeof(r));
	u64 *w = (u64 *)&r;
	for (int b = 0; b < 15; ++b) {
		w[2 * b] = rng() % 4 == 0 ? 0 : 1 + rng() % 9;
		w[2 * b + 1] = w[2 * b] * (1 + rng() % 5000);
		w[30] += w[2 * b];
	}
	return r;
}

void add_counts(gys_hist_rec &dst, const gys_hist_rec &src) // the cumulative record grows: counts, sums and the total
{
	u64 *d = (u64 *)&dst;
	const u64 *s = (const u64 *)&src;
	for (int i = 0; i < 31; ++i) d[i] += s[i];
}

void merge(gys_hist_rec &dst, const gys_hist_rec &src) // through the oracle's GY_HISTOGRAM::add_histogram
{
	gyo_hist a, b;
	gyo_hist_init(&a, GYO_RESP_TIME_HASH);
	gyo_hist_init(&b, GYO_RESP_TIME_HASH);
	const u64 *d = (const u64 *)&dst, *s = (const u64 *)&src;
	for (int i = 0; i < 15; ++i) {
		a.stats[i].count = d[2 * i];
		a.stats[i].sum = (int64_t)d[2 * i + 1];
		b.stats[i].count = s[2 * i];
		b.stats[i].sum = (int64_t)s[2 * i + 1];
	}
	a.total_count = d[30];
	a.max_val_seen = (int64_t)d[31];
	b.total_count = s[30];
	b.max_val_seen = (int64_t)s[31];
	u64 *o = (u64 *)&dst;
	gyo_hist_merge(&a, &b);
	for (int i = 0; i < 15; ++i) {
		o[2 * i] = a.stats[i].count;
		o[2 * i + 1] = (u64)a.stats[i].sum;
	}
	o[30] = a.total_count;
	o[31] = (u64)a.max_val_seen;
}

struct World {
	uint32_t nsvc;
	Recs bnd[GYS_PERIOD_MAXB + 1]; // C(boundary i): increasing
	Recs all, win, last;
	std::vector<TdMeta> meta;
	std::vector<uint32_t> tag;
	std::vector<int64_t> first_sec;
};

const int64_t T_NOW = 1700000400;

World make_world(std::mt19937_64 &rng, uint32_t nsvc, uint32_t epoch_open, uint32_t last_epoch)
{
	World w;
	w.nsvc = nsvc;
	for (auto &b : w.bnd) b.resize(nsvc);
	w.all.resize(nsvc);
	w.win.resize(nsvc);
	w.last.resize(nsvc);
	w.meta.resize(nsvc);
	w.tag.resize(nsvc);
	w.first_sec.resize(nsvc);
	for (uint32_t s = 0; s < nsvc; ++s) {
		gys_hist_rec c;
		memset(&c, 0, sizeof(c)); // (snapshots never written are zero)
		for (uint32_t i = 0; i <= GYS_PERIOD_MAXB; ++i) {
			if (i || s % 3) add_counts(c, delta_rec(rng));
			w.bnd[i][s] = c;
		}
		if (s % 13) add_counts(c, delta_rec(rng)); // the closes after the last boundary
		memset(&w.meta[s], 0, sizeof(TdMeta));
		w.meta[s].hw_epoch = s % 4 == 1 ? epoch_open : (s % 4 == 2 ? epoch_open - 1u : (uint32_t)(rng() % (epoch_open + 2u)));
		w.win[s] = s % 5 == 0 ? empty_rec() : delta_rec(rng);
		((u64 *)&w.win[s])[31] = (u64)(long long)(rng() % 9000);
		w.all[s] = c; // (with meta and hw_epoch == epoch_open the kernel takes win out again: for those services `all` is "too small" by win
		              //  in the eager reading and right in the lazy one after the add below)
		if (w.meta[s].hw_epoch == epoch_open) add_counts(w.all[s], w.win[s]);
		((u64 *)&w.all[s])[31] = s % 7 == 0 ? (u64)INT64_MIN : (u64)(long long)(rng() % 2000000);
		w.last[s] = delta_rec(rng);
		w.tag[s] = s % 3 == 0 ? last_epoch : (uint32_t)(rng() % (last_epoch + 2u));
		// mode 3, the interval [T_NOW - 300, T_NOW - 100): no close yet / the service's bucket inside the interval's reach or not
		const int64_t choices[] = {0, T_NOW - 1000, T_NOW - 250, T_NOW - 100, T_NOW - 50, T_NOW - 299, T_NOW - 301};
		w.first_sec[s] = choices[rng() % 7];
	}
	return w;
}

struct Case {
	const char *name;
	int mode;
	bool meta, tags;
	uint32_t nrb, whole_mask;
	bool tail_now;  // mode 0: the last boundary is the cumulative record now
	int64_t start, end; // mode 3
	bool truncates; // the shortcut must differ
};

LevelPeriodP period_params(const World &w, const Case &cs, uint32_t epoch_open, uint32_t last_epoch)
{
	LevelPeriodP p{};
	p.win = w.win.data();
	p.all = w.all.data();
	p.meta = cs.meta ? w.meta.data() : nullptr;
	p.epoch_open = epoch_open;
	p.mode = cs.mode;
	if (cs.mode == 0) {
		p.nrb = cs.nrb;
		p.whole_mask = cs.whole_mask;
		const uint32_t b0 = GYS_PERIOD_MAXB - cs.nrb; // the youngest nrb ring buckets
		for (uint32_t i = 0; i <= cs.nrb; ++i) p.bnd[i] = w.bnd[b0 + i].data();
		if (cs.tail_now) p.bnd[cs.nrb] = nullptr;
		for (uint32_t i = 0; i < cs.nrb; ++i) p.scale[i] = (cs.whole_mask >> i) & 1u ? 1.f : (float)(3 + (i * 2) % 7) / 10.f; // 0.3 .. 0.9
	} else if (cs.mode == 2) {
		p.last = w.last.data();
		p.last_tag = cs.tags ? w.tag.data() : nullptr;
		p.last_epoch = last_epoch;
	} else if (cs.mode == 3) {
		p.first_sec = w.first_sec.data();
		p.start = cs.start;
		p.end = cs.end;
		p.latest = T_NOW;
	}
	return p;
}

// the plain loop: one member's record by the shared rule
gys_hist_rec member_record(const LevelPeriodP &p, uint32_t slot)
{
	gys_hist_rec r;
	ulonglong2 *o = (ulonglong2 *)&r;
	u64 tot = 0;
	for (uint32_t k = 0; k < 16; ++k) {
		const PeriodPair in = period_pair_load<false>(p, slot, k);
		o[k] = period_pair_value(p, in, k);
		if (k < 15) tot += o[k].x;
	}
	o[15].x = tot;
	return r;
}

bool total_is_sum(const gys_hist_rec &r)
{
	const u64 *w = (const u64 *)&r;
	u64 t = 0;
	for (int b = 0; b < 15; ++b) t += w[2 * b];
	return t == w[30];
}

void test_case(std::mt19937_64 &rng, const World &w, const Case &cs, uint32_t epoch_open, uint32_t last_epoch)
{
	const LevelPeriodP base = period_params(w, cs, epoch_open, last_epoch);
	Recs view(w.nsvc);
	for (uint32_t s = 0; s < w.nsvc; ++s) view[s] = member_record(base, s);
	{ // k_level_period stores exactly these records (its own 16-lane total included)
		Recs got(w.nsvc + 1);
		memset(got.data(), 0xEE, got.size() * 256);
		LevelPeriodP v = base;
		v.first = 0;
		v.n = w.nsvc;
		v.out = got.data();
		kemu::launch((w.nsvc * 16u + 255u) / 256u, 256, 0, [=] { k_level_period(v); });
		CHECK(memcmp(got.data(), view.data(), (size_t)w.nsvc * 256) == 0, "%s: k_level_period differs from the plain loop of the rule", cs.name);
		CHECK(((const uint8_t *)&got[w.nsvc])[0] == 0xEE, "%s: k_level_period wrote past its output", cs.name);
	}
	const uint32_t sizes[] = {1, 15, 16, 17, 1023, 1024, 0, 2100};
	const uint32_t ng = sizeof(sizes) / sizeof(sizes[0]);
	std::vector<uint32_t> off(ng + 1, 0), members;
	for (uint32_t g = 0; g < ng; ++g) {
		for (uint32_t i = 0; i < sizes[g]; ++i) members.push_back((uint32_t)(rng() % w.nsvc)); // (shuffled, with repeats)
		off[g + 1] = (uint32_t)members.size();
	}
	std::vector<RollupChunk> chunks, gchunks;
	for (uint32_t g = 0; g < ng; ++g) {
		const uint32_t c0 = (uint32_t)chunks.size();
		for (uint32_t a = off[g]; a < off[g + 1]; a += 1024u) chunks.push_back(RollupChunk{g, a, std::min(off[g + 1], a + 1024u), 0u});
		gchunks.push_back(RollupChunk{g, c0, (uint32_t)chunks.size(), 0u});
	}
	CHECK(gchunks[ng - 1].m1 - gchunks[ng - 1].m0 == 3u && gchunks[ng - 2].m1 == gchunks[ng - 2].m0, "a group of three chunks and an empty group");
	Recs wantpart(chunks.size()), wantrow(ng);
	for (size_t ci = 0; ci < chunks.size(); ++ci) {
		wantpart[ci] = empty_rec();
		for (uint32_t a = chunks[ci].m0; a < chunks[ci].m1; ++a) merge(wantpart[ci], view[members[a]]);
	}
	for (uint32_t g = 0; g < ng; ++g) {
		wantrow[g] = empty_rec();
		for (uint32_t a = off[g]; a < off[g + 1]; ++a) merge(wantrow[g], view[members[a]]);
		CHECK(total_is_sum(wantrow[g]), "%s: total_count of group %u is not the sum of its counts", cs.name, g);
	}
	if (cs.mode == 0) {
		// the shortcut: the group's summed ring buckets, scaled once.  It must differ wherever the test claims that truncation bites.
		const uint32_t g = ng - 1, b0 = GYS_PERIOD_MAXB - cs.nrb;
		bool differs = false;
		for (int b = 0; b < 15 && !differs; ++b) {
			long long ac = 0;
			for (uint32_t i = 0; i < cs.nrb; ++i) {
				long long c = 0;
				for (uint32_t a = off[g]; a < off[g + 1]; ++a) {
					const uint32_t s = members[a];
					const PeriodPair in = period_pair_load<false>(base, s, (uint32_t)b);
					ulonglong2 cum = in.cum;
					if (base.meta && in.hw == base.epoch_open) cum.x -= in.w.x;
					const u64 hi = base.bnd[i + 1] ? ((const u64 *)&w.bnd[b0 + i + 1][s])[2 * b] : cum.x;
					c += (long long)(hi - ((const u64 *)&w.bnd[b0 + i][s])[2 * b]);
				}
				ac += (cs.whole_mask >> i) & 1u ? c : range_adjust(c, base.scale[i]);
			}
			differs = (u64)ac != ((const u64 *)&wantrow[g])[2 * b];
		}
		CHECK(differs == cs.truncates, "%s: scaling the group's summed ring buckets %s the per-member rule", cs.name, differs ? "differs from" : "equals");
	}
	for (uint32_t grid : {1u, 3u, 32u}) {
		Recs part(chunks.size() + 1), out(ng + 1);
		memset(part.data(), 0xEE, part.size() * sizeof(gys_hist_rec));
		memset(out.data(), 0xEE, out.size() * sizeof(gys_hist_rec)); // (no pre-zeroed output needed)
		HistPeriodUnionP q{};
		q.v = base;
		q.dst = part.data();
		q.chunks = chunks.data();
		q.members = members.data();
		q.nchunks = (uint32_t)chunks.size();
		kemu::launch(grid, GYS_HR_NT, 0, [=] { k_hist_period_union(q); });
		HistUnionP r{}; // the second stage: the existing plain mode of k_hist_level_union
		r.plain = 1;
		r.src = part.data();
		r.dst = out.data();
		r.chunks = gchunks.data();
		r.nchunks = ng;
		kemu::launch(grid, GYS_HR_NT, 0, [=] { k_hist_level_union(r); });
		for (size_t ci = 0; ci < chunks.size(); ++ci) {
			CHECK(memcmp(&part[ci], &wantpart[ci], 256) == 0, "%s grid %u: partial record of chunk %zu (group %u, %u members) differs", cs.name, grid, ci, chunks[ci].group,
			      chunks[ci].m1 - chunks[ci].m0);
			CHECK(total_is_sum(part[ci]), "%s grid %u: total_count of chunk %zu is not the sum of its counts", cs.name, grid, ci);
		}
		for (uint32_t g = 0; g < ng; ++g) CHECK(memcmp(&out[g], &wantrow[g], 256) == 0, "%s grid %u: record of group %u (%u members) differs", cs.name, grid, g, sizes[g]);
		const uint8_t *t1 = (const uint8_t *)&part[chunks.size()], *t2 = (const uint8_t *)&out[ng];
		for (int i = 0; i < 256; ++i) CHECK(t1[i] == 0xEE && t2[i] == 0xEE, "%s grid %u: the union kernel wrote past its output", cs.name, grid);
	}
}
} // namespace

int main(int argc, char **argv)
{
	if (!kemu::can_run(GYS_HR_NT)) {
		printf("kemu: this process cannot have 256 threads\n");
		return 77;
	}
	std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
	const uint32_t epoch_open = 9, last_epoch = 8;
	const World w = make_world(rng, 700, epoch_open, last_epoch);
	const Case cases[] = {
		{"mode 0 lazy nrb 1 whole", 0, true, false, 1, 0x1u, false, 0, 0, false},
		{"mode 0 eager nrb 1 partly", 0, false, false, 1, 0x0u, true, 0, 0, true},
		{"mode 0 lazy nrb 2 partly", 0, true, false, 2, 0x0u, true, 0, 0, true},
		{"mode 0 eager nrb 2 whole + partly", 0, false, false, 2, 0x1u, false, 0, 0, true},
		{"mode 0 lazy nrb 10 whole", 0, true, false, 10, 0x3FFu, true, 0, 0, false},
		{"mode 0 eager nrb 10 whole", 0, false, false, 10, 0x3FFu, false, 0, 0, false},
		{"mode 0 lazy nrb 10 ends partly", 0, true, false, 10, 0x1FEu, true, 0, 0, true},
		{"mode 0 eager nrb 10 ends partly", 0, false, false, 10, 0x1FEu, true, 0, 0, true},
		{"mode 1 lazy", 1, true, false, 0, 0, false, 0, 0, false},
		{"mode 1 eager", 1, false, false, 0, 0, false, 0, 0, false},
		{"mode 2 lazy tags", 2, true, true, 0, 0, false, 0, 0, false},
		{"mode 2 eager", 2, false, false, 0, 0, false, 0, 0, false},
		{"mode 3 lazy partly", 3, true, false, 0, 0, false, T_NOW - 300, T_NOW - 100, false},
		{"mode 3 eager partly", 3, false, false, 0, 0, false, T_NOW - 300, T_NOW - 100, false},
		{"mode 3 lazy whole", 3, true, false, 0, 0, false, 0, T_NOW + 6, false},
	};
	for (const Case &cs : cases) test_case(rng, w, cs, epoch_open, last_epoch);
	if (fails) {
		printf("kemu histperiod: %d failures\n", fails);
		return 1;
	}
	printf("kemu histperiod ok\n");
	return 0;
}
