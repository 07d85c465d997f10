// TEST INFRASTRUCTURE (CPU): the LOGIC of the group-histogram kernel k_hist_level_union (gyeeta_amd/csrc/gys_histroll.hpp) under the CPU
// stand-in of the device model, on synthetic hist_all / hist_win / td_meta / snapshot / last + tag arrays:
//   * the three modes of a level (0 cumulative - snapshot, with and without a snapshot; 1 empty; 2 the last-window records, with and without
//     tags), each with lazily folded records (meta: some services' open window partly folded) and with eagerly kept ones (no meta);
//   * chunk sizes 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1023, 1024, a group of three chunks (2100 members), an empty group, shuffled member lists
//     with repeats, several grid sizes, outputs pre-filled with garbage (no pre-zeroed output needed);
//   * expected: every chunk's partial record and every row's record equal a plain loop of the shared level-view rule (k_level_view itself,
//     run on the same arrays) followed by gyo_hist_merge, byte for byte; counts near 2^64 wrap alike;
//   * plain mode over the partials (per-row chunk ranges, and a contiguous array cut into equal chunks) equals the direct sum.
// Build + run: tests/test_kernel_logic_histroll_cpu.py.
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

// a record as an ingest leaves it; `big` records carry any 64-bit counts (the adds wrap) and large sums of either sign
gys_hist_rec rnd_rec(std::mt19937_64 &rng, bool big)
{
	gys_hist_rec r;
	memset(&r, 0, sizeof(r));
	unsigned long long *w = (unsigned long long *)&r;
	for (int b = 0; b < 15; ++b) {
		w[2 * b] = big ? rng() : rng() % 1000;
		w[2 * b + 1] = big ? (unsigned long long)((long long)(rng() >> 14) - (1ll << 49)) : (rng() % 100000) * w[2 * b]; // (|sum| < 2^50: no signed overflow in any sum here)
	}
	w[30] = big ? rng() : rng() % 15000;
	w[31] = rng() % 7 == 0 ? (unsigned long long)INT64_MIN : (unsigned long long)((long long)(rng() % 2000000) - 1000);
	return r;
}

gys_hist_rec empty_rec()
{
	gys_hist_rec r;
	memset(&r, 0, sizeof(r));
	((unsigned long long *)&r)[31] = (unsigned long long)INT64_MIN;
	return r;
}

void merge(gys_hist_rec &dst, const gys_hist_rec &src) // through the oracle's GY_HISTOGRAM::add_histogram
{
	gyo_hist a, b;
	gyo_hist_init(&a, GYO_RESP_TIME_HASH);
	gyo_hist_init(&b, GYO_RESP_TIME_HASH);
	const unsigned long long *d = (const unsigned long long *)&dst, *s = (const unsigned long long *)&src;
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
	unsigned long long *o = (unsigned long long *)&dst;
	gyo_hist_merge(&a, &b);
	for (int i = 0; i < 15; ++i) {
		o[2 * i] = a.stats[i].count;
		o[2 * i + 1] = (unsigned long long)a.stats[i].sum;
	}
	o[30] = a.total_count;
	o[31] = (unsigned long long)a.max_val_seen;
}

struct World {
	uint32_t nsvc;
	Recs all, win, snap, last;
	std::vector<TdMeta> meta;
	std::vector<uint32_t> tag;
};

World make_world(std::mt19937_64 &rng, uint32_t nsvc, uint32_t epoch_open, uint32_t last_epoch)
{
	World w;
	w.nsvc = nsvc;
	w.all.resize(nsvc);
	w.win.resize(nsvc);
	w.snap.resize(nsvc);
	w.last.resize(nsvc);
	w.meta.resize(nsvc);
	w.tag.resize(nsvc);
	for (uint32_t s = 0; s < nsvc; ++s) {
		const bool big = s % 97 == 5;
		w.all[s] = s % 13 == 0 ? empty_rec() : rnd_rec(rng, big);
		w.win[s] = s % 5 == 0 ? empty_rec() : rnd_rec(rng, big);
		w.snap[s] = s % 3 == 0 ? gys_hist_rec{} : rnd_rec(rng, big);
		w.last[s] = rnd_rec(rng, false);
		memset(&w.meta[s], 0, sizeof(TdMeta));
		w.meta[s].hw_epoch = s % 4 == 1 ? epoch_open : (s % 4 == 2 ? epoch_open - 1u : (uint32_t)(rng() % (epoch_open + 2u)));
		w.tag[s] = s % 3 == 0 ? last_epoch : (uint32_t)(rng() % (last_epoch + 2u));
	}
	return w;
}

struct Case {
	const char *name;
	int mode;
	bool meta, sub, tags;
};

LevelViewP view_params(const World &w, const Case &cs, uint32_t epoch_open, uint32_t last_epoch)
{
	LevelViewP v{};
	v.win = w.win.data();
	v.all = w.all.data();
	v.meta = cs.meta ? w.meta.data() : nullptr;
	v.epoch_open = epoch_open;
	v.mode = cs.mode;
	v.sub = cs.mode == 2 ? w.last.data() : (cs.mode == 0 && cs.sub ? w.snap.data() : nullptr);
	v.last_tag = cs.tags ? w.tag.data() : nullptr;
	v.last_epoch = last_epoch;
	return v;
}

void launch_union(HistUnionP q, uint32_t grid)
{
	kemu::launch(grid, GYS_HR_NT, 0, [=] { k_hist_level_union(q); });
}

void test_case(std::mt19937_64 &rng, const World &w, const Case &cs, uint32_t epoch_open, uint32_t last_epoch)
{
	// the shared rule, one service at a time, as k_level_view stores it
	Recs view(w.nsvc + 1);
	memset(&view[w.nsvc], 0xEE, sizeof(gys_hist_rec));
	{
		LevelViewP v = view_params(w, cs, epoch_open, last_epoch);
		v.first = 0;
		v.n = w.nsvc;
		v.out = view.data();
		kemu::launch((w.nsvc * 16u + 255u) / 256u, 256, 0, [=] { k_level_view(v); });
		const uint8_t *tail = (const uint8_t *)&view[w.nsvc];
		CHECK(tail[0] == 0xEE && tail[255] == 0xEE, "%s: k_level_view wrote past its output", cs.name);
	}
	const uint32_t sizes[] = {1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1023, 1024, 0, 2100};
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
	}
	for (uint32_t grid : {1u, 3u, 32u}) {
		Recs part(chunks.size() + 1), out(ng + 1);
		memset(part.data(), 0xEE, part.size() * sizeof(gys_hist_rec));
		memset(out.data(), 0xEE, out.size() * sizeof(gys_hist_rec)); // (no pre-zeroed output needed)
		HistUnionP q{};
		q.v = view_params(w, cs, epoch_open, last_epoch);
		q.dst = part.data();
		q.chunks = chunks.data();
		q.members = members.data();
		q.nchunks = (uint32_t)chunks.size();
		launch_union(q, grid);
		HistUnionP r{};
		r.plain = 1;
		r.src = part.data();
		r.dst = out.data();
		r.chunks = gchunks.data();
		r.nchunks = ng;
		launch_union(r, grid);
		for (size_t ci = 0; ci < chunks.size(); ++ci)
			CHECK(memcmp(&part[ci], &wantpart[ci], 256) == 0, "%s grid %u: partial record of chunk %zu (group %u, %u members) differs", cs.name, grid, ci, chunks[ci].group,
			      chunks[ci].m1 - chunks[ci].m0);
		for (uint32_t g = 0; g < ng; ++g) CHECK(memcmp(&out[g], &wantrow[g], 256) == 0, "%s grid %u: record of group %u (%u members) differs", cs.name, grid, g, sizes[g]);
		const uint8_t *t1 = (const uint8_t *)&part[chunks.size()], *t2 = (const uint8_t *)&out[ng];
		for (int i = 0; i < 256; ++i) CHECK(t1[i] == 0xEE && t2[i] == 0xEE, "%s grid %u: the union kernel wrote past its output", cs.name, grid);
	}
}

// plain mode on records as they stand: list-free equal chunks then the chunks' records (the rank's record from the host records), and with a
// member list (cluster records from host records)
void test_plain(std::mt19937_64 &rng)
{
	const uint32_t nrec = 2300;
	Recs recs(nrec);
	for (uint32_t i = 0; i < nrec; ++i) recs[i] = i % 11 == 0 ? empty_rec() : rnd_rec(rng, i % 53 == 7);
	for (uint32_t n : {0u, 1u, 17u, 1024u, 1025u, 2300u}) {
		for (uint32_t per : {1024u, 100u, 7u}) {
			const uint32_t nch = std::max(1u, (n + per - 1) / per);
			Recs p1(nch + 1), res(2);
			memset(p1.data(), 0xEE, p1.size() * 256);
			memset(res.data(), 0xEE, res.size() * 256);
			HistUnionP a{};
			a.plain = 1;
			a.src = recs.data();
			a.dst = p1.data();
			a.n = n;
			a.per = per;
			a.nchunks = nch;
			launch_union(a, 2);
			HistUnionP b{};
			b.plain = 1;
			b.src = p1.data();
			b.dst = res.data();
			b.n = nch;
			b.per = nch;
			b.nchunks = 1;
			launch_union(b, 1);
			gys_hist_rec want = empty_rec();
			for (uint32_t i = 0; i < n; ++i) merge(want, recs[i]);
			CHECK(memcmp(&res[0], &want, 256) == 0, "plain: the sum of the first %u records in chunks of %u differs", n, per);
			CHECK(((const uint8_t *)&res[1])[0] == 0xEE && ((const uint8_t *)&p1[nch])[0] == 0xEE, "plain: wrote past the output (n %u per %u)", n, per);
		}
	}
	std::vector<uint32_t> members(777);
	for (auto &m : members) m = (uint32_t)(rng() % nrec);
	RollupChunk ch{0u, 0u, 777u, 0u};
	Recs res(2);
	memset(res.data(), 0xEE, res.size() * 256);
	HistUnionP a{};
	a.plain = 1;
	a.src = recs.data();
	a.dst = res.data();
	a.chunks = &ch;
	a.members = members.data();
	a.nchunks = 1;
	launch_union(a, 1);
	gys_hist_rec want = empty_rec();
	for (uint32_t m : members) merge(want, recs[m]);
	CHECK(memcmp(&res[0], &want, 256) == 0, "plain: the sum of 777 listed records differs");
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
		{"mode 0 lazy snapshot", 0, true, true, false},   {"mode 0 lazy all-time", 0, true, false, false}, {"mode 0 eager snapshot", 0, false, true, false},
		{"mode 0 eager all-time", 0, false, false, false}, {"mode 1 lazy", 1, true, false, false},         {"mode 1 eager", 1, false, false, false},
		{"mode 2 lazy tags", 2, true, false, true},       {"mode 2 eager", 2, false, false, false},
	};
	for (const Case &cs : cases) test_case(rng, w, cs, epoch_open, last_epoch);
	test_plain(rng);
	if (fails) {
		printf("kemu histroll: %d failures\n", fails);
		return 1;
	}
	printf("kemu histroll ok\n");
	return 0;
}
