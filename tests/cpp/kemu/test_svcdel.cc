// TEST INFRASTRUCTURE (CPU): the LOGIC of the listener-deletion kernels (gyeeta_amd/csrc/gys_svcdel.hpp) under the CPU stand-in of the
// device model:
//   * key tables: a 64-entry table with at most 32 live keys; a probe run of keys that all hash to one entry (and one that wraps round the
//     table's end) with erases from its middle, head and tail; then 10 000 random steps of k_table_insert_vals /
//     k_table_erase (of live keys, of keys that are not there, re-inserts of live keys with a new value) against std::unordered_map.  After
//     EVERY step every live key is found with its value by tbl_lookup, every other key of the universe is not, no insert has failed and
//     the table holds exactly as many entries as there are live keys (no tombstone, nothing lost, nothing doubled);
//   * the stale scan (k_svc_stale_mark / _scan / _emit) on 5 000 kept records -- ids zero and non-zero, window words 0, recent and old --
//     against a plain loop: each flag and both, cap 0, below, at and above the hit count, several grid sizes; the ids in slot order;
//   * k_svc_clear on segments of 2, 4, 8, 24, 96, 256 bytes per service: the listed slots hold the fill, the others are untouched.
// Build + run: tests/test_kernel_logic_svcdel_cpu.py.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../../gyeeta_amd/csrc/gys_rollup.hpp"
#include "../../../gyeeta_amd/csrc/gys_hllroll.hpp"
#include "../../../gyeeta_amd/csrc/gys_svcquery.hpp"
#include "../../../gyeeta_amd/csrc/gys_rollsel.hpp"
#include "../../../gyeeta_amd/csrc/gys_svcdel.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <unordered_map>

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

constexpr uint32_t CAP = 64;

struct Table {
	std::vector<TblEnt> ent;
	DevTable t;
	std::vector<uint32_t> nfail;
	Table() : ent(CAP), nfail(1, 0)
	{
		memset(ent.data(), 0xFF, CAP * sizeof(TblEnt));
		t.ent = ent.data();
		t.mask = CAP - 1;
	}
	void insert(uint64_t key, uint32_t val)
	{
		std::vector<uint64_t> k(1, key);
		std::vector<uint32_t> v(1, val);
		const DevTable tt = t;
		const uint64_t *kp = k.data();
		const uint32_t *vp = v.data();
		uint32_t *nf = nfail.data();
		kemu::launch(1, 1, 0, [=] { k_table_insert_vals(tt, kp, vp, 1u, nf); });
	}
	uint32_t erase(const std::vector<uint64_t> &keys)
	{
		std::vector<uint32_t> ne(1, 0);
		const DevTable tt = t;
		const uint64_t *kp = keys.data();
		const uint32_t n = (uint32_t)keys.size();
		uint32_t *np = ne.data();
		kemu::launch(1, 2, 0, [=] { k_table_erase(tt, kp, n, np); }); // (two threads: only the first acts)
		return ne[0];
	}
	uint32_t used() const
	{
		uint32_t u = 0;
		for (const TblEnt &e : ent) u += e.key != GYS_EMPTY_KEY;
		return u;
	}
};

void verify(const Table &tb, const std::unordered_map<uint64_t, uint32_t> &live, const std::vector<uint64_t> &universe, const char *what, int step)
{
	for (uint64_t k : universe) {
		const uint32_t got = tbl_lookup(tb.t, k);
		auto it = live.find(k);
		if (it == live.end())
			CHECK(got == GYS_NOSLOT, "%s step %d: erased key %llx found with %u", what, step, (unsigned long long)k, got);
		else
			CHECK(got == it->second, "%s step %d: key %llx gives %u, expected %u", what, step, (unsigned long long)k, got, it->second);
	}
	CHECK(tb.used() == live.size(), "%s step %d: %u entries for %zu live keys", what, step, tb.used(), live.size());
	CHECK(tb.nfail[0] == 0, "%s step %d: %u inserts failed", what, step, tb.nfail[0]);
}

std::vector<uint64_t> keys_with_home(std::mt19937_64 &rng, uint32_t home, uint32_t n)
{
	std::vector<uint64_t> v;
	while (v.size() < n) {
		const uint64_t k = rng() >> 1; // (never the reserved ~0)
		if ((get_uint64_hash(k) & (CAP - 1)) == home) v.push_back(k);
	}
	return v;
}

void test_tables(uint64_t seed)
{
	std::mt19937_64 rng(seed);
	const std::vector<uint64_t> run5 = keys_with_home(rng, 5, 12), run62 = keys_with_home(rng, 62, 8), run6 = keys_with_home(rng, 6, 4), run8 = keys_with_home(rng, 8, 4);
	std::vector<uint64_t> universe;
	for (const auto *v : {&run5, &run62, &run6, &run8}) universe.insert(universe.end(), v->begin(), v->end());
	for (int i = 0; i < 44; ++i) universe.push_back(rng() >> 1);

	{ // one probe run: ten keys of home 5 in entries 5..14, behind them keys of homes 6 and 8 pushed further out
		Table tb;
		std::unordered_map<uint64_t, uint32_t> live;
		uint32_t val = 100;
		auto ins = [&](uint64_t k) {
			tb.insert(k, val);
			live[k] = val++;
		};
		for (int i = 0; i < 10; ++i) ins(run5[i]);
		for (uint64_t k : run6) ins(k);
		for (uint64_t k : run8) ins(k);
		verify(tb, live, universe, "run", 0);
		auto del = [&](uint64_t k, int step) {
			CHECK(tb.erase({k}) == 1u, "run: erase found nothing");
			live.erase(k);
			verify(tb, live, universe, "run", step);
		};
		del(run5[4], 1);  // middle
		del(run5[0], 2);  // head
		del(run8[3], 3);  // tail (the run's last entry)
		del(run6[1], 4);
		del(run5[9], 5);
		CHECK(tb.erase({run5[4]}) == 0u, "run: a key erased twice was found again");
		verify(tb, live, universe, "run", 6);
		// the wrap: eight keys of home 62 occupy 62, 63, 0..5 -- in front of the home-5 keys
		for (uint64_t k : run62) ins(k);
		verify(tb, live, universe, "wrap", 7);
		del(run62[1], 8);
		del(run62[0], 9);
		del(run62[7], 10);
		while (!live.empty()) del(live.begin()->first, 11);
		CHECK(tb.used() == 0, "run: the table is not empty at the end");
	}

	Table tb;
	std::unordered_map<uint64_t, uint32_t> live;
	for (int step = 0; step < 10000; ++step) {
		const uint32_t r = (uint32_t)(rng() % 100);
		if (live.size() < 32 && (r < 50 || live.size() < 4)) {
			const uint64_t k = universe[rng() % universe.size()]; // (a live key: rebound to the new value)
			const uint32_t v = (uint32_t)(rng() % 1000000);
			tb.insert(k, v);
			live[k] = v;
		} else if (r < 90 || live.size() >= 32) {
			// one to three keys in one launch: live ones, and now and then one that is not there
			std::vector<uint64_t> ks;
			const uint32_t nk = 1 + (uint32_t)(rng() % 3);
			uint32_t expect = 0;
			for (uint32_t i = 0; i < nk; ++i) {
				uint64_t k;
				if (rng() % 8 == 0 || live.empty()) {
					k = universe[rng() % universe.size()];
				} else {
					auto it = live.begin();
					std::advance(it, rng() % live.size());
					k = it->first;
				}
				ks.push_back(k);
				expect += (uint32_t)live.erase(k);
			}
			CHECK(tb.erase(ks) == expect, "random step %d: erase count", step);
		} else {
			CHECK(tb.erase({rng() >> 1}) == 0u, "random step %d: a key never inserted was erased", step); // (a stranger)
		}
		verify(tb, live, universe, "random", step);
		if (fails) return;
	}
}

void test_stale(uint64_t seed)
{
	std::mt19937_64 rng(seed);
	const uint32_t n = 5000, epoch = 1000;
	std::vector<uint32_t> rec((size_t)n * 24, 0);
	for (uint32_t s = 0; s < n; ++s) {
		uint32_t *r = &rec[(size_t)s * 24];
		for (int w = 2; w < 22; ++w) r[w] = (uint32_t)rng();
		const uint32_t kind = (uint32_t)(rng() % 10);
		if (kind == 0) { // never reported / free: all zero
			memset(r, 0, 96);
			continue;
		}
		const uint64_t id = rng() | 1ull;
		r[0] = (uint32_t)id;
		r[1] = (uint32_t)(id >> 32);
		r[23] = (uint32_t)(rng() % 7);
		r[22] = kind <= 2 ? 0u : kind <= 5 ? epoch - (uint32_t)(rng() % 3) : 1u + (uint32_t)(rng() % (epoch - 1));
		if (s % 1024 == 1023 || s % 1024 == 0) r[22] = 0; // (hits on both sides of every tile boundary)
	}
	const uint32_t ntiles = (n + GYS_STALE_TILE - 1) / GYS_STALE_TILE;
	for (uint32_t flags = 1; flags <= 3; ++flags)
		for (uint32_t max_age : {0u, 360u, 990u}) {
			std::vector<uint64_t> want;
			for (uint32_t s = 0; s < n; ++s) {
				const uint32_t *r = &rec[(size_t)s * 24];
				const uint64_t id = (uint64_t)r[0] | ((uint64_t)r[1] << 32);
				const bool hit = r[22] == 0 ? ((flags & 1u) && id != 0) : ((flags & 2u) && epoch - r[22] > max_age);
				if (hit) want.push_back(id);
			}
			for (uint32_t cap : {0u, 1u, (uint32_t)want.size() / 2u, (uint32_t)want.size(), (uint32_t)want.size() + 100u})
				for (uint32_t grid : {1u, 3u}) {
					std::vector<unsigned long long> bits((size_t)ntiles * 16, 0xDEADBEEFDEADBEEFull);
					std::vector<uint32_t> tiles(ntiles + 1, 0xABABABABu);
					std::vector<uint64_t> ids(cap + 1, 0x5555555555555555ull);
					SvcStaleP p{};
					p.svc_state = (const uint8_t *)rec.data();
					p.nsvc = n;
					p.ntiles = ntiles;
					p.epoch = epoch;
					p.flags = flags;
					p.max_age = max_age;
					p.bits = bits.data();
					p.tile_cnt = tiles.data();
					p.ids = ids.data();
					p.cap = cap;
					kemu::launch(grid, GYS_STALE_NT, 0, [=] { k_svc_stale_mark(p); });
					kemu::launch(1, GYS_STALE_NT, 0, [=] { k_svc_stale_scan(p); });
					kemu::launch(grid, GYS_STALE_NT, 0, [=] { k_svc_stale_emit(p); });
					CHECK(tiles[ntiles] == want.size(), "stale flags %u age %u: %u hits, expected %zu", flags, max_age, tiles[ntiles], want.size());
					const uint32_t nw = std::min<uint32_t>(cap, (uint32_t)want.size());
					for (uint32_t i = 0; i < nw; ++i) CHECK(ids[i] == want[i], "stale flags %u age %u cap %u grid %u: id %u", flags, max_age, cap, grid, i);
					for (uint32_t i = nw; i <= cap; ++i) CHECK(ids[i] == 0x5555555555555555ull, "stale: id %u beyond the hits / the cap was written", i);
				}
			CHECK(!want.empty() && want.size() < n, "stale flags %u age %u: the case is trivial", flags, max_age);
		}
}

void test_clear()
{
	const uint32_t S = 40;
	const uint64_t sizes[] = {2, 4, 8, 24, 96, 256};
	std::vector<std::vector<uint8_t>> arr;
	std::vector<SvcClearSeg> segs;
	for (uint64_t b : sizes) {
		arr.emplace_back(S * b + 16, (uint8_t)0xA5);
	}
	for (size_t i = 0; i < arr.size(); ++i) {
		uint8_t *base = (uint8_t *)(((uintptr_t)arr[i].data() + 15) & ~(uintptr_t)15);
		segs.push_back(SvcClearSeg{base, sizes[i], make_uint4(0x11111111u, 0x22222222u, 0x33333333u, 0x44444444u), make_uint4(1u, 2u, 3u, 4u)});
	}
	const std::vector<uint32_t> slots = {0, 7, 8, 39, 1000 /* beyond max_services: skipped */};
	const SvcClearSeg *sp = segs.data();
	const uint32_t *lp = slots.data();
	const uint32_t ns = (uint32_t)segs.size(), nl = (uint32_t)slots.size();
	kemu::launch(2, GYS_SVCCLEAR_NT, 0, [=] { k_svc_clear(sp, ns, lp, nl, S); });
	for (size_t i = 0; i < segs.size(); ++i)
		for (uint32_t s = 0; s < S; ++s) {
			const bool listed = s == 0 || s == 7 || s == 8 || s == 39;
			const uint8_t *d = segs[i].base + s * sizes[i];
			for (uint64_t b = 0; b < sizes[i]; ++b) {
				uint8_t want = 0xA5;
				if (listed) {
					const uint32_t f[4] = {0x11111111u, 0x22222222u, 0x33333333u, 0x44444444u}, l[4] = {1u, 2u, 3u, 4u};
					const bool vec = sizes[i] % 16 == 0, last = vec && b >= sizes[i] - 16;
					const uint32_t w = (uint32_t)(b / 4) & 3u;
					want = (uint8_t)((last ? l[w] : f[w]) >> (8 * (b & 3)));
				}
				CHECK(d[b] == want, "clear: segment of %llu bytes, slot %u, byte %llu: %02x, expected %02x", (unsigned long long)sizes[i], s, (unsigned long long)b, d[b], want);
			}
		}
}

} // namespace

int main(int argc, char **argv)
{
	const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
	if (!kemu::can_run(GYS_STALE_NT)) {
		printf("cannot start %u threads here\n", GYS_STALE_NT);
		return 77;
	}
	test_tables(seed);
	test_stale(seed);
	test_clear();
	if (fails) {
		printf("kemu svcdel: %d failures\n", fails);
		return 1;
	}
	printf("kemu svcdel ok\n");
	return 0;
}
