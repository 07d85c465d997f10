// TEST INFRASTRUCTURE (CPU): the LOGIC of the service components (gyeeta_amd/csrc/gys_svccomp.hpp: k_cc_init, k_cc_hook, k_cc_flatten,
// k_cc_sizes, k_cc_roots, k_cc_rows, k_cc_labels) under the CPU stand-in of the device model, against a sequential union-find over the same
// pair array (then the minimum slot per set) and a std::map of the figures over the table's entries, written here from the definition
// ("Service components" in include/gysketch.h).  A workgroup's 256 threads are real threads here, so the hooks of one launch do race.
//   * a path of 300 slots in a random order along the path, its pair array as generated / ascending / descending (deep trees, hooks
//     arriving in the worst order); two components of about 100 slots joined by one extra edge placed last; a slot with only a self edge;
//     free slots between members; a pair naming an index at or above nsvc (skipped, nothing written out of bounds); an empty pair array;
//     a random graph of 400 slots and about 4 000 pairs from the seed in argv[1];
//   * a table filled by the ingest kernels of gys_actpairs.hpp: one task group bound to 70 listeners calling one service (one entry, 70
//     edges, ONE flow), random rows of both kinds, dead entries, rows that give no edge: the pair array of k_dep_edges<false>, the
//     partition, and the figures of k_cc_rows entry by entry;
//   * every case at min_services 0, 1, 2 and a value above the largest component, and with every kernel at one workgroup and at several.
// The termination counter word is 0 in every case.  Every array a kernel writes is a heap array of its exact size.
// Build + run: tests/test_kernel_logic_svccomp_cpu.py.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../../gyeeta_amd/csrc/gys_actpairs.hpp"
#include "../../../gyeeta_amd/csrc/gys_svcdeps.hpp"
#include "../../../gyeeta_amd/csrc/gys_svcdeps_host.hpp"
#include "../../../gyeeta_amd/csrc/gys_svccomp.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <array>
#include <map>
#include <numeric>
#include <random>
#include <set>
#include <tuple>

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

// ---- the model: a sequential union-find, then the minimum slot per set
std::vector<uint32_t> model_comp(const std::vector<uint2> &pairs, const std::vector<uint32_t> &host)
{
	const uint32_t nsvc = (uint32_t)host.size();
	std::vector<uint32_t> par(nsvc);
	std::iota(par.begin(), par.end(), 0u);
	auto find = [&](uint32_t x) {
		while (par[x] != x) x = par[x];
		return x;
	};
	for (const uint2 &e : pairs) {
		if (e.x >= nsvc || e.y >= nsvc || e.x == e.y) continue;
		const uint32_t a = find(e.x), b = find(e.y);
		if (a != b) par[a] = b; // (any orientation: the minimum is taken below)
	}
	std::vector<uint32_t> low(nsvc, GYS_NOSLOT), comp(nsvc, GYS_NOSLOT);
	for (uint32_t s = 0; s < nsvc; ++s)
		if (host[s] != GYS_NOSLOT) low[find(s)] = std::min(low[find(s)], s);
	for (uint32_t s = 0; s < nsvc; ++s)
		if (host[s] != GYS_NOSLOT) comp[s] = low[find(s)];
	return comp;
}

struct Parts {
	std::vector<uint32_t> comp, size;
};

// the partition kernels at `grid` workgroups; comp against the model
Parts run_partition(const std::vector<uint2> &pairs, const std::vector<uint32_t> &host, uint32_t grid, const char *what)
{
	const uint32_t nsvc = (uint32_t)host.size();
	Parts r;
	std::vector<uint32_t> parent(nsvc, 0x77777777u);
	r.comp.assign(nsvc, 0x66666666u);
	unsigned long long capped = 0, *cp = &capped;
	uint32_t *pp = parent.data(), *cmp = r.comp.data();
	const uint32_t *hp = host.data();
	const uint2 *ep = pairs.data();
	const uint64_t ne = pairs.size();
	kemu::launch(grid, 256, 0, [=] { k_cc_init(pp, hp, nsvc); });
	if (ne) kemu::launch(grid, 256, 0, [=] { k_cc_hook(ep, ne, pp, nsvc, cp); });
	for (uint32_t s = 0; s < nsvc; ++s) CHECK(host[s] == GYS_NOSLOT ? parent[s] == GYS_NOSLOT : parent[s] <= s, "%s grid %u: parent[%u] = %u points upwards", what, grid, s, parent[s]);
	kemu::launch(grid, 256, 0, [=] { k_cc_flatten(pp, cmp, nsvc, cp); });
	CHECK(capped == 0, "%s grid %u: %llu walks reached their step limit", what, grid, capped);
	const std::vector<uint32_t> want = model_comp(pairs, host);
	for (uint32_t s = 0; s < nsvc; ++s) CHECK(r.comp[s] == want[s], "%s grid %u: comp[%u] = %u, expected %u", what, grid, s, r.comp[s], want[s]);
	for (uint32_t s = 0; s < nsvc; ++s)
		if (want[s] != GYS_NOSLOT) CHECK(want[want[s]] == want[s] && want[s] <= s, "the model itself: comp[comp[%u]]", s);
	r.comp = want; // (what follows is checked on its own terms)
	r.size.assign(nsvc, 0u);
	uint32_t *sp = r.size.data();
	const uint32_t *ccp = r.comp.data();
	kemu::launch(grid, 256, 0, [=] { k_cc_sizes(ccp, sp, nsvc); });
	std::vector<uint32_t> wsize(nsvc, 0u);
	for (uint32_t s = 0; s < nsvc; ++s)
		if (want[s] != GYS_NOSLOT) wsize[want[s]]++;
	CHECK(r.size == wsize, "%s grid %u: the sizes", what, grid);
	r.size = wsize;
	return r;
}

struct Listed {
	std::vector<uint2> list;
	std::vector<uint32_t> index;
};

// k_cc_roots and k_cc_labels at one min_services
Listed run_roots(const Parts &pt, uint32_t min_services, uint32_t grid, const char *what)
{
	const uint32_t nsvc = (uint32_t)pt.comp.size();
	uint32_t ncomp = 0, nlinked = 0;
	std::map<uint32_t, uint32_t> want; // root -> size, of the listed
	for (uint32_t s = 0; s < nsvc; ++s)
		if (pt.comp[s] == s) {
			ncomp++;
			nlinked += pt.size[s] >= 2u;
			if (pt.size[s] >= min_services) want[s] = pt.size[s];
		}
	Listed l;
	for (int with_list = 0; with_list < 2; ++with_list) {
		l.list.assign(nsvc, make_uint2(0x5A5A5A5Au, 0x5A5A5A5Au));
		l.index.assign(nsvc, 0x5A5A5A5Au);
		std::vector<unsigned long long> ctr(CCC_NUM, 0);
		CcRootsP p{};
		p.comp = pt.comp.data();
		p.size = pt.size.data();
		p.nsvc = nsvc;
		p.min_services = min_services;
		p.list = with_list ? l.list.data() : nullptr;
		p.index = with_list ? l.index.data() : nullptr;
		p.ctr = ctr.data();
		kemu::launch(grid, 256, 0, [=] { k_cc_roots(p); });
		CHECK(ctr[CCC_NCOMP] == ncomp && ctr[CCC_NLINKED] == nlinked && ctr[CCC_NMATCH] == want.size(), "%s min %u grid %u: counts %llu %llu %llu, expected %u %u %zu", what, min_services, grid,
		      ctr[CCC_NCOMP], ctr[CCC_NLINKED], ctr[CCC_NMATCH], ncomp, nlinked, want.size());
		CHECK(ctr[CCC_CURSOR] == (with_list ? want.size() : 0u) && ctr[CCC_CAPPED] == 0, "%s min %u: the cursor", what, min_services);
		if (!with_list) {
			CHECK(l.index[0] == 0x5A5A5A5Au && l.list[0].x == 0x5A5A5A5Au, "%s: a count wrote the list", what);
			continue;
		}
		std::set<uint32_t> seen;
		for (uint32_t i = 0; i < (uint32_t)want.size() && i < nsvc; ++i) {
			auto it = want.find(l.list[i].x);
			CHECK(it != want.end() && it->second == l.list[i].y && seen.insert(l.list[i].x).second, "%s min %u: list[%u] = (%u, %u)", what, min_services, i, l.list[i].x, l.list[i].y);
			if (l.list[i].x < nsvc) CHECK(l.index[l.list[i].x] == i, "%s min %u: index[%u] = %u, expected %u", what, min_services, l.list[i].x, l.index[l.list[i].x], i);
		}
		for (uint32_t i = (uint32_t)want.size(); i < nsvc; ++i) CHECK(l.list[i].x == 0x5A5A5A5Au, "%s min %u: list[%u] behind the listed was written", what, min_services, i);
		for (uint32_t s = 0; s < nsvc; ++s)
			if (!want.count(s)) CHECK(l.index[s] == GYS_NOSLOT, "%s min %u: index[%u] = %u of a slot that is not listed", what, min_services, s, l.index[s]);
	}
	std::vector<uint32_t> labels(nsvc, 0x5A5A5A5Au);
	uint32_t *lp = labels.data();
	const uint32_t *cp = pt.comp.data(), *sp = pt.size.data();
	kemu::launch(grid, 256, 0, [=] { k_cc_labels(cp, sp, nsvc, min_services, lp); });
	for (uint32_t s = 0; s < nsvc; ++s) {
		const uint32_t w = (pt.comp[s] != GYS_NOSLOT && pt.size[pt.comp[s]] >= min_services) ? pt.comp[s] : GYS_NO_GROUP;
		CHECK(labels[s] == w, "%s min %u: label[%u] = %u, expected %u", what, min_services, s, labels[s], w);
	}
	return l;
}

// a pair array through everything but k_cc_rows, at one workgroup and at several
void check_pairs(const std::vector<uint2> &pairs, const std::vector<uint32_t> &host, const char *what, uint32_t *largest = nullptr)
{
	for (uint32_t grid : {1u, 3u}) {
		const Parts pt = run_partition(pairs, host, grid, what);
		const uint32_t big = pt.size.empty() ? 0u : *std::max_element(pt.size.begin(), pt.size.end());
		if (largest) *largest = big;
		for (uint32_t ms : {0u, 1u, 2u, big + 1u}) (void)run_roots(pt, ms, grid, what);
	}
}

void test_path(uint64_t seed)
{
	std::mt19937_64 rng(seed);
	const uint32_t nsvc = 300;
	std::vector<uint32_t> host(nsvc, 0u), order(nsvc);
	std::iota(order.begin(), order.end(), 0u);
	std::shuffle(order.begin(), order.end(), rng);
	std::vector<uint2> pairs;
	for (uint32_t i = 0; i + 1 < nsvc; ++i) pairs.push_back(rng() & 1u ? make_uint2(order[i], order[i + 1]) : make_uint2(order[i + 1], order[i]));
	uint32_t big = 0;
	check_pairs(pairs, host, "path as generated", &big);
	CHECK(big == nsvc, "path: the largest component has %u slots", big);
	auto key = [](const uint2 &e) { return std::make_pair(std::max(e.x, e.y), std::min(e.x, e.y)); };
	std::sort(pairs.begin(), pairs.end(), [&](const uint2 &a, const uint2 &b) { return key(a) < key(b); });
	check_pairs(pairs, host, "path ascending");
	std::reverse(pairs.begin(), pairs.end());
	check_pairs(pairs, host, "path descending");
}

void test_two_joined_last_self_free_and_out_of_range()
{
	// slots 0 .. 219: every 11th is free; the others alternate between two sets (even / odd position among the registered), each a chain;
	// slot 5 has only a self edge (it is taken out of its chain); one pair names nsvc and one nsvc + 7: both are skipped
	const uint32_t nsvc = 220;
	std::vector<uint32_t> host(nsvc, 0u);
	std::vector<uint32_t> set[2];
	uint32_t k = 0;
	for (uint32_t s = 0; s < nsvc; ++s) {
		if (s % 11 == 10) {
			host[s] = GYS_NOSLOT;
			continue;
		}
		if (s == 5) continue;
		set[k++ & 1u].push_back(s);
	}
	std::vector<uint2> pairs;
	for (int h = 0; h < 2; ++h)
		for (size_t i = 0; i + 1 < set[h].size(); ++i) pairs.push_back(make_uint2(set[h][i + 1], set[h][i]));
	pairs.push_back(make_uint2(5, 5));
	pairs.push_back(make_uint2(nsvc, 3));
	pairs.push_back(make_uint2(4, nsvc + 7));
	pairs.push_back(make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu));
	uint32_t big = 0;
	check_pairs(pairs, host, "two sets", &big);
	CHECK(set[0].size() >= 95 && big == set[0].size(), "two sets: %zu and %zu slots, largest %u", set[0].size(), set[1].size(), big);
	const std::vector<uint32_t> c = model_comp(pairs, host);
	CHECK(c[5] == 5 && c[10] == GYS_NOSLOT && c[set[0].back()] != c[set[1].back()], "two sets: the self edge, the free slot, the sets");
	pairs.push_back(make_uint2(set[0].back(), set[1].back())); // the one edge that joins them, last
	check_pairs(pairs, host, "two sets joined last", &big);
	CHECK(big == set[0].size() + set[1].size(), "joined: largest %u", big);
	check_pairs({}, host, "no pair", &big);
	CHECK(big == 1, "no pair: largest %u", big);
	check_pairs({}, std::vector<uint32_t>(7, GYS_NOSLOT), "only free slots");
}

void test_random_pairs(uint64_t seed)
{
	std::mt19937_64 rng(seed * 7919u + 1u);
	const uint32_t nsvc = 400;
	std::vector<uint32_t> host(nsvc, 0u);
	for (uint32_t s = 0; s < nsvc; ++s)
		if (rng() % 9 == 0) host[s] = GYS_NOSLOT;
	std::vector<uint32_t> reg;
	for (uint32_t s = 0; s < nsvc; ++s)
		if (host[s] != GYS_NOSLOT) reg.push_back(s);
	// ~4 000 pairs inside blocks of ~40 registered slots (several components, each hooked from many threads at once), with repeats and self edges
	std::vector<uint2> pairs;
	for (int i = 0; i < 4000; ++i) {
		const uint32_t blk = (uint32_t)(rng() % ((reg.size() + 39) / 40));
		const uint32_t lo = blk * 40, n = std::min<uint32_t>(40, (uint32_t)reg.size() - lo);
		pairs.push_back(make_uint2(reg[lo + rng() % n], reg[lo + rng() % n]));
	}
	check_pairs(pairs, host, "random pairs");
	// and sparse: about as many pairs as slots, over everything
	pairs.clear();
	for (int i = 0; i < 300; ++i) pairs.push_back(make_uint2(reg[rng() % reg.size()], reg[rng() % reg.size()]));
	check_pairs(pairs, host, "sparse random pairs");
}

// ---- the table: the figures of k_cc_rows
struct Row { // comm::ACTIVE_CONN_STATS, 104 bytes
	uint64_t lid, cid;
	char ser_comm[16], cli_comm[16];
	uint64_t rmid[2], rmad, sent, rcvd;
	uint32_t cdel, sdel;
	float rtt;
	uint16_t act;
	uint8_t flags, tail;
};
static_assert(sizeof(Row) == 104, "row layout");

struct Fig {
	uint32_t window = 0;
	uint64_t act = 0, sent = 0, rcvd = 0;
};
using RowKey = std::tuple<uint64_t, uint64_t, uint32_t>; // listener id, client id, kind

struct World {
	uint32_t nsvc, entries;
	std::vector<ActPairKey> key;
	std::vector<ActPairEnt> ent;
	std::vector<unsigned long long> actr;
	std::vector<TblEnt> gent;
	std::vector<uint64_t> svc_gid, task;
	std::vector<uint32_t> host; // GYS_NOSLOT = free
	TaskLists tl;
	std::map<RowKey, Fig> model;
	World(uint32_t nsvc_, uint32_t entries_) : nsvc(nsvc_), entries(entries_), key(entries_), ent(entries_, ActPairEnt{}), actr(APC_NUM, 0), svc_gid(nsvc_, 0), task(nsvc_, 0), host(nsvc_, 0)
	{
		memset(key.data(), 0xFF, entries * sizeof(ActPairKey));
		uint32_t g = 16;
		while (g < 2 * nsvc) g *= 2;
		gent.assign(g, TblEnt{GYS_EMPTY_KEY, 0xFFFFFFFFu, 0xFFFFFFFFu});
	}
	void reg(uint32_t s, uint64_t id)
	{
		const uint32_t mask = (uint32_t)gent.size() - 1u;
		uint32_t h = get_uint64_hash(id) & mask;
		while (gent[h].key != GYS_EMPTY_KEY) h = (h + 1) & mask;
		gent[h] = TblEnt{id, s, 0};
		svc_gid[s] = id;
	}
	void bind() { tl = task_lists_build(task.data(), host.data(), GYS_NOSLOT, nsvc); }
	void ingest(const std::vector<Row> &rows, uint32_t epoch)
	{
		const uint32_t n = (uint32_t)rows.size();
		std::vector<uint32_t> row_ent(n, 0xABABABABu);
		ActPairP p{};
		p.batch = (const uint8_t *)rows.data();
		p.n = n;
		p.t = ActPairTbl{key.data(), ent.data(), entries - 1};
		p.epoch = epoch;
		p.row_ent = row_ent.data();
		p.ctr = actr.data();
		const uint32_t grid = (n + 255) / 256;
		kemu::launch(grid, 256, 0, [=] { k_actp_find(p); });
		kemu::launch(grid, 256, 0, [=] { k_actp_keep(p); });
		kemu::launch(grid, 256, 0, [=] { k_actp_add(p); });
		for (const Row &r : rows) {
			Fig &m = model[RowKey(r.lid, r.cid, (r.flags >> 1) & 1u)];
			if (m.window != epoch) {
				m = Fig{};
				m.window = epoch;
			}
			m.act += r.act;
			m.sent += r.sent;
			m.rcvd += r.rcvd;
		}
	}
	DepEdgeP params(uint32_t epoch)
	{
		DepEdgeP p{};
		p.t = ActPairTbl{key.data(), ent.data(), entries - 1};
		p.epoch = epoch;
		p.gid = DevTable{gent.data(), (uint32_t)gent.size() - 1u};
		p.task_id = tl.ids.data();
		p.task_off = tl.off.data();
		p.task_slot = tl.slots.data();
		p.ntask = tl.ntasks();
		p.nsvc = nsvc;
		p.svc_gid = svc_gid.data();
		p.src_slot = p.dst_slot = GYS_NOSLOT;
		return p;
	}
};

Row make_row(std::mt19937_64 &rng, uint64_t lid, uint64_t cid, uint32_t kind)
{
	Row r{};
	r.lid = lid;
	r.cid = cid;
	r.sent = rng() % 100000;
	r.rcvd = rng() % 100000;
	r.act = (uint16_t)(rng() % 200);
	r.flags = (uint8_t)(kind ? 2u : 0u);
	return r;
}

void test_table(uint64_t seed)
{
	std::mt19937_64 rng(seed + 99u);
	const uint32_t nsvc = 300;
	World w(nsvc, 2048);
	// slots 100 .. 174 but for the free ones share task 0x7070 (70 listeners); every 17th slot is free; the others have a task of their own
	// but for every fifth, which is unbound
	for (uint32_t s = 0; s < nsvc; ++s) {
		if (s % 17 == 16) {
			w.host[s] = GYS_NOSLOT;
			w.task[s] = 0x6000 + s; // (a stale binding of a free slot must not count)
			continue;
		}
		w.reg(s, 0x1000 + s);
		if (s >= 100 && s < 175) w.task[s] = 0x7070;
		else if (s % 5) w.task[s] = 0x9000 + s;
	}
	w.bind();
	CHECK(w.tl.longest() == 70, "the large task group has %u listeners, expected 70", w.tl.longest());
	for (uint32_t epoch = 1; epoch <= 6; ++epoch) {
		std::vector<Row> rows;
		if (epoch == 4) rows.push_back(make_row(rng, 0x1000 + 7, 0x7070, 0)); // the star: 70 listeners' group calls slot 7 -- one entry, 70 edges
		for (int i = 0; i < 25; ++i) {
			const uint32_t r = (uint32_t)(rng() % 10);
			const uint64_t cid = r == 0 ? 0 : r == 1 ? 0xDEAD0000 + rng() % 50 : r == 2 ? 0x6000 + 16 : 0x9000 + rng() % 300;
			rows.push_back(make_row(rng, 0x1000 + rng() % 330, cid, (uint32_t)(rng() % 4 == 0)));
		}
		rows.push_back(make_row(rng, 0x1000 + 12, 0x9000 + 12, 0)); // a self-call
		rows.push_back(make_row(rng, 0x1000 + 49, 0x9000 + 48, 0)); // the same pair in both kinds: two entries, two edges
		rows.push_back(make_row(rng, 0x1000 + 49, 0x9000 + 48, 1));
		w.ingest(rows, epoch);
	}
	for (uint32_t epoch : {6u, 8u, 10u})
		for (uint32_t grid : {1u, 3u}) {
			// the pair array of the traversal: count, then write
			DepEdgeP p = w.params(epoch);
			std::vector<unsigned long long> dctr(DPC_NUM, 0);
			p.ctr = dctr.data();
			kemu::launch(2, 256, 0, [=] { k_dep_edges<false>(p); });
			std::vector<uint2> pairs(dctr[DPC_EDGES]);
			dctr[DPC_EDGES] = 0;
			p.out = pairs.data();
			p.cap = (uint32_t)pairs.size();
			kemu::launch(2, 256, 0, [=] { k_dep_edges<false>(p); });
			CHECK(dctr[DPC_EDGES] == pairs.size(), "table: the count moved between the passes");
			const Parts pt = run_partition(pairs, w.host, grid, "table");
			// the model's figures: the live entries with a registered listener and a client group that owns a service
			std::map<uint64_t, uint32_t> slot_of;
			std::map<uint64_t, uint32_t> owned;
			for (uint32_t s = 0; s < nsvc; ++s)
				if (w.host[s] != GYS_NOSLOT) {
					slot_of[w.svc_gid[s]] = s;
					if (w.task[s]) owned[w.task[s]]++;
				}
			std::map<uint32_t, std::array<uint64_t, GYS_CC_ACC>> want; // root -> entries, edges, active_conns, sent, received
			uint64_t nedges = 0;
			for (const auto &kv : w.model) {
				if (!(epoch - kv.second.window <= 3u)) continue;
				const uint64_t l = std::get<0>(kv.first), c = std::get<1>(kv.first);
				if (!slot_of.count(l) || c == 0 || !owned.count(c)) continue;
				auto &a = want[pt.comp[slot_of[l]]];
				a[0] += 1;
				a[1] += owned[c];
				a[2] += kv.second.act;
				a[3] += kv.second.sent;
				a[4] += kv.second.rcvd;
				nedges += owned[c];
			}
			CHECK(nedges == pairs.size(), "table epoch %u: %zu pairs, the model has %llu edges", epoch, pairs.size(), (unsigned long long)nedges);
			if (epoch == 6) CHECK(pairs.size() > 80 &&pt.size[pt.comp[7]] >= 71 && pt.comp[7] == pt.comp[100] && pt.comp[7] == pt.comp[174], "table: the star is not there (%zu pairs)", pairs.size());
			if (epoch == 10) CHECK(pairs.empty(), "table: entries that should be dead");
			const uint32_t big = *std::max_element(pt.size.begin(), pt.size.end());
			for (uint32_t ms : {0u, 2u, big + 1u}) {
				const Listed l = run_roots(pt, ms, grid, "table");
				uint32_t nl = 0;
				for (uint32_t s = 0; s < nsvc; ++s) nl += pt.comp[s] == s && pt.size[s] >= ms;
				std::vector<unsigned long long> acc((size_t)nl * GYS_CC_ACC, 0);
				unsigned long long *ap = acc.data(); // (nullptr when nothing is listed: nothing may be added then)
				const uint32_t *cp = pt.comp.data(), *ip = l.index.data();
				DepEdgeP q = w.params(epoch);
				kemu::launch(grid, 256, 0, [=] { k_cc_rows(q, cp, ip, nl, ap); });
				for (uint32_t i = 0; i < nl; ++i) {
					const uint32_t root = l.list[i].x;
					std::array<uint64_t, GYS_CC_ACC> a{};
					if (want.count(root)) a = want[root];
					for (uint32_t f = 0; f < GYS_CC_ACC; ++f)
						CHECK(acc[(size_t)i * GYS_CC_ACC + f] == a[f], "table epoch %u min %u grid %u: figure %u of root %u = %llu, expected %llu", epoch, ms, grid, f, root,
						      acc[(size_t)i * GYS_CC_ACC + f], (unsigned long long)a[f]);
				}
			}
		}
}

} // namespace

int main(int argc, char **argv)
{
	const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
	if (!kemu::can_run(256)) {
		printf("cannot start 256 threads here\n");
		return 77;
	}
	test_path(seed);
	test_two_joined_last_self_free_and_out_of_range();
	test_random_pairs(seed);
	test_table(seed);
	if (fails) {
		printf("kemu svccomp: %d failures\n", fails);
		return 1;
	}
	printf("kemu svccomp ok\n");
	return 0;
}
