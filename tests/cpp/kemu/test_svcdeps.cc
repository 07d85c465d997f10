// TEST INFRASTRUCTURE (CPU): the LOGIC of the service dependency graph (gyeeta_amd/csrc/gys_svcdeps.hpp: k_dep_edges<false / true>,
// k_dep_seed, k_dep_level, k_dep_collect) under the CPU stand-in of the device model, against a std::map and a deque BFS written here from
// the definition ("Service dependency graph" in include/gysketch.h):
//   * 700 random rows over registered / unregistered listeners, bound / unbound / zero client ids and both kinds, reported over several
//     windows so that some entries are dead; one task group bound to 70 services (more than a wave of emits from one row), one bound to two;
//     free slots; the edge rows field for field, the counters, the selections, caps of all / half / none with a guard row behind the cap;
//   * the traversal for every direction and max_hops 0 / 1 / 2 / 5 from several roots, and a chain 300 hops long with max_hops 0 and 299.
// The table is filled by the ingest kernels of gys_actpairs.hpp.  Every array a kernel writes is a heap array of its exact size.
// Build + run: tests/test_kernel_logic_svcdeps_cpu.py.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../../gyeeta_amd/csrc/gys_actpairs.hpp"
#include "../../../gyeeta_amd/csrc/gys_svcdeps.hpp"
#include "../../../gyeeta_amd/csrc/gys_svcdeps_host.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <deque>
#include <map>
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
	uint32_t window = 0, act = 0, nrows = 0, flags = 0;
	uint64_t sent = 0, rcvd = 0;
};
using RowKey = std::tuple<uint64_t, uint64_t, uint32_t>;  // listener id, client id, kind
using EdgeKey = std::tuple<uint32_t, uint32_t, uint32_t>; // src slot, dst slot, kind

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
	ActPairTbl view() { return ActPairTbl{key.data(), ent.data(), entries - 1}; }
	DevTable gid() { return DevTable{gent.data(), (uint32_t)gent.size() - 1u}; }
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
		p.t = view();
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
			m.nrows += 1;
			m.sent += r.sent;
			m.rcvd += r.rcvd;
			m.flags |= r.flags;
		}
	}
	DepEdgeP params(uint32_t epoch)
	{
		DepEdgeP p{};
		p.t = view();
		p.epoch = epoch;
		p.gid = gid();
		p.task_id = tl.ids.data();
		p.task_off = tl.off.data();
		p.task_slot = tl.slots.data();
		p.ntask = tl.ntasks();
		p.nsvc = nsvc;
		p.svc_gid = svc_gid.data();
		p.src_slot = p.dst_slot = GYS_NOSLOT;
		return p;
	}
	// the model's edges at `epoch`, and the counters of the definition
	std::map<EdgeKey, std::pair<RowKey, Fig>> edges(uint32_t epoch, uint64_t stat[3])
	{
		std::map<uint64_t, uint32_t> slot_of;
		std::map<uint64_t, std::vector<uint32_t>> bound;
		for (uint32_t s = 0; s < nsvc; ++s)
			if (host[s] != GYS_NOSLOT) {
				slot_of[svc_gid[s]] = s;
				if (task[s]) bound[task[s]].push_back(s);
			}
		std::map<EdgeKey, std::pair<RowKey, Fig>> e;
		stat[0] = stat[1] = stat[2] = 0;
		for (const auto &kv : model) {
			if (!(epoch - kv.second.window <= 3u)) continue;
			const uint64_t l = std::get<0>(kv.first), c = std::get<1>(kv.first);
			stat[0]++;
			const bool nol = !slot_of.count(l), noc = c == 0 || !bound.count(c);
			stat[1] += nol;
			stat[2] += noc;
			if (nol || noc) continue;
			for (uint32_t u : bound[c]) {
				const EdgeKey ek(u, slot_of[l], std::get<2>(kv.first));
				CHECK(!e.count(ek), "the model itself: an edge key twice");
				e[ek] = {kv.first, kv.second};
			}
		}
		return e;
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
	r.flags = (uint8_t)((kind ? 2u : 0u) | (rng() % 4 == 0 ? 1u : 0u));
	return r;
}

// every edge of the model with its figures, nothing else, nothing beyond the cap
void check_edges(World &w, uint32_t epoch, const gys_svc_edge_sel *sel, const char *what)
{
	uint64_t stat[3];
	auto all = w.edges(epoch, stat);
	std::map<EdgeKey, std::pair<RowKey, Fig>> want;
	DepEdgeP p = w.params(epoch);
	if (sel) {
		p.sel_flags = sel->flags;
		for (uint32_t s = 0; s < w.nsvc; ++s)
			if (w.host[s] != GYS_NOSLOT) {
				if ((sel->flags & GYS_SES_BY_SRC) && w.svc_gid[s] == sel->src_glob_id) p.src_slot = s, p.src_task = w.task[s];
				if ((sel->flags & GYS_SES_BY_DST) && w.svc_gid[s] == sel->dst_glob_id) p.dst_slot = s;
			}
	}
	for (const auto &kv : all) {
		if (sel && (sel->flags & GYS_SES_BY_SRC) && std::get<0>(kv.first) != p.src_slot) continue;
		if (sel && (sel->flags & GYS_SES_BY_DST) && std::get<1>(kv.first) != p.dst_slot) continue;
		want.insert(kv);
	}
	const uint32_t nw = (uint32_t)want.size();
	for (uint32_t cap : {nw + 5u, nw, nw / 2u, 0u}) {
		std::vector<gys_svc_edge> out(cap + 1);
		memset(out.data(), 0x5A, out.size() * sizeof(gys_svc_edge));
		std::vector<unsigned long long> ctr(DPC_NUM, 0);
		DepEdgeP q = p;
		q.out = out.data();
		q.cap = cap;
		q.ctr = ctr.data();
		q.stats = cap == nw;
		kemu::launch(2, 256, 0, [=] { k_dep_edges<true>(q); });
		CHECK(ctr[DPC_EDGES] == nw, "%s cap %u: %llu edges, expected %u", what, cap, ctr[DPC_EDGES], nw);
		if (q.stats) CHECK(ctr[DPC_LIVE] == stat[0] && ctr[DPC_NOLISTENER] == stat[1] && ctr[DPC_NOCLIENT] == stat[2], "%s: counters %llu %llu %llu, expected %llu %llu %llu", what, ctr[DPC_LIVE], ctr[DPC_NOLISTENER], ctr[DPC_NOCLIENT], (unsigned long long)stat[0], (unsigned long long)stat[1], (unsigned long long)stat[2]);
		else CHECK(ctr[DPC_LIVE] == 0, "%s: counters touched without `stats`", what);
		for (uint32_t i = std::min(cap, nw); i <= cap; ++i) {
			const uint8_t *g = (const uint8_t *)&out[i];
			bool clean = true;
			for (size_t b = 0; b < sizeof(gys_svc_edge); ++b) clean &= g[b] == 0x5A;
			CHECK(clean, "%s cap %u: row %u beyond min(edges, cap) was written", what, cap, i);
		}
		std::set<EdgeKey> seen;
		for (uint32_t i = 0; i < std::min(cap, nw); ++i) {
			const gys_svc_edge &r = out[i];
			const EdgeKey ek(r.src_slot, r.dst_slot, r.kind);
			CHECK(seen.insert(ek).second, "%s: edge %u -> %u kind %u twice", what, r.src_slot, r.dst_slot, r.kind);
			auto it = want.find(ek);
			if (it == want.end()) {
				CHECK(false, "%s: edge %u -> %u kind %u is not in the model", what, r.src_slot, r.dst_slot, r.kind);
				continue;
			}
			const Fig &m = it->second.second;
			CHECK(r.src_glob_id == w.svc_gid[r.src_slot] && r.dst_glob_id == std::get<0>(it->second.first) && r.cli_aggr_task_id == std::get<1>(it->second.first), "%s: ids of %u -> %u", what, r.src_slot, r.dst_slot);
			CHECK(r.bytes_sent == m.sent && r.bytes_received == m.rcvd && r.active_conns == m.act && r.nrows == m.nrows && r.window == m.window && r.flags == m.flags && r.pad[0] == 0 && r.pad[1] == 0,
			      "%s: figures of %u -> %u", what, r.src_slot, r.dst_slot);
		}
	}
}

std::vector<uint2> pairs_of(World &w, uint32_t epoch)
{
	DepEdgeP p = w.params(epoch);
	std::vector<unsigned long long> ctr(DPC_NUM, 0);
	p.ctr = ctr.data();
	kemu::launch(2, 256, 0, [=] { k_dep_edges<false>(p); }); // the count: nothing to write to
	std::vector<uint2> pairs(ctr[DPC_EDGES]);
	ctr[DPC_EDGES] = 0;
	p.out = pairs.data();
	p.cap = (uint32_t)pairs.size();
	kemu::launch(2, 256, 0, [=] { k_dep_edges<false>(p); });
	CHECK(ctr[DPC_EDGES] == pairs.size(), "pairs: the count moved between the passes");
	return pairs;
}

// seed, levels until nothing changes (the engine's loop: four levels per look at the word), collect -- against a deque BFS over the pairs
void check_deps(const std::vector<uint2> &pairs, uint32_t nsvc, std::vector<uint32_t> roots, uint32_t dir, uint32_t max_hops, const char *what)
{
	std::sort(roots.begin(), roots.end());
	roots.erase(std::unique(roots.begin(), roots.end()), roots.end());
	std::vector<uint32_t> hops(nsvc, 0x77777777u), want(nsvc, GYS_NOSLOT);
	uint32_t *hp = hops.data();
	const uint32_t *rp = roots.data();
	const uint32_t nr = (uint32_t)roots.size();
	kemu::launch(2, 256, 0, [=] { k_dep_seed(hp, nsvc, rp, nr); });
	const uint2 *pp = pairs.data();
	const uint64_t ne = pairs.size();
	unsigned long long changed = 0, *cp = &changed;
	const uint32_t last = max_hops ? std::min(max_hops, nsvc) : nsvc;
	uint32_t launched = 0;
	for (uint32_t level = 0; level < last && ne;) {
		changed = 0;
		const uint32_t upto = std::min(last, level + 4u);
		for (; level < upto; ++level, ++launched) kemu::launch(ne > 512 ? 2 : 1, ne > 512 ? 256 : 64, 0, [=] { k_dep_level(pp, ne, hp, nsvc, level, dir, cp); }); // (a grid-stride loop: any shape)
		if (!changed) break;
	}
	std::vector<std::vector<uint32_t>> adj(nsvc);
	for (const uint2 &e : pairs) {
		if (dir & 1u) adj[e.x].push_back(e.y);
		if (dir & 2u) adj[e.y].push_back(e.x);
	}
	std::deque<uint32_t> q;
	for (uint32_t r : roots) want[r] = 0, q.push_back(r);
	while (!q.empty()) {
		const uint32_t u = q.front();
		q.pop_front();
		if (max_hops && want[u] >= max_hops) continue;
		for (uint32_t v : adj[u])
			if (want[v] == GYS_NOSLOT) want[v] = want[u] + 1, q.push_back(v);
	}
	uint32_t nreach = 0;
	for (uint32_t s = 0; s < nsvc; ++s) {
		CHECK(hops[s] == want[s], "%s dir %u max %u: hops[%u] = %u, expected %u", what, dir, max_hops, s, hops[s], want[s]);
		nreach += want[s] != GYS_NOSLOT;
	}
	for (uint32_t cap : {nreach, nreach / 2u, 0u}) {
		std::vector<uint2> hits(cap + 1, make_uint2(0x5A5A5A5Au, 0x5A5A5A5Au));
		unsigned long long cnt = 0, *np = &cnt;
		uint2 *op = hits.data();
		kemu::launch(2, 256, 0, [=] { k_dep_collect(hp, nsvc, op, cap, np); });
		CHECK(cnt == nreach, "%s: %llu reached, expected %u", what, cnt, nreach);
		CHECK(hits[cap].x == 0x5A5A5A5Au, "%s: collect wrote beyond its cap", what);
		std::set<uint32_t> seen;
		for (uint32_t i = 0; i < std::min(cap, nreach); ++i) CHECK(hits[i].x < nsvc && want[hits[i].x] == hits[i].y && seen.insert(hits[i].x).second, "%s: hit %u", what, i);
	}
	(void)launched;
}

void test_random(uint64_t seed)
{
	std::mt19937_64 rng(seed);
	const uint32_t nsvc = 300;
	World w(nsvc, 2048);
	// slots 0 .. 299 registered as 0x1000 + s but for every 17th, which is free; slots 100 .. 174 but for the free ones share task 0x7070 (70
	// services), 10 and 11 share 0x2020, every third of the others has a task of its own, the rest are unbound
	for (uint32_t s = 0; s < nsvc; ++s) {
		if (s % 17 == 16) {
			w.host[s] = GYS_NOSLOT;
			w.task[s] = 0x6000 + s; // (a stale binding of a free slot must not count)
			continue;
		}
		w.reg(s, 0x1000 + s);
		if (s >= 100 && s < 175) w.task[s] = 0x7070;
		else if (s == 10 || s == 11) w.task[s] = 0x2020;
		else if (s % 3 == 0) w.task[s] = 0x9000 + s;
	}
	w.bind();
	CHECK(w.tl.longest() == 70, "the large task group has %u services, expected 70", w.tl.longest());
	auto pick_cid = [&]() -> uint64_t {
		const uint32_t r = (uint32_t)(rng() % 10);
		if (r == 0) return 0;
		if (r == 1) return 0x7070;
		if (r == 2) return 0x2020;
		if (r == 3) return 0xDEAD0000 + rng() % 50; // bound to nothing
		if (r == 4) return 0x6000 + 16;             // the stale binding of a free slot
		return 0x9000 + 3 * (rng() % 100);
	};
	for (uint32_t epoch = 1; epoch <= 7; ++epoch) {
		std::vector<Row> rows;
		for (int i = 0; i < 100; ++i) rows.push_back(make_row(rng, 0x1000 + rng() % 340, pick_cid(), (uint32_t)(rng() % 4 == 0)));
		rows.push_back(make_row(rng, 0x1000 + 49, 0x9000 + 48, 0)); // the same pair in both kinds: two edges
		rows.push_back(make_row(rng, 0x1000 + 49, 0x9000 + 48, 1));
		rows.push_back(make_row(rng, 0x1000 + 12, 0x9000 + 12, 0)); // a self-call
		w.ingest(rows, epoch);
	}
	for (uint32_t epoch : {7u, 9u, 11u}) {
		check_edges(w, epoch, nullptr, "all");
		gys_svc_edge_sel s{};
		s.struct_size = sizeof(s);
		s.flags = GYS_SES_BY_DST;
		s.dst_glob_id = 0x1000 + 49;
		check_edges(w, epoch, &s, "by dst");
		s.flags = GYS_SES_BY_SRC;
		s.src_glob_id = 0x1000 + 130; // one of the 70
		check_edges(w, epoch, &s, "by src of 70");
		s.src_glob_id = 0x1000 + 48;
		check_edges(w, epoch, &s, "by src");
		s.flags = GYS_SES_BY_SRC | GYS_SES_BY_DST;
		check_edges(w, epoch, &s, "by both");
		s.src_glob_id = 0x1000 + 1; // registered, unbound
		check_edges(w, epoch, &s, "by unbound src");
		s.src_glob_id = 0x55; // not registered
		check_edges(w, epoch, &s, "by unknown src");
	}
	uint64_t stat[3];
	const auto e7 = w.edges(7, stat);
	CHECK(e7.size() > 400 && stat[1] > 10 && stat[2] > 30 && w.edges(11, stat).empty() && !w.edges(9, stat).empty(), "random: trivial cases (%zu edges)", e7.size());
	CHECK(e7.count(EdgeKey(48, 49, 0)) && e7.count(EdgeKey(48, 49, 1)) && e7.count(EdgeKey(12, 12, 0)), "random: the two kinds / the self-call");
	const std::vector<uint2> pairs = pairs_of(w, 7);
	CHECK(pairs.size() == e7.size(), "pairs: %zu, expected %zu", pairs.size(), e7.size());
	std::multiset<std::pair<uint32_t, uint32_t>> a, b;
	for (const uint2 &p : pairs) a.insert({p.x, p.y});
	for (const auto &kv : e7) b.insert({std::get<0>(kv.first), std::get<1>(kv.first)});
	CHECK(a == b, "pairs: not the model's");
	for (uint32_t dir : {1u, 2u, 3u})
		for (uint32_t max_hops : {0u, 1u, 2u, 5u}) {
			check_deps(pairs, nsvc, {48}, dir, max_hops, "one root");
			check_deps(pairs, nsvc, {3, 130, 3, 299, 16}, dir, max_hops, "several roots"); // (16: a free slot as a root stands alone)
		}
	check_deps(pairs, nsvc, {}, 3, 0, "no root");
}

void test_chain()
{
	// 0 -> 1 -> ... -> 300, written back to front, and a back edge 300 -> 150
	const uint32_t nsvc = 310;
	std::vector<uint2> pairs;
	for (uint32_t i = 300; i-- > 0;) pairs.push_back(make_uint2(i, i + 1));
	pairs.push_back(make_uint2(300, 150));
	for (uint32_t max_hops : {0u, 299u}) check_deps(pairs, nsvc, {0}, 1, max_hops, "chain forward");
	check_deps(pairs, nsvc, {300}, 2, 0, "chain backward");
	check_deps(pairs, nsvc, {150}, 3, 0, "chain both ways");
}

} // namespace

int main(int argc, char **argv)
{
	const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
	if (!kemu::can_run(256)) {
		printf("cannot start 256 threads here\n");
		return 77;
	}
	test_random(seed);
	test_chain();
	if (fails) {
		printf("kemu svcdeps: %d failures\n", fails);
		return 1;
	}
	printf("kemu svcdeps ok\n");
	return 0;
}
