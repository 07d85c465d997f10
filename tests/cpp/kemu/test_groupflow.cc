// TEST INFRASTRUCTURE (CPU): the LOGIC of the group flow map (gyeeta_amd/csrc/gys_groupflow.hpp: k_gf_first_min, k_gf_first_flag,
// k_gf_accum, k_gf_rows) under the CPU stand-in of the device model, against a std::map of the group edges written here from the
// definition ("Group flow map" in include/gysketch.h), and the search kernels of gys_svcdeps.hpp over the group pairs against a deque BFS.
// A workgroup's 256 threads are real threads here, so the claims and sums of one launch do race.
//   * a table filled by the ingest kernels of gys_actpairs.hpp: one task group bound to 70 listeners on eight hosts, random rows of both
//     kinds, dead entries, rows that give no edge, a self-call, one pair in both kinds with different flag bytes; grouped by host (30),
//     by cluster (4) and by label (labels at random, some slots without one, some labels at or above the domain), at three epochs (the
//     last: everything has expired), with every kernel at one workgroup and at several;
//   * the first-of-group flags against "no earlier member of the task has the group", member by member;
//   * every selection flag alone and combined, a group that does not exist, a row buffer one short and a count;
//   * both ends of the contention range: every edge on ONE key, and a one-tile table whose 12 entries of the 70-listener task give 840
//     distinct keys -- more than GYS_GF_LDS_KEYS, which the test asserts for itself -- so that keys go past the LDS table;
//   * a global table too small for the keys: the error word is raised, nothing is written out of bounds.
// Every array a kernel writes is a heap array of its exact size.  Build + run: tests/test_kernel_logic_groupflow_cpu.py.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../../gyeeta_amd/csrc/gys_actpairs.hpp"
#include "../../../gyeeta_amd/csrc/gys_svcdeps.hpp"
#include "../../../gyeeta_amd/csrc/gys_svcdeps_host.hpp"
#include "../../../gyeeta_amd/csrc/gys_groupflow.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <array>
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
	uint32_t window = 0, flags = 0;
	uint64_t act = 0, sent = 0, rcvd = 0;
};
using RowKey = std::tuple<uint64_t, uint64_t, uint32_t>; // listener id, client id, kind

struct GEdge { // the figures of a group edge
	uint64_t nedges = 0, nrows = 0, act = 0, sent = 0, rcvd = 0;
	uint32_t window = 0, kinds = 0, flags = 0;
};
using GMap = std::map<std::pair<uint32_t, uint32_t>, GEdge>;

struct World {
	uint32_t nsvc, entries;
	std::vector<ActPairKey> key;
	std::vector<ActPairEnt> ent;
	std::vector<unsigned long long> actr;
	std::vector<TblEnt> gent;
	std::vector<uint64_t> svc_gid, task;
	std::vector<uint32_t> host, host_cluster, labels; // host: GYS_NOSLOT = free
	TaskLists tl;
	std::map<RowKey, Fig> model;
	World(uint32_t nsvc_, uint32_t entries_) : nsvc(nsvc_), entries(entries_), key(entries_), ent(entries_, ActPairEnt{}), actr(APC_NUM, 0), svc_gid(nsvc_, 0), task(nsvc_, 0), host(nsvc_, 0), labels(nsvc_, GYS_NO_GROUP)
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
			m.flags |= r.flags;
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
	GfGroupP grouping(uint32_t group_by, uint32_t ndomain)
	{
		GfGroupP g{};
		g.group_by = group_by;
		g.ndomain = ndomain;
		g.svc_host = host.data();
		g.host_cluster = host_cluster.data();
		g.labels = labels.data();
		g.nsvc = nsvc;
		return g;
	}
	// ---- the definition
	uint32_t group(uint32_t group_by, uint32_t ndomain, uint32_t s) const
	{
		if (host[s] == GYS_NOSLOT) return GYS_NO_GROUP;
		const uint32_t g = group_by == GYS_GROUP_HOST ? host[s] : group_by == GYS_GROUP_CLUSTER ? host_cluster[host[s]] : labels[s];
		return g < ndomain ? g : GYS_NO_GROUP;
	}
	GMap flow(uint32_t epoch, uint32_t group_by, uint32_t ndomain, uint64_t &edges, uint64_t &nogroup) const
	{
		std::map<uint64_t, uint32_t> slot_of;
		std::map<uint64_t, std::vector<uint32_t>> bound;
		for (uint32_t s = 0; s < nsvc; ++s)
			if (host[s] != GYS_NOSLOT) {
				slot_of[svc_gid[s]] = s;
				if (task[s]) bound[task[s]].push_back(s);
			}
		GMap gm;
		edges = nogroup = 0;
		for (const auto &kv : model) {
			if (!(kv.second.window != 0 && epoch >= kv.second.window && epoch - kv.second.window <= 3u)) continue;
			const uint64_t l = std::get<0>(kv.first), c = std::get<1>(kv.first);
			if (!slot_of.count(l) || c == 0 || !bound.count(c)) continue;
			const uint32_t gv = group(group_by, ndomain, slot_of[l]);
			std::set<uint32_t> distinct;
			for (uint32_t u : bound[c]) {
				const uint32_t gu = group(group_by, ndomain, u);
				edges++;
				if (gu == GYS_NO_GROUP || gv == GYS_NO_GROUP) {
					nogroup++;
					continue;
				}
				gm[{gu, gv}].nedges++;
				distinct.insert(gu);
			}
			for (uint32_t gu : distinct) {
				GEdge &e = gm[{gu, gv}];
				e.nrows++;
				e.act += kv.second.act;
				e.sent += kv.second.sent;
				e.rcvd += kv.second.rcvd;
				e.window = std::max(e.window, kv.second.window);
				e.kinds |= 1u << std::get<2>(kv.first);
				e.flags |= kv.second.flags;
			}
		}
		return gm;
	}
};

Row make_row(std::mt19937_64 &rng, uint64_t lid, uint64_t cid, uint32_t kind, uint8_t more_flags = 0)
{
	Row r{};
	r.lid = lid;
	r.cid = cid;
	r.sent = rng() % 100000;
	r.rcvd = rng() % 100000;
	r.act = (uint16_t)(rng() % 200);
	r.flags = (uint8_t)((kind ? 2u : 0u) | more_flags);
	return r;
}

struct Built {
	std::vector<unsigned long long> keys, acc, ctr;
	std::vector<uint32_t> first;
	uint32_t tcap = 0;
};

// the first flags and the accumulation, sized as the engine sizes them (or with the table `force_tcap` entries)
Built run_accum(World &w, uint32_t epoch, uint32_t group_by, uint32_t ndomain, uint32_t grid, uint64_t edges, const char *what, uint32_t force_tcap = 0)
{
	Built b;
	b.ctr.assign(GFC_NUM, 0);
	const uint32_t nmem = w.tl.nbound();
	uint32_t hcap = 256;
	while (hcap < 2 * (uint64_t)nmem) hcap <<= 1;
	std::vector<unsigned long long> hkey(hcap, GYS_EMPTY_KEY);
	std::vector<uint32_t> hmin(hcap, 0xFFFFFFFFu);
	b.first.assign(nmem, 0x5A5A5A5Au);
	const GfGroupP g = w.grouping(group_by, ndomain);
	if (nmem) {
		GfFirstP fp{};
		fp.g = g;
		fp.task_off = w.tl.off.data();
		fp.task_slot = w.tl.slots.data();
		fp.ntask = w.tl.ntasks();
		fp.nmem = nmem;
		fp.hkey = hkey.data();
		fp.hmin = hmin.data();
		fp.hmask = hcap - 1;
		fp.first = b.first.data();
		fp.ctr = b.ctr.data();
		uint32_t *fpp = b.first.data();
		const uint32_t *hm = hmin.data();
		kemu::launch(grid, 256, 0, [=] { k_gf_first_min(fp); });
		kemu::launch(grid, 256, 0, [=] { k_gf_first_flag(fpp, hm, hcap - 1, nmem); });
		// the flags from the definition: no earlier member of the task has the group
		for (uint32_t t = 0; t < w.tl.ntasks(); ++t) {
			std::set<uint32_t> seen;
			for (uint32_t j = w.tl.off[t]; j < w.tl.off[t + 1]; ++j) {
				const uint32_t gu = w.group(group_by, ndomain, w.tl.slots[j]);
				const uint32_t want = gu != GYS_NO_GROUP && seen.insert(gu).second ? 1u : 0u;
				CHECK(b.first[j] == want, "%s grid %u: first[%u] (task %u, slot %u, group %u) = %u, expected %u", what, grid, j, t, w.tl.slots[j], gu, b.first[j], want);
			}
		}
	}
	const uint64_t want = std::min<uint64_t>(edges, (uint64_t)ndomain * ndomain);
	uint32_t tcap = 256;
	while (tcap < 2 * want) tcap <<= 1;
	if (force_tcap) tcap = force_tcap;
	b.tcap = tcap;
	b.keys.assign(tcap, GYS_EMPTY_KEY);
	b.acc.assign((size_t)tcap * GYS_GF_ACC, 0);
	GfAccP ap{};
	ap.d = w.params(epoch);
	ap.g = g;
	ap.first = b.first.data();
	ap.keys = b.keys.data();
	ap.acc = b.acc.data();
	ap.mask = tcap - 1;
	ap.ctr = b.ctr.data();
	kemu::launch(grid, 256, 0, [=] { k_gf_accum(ap); });
	return b;
}

struct Sel {
	uint32_t flags, src, dst;
};

bool sel_match(const Sel &s, uint32_t gu, uint32_t gv)
{
	if ((s.flags & GYS_GES_BY_SRC) && gu != s.src) return false;
	if ((s.flags & GYS_GES_BY_DST) && gv != s.dst) return false;
	if ((s.flags & GYS_GES_NO_SELF) && gu == gv) return false;
	return true;
}

// k_gf_rows under `s` with room for `cap` rows and (with_pairs) the pair array of its exact size; everything against the model
std::vector<uint2> run_rows(Built &b, const GMap &gm, const Sel &s, uint32_t cap, bool with_pairs, uint32_t grid, const char *what)
{
	uint32_t nmatch = 0, nself = 0, npairs = 0;
	for (const auto &kv : gm) {
		nmatch += sel_match(s, kv.first.first, kv.first.second);
		nself += kv.first.first == kv.first.second;
	}
	npairs = (uint32_t)gm.size() - nself;
	std::vector<gys_group_edge> out(cap);
	memset(out.data(), 0x5A, cap * sizeof(gys_group_edge));
	std::vector<uint2> pairs(with_pairs ? npairs : 0u, make_uint2(0x5A5A5A5Au, 0x5A5A5A5Au));
	for (uint32_t f = GFC_GROUP_EDGES; f < GFC_NUM; ++f) b.ctr[f] = 0;
	GfRowsP rp{};
	rp.keys = b.keys.data();
	rp.acc = b.acc.data();
	rp.mask = b.tcap - 1;
	rp.sel_flags = s.flags;
	rp.src_group = s.src;
	rp.dst_group = s.dst;
	rp.out = cap ? out.data() : nullptr;
	rp.cap = cap;
	// (a non-null pointer even where no pair exists: the kernel takes nullptr as "no pairs asked for")
	static uint2 none;
	rp.pairs = with_pairs ? (npairs ? pairs.data() : &none) : nullptr;
	rp.pcap = with_pairs ? npairs : 0u;
	rp.ctr = b.ctr.data();
	kemu::launch(grid, 256, 0, [=] { k_gf_rows(rp); });
	CHECK(b.ctr[GFC_GROUP_EDGES] == gm.size() && b.ctr[GFC_SELF] == nself, "%s: %llu group edges, %llu self; expected %zu, %u", what, b.ctr[GFC_GROUP_EDGES], b.ctr[GFC_SELF], gm.size(), nself);
	CHECK(b.ctr[GFC_NMATCH] == nmatch, "%s sel %u/%u/%u: %llu matches, expected %u", what, s.flags, s.src, s.dst, b.ctr[GFC_NMATCH], nmatch);
	CHECK(b.ctr[GFC_NPAIRS] == (with_pairs ? npairs : 0u), "%s: %llu pairs, expected %u", what, b.ctr[GFC_NPAIRS], with_pairs ? npairs : 0u);
	std::set<std::pair<uint32_t, uint32_t>> seen;
	const uint32_t nw = std::min(cap, nmatch);
	for (uint32_t i = 0; i < nw; ++i) {
		const gys_group_edge &r = out[i];
		auto it = gm.find({r.src_group, r.dst_group});
		CHECK(it != gm.end() && sel_match(s, r.src_group, r.dst_group) && seen.insert({r.src_group, r.dst_group}).second, "%s: row %u is (%u, %u)", what, i, r.src_group, r.dst_group);
		if (it == gm.end()) continue;
		const GEdge &e = it->second;
		CHECK(r.nedges == e.nedges && r.nrows == e.nrows && r.active_conns == e.act && r.bytes_sent == e.sent && r.bytes_received == e.rcvd, "%s: (%u, %u) edges %llu rows %llu conns %llu sent %llu rcvd %llu, expected %llu %llu %llu %llu %llu",
		      what, r.src_group, r.dst_group, (unsigned long long)r.nedges, (unsigned long long)r.nrows, (unsigned long long)r.active_conns, (unsigned long long)r.bytes_sent, (unsigned long long)r.bytes_received,
		      (unsigned long long)e.nedges, (unsigned long long)e.nrows, (unsigned long long)e.act, (unsigned long long)e.sent, (unsigned long long)e.rcvd);
		CHECK(r.last_window == e.window && r.kinds == e.kinds && r.flags == e.flags && r.pad[0] == 0 && r.pad[1] == 0 && r.reserved == 0, "%s: (%u, %u) window %u kinds %u flags %u, expected %u %u %u", what, r.src_group,
		      r.dst_group, r.last_window, r.kinds, r.flags, e.window, e.kinds, e.flags);
	}
	for (uint32_t i = nw; i < cap; ++i) CHECK(out[i].src_group == 0x5A5A5A5Au, "%s: row %u behind the matches was written", what, i);
	if (with_pairs) {
		std::set<std::pair<uint32_t, uint32_t>> ps;
		for (const uint2 &q : pairs) CHECK(q.x != q.y && gm.count({q.x, q.y}) && ps.insert({q.x, q.y}).second, "%s: pair (%u, %u)", what, q.x, q.y);
	}
	return pairs;
}

// the search kernels over the group pairs against a deque BFS
void check_search(const std::vector<uint2> &pairs, const GMap &gm, uint32_t ndomain, const std::vector<uint32_t> &roots_in, uint32_t dir, uint32_t max_hops, const char *what)
{
	std::vector<uint32_t> roots;
	for (uint32_t r : roots_in)
		if (r < ndomain) roots.push_back(r);
	std::sort(roots.begin(), roots.end());
	roots.erase(std::unique(roots.begin(), roots.end()), roots.end());
	std::vector<uint32_t> hops(ndomain, 0x5A5A5A5Au);
	uint32_t *hp = hops.data();
	static uint32_t none_root;
	const uint32_t *rp = roots.empty() ? &none_root : roots.data();
	const uint32_t nroots = (uint32_t)roots.size();
	kemu::launch(2, 256, 0, [=] { k_dep_seed(hp, ndomain, rp, nroots); });
	const uint32_t last = max_hops ? std::min(max_hops, ndomain) : ndomain;
	const uint2 *pp = pairs.data();
	const uint64_t ne = pairs.size();
	for (uint32_t level = 0; level < last && ne; ++level) {
		unsigned long long changed = 0, *cp = &changed;
		kemu::launch(2, 256, 0, [=] { k_dep_level(pp, ne, hp, ndomain, level, dir, cp); });
		if (!changed) break;
	}
	std::vector<uint32_t> want(ndomain, GYS_NOSLOT);
	std::deque<uint32_t> q;
	for (uint32_t r : roots) {
		want[r] = 0;
		q.push_back(r);
	}
	while (!q.empty()) {
		const uint32_t x = q.front();
		q.pop_front();
		if (max_hops && want[x] >= max_hops) continue;
		for (const auto &kv : gm) {
			const uint32_t gu = kv.first.first, gv = kv.first.second;
			if (gu == gv) continue;
			if ((dir & GYS_DEP_CALLEES) && gu == x && want[gv] == GYS_NOSLOT) {
				want[gv] = want[x] + 1;
				q.push_back(gv);
			}
			if ((dir & GYS_DEP_CALLERS) && gv == x && want[gu] == GYS_NOSLOT) {
				want[gu] = want[x] + 1;
				q.push_back(gu);
			}
		}
	}
	for (uint32_t g = 0; g < ndomain; ++g) CHECK(hops[g] == want[g], "%s dir %u max %u: hops[%u] = %u, expected %u", what, dir, max_hops, g, hops[g], want[g]);
}

void check_map(World &w, uint32_t epoch, uint32_t group_by, uint32_t ndomain, const char *what, bool full)
{
	uint64_t edges = 0, nogroup = 0;
	const GMap gm = w.flow(epoch, group_by, ndomain, edges, nogroup);
	for (uint32_t grid : {1u, 3u}) {
		Built b = run_accum(w, epoch, group_by, ndomain, grid, edges, what);
		CHECK(b.ctr[GFC_ERR] == 0, "%s grid %u: the error word is %llu", what, grid, b.ctr[GFC_ERR]);
		CHECK(b.ctr[GFC_EDGES] == edges && b.ctr[GFC_NOGROUP] == nogroup, "%s grid %u: %llu edges, %llu in no group; expected %llu, %llu", what, grid, b.ctr[GFC_EDGES], b.ctr[GFC_NOGROUP], (unsigned long long)edges,
		      (unsigned long long)nogroup);
		const uint32_t nge = (uint32_t)gm.size();
		const std::vector<uint2> pairs = run_rows(b, gm, Sel{0, 0, 0}, nge, true, grid, what);
		run_rows(b, gm, Sel{0, 0, 0}, 0, false, grid, what); // a count
		if (nge) run_rows(b, gm, Sel{0, 0, 0}, nge - 1, false, grid, what);
		if (!full || grid != 3u) continue;
		const uint32_t a = gm.empty() ? 0u : gm.begin()->first.first, z = gm.empty() ? 0u : gm.rbegin()->first.second;
		for (const Sel &s : {Sel{GYS_GES_BY_SRC, a, 0}, Sel{GYS_GES_BY_DST, 0, z}, Sel{GYS_GES_BY_SRC | GYS_GES_BY_DST, a, a}, Sel{GYS_GES_NO_SELF, 0, 0}, Sel{GYS_GES_BY_SRC | GYS_GES_NO_SELF, a, 0},
				     Sel{GYS_GES_BY_SRC, ndomain + 5, 0}, Sel{GYS_GES_BY_DST, 0, GYS_NO_GROUP}})
			run_rows(b, gm, s, nge, false, grid, what);
		for (uint32_t dir : {1u, 2u, 3u})
			for (uint32_t mh : {0u, 1u, 2u}) check_search(pairs, gm, ndomain, {a, a, ndomain + 3, ndomain - 1}, dir, mh, what);
		check_search(pairs, gm, ndomain, {}, 3u, 0u, what);
	}
}

void test_table(uint64_t seed)
{
	std::mt19937_64 rng(seed + 4711u);
	const uint32_t nsvc = 300;
	World w(nsvc, 2048);
	w.host_cluster.resize(30);
	for (uint32_t h = 0; h < 30; ++h) w.host_cluster[h] = h % 4;
	// slots 100 .. 174 but for the free ones share task 0x7070 (70 listeners on hosts 10 .. 17); every 17th slot is free; the others have
	// a task of their own but for every fifth, which is unbound.  Labels: a third of the slots have none, the others 0 .. 59 (domain 50)
	for (uint32_t s = 0; s < nsvc; ++s) {
		w.host[s] = s / 10;
		w.labels[s] = rng() % 3 == 0 ? GYS_NO_GROUP : (uint32_t)(rng() % 60);
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
		if (epoch == 4) {
			rows.push_back(make_row(rng, 0x1000 + 7, 0x7070, 0));   // 70 listeners' group calls slot 7: one entry, 70 edges, eight hosts
			rows.push_back(make_row(rng, 0x1000 + 103, 0x7070, 1)); // ... and one of its own
		}
		for (int i = 0; i < 25; ++i) {
			const uint32_t r = (uint32_t)(rng() % 10);
			const uint64_t cid = r == 0 ? 0 : r == 1 ? 0xDEAD0000 + rng() % 50 : r == 2 ? 0x6000 + 16 : 0x9000 + rng() % 300;
			rows.push_back(make_row(rng, 0x1000 + rng() % 330, cid, (uint32_t)(rng() % 4 == 0), (uint8_t)(rng() & 1u)));
		}
		rows.push_back(make_row(rng, 0x1000 + 12, 0x9000 + 12, 0));    // a self-call
		rows.push_back(make_row(rng, 0x1000 + 49, 0x9000 + 48, 0, 1)); // the same pair in both kinds, other flag bits: kinds 3, flags ORed
		rows.push_back(make_row(rng, 0x1000 + 49, 0x9000 + 48, 1, 4));
		rows.push_back(make_row(rng, 0x1000 + 41, 0x9000 + 48, 0)); // u != v on one host
		w.ingest(rows, epoch);
	}
	for (uint32_t epoch : {6u, 8u, 10u}) {
		check_map(w, epoch, GYS_GROUP_HOST, 30, "by host", epoch == 6);
		check_map(w, epoch, GYS_GROUP_CLUSTER, 4, "by cluster", epoch == 6);
		check_map(w, epoch, GYS_GROUP_LABEL, 50, "by label", epoch == 6);
	}
	uint64_t edges = 0, nogroup = 0;
	const GMap gm = w.flow(6, GYS_GROUP_HOST, 30, edges, nogroup);
	CHECK(edges > 80 && gm.count({4, 4}) && gm.at({4, 4}).kinds == 3 && (gm.at({4, 4}).flags & 7u) == 7u, "by host: the pair in both kinds is not there (%llu edges)", (unsigned long long)edges);
	CHECK(gm.count({10, 0}) && gm.at({10, 0}).nedges >= 5 && gm.at({10, 0}).nrows >= 1 && gm.at({10, 0}).nrows < gm.at({10, 0}).nedges, "by host: the 70-listener entry is not one row per host");
	CHECK(w.flow(10, GYS_GROUP_HOST, 30, edges, nogroup).empty() && edges == 0, "entries that should be dead");
	// ONE key for everything: one cluster
	for (uint32_t h = 0; h < 30; ++h) w.host_cluster[h] = 0;
	const GMap one = w.flow(6, GYS_GROUP_CLUSTER, 1, edges, nogroup);
	CHECK(one.size() == 1 && nogroup == 0 && one.begin()->second.nedges == edges, "one cluster: %zu keys", one.size());
	check_map(w, 6, GYS_GROUP_CLUSTER, 1, "one cluster", false);
}

void test_past_the_lds_table_and_a_table_too_small(uint64_t seed)
{
	std::mt19937_64 rng(seed + 31u);
	const uint32_t nsvc = 300;
	World w(nsvc, 256); // ONE tile
	for (uint32_t s = 0; s < nsvc; ++s) {
		w.host[s] = s / 10;
		w.labels[s] = s; // every service its own label
		w.reg(s, 0x1000 + s);
		if (s >= 100 && s < 170) w.task[s] = 0x7070;
	}
	w.host_cluster.assign(30, 0);
	w.bind();
	std::vector<Row> rows;
	for (uint32_t i = 0; i < 12; ++i) rows.push_back(make_row(rng, 0x1000 + i, 0x7070, i & 1u));
	w.ingest(rows, 1);
	uint64_t edges = 0, nogroup = 0;
	const GMap gm = w.flow(1, GYS_GROUP_LABEL, nsvc, edges, nogroup);
	CHECK(w.entries == 256 && gm.size() == 840 && gm.size() > GYS_GF_LDS_KEYS, "scenario no longer reaches its edge: %zu distinct keys in one tile, the LDS table holds %u", gm.size(), GYS_GF_LDS_KEYS);
	check_map(w, 1, GYS_GROUP_LABEL, nsvc, "past the LDS table", false);
	// 840 keys into a global table of 256: 584 keys or more find no place -- counted, nothing written outside
	Built b = run_accum(w, 1, GYS_GROUP_LABEL, nsvc, 1, edges, "table too small", 256);
	CHECK(b.ctr[GFC_ERR] >= 840 - 256, "a table of 256 entries took 840 keys (error word %llu)", b.ctr[GFC_ERR]);
	uint32_t occ = 0;
	for (unsigned long long k : b.keys) occ += k != GYS_EMPTY_KEY;
	CHECK(occ == 256, "the small table holds %u keys", occ);
}

} // namespace

int main(int argc, char **argv)
{
	const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
	if (!kemu::can_run(256)) {
		printf("cannot start 256 threads here\n");
		return 77;
	}
	test_table(seed);
	test_past_the_lds_table_and_a_table_too_small(seed);
	if (fails) {
		printf("kemu groupflow: %d failures\n", fails);
		return 1;
	}
	printf("kemu groupflow ok\n");
	return 0;
}
