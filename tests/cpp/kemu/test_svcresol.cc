// TEST INFRASTRUCTURE (CPU): the LOGIC of the issue resolution (gyeeta_amd/csrc/gys_svcresol.hpp: k_resol_seed, k_resol_level,
// k_resol_settle, k_resol_finish, k_resol_rows) under the CPU stand-in of the device model, against a level-by-level search over
// std::map written here from the definition ("Issue resolution" in include/gysketch.h).  A workgroup's 256 threads are real threads
// here, so the 64-bit minima and the counts of one launch do race.
//   * the tier cap on a chain of 11 (max_tiers 0, 3, 8); the ties (two sources at equal distance, one source through two neighbours, a
//     nearer source against a lower-numbered farther one, 70 callers in one level, 1 500 callers of two sources at once); blocking (Good,
//     Idle, no state, a SOURCE in the middle, an OK carrier, an OK slot nobody reaches, Down with issue 7); cycles (a self edge, a ring
//     of four without and with a source);
//   * the currency rule of the kept state entries (the open window, the one before, two back, deleted, another host, another id, a free
//     slot, a state byte above 5) and a decision array that overrides them, stale ones included;
//   * random worlds at nsvc 1, 255, 256, 257 and 600 whose pair arrays also hold indices >= nsvc (they must be skipped), self edges and
//     parallel edges; every kernel at one workgroup and at several;
//   * the row list under every kind of mask, with room for all rows and one short.
// Every array a kernel writes is a heap array of its exact size.  Build + run: tests/test_kernel_logic_svcresol_cpu.py.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../../gyeeta_amd/csrc/gys_actpairs.hpp"
#include "../../../gyeeta_amd/csrc/gys_svcdeps.hpp"
#include "../../../gyeeta_amd/csrc/gys_svcresol.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <random>
#include <vector>

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

enum { IDLE = 0, GOOD = 1, OK = 2, BAD = 3, SEVERE = 4, DOWN = 5 };
constexpr uint32_t EPOCH = 9;

struct Slot {
	bool has = false; // a state, as the definition sees it
	uint32_t state = 0, issue = 0;
};

struct World {
	uint32_t nsvc;
	std::vector<uint8_t> svc_state; // the kept entries
	std::vector<uint32_t> host;
	std::vector<uint64_t> gid;
	std::vector<Slot> slot;         // the definition's view of the kept entries
	std::vector<uint2> pairs;
	explicit World(uint32_t n) : nsvc(n), svc_state((size_t)n * 96, 0), host(n), gid(n), slot(n)
	{
		for (uint32_t s = 0; s < n; ++s) {
			host[s] = s / 7;
			gid[s] = 0x1000 + s;
		}
	}
	// a kept entry; `window` = the window it was kept in
	void keep(uint32_t s, uint32_t state, uint32_t issue, uint32_t window = EPOCH, uint32_t rec_host = GYS_NOSLOT, uint64_t rec_gid = 0)
	{
		uint8_t *d = &svc_state[(size_t)s * 96];
		memset(d, 0xA5, 88); // (the other fields of the record are not read)
		const uint64_t g = rec_gid ? rec_gid : gid[s];
		const uint32_t h = rec_host != GYS_NOSLOT ? rec_host : host[s];
		memcpy(d, &g, 8);
		d[79] = (uint8_t)state;
		d[80] = (uint8_t)issue;
		memcpy(d + 88, &window, 4);
		memcpy(d + 92, &h, 4);
		slot[s].has = host[s] != GYS_NOSLOT && window != 0 && window + 1 >= EPOCH && h == host[s] && g == gid[s] && state <= 5;
		slot[s].state = slot[s].has ? state : 0;
		slot[s].issue = slot[s].has ? issue : 0;
	}
	void src(uint32_t s, uint32_t state = BAD, uint32_t issue = 3) { keep(s, state, issue); }
	void dep(uint32_t s, uint32_t state = BAD) { keep(s, state, 7); }
	void edge(uint32_t u, uint32_t v) { pairs.push_back(make_uint2(u, v)); }
};

struct Want {
	std::vector<gys_svc_resol> rec;
	unsigned long long ctr[RSC_NUM] = {};
};

// the definition, level by level
Want model(const World &w, const std::vector<Slot> &st, uint32_t max_tiers)
{
	const uint32_t tiers = max_tiers ? max_tiers : GYS_RESOL_MAX_TIERS;
	auto cls = [&](uint32_t s) { return resol_class(st[s].has, st[s].state, st[s].issue); };
	std::map<uint32_t, uint32_t> tier, src, via;
	for (uint32_t s = 0; s < w.nsvc; ++s)
		if (cls(s) == RS_CL_SOURCE) {
			tier[s] = 0;
			src[s] = s;
		}
	for (uint32_t t = 0; t < tiers; ++t) {
		std::map<uint32_t, std::pair<uint32_t, uint32_t>> cand;
		for (const uint2 &e : w.pairs) {
			if (e.x >= w.nsvc || e.y >= w.nsvc) continue;
			if (!tier.count(e.y) || tier[e.y] != t || tier.count(e.x)) continue;
			if (cls(e.x) != RS_CL_DEPENDENT && cls(e.x) != RS_CL_CARRIER) continue;
			const std::pair<uint32_t, uint32_t> c(src[e.y], e.y);
			if (!cand.count(e.x) || c < cand[e.x]) cand[e.x] = c;
		}
		for (const auto &kv : cand) {
			tier[kv.first] = t + 1;
			src[kv.first] = kv.second.first;
			via[kv.first] = kv.second.second;
		}
	}
	Want o;
	o.rec.resize(w.nsvc);
	for (uint32_t s = 0; s < w.nsvc; ++s) {
		gys_svc_resol &r = o.rec[s];
		const uint32_t c = cls(s);
		r.src_slot = r.via_slot = GYS_NOSLOT;
		r.role = GYS_RS_NONE;
		r.tier = 0;
		r.state = c == RS_CL_NOSTATE ? 0 : (uint8_t)st[s].state;
		r.issue = c == RS_CL_NOSTATE ? 0 : (uint8_t)st[s].issue;
		r.nresolved = 0;
		o.ctr[RSC_WITH_STATE] += c != RS_CL_NOSTATE;
		if (c == RS_CL_SOURCE) {
			r.role = GYS_RS_SOURCE;
			r.src_slot = s;
			o.ctr[RSC_SOURCES]++;
		} else if (tier.count(s)) {
			r.role = c == RS_CL_DEPENDENT ? GYS_RS_RESOLVED : GYS_RS_CARRIER;
			r.tier = (uint8_t)tier[s];
			r.src_slot = src[s];
			r.via_slot = via[s];
			if (c == RS_CL_DEPENDENT) {
				o.ctr[RSC_RESOLVED]++;
				o.ctr[RSC_TIER0 + tier[s] - 1]++;
			} else {
				o.ctr[RSC_CARRIERS]++;
			}
		} else if (c == RS_CL_DEPENDENT) {
			r.role = GYS_RS_UNRESOLVED;
			o.ctr[RSC_UNRESOLVED]++;
		}
	}
	for (uint32_t s = 0; s < w.nsvc; ++s)
		if (o.rec[s].role == GYS_RS_RESOLVED) o.rec[o.rec[s].src_slot].nresolved++;
	return o;
}

bool same(const gys_svc_resol &a, const gys_svc_resol &b) { return memcmp(&a, &b, sizeof(a)) == 0; }

// the kernels as the engine launches them; dec: the decisions that replace the kept entries, or nullptr
Want run(const World &w, const gys_listener_decision *dec, uint32_t max_tiers, uint32_t grid, std::vector<double> &impact)
{
	const uint32_t n = w.nsvc;
	std::vector<uint32_t> word(n, 0x5A5A5A5Au), nres(n, 0x5A5A5A5Au);
	std::vector<unsigned long long> best(n, 0x5A5A5A5A5A5A5A5Aull);
	Want o;
	o.rec.resize(n);
	memset(o.rec.data(), 0x5A, n * sizeof(gys_svc_resol));
	impact.assign(n, 1e300);
	ResolSeedP sp{};
	sp.svc_state = w.svc_state.data();
	sp.svc_host = w.host.data();
	sp.svc_gid = w.gid.data();
	sp.dec = dec;
	sp.nsvc = n;
	sp.epoch = EPOCH;
	sp.word = word.data();
	sp.best = best.data();
	sp.nres = nres.data();
	kemu::launch(grid, 256, 0, [=] { k_resol_seed(sp); });
	const uint32_t tiers = max_tiers ? max_tiers : GYS_RESOL_MAX_TIERS;
	static uint2 none;
	const uint2 *pp = w.pairs.empty() ? &none : w.pairs.data();
	const uint64_t ne = w.pairs.size();
	uint32_t *wp = word.data(), *np = nres.data();
	unsigned long long *bp = best.data();
	for (uint32_t level = 0; level < tiers && ne; ++level) {
		kemu::launch(grid, 256, 0, [=] { k_resol_level(pp, ne, wp, bp, n, level); });
		kemu::launch(grid, 256, 0, [=] { k_resol_settle(wp, bp, np, n, level); });
	}
	ResolFinP fp{};
	fp.word = wp;
	fp.best = bp;
	fp.nres = np;
	fp.nsvc = n;
	fp.out = o.rec.data();
	fp.impact = impact.data();
	fp.ctr = o.ctr;
	unsigned long long *cp = o.ctr;
	(void)cp;
	kemu::launch(grid, 256, 0, [=] { k_resol_finish(fp); });
	return o;
}

void check_rows(const World &w, const Want &want, uint32_t mask, uint32_t short_by, uint32_t grid, const char *what)
{
	std::vector<uint32_t> hits;
	for (uint32_t s = 0; s < w.nsvc; ++s)
		if ((mask >> want.rec[s].role) & 1u) hits.push_back(s);
	const uint32_t nm = (uint32_t)hits.size(), cap = nm > short_by ? nm - short_by : 0u;
	std::vector<gys_svc_resol_row> rows(cap);
	memset(rows.data(), 0x5A, cap * sizeof(gys_svc_resol_row));
	static gys_svc_resol_row none;
	unsigned long long cursor = 0;
	ResolRowsP rp{};
	rp.rec = want.rec.data();
	rp.svc_gid = w.gid.data();
	rp.svc_host = w.host.data();
	rp.nsvc = w.nsvc;
	rp.role_mask = mask;
	rp.out = cap ? rows.data() : &none;
	rp.cap = cap;
	rp.cursor = &cursor;
	kemu::launch(grid, 256, 0, [=] { k_resol_rows(rp); });
	CHECK(cursor == nm, "%s mask %#x: %llu rows listed, expected %u", what, mask, cursor, nm);
	std::sort(rows.begin(), rows.end(), [](const gys_svc_resol_row &a, const gys_svc_resol_row &b) { return a.slot < b.slot; });
	for (uint32_t i = 0; i < cap; ++i) {
		const gys_svc_resol_row &r = rows[i];
		CHECK(r.slot < w.nsvc && ((mask >> want.rec[r.slot].role) & 1u) && (i == 0 || rows[i - 1].slot != r.slot), "%s mask %#x: row %u names slot %u", what, mask, i, r.slot);
		if (r.slot >= w.nsvc) continue;
		if (!short_by) CHECK(r.slot == hits[i], "%s mask %#x: row %u is slot %u, expected %u", what, mask, i, r.slot, hits[i]);
		const gys_svc_resol &q = want.rec[r.slot];
		gys_svc_resol_row e{};
		e.glob_id = w.host[r.slot] != GYS_NOSLOT ? w.gid[r.slot] : 0;
		e.slot = r.slot;
		e.src_slot = q.src_slot;
		e.via_slot = q.via_slot;
		e.nresolved = q.nresolved;
		e.role = q.role;
		e.tier = q.tier;
		e.state = q.state;
		e.issue = q.issue;
		if (q.src_slot != GYS_NOSLOT) {
			e.src_glob_id = w.gid[q.src_slot];
			e.src_state = want.rec[q.src_slot].state;
			e.src_issue = want.rec[q.src_slot].issue;
		}
		if (q.via_slot != GYS_NOSLOT) e.via_glob_id = w.gid[q.via_slot];
		CHECK(memcmp(&r, &e, sizeof(e)) == 0, "%s mask %#x: the row of slot %u (role %u src %u via %u tier %u) differs", what, mask, r.slot, r.role, r.src_slot, r.via_slot, r.tier);
	}
}

// kernels against the model: kept entries, or `dec` in their place (st = what the definition sees then)
Want check(const World &w, uint32_t max_tiers, const char *what, const gys_listener_decision *dec = nullptr, const std::vector<Slot> *st = nullptr)
{
	const Want want = model(w, st ? *st : w.slot, max_tiers);
	for (uint32_t grid : {1u, 3u}) {
		std::vector<double> impact;
		const Want got = run(w, dec, max_tiers, grid, impact);
		for (uint32_t s = 0; s < w.nsvc; ++s) {
			const gys_svc_resol &a = got.rec[s], &b = want.rec[s];
			CHECK(same(a, b), "%s tiers %u grid %u: slot %u role %u src %u via %u tier %u state %u issue %u n %u, expected %u %u %u %u %u %u %u", what, max_tiers, grid, s, a.role, a.src_slot, a.via_slot, a.tier,
			      a.state, a.issue, a.nresolved, b.role, b.src_slot, b.via_slot, b.tier, b.state, b.issue, b.nresolved);
			const bool ok = b.role == GYS_RS_SOURCE ? impact[s] == (double)b.nresolved : isnan(impact[s]);
			CHECK(ok, "%s tiers %u grid %u: impact[%u] = %g (role %u, nresolved %u)", what, max_tiers, grid, s, impact[s], b.role, b.nresolved);
		}
		for (uint32_t f = 0; f < RSC_NUM; ++f) CHECK(got.ctr[f] == want.ctr[f], "%s tiers %u grid %u: counter %u = %llu, expected %llu", what, max_tiers, grid, f, got.ctr[f], want.ctr[f]);
		for (uint32_t mask : {0x1Eu, 0x1Fu, 0x02u, 0x14u, 0x01u}) check_rows(w, want, mask, 0, grid, what);
		check_rows(w, want, 0x1Eu, 1, grid, what);
	}
	return want;
}

void test_tier_cap()
{
	World w(11);
	w.src(0);
	for (uint32_t s = 1; s <= 10; ++s) {
		w.dep(s);
		w.edge(s, s - 1);
	}
	const Want a = check(w, 0, "chain");
	for (uint32_t s = 1; s <= 8; ++s) CHECK(a.rec[s].role == GYS_RS_RESOLVED && a.rec[s].tier == s && a.rec[s].src_slot == 0 && a.rec[s].via_slot == s - 1, "chain: slot %u", s);
	CHECK(a.rec[9].role == GYS_RS_UNRESOLVED && a.rec[10].role == GYS_RS_UNRESOLVED && a.rec[0].nresolved == 8, "chain: the cap at 8");
	const Want b = check(w, 3, "chain");
	CHECK(b.rec[3].role == GYS_RS_RESOLVED && b.rec[4].role == GYS_RS_UNRESOLVED && b.rec[0].nresolved == 3, "chain: the cap at 3");
	const Want c = check(w, 8, "chain");
	CHECK(memcmp(a.rec.data(), c.rec.data(), 11 * sizeof(gys_svc_resol)) == 0, "chain: max_tiers 8 and 0 differ");
	check(w, 1, "chain");
}

void test_ties()
{
	{ // two sources at equal distance; one source through two neighbours; a nearer source against a lower farther one
		World w(20);
		w.src(5);
		w.src(2, SEVERE, 1);
		w.dep(9);
		w.edge(9, 5);
		w.edge(9, 2);
		w.src(10);
		w.dep(12);
		w.dep(11);
		w.dep(13);
		w.edge(12, 10);
		w.edge(11, 10);
		w.edge(13, 12);
		w.edge(13, 11);
		w.src(14); // far and low ...
		w.dep(15);
		w.dep(16);
		w.src(18); // ... near and high
		w.dep(17);
		w.edge(15, 14);
		w.edge(16, 15);
		w.edge(17, 16);
		w.edge(17, 18);
		const Want a = check(w, 0, "ties");
		CHECK(a.rec[9].src_slot == 2 && a.rec[9].via_slot == 2, "ties: the lower source");
		CHECK(a.rec[13].src_slot == 10 && a.rec[13].via_slot == 11 && a.rec[13].tier == 2, "ties: the lower via");
		CHECK(a.rec[17].src_slot == 18 && a.rec[17].tier == 1, "ties: the nearer source");
	}
	{ // 70 callers in one level
		World w(100);
		w.src(3);
		for (uint32_t s = 20; s < 90; ++s) {
			w.dep(s);
			w.edge(s, 3);
		}
		const Want a = check(w, 0, "70 callers");
		CHECK(a.rec[3].nresolved == 70 && a.ctr[RSC_TIER0] == 70, "70 callers: %u resolved", a.rec[3].nresolved);
	}
	{ // 1 500 callers of two sources, each calling both
		World w(1600);
		w.src(40);
		w.src(7);
		for (uint32_t s = 100; s < 1600; ++s) {
			w.dep(s);
			w.edge(s, 40);
			w.edge(s, 7);
		}
		const Want a = check(w, 0, "contention");
		CHECK(a.rec[7].nresolved == 1500 && a.rec[40].nresolved == 0, "contention: %u and %u resolved", a.rec[7].nresolved, a.rec[40].nresolved);
	}
}

void test_blocking_and_cycles()
{
	World w(60);
	// chains s <- m <- f with the middle Good / Idle / without a state / OK / a SOURCE
	const uint32_t mids[5] = {GOOD, IDLE, 99, OK, BAD};
	for (uint32_t k = 0; k < 5; ++k) {
		const uint32_t s = 3 * k, m = s + 1, f = s + 2;
		w.src(s);
		if (mids[k] != 99) w.keep(m, mids[k], mids[k] == BAD ? 2 : 0);
		w.dep(f);
		w.edge(m, s);
		w.edge(f, m);
	}
	w.keep(20, OK, 0);     // an OK slot nobody reaches
	w.src(21);
	w.dep(22, DOWN);       // Down with issue 7 is a DEPENDENT
	w.edge(22, 21);
	w.dep(25);             // a self edge without a source
	w.edge(25, 25);
	for (uint32_t i = 0; i < 4; ++i) { // a ring without a source
		w.dep(30 + i);
		w.edge(30 + i, 30 + (i + 1) % 4);
	}
	for (uint32_t i = 0; i < 4; ++i) { // the same ring, 40 calls the source 45
		w.dep(40 + i);
		w.edge(40 + i, 40 + (i + 1) % 4);
	}
	w.src(45);
	w.edge(40, 45);
	const Want a = check(w, 0, "blocking");
	CHECK(a.rec[2].role == GYS_RS_UNRESOLVED && a.rec[5].role == GYS_RS_UNRESOLVED && a.rec[8].role == GYS_RS_UNRESOLVED, "blocking: Good / Idle / no state");
	CHECK(a.rec[10].role == GYS_RS_CARRIER && a.rec[11].role == GYS_RS_RESOLVED && a.rec[11].tier == 2 && a.rec[9].nresolved == 1, "blocking: the carrier");
	CHECK(a.rec[13].role == GYS_RS_SOURCE && a.rec[13].src_slot == 13 && a.rec[14].src_slot == 13 && a.rec[12].nresolved == 0, "blocking: a source in the middle");
	CHECK(a.rec[20].role == GYS_RS_NONE && a.rec[20].state == OK && a.rec[22].role == GYS_RS_RESOLVED && a.rec[25].role == GYS_RS_UNRESOLVED, "blocking: OK unreached, Down, self edge");
	for (uint32_t i = 0; i < 4; ++i) CHECK(a.rec[30 + i].role == GYS_RS_UNRESOLVED, "ring without a source: slot %u", 30 + i);
	CHECK(a.rec[40].tier == 1 && a.rec[43].tier == 2 && a.rec[42].tier == 3 && a.rec[41].tier == 4, "ring with a source: tiers %u %u %u %u", a.rec[40].tier, a.rec[43].tier, a.rec[42].tier, a.rec[41].tier);
}

void test_currency_and_decisions()
{
	World w(40);
	for (uint32_t k = 0; k < 8; ++k) {
		w.src(4 * k);
		w.dep(4 * k + 2);
		w.edge(4 * k + 1, 4 * k);
		w.edge(4 * k + 2, 4 * k + 1);
	}
	w.keep(1, BAD, 7, EPOCH);                 // the open window
	w.keep(5, BAD, 7, EPOCH - 1);             // the one before
	w.keep(9, BAD, 7, EPOCH - 2);             // stale
	w.keep(13, BAD, 7, 0);                    // deleted
	w.keep(17, BAD, 7, EPOCH, w.host[17] + 1); // another host's record
	w.keep(21, BAD, 7, EPOCH, GYS_NOSLOT, 0x77777); // another listener's record
	w.keep(25, BAD, 7);
	w.host[25] = GYS_NOSLOT;                  // a free slot
	w.keep(25, BAD, 7);
	w.keep(29, 6, 7);                         // a state byte above 5
	const Want a = check(w, 0, "currency");
	CHECK(a.rec[2].role == GYS_RS_RESOLVED && a.rec[6].role == GYS_RS_RESOLVED, "currency: the open window and the one before");
	for (uint32_t s : {10u, 14u, 18u, 22u, 26u, 30u}) CHECK(a.rec[s].role == GYS_RS_UNRESOLVED && a.rec[s - 1].role == GYS_RS_NONE && a.rec[s - 1].state == 0 && a.rec[s - 1].issue == 0, "currency: slot %u", s);
	// decisions: the same states give the same result; others override, stale slots included; a free slot has no state whatever they say
	std::vector<gys_listener_decision> dec(w.nsvc);
	std::vector<Slot> st = w.slot;
	memset(dec.data(), 0x5A, dec.size() * sizeof(dec[0]));
	for (uint32_t s = 0; s < w.nsvc; ++s) {
		dec[s].state = st[s].has ? (uint8_t)st[s].state : 9;
		dec[s].issue = (uint8_t)st[s].issue;
	}
	const Want b = check(w, 0, "decisions as kept", dec.data(), &st);
	CHECK(memcmp(a.rec.data(), b.rec.data(), w.nsvc * sizeof(gys_svc_resol)) == 0, "decisions as kept: the result differs");
	for (uint32_t s : {9u, 13u, 17u, 21u, 25u, 29u}) {
		dec[s].state = SEVERE;
		dec[s].issue = 7;
		st[s] = Slot{s != 25u, s != 25u ? (uint32_t)SEVERE : 0u, s != 25u ? 7u : 0u};
	}
	dec[0].state = GOOD; // the source of the first chain is well now
	st[0] = Slot{true, GOOD, dec[0].issue};
	const Want c = check(w, 0, "decisions override", dec.data(), &st);
	CHECK(c.rec[10].role == GYS_RS_RESOLVED && c.rec[10].tier == 2 && c.rec[26].role == GYS_RS_UNRESOLVED && c.rec[2].role == GYS_RS_UNRESOLVED && c.rec[0].role == GYS_RS_NONE, "decisions override");
}

void test_random(uint64_t seed, uint32_t nsvc)
{
	std::mt19937_64 rng(seed * 1000 + nsvc);
	World w(nsvc);
	for (uint32_t s = 0; s < nsvc; ++s) {
		const uint32_t r = (uint32_t)(rng() % 100);
		if (r < 5) w.src(s, BAD + (uint32_t)(rng() % 3), (uint32_t)(rng() % 7));
		else if (r < 40) w.dep(s, BAD + (uint32_t)(rng() % 3));
		else if (r < 70) w.keep(s, OK, (uint32_t)(rng() % 16));
		else if (r < 95) w.keep(s, (uint32_t)(rng() % 2), 0);
		else if (r < 97) w.keep(s, BAD, 7, EPOCH - 3);
		if (r == 99) w.host[s] = GYS_NOSLOT, w.keep(s, BAD, 1);
	}
	const uint32_t ne = nsvc * 3 + 2;
	for (uint32_t e = 0; e < ne; ++e) {
		uint32_t u = (uint32_t)(rng() % nsvc), v = (uint32_t)(rng() % nsvc);
		const uint32_t r = (uint32_t)(rng() % 50);
		if (r == 0) u = nsvc + (uint32_t)(rng() % 5);
		if (r == 1) v = nsvc;
		if (r == 2) v = GYS_NOSLOT;
		if (r == 3) v = u;
		w.edge(u, v);
		if (r == 4) w.edge(u, v);
	}
	char what[64];
	snprintf(what, sizeof(what), "random %u", nsvc);
	const Want a = check(w, 0, what);
	check(w, 2, what);
	if (nsvc >= 600) CHECK(a.ctr[RSC_SOURCES] >= 10 && a.ctr[RSC_RESOLVED] >= 50 && a.ctr[RSC_CARRIERS] >= 50 && a.ctr[RSC_UNRESOLVED] >= 5 && a.ctr[RSC_TIER0 + 2] >= 5,
				 "%s no longer reaches its edge: %llu sources, %llu resolved, %llu carriers, %llu unresolved, %llu at tier 3", what, a.ctr[RSC_SOURCES], a.ctr[RSC_RESOLVED], a.ctr[RSC_CARRIERS],
				 a.ctr[RSC_UNRESOLVED], a.ctr[RSC_TIER0 + 2]);
}

} // namespace

int main(int argc, char **argv)
{
	const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
	if (!kemu::can_run(256)) {
		printf("cannot start 256 threads here\n");
		return 77;
	}
	test_tier_cap();
	test_ties();
	test_blocking_and_cycles();
	test_currency_and_decisions();
	for (uint32_t nsvc : {1u, 255u, 256u, 257u, 600u}) test_random(seed, nsvc);
	{ // no edge at all: the seed's words stand
		World w(5);
		w.src(1);
		w.dep(2);
		w.keep(3, OK, 0);
		check(w, 0, "no edges");
	}
	if (fails) {
		printf("kemu svcresol: %d failures\n", fails);
		return 1;
	}
	printf("kemu svcresol ok\n");
	return 0;
}
