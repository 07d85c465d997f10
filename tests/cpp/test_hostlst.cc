// TEST INFRASTRUCTURE (CPU): the host mirror of a host's listeners, gyeeta_amd/csrc/gys_hostlst.hpp (host_lst_insert / host_lst_remove and
// what they drive: sub-tables, the cut into parts, chains, the overflow fallback, the dirty / rebuild protocol), against the plain
// statement of the reference rule that oracle/gy_oracle_engine.c restates (gyo_engine_register_addr / lookup): per (netns, port) key an
// ordered list of (slot, address); a new listener replaces in place the first entry that is any-address or equal to it under laddr_equal,
// else it is appended; a deleted listener leaves its list; an event resolves to the first entry that is any-address or equals the event's
// server address.
// The READ side goes through the mirror the way the device does: the sub-table of the key's part is probed, a plain entry names a local
// (slot = slots[local]), a GYS_LOCAL_GROUP entry is followed through `cands` up to the record flagged last; an overflow host resolves
// through okey / cand_first / cands.  After EVERY call of a sequence:
//   * every (registered key x each address ever registered on it, plus one that never was) resolves to the model's slot or to nothing;
//   * all_slots = the model's live-or-replaced slots in registration order; keys_gone = the touched keys the model has emptied;
//   * no part holds more than GYS_HOST_MAX_LOCAL locals, every local sits in the part of its key, every table's size is a power of two of
//     at least host_tbl_capacity(locals) that never shrinks, no key has two entries in a table, every candidate record names the local of
//     its listener, and the descriptor counter advanced by exactly the parts of each cut.
// Named cases (the smallest that reach each edge) + seeded random sequences on a small host, a host that gets cut and one that overflows.
// A second mode (--tables FILE) prints the sub-tables the mirror builds for key lists from a file: the pin of tests/lstkeys.py.
// Build (g++ -fsanitize=address,undefined) + run: tests/test_hostlst_cpu.py.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../gyeeta_amd/csrc/gys_hostlst.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <random>
#include <set>
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

using LAddr = HostListeners::LAddr;

// address kinds: 0 any; 1 .. 3 IPv4 10.0.0.k; 4, 5 plain IPv6; 6 ::ffff:10.0.0.1 (embeds kind 1); 7 an IPv4 address nobody registers
enum { A_ANY = 0, A_V4_1, A_V4_2, A_V4_3, A_V6_1, A_V6_2, A_V6_MAPPED_1, A_NOBODY, A_KINDS };

gys_listener_info listener(uint32_t netns, uint16_t port, int kind)
{
	gys_listener_info li{};
	li.netns = netns;
	li.port = port;
	li.is_any_ip = kind == A_ANY;
	if (kind >= A_V4_1 && kind <= A_V4_3) {
		const uint8_t a[4] = {10, 0, 0, (uint8_t)kind};
		memcpy(li.addr, a, 4);
	} else if (kind == A_NOBODY) {
		const uint8_t a[4] = {10, 9, 9, 9};
		memcpy(li.addr, a, 4);
	} else if (kind == A_V6_1 || kind == A_V6_2) {
		li.addr_is_v6 = 1;
		li.addr[0] = 0x20, li.addr[1] = 0x01, li.addr[2] = 0x0d, li.addr[3] = 0xb8, li.addr[15] = (uint8_t)(kind - A_V6_1 + 1);
	} else if (kind == A_V6_MAPPED_1) {
		li.addr_is_v6 = 1;
		li.addr[10] = li.addr[11] = 0xFF, li.addr[12] = 10, li.addr[15] = 1;
	}
	return li;
}
int kind_of(const gys_listener_info &li)
{
	for (int kind = 0; kind < A_KINDS; ++kind) {
		const gys_listener_info k = listener(0, 0, kind);
		if (k.is_any_ip == li.is_any_ip && k.addr_is_v6 == li.addr_is_v6 && memcmp(k.addr, li.addr, 16) == 0) return kind;
	}
	abort();
}
// the server address of an event, normalised as a listener's is (k_resp_host does the same with the event's bytes)
LAddr event_addr(int kind) { return listener_addr(listener(0, 0, kind)); }

constexpr uint32_t NONE = GYS_NOSLOT;

struct World {
	HostListeners hl;
	uint32_t desc_used = 0, desc_cap = 1000;
	// the model
	struct Ent {
		uint32_t slot;
		LAddr a;
	};
	std::map<uint64_t, std::vector<Ent>> lists;
	std::vector<uint32_t> all; // live-or-replaced slots in registration order
	// what the engine keeps next to the mirror
	std::vector<uint64_t> key_of_slot;
	std::set<uint32_t> free_slots;
	std::map<uint64_t, std::set<int>> kinds_seen; // per key ever registered: the address kinds registered on it
	std::vector<size_t> tbl_sizes;                // of the current cut, for "never shrinks"
	const char *what = "";
	int step = 0;

	World() { hl.tbl.assign(16, GYS_HOST_TBL_EMPTY); } // (as gys_register_host leaves a new host)

	uint32_t model_resolve(uint64_t key, const LAddr &ev) const
	{
		auto it = lists.find(key);
		if (it == lists.end()) return NONE;
		for (const Ent &e : it->second)
			if (e.a.any || laddr_equal(e.a, ev)) return e.slot;
		return NONE;
	}

	// the device's walk of a candidate chain (cand_resolve in gys_device.hpp); t: the key's sub-table (nullptr: overflow host)
	uint32_t walk(uint32_t idx, uint64_t key, const LAddr &ev, const HostListeners *t) const
	{
		for (;; ++idx) {
			if (idx >= hl.cands.size()) {
				CHECK(false, "%s step %d: the chain of key %llx runs off the records", what, step, (unsigned long long)key);
				return NONE;
			}
			const ListenerCand &cd = hl.cands[idx];
			const bool same = (cd.ip32 | ev.ip32) ? cd.ip32 == ev.ip32 : memcmp(cd.ip128, ev.ip128, 16) == 0;
			if ((cd.flags & 1u) || same) {
				if (t)
					CHECK(cd.local < t->slots.size() && t->slots[cd.local] == cd.slot && t->keys[cd.local] == key, "%s step %d: record %u of key %llx names local %u, which is not its listener's",
					      what, step, idx, (unsigned long long)key, cd.local);
				return cd.slot;
			}
			if (cd.flags & 2u) return NONE;
		}
	}
	uint32_t mirror_resolve(uint64_t key, const LAddr &ev) const
	{
		if (hl.overflow) {
			auto ok = hl.okey.find(key);
			auto cf = hl.cand_first.find(key);
			CHECK(ok == hl.okey.end() || cf == hl.cand_first.end(), "%s step %d: key %llx is in okey and has candidates", what, step, (unsigned long long)key);
			if (ok != hl.okey.end()) return ok->second;
			return cf != hl.cand_first.end() ? walk(cf->second, key, ev, nullptr) : NONE;
		}
		const HostListeners &t = hl.sub.empty() ? hl : hl.sub[host_part_of(key, (uint32_t)hl.sub.size())];
		const uint32_t mask = (uint32_t)t.tbl.size() - 1;
		uint32_t h = host_tbl_slot(host_tbl_hash(key), mask);
		for (uint32_t probes = 0; probes <= mask; ++probes, h = (h + 1) & mask) {
			const uint64_t e = t.tbl[h];
			if (e == GYS_HOST_TBL_EMPTY) return NONE;
			if ((e >> 16) != key) continue;
			const uint32_t local = (uint32_t)(e & 0xFFFFu);
			if (local & GYS_LOCAL_GROUP) return walk(local & (GYS_LOCAL_GROUP - 1u), key, ev, &t);
			if (local >= t.slots.size()) {
				CHECK(false, "%s step %d: the entry of key %llx names local %u of %zu", what, step, (unsigned long long)key, local, t.slots.size());
				return NONE;
			}
			return t.slots[local];
		}
		return NONE;
	}

	void check_table(const HostListeners &t, uint32_t part, uint32_t nparts, size_t *prev_size)
	{
		CHECK(t.slots.size() <= GYS_HOST_MAX_LOCAL, "%s step %d: part %u holds %zu locals", what, step, part, t.slots.size());
		CHECK(t.keys.size() == t.slots.size(), "%s step %d: part %u has %zu keys, %zu slots", what, step, part, t.keys.size(), t.slots.size());
		const size_t sz = t.tbl.size();
		CHECK(sz >= 16 && (sz & (sz - 1)) == 0 && sz >= host_tbl_capacity(t.slots.size()), "%s step %d: part %u: table of %zu entries for %zu locals", what, step, part, sz, t.slots.size());
		CHECK(sz >= *prev_size, "%s step %d: part %u: the table shrank from %zu to %zu entries", what, step, part, *prev_size, sz);
		*prev_size = sz;
		std::set<uint64_t> keys(t.keys.begin(), t.keys.end()), in_tbl;
		for (uint64_t k : keys) CHECK(host_part_of(k, nparts) == part, "%s step %d: key %llx sits in part %u of %u", what, step, (unsigned long long)k, part, nparts);
		size_t used = 0;
		for (uint64_t e : t.tbl)
			if (e != GYS_HOST_TBL_EMPTY) {
				++used;
				CHECK(in_tbl.insert(e >> 16).second, "%s step %d: part %u: key %llx has two entries", what, step, part, (unsigned long long)(e >> 16));
			}
		CHECK(used == keys.size() && in_tbl == keys, "%s step %d: part %u: %zu entries for %zu keys", what, step, part, used, keys.size());
	}

	// everything the mirror promises, after a call (the engine's host_lst_flush rebuilds a dirty mirror before it uploads it)
	void verify(bool rebuild = true)
	{
		if (rebuild && hl.dirty) host_rebuild(hl);
		CHECK(hl.all_slots == all, "%s step %d: all_slots has %zu slots, the model %zu (or another order)", what, step, hl.all_slots.size(), all.size());
		if (!hl.overflow) {
			const uint32_t nparts = hl.sub.empty() ? 1u : (uint32_t)hl.sub.size();
			if (tbl_sizes.size() != nparts) tbl_sizes.assign(nparts, 0);
			if (hl.sub.empty()) check_table(hl, 0, 1, &tbl_sizes[0]);
			else {
				CHECK(hl.slots.empty() && hl.keys.empty(), "%s step %d: a cut host kept locals of its own", what, step);
				for (uint32_t p = 0; p < nparts; ++p) check_table(hl.sub[p], p, nparts, &tbl_sizes[p]);
			}
		}
		for (const auto &ks : kinds_seen) {
			std::set<int> kinds = ks.second;
			kinds.insert(A_NOBODY);
			kinds.erase(A_ANY);
			for (int kind : kinds) {
				const LAddr ev = event_addr(kind);
				const uint32_t want = model_resolve(ks.first, ev), got = mirror_resolve(ks.first, ev);
				CHECK(got == want, "%s step %d: key %llx address kind %d resolves to slot %d, the model says %d", what, step, (unsigned long long)ks.first, kind, (int)got, (int)want);
			}
		}
		++step;
	}

	uint32_t new_slot(bool reuse)
	{
		if (reuse && !free_slots.empty()) {
			const uint32_t s = *free_slots.begin();
			free_slots.erase(free_slots.begin());
			return s;
		}
		key_of_slot.push_back(0);
		return (uint32_t)key_of_slot.size() - 1;
	}

	// one registration call; returns the slots.  `check`: verify() afterwards
	std::vector<uint32_t> reg(const std::vector<gys_listener_info> &arr, bool reuse = false, bool check = true)
	{
		std::vector<uint32_t> sl;
		for (const gys_listener_info &li : arr) {
			const uint32_t s = new_slot(reuse);
			const uint64_t key = host_key48(li.netns, li.port);
			const LAddr a = listener_addr(li);
			sl.push_back(s);
			key_of_slot[s] = key;
			kinds_seen[key].insert(kind_of(li));
			std::vector<Ent> &v = lists[key];
			bool replaced = false;
			for (Ent &e : v)
				if (e.a.any || laddr_equal(e.a, a)) {
					e = Ent{s, a};
					replaced = true;
					break;
				}
			if (!replaced) v.push_back(Ent{s, a});
			all.push_back(s);
		}
		const uint32_t p0 = (uint32_t)hl.sub.size(), d0 = desc_used;
		host_lst_insert(hl, arr.data(), (uint32_t)arr.size(), sl.data(), desc_used, desc_cap);
		for (uint32_t s : sl) hl.all_slots.push_back(s); // (the engine's part, once the device has followed)
		const uint32_t p1 = (uint32_t)hl.sub.size();
		uint32_t cut = 0;
		for (uint32_t p = std::max(p0, 1u) * 2u; p <= p1; p *= 2u) cut += p;
		CHECK(desc_used - d0 == cut, "%s step %d: %u -> %u parts took %u descriptors, not %u", what, step, p0, p1, desc_used - d0, cut);
		CHECK(!cut || hl.sub_desc + p1 == desc_used, "%s step %d: the parts' descriptors start at %u of %u", what, step, hl.sub_desc, desc_used);
		CHECK(desc_used <= desc_cap, "%s step %d: %u descriptors of %u", what, step, desc_used, desc_cap);
		if (check) verify();
		return sl;
	}
	uint32_t reg1(uint32_t netns, uint16_t port, int kind) { return reg({listener(netns, port, kind)})[0]; }

	void del(const std::vector<uint32_t> &slots, bool check = true)
	{
		std::unordered_set<uint32_t> dead(slots.begin(), slots.end());
		std::set<uint64_t> touched, want_gone;
		for (uint32_t s : dead) {
			const uint64_t key = key_of_slot[s];
			touched.insert(key);
			auto it = lists.find(key);
			if (it != lists.end()) {
				auto &v = it->second;
				v.erase(std::remove_if(v.begin(), v.end(), [&](const Ent &e) { return e.slot == s; }), v.end());
				if (v.empty()) lists.erase(it);
			}
		}
		all.erase(std::remove_if(all.begin(), all.end(), [&](uint32_t s) { return dead.count(s) != 0; }), all.end());
		for (uint64_t k : touched)
			if (!lists.count(k)) want_gone.insert(k);
		std::vector<uint64_t> gone;
		host_lst_remove(hl, dead, key_of_slot.data(), gone);
		CHECK(std::set<uint64_t>(gone.begin(), gone.end()) == want_gone && gone.size() == want_gone.size(), "%s step %d: %zu keys reported gone, the model emptied %zu", what, step,
		      gone.size(), want_gone.size());
		for (uint32_t s : dead) {
			key_of_slot[s] = 0;
			free_slots.insert(s);
		}
		if (check) verify();
	}

	uint32_t at(uint32_t netns, uint16_t port, int kind) const { return mirror_resolve(host_key48(netns, port), event_addr(kind)); }
	bool in_all(uint32_t s) const { return std::find(hl.all_slots.begin(), hl.all_slots.end(), s) != hl.all_slots.end(); }
};

// n any-address listeners on distinct keys (netns 1, ports first ..)
std::vector<gys_listener_info> plain(uint32_t n, uint32_t first = 0)
{
	std::vector<gys_listener_info> v;
	for (uint32_t i = 0; i < n; ++i) v.push_back(listener(1 + (first + i) / 60000u, (uint16_t)(1 + (first + i) % 60000u), A_ANY));
	return v;
}

void test_sizes()
{
	CHECK(host_tbl_capacity(0) == 16 && host_tbl_capacity(4) == 16 && host_tbl_capacity(5) == 32, "capacity: small tables are a quarter full");
	CHECK(host_tbl_capacity(512) == 2048 && host_tbl_capacity(513) == 4096, "capacity: 512 / 513");
	CHECK(host_tbl_capacity(1024) == 4096 && host_tbl_capacity(1025) == 4096, "capacity: 1024 (a quarter) / 1025 (half full) share 4096 entries");
	CHECK(host_tbl_capacity(2048) == 4096 && host_tbl_capacity(2049) == 8192, "capacity: 2048 / 2049");
	for (uint32_t n : {1024u, 1025u, 2048u}) {
		World w;
		w.what = "one table";
		w.reg(plain(n - 1));
		w.reg(plain(1, n - 1));
		CHECK(w.hl.sub.empty() && !w.hl.overflow && w.hl.slots.size() == n && w.hl.tbl.size() == 4096 && w.desc_used == 0, "%u listeners: %zu parts, table of %zu", n, w.hl.sub.size(),
		      w.hl.tbl.size());
	}
	{
		World w;
		w.what = "2049";
		w.reg(plain(2048));
		w.reg(plain(1, 2048));
		CHECK(w.hl.sub.size() == 2 && !w.hl.overflow && w.desc_used == 2 && w.hl.sub_desc == 0, "2049 listeners: %zu parts, %u descriptors", w.hl.sub.size(), w.desc_used);
		if (w.hl.sub.size() == 2)
			CHECK(w.hl.sub[0].slots.size() + w.hl.sub[1].slots.size() == 2049, "2049 listeners: the parts hold %zu + %zu", w.hl.sub[0].slots.size(), w.hl.sub[1].slots.size());
		// deletion from a cut host: a few listeners of either part, one of them re-registered
		w.del({0, 1, 2, 3, 2048});
		w.reg(plain(1, 2));
		w.del({5});
	}
	{
		World w;
		w.what = "no descriptor room";
		w.desc_cap = 1; // one short of the first cut
		w.reg(plain(2048));
		CHECK(!w.hl.overflow, "2048 listeners overflowed");
		w.reg(plain(1, 2048));
		CHECK(w.hl.overflow && w.hl.sub.empty() && w.desc_used == 0 && w.hl.okey.size() == 2049, "descriptor room one short: overflow %d, %zu parts, %zu okey", (int)w.hl.overflow,
		      w.hl.sub.size(), w.hl.okey.size());
	}
}

// 2049 keys of ONE part under every cut: no cut relieves the full part, the parts double 2 -> 4 -> 8 -> 16, then the host overflows
void test_equal_part()
{
	World w;
	w.what = "equal part";
	std::vector<gys_listener_info> arr;
	uint32_t nany = 0;
	for (uint32_t netns = 1; arr.size() < 2049; ++netns) {
		if (host_part_of(host_key48(netns, 443), 16) != 5) continue;
		const bool bound = arr.size() % 8 == 3;
		arr.push_back(listener(netns, 443, bound ? A_V4_2 : A_ANY));
		nany += !bound;
	}
	const gys_listener_info last = arr.back();
	arr.pop_back();
	w.reg(arr);
	CHECK(w.hl.sub.empty() && !w.hl.overflow && w.desc_used == 0, "equal part: 2048 listeners are one table");
	w.reg({last});
	CHECK(w.hl.overflow && w.hl.sub.size() == 16 && w.desc_used == 2 + 4 + 8 + 16, "equal part: overflow %d with %zu parts and %u descriptors", (int)w.hl.overflow, w.hl.sub.size(),
	      w.desc_used);
	CHECK(w.hl.okey.size() == nany, "equal part: okey holds %zu keys, %u are any-address", w.hl.okey.size(), nany);
	for (const auto &kv : w.hl.okey) {
		auto it = w.lists.find(kv.first);
		CHECK(it != w.lists.end() && it->second.size() == 1 && it->second[0].a.any && it->second[0].slot == kv.second && !w.hl.chain.count(kv.first), "equal part: okey[%llx]",
		      (unsigned long long)kv.first);
	}
	// deletion from an overflow host: an any-address listener, a bound one, then new listeners on both keys
	const uint32_t s_any = 0, s_bound = 3;
	const uint64_t k_any = w.key_of_slot[s_any], k_bound = w.key_of_slot[s_bound];
	w.del({s_any, s_bound});
	CHECK(!w.hl.okey.count(k_any) && !w.hl.chain.count(k_bound), "equal part: the deleted keys stayed");
	w.reg({listener((uint32_t)(k_any >> 16), 443, A_V4_1), listener((uint32_t)(k_bound >> 16), 443, A_ANY)}, true);
	w.del({5});
}

void test_chains()
{
	{ // any -> bound replaces in place; the old slot is unreachable but still in all_slots
		World w;
		w.what = "any then bound";
		const uint32_t a = w.reg1(7, 80, A_ANY), b = w.reg1(7, 80, A_V4_1);
		CHECK(w.at(7, 80, A_V4_1) == b && w.at(7, 80, A_V4_2) == NONE && w.in_all(a) && w.in_all(b), "any then bound: %d / %d", (int)w.at(7, 80, A_V4_1), (int)w.at(7, 80, A_V4_2));
		CHECK(w.hl.slots.size() == 1, "any then bound: %zu locals", w.hl.slots.size());
		w.del({a}); // (the replaced one: nothing reachable changes)
		CHECK(w.at(7, 80, A_V4_1) == b, "any then bound: the replaced listener's deletion took the key");
	}
	{ // bound + bound: another address appends, the same address replaces; the IPv6 address that embeds an IPv4 one replaces that one
		World w;
		w.what = "bound and bound";
		const uint32_t a = w.reg1(7, 80, A_V4_1), b = w.reg1(7, 80, A_V4_2);
		CHECK(w.at(7, 80, A_V4_1) == a && w.at(7, 80, A_V4_2) == b && w.hl.slots.size() == 2, "bound + bound appends");
		const uint32_t c = w.reg1(7, 80, A_V4_2);
		CHECK(w.at(7, 80, A_V4_1) == a && w.at(7, 80, A_V4_2) == c && w.hl.slots.size() == 2 && w.in_all(b), "bound + the same address replaces");
		const uint32_t d = w.reg1(7, 80, A_V6_MAPPED_1);
		CHECK(w.at(7, 80, A_V4_1) == d && w.at(7, 80, A_V6_MAPPED_1) == d && w.at(7, 80, A_V4_2) == c && w.hl.slots.size() == 2, "the mapped IPv6 address replaces the IPv4 listener");
		// an any-address listener behind two bound ones takes what they leave
		const uint32_t e = w.reg1(7, 80, A_ANY);
		CHECK(w.at(7, 80, A_V4_1) == d && w.at(7, 80, A_V4_2) == c && w.at(7, 80, A_V6_1) == e && w.at(7, 80, A_NOBODY) == e && w.hl.slots.size() == 3, "any behind two bound");
		// deletion: the first, the last, the only listener of a chain
		w.del({d});
		CHECK(w.at(7, 80, A_V4_1) == e && w.at(7, 80, A_V4_2) == c, "the chain's first listener left");
		w.del({e});
		CHECK(w.at(7, 80, A_V4_1) == NONE && w.at(7, 80, A_V4_2) == c, "the chain's last listener left");
		w.del({c});
		CHECK(w.at(7, 80, A_V4_2) == NONE && w.hl.chain.empty() && w.hl.slots.empty(), "the chain's only listener left");
		// every listener of the key is gone: the key again, from free slots
		const uint32_t f = w.reg({listener(7, 80, A_V6_2)}, true)[0], g = w.reg({listener(7, 80, A_ANY)}, true)[0];
		CHECK(w.at(7, 80, A_V6_2) == f && w.at(7, 80, A_V4_3) == g, "the key registered again");
	}
	{ // two listeners of one key in ONE call, next to plain keys; then all of the key's listeners deleted in one call
		World w;
		w.what = "one call";
		const std::vector<uint32_t> s = w.reg({listener(3, 22, A_ANY), listener(7, 80, A_V6_1), listener(7, 80, A_V6_2), listener(3, 23, A_ANY)});
		CHECK(w.at(7, 80, A_V6_1) == s[1] && w.at(7, 80, A_V6_2) == s[2] && w.at(7, 80, A_V4_1) == NONE && w.at(3, 22, A_V4_1) == s[0], "two bound listeners in one call");
		w.del({s[1], s[2], s[0]});
		CHECK(w.at(7, 80, A_V6_1) == NONE && w.at(3, 23, A_V4_1) == s[3] && w.hl.slots.size() == 1, "a key's listeners deleted together");
	}
}

// a mirror left dirty (a flush that failed after a deletion compacted the locals): the next insert has to rebuild before it looks keys up
void test_dirty_recovery()
{
	World w;
	w.what = "dirty";
	const std::vector<uint32_t> s = w.reg(plain(6));
	w.del({s[1]}, false); // (no verify: nobody rebuilds)
	CHECK(w.hl.dirty, "dirty: a deletion left the mirror clean");
	const gys_listener_info again = plain(1, 4)[0]; // the key of s[4], whose local moved up
	const uint32_t t = w.reg({again}, false, false)[0];
	CHECK(!w.hl.dirty, "dirty: the insert did not rebuild");
	w.verify(false);
	CHECK(w.at(again.netns, again.port, A_V4_1) == t && w.at(1, 6, A_V4_1) == s[5], "dirty: the re-registered key resolves to %d", (int)w.at(again.netns, again.port, A_V4_1));
}

// seeded random calls: registrations of 1 .. 4 listeners on a small universe of keys and addresses, deletions of 1 .. 3 live-or-replaced slots
void random_steps(World &w, std::mt19937_64 &rng, int steps, uint32_t nkeys, uint32_t fresh_first)
{
	auto r = [&](uint64_t m) { return (uint32_t)(rng() % m); };
	uint32_t fresh = fresh_first;
	for (int i = 0; i < steps; ++i) {
		if (w.all.empty() || r(100) < 60) {
			std::vector<gys_listener_info> arr;
			for (uint32_t k = 1 + r(4); k; --k) {
				if (fresh_first && r(3) == 0) arr.push_back(plain(1, fresh++)[0]); // (a key nobody has: the host grows)
				else arr.push_back(listener(100 + r(nkeys) / 4u, (uint16_t)(8000 + r(4)), r(3) ? 1 + (int)r(A_NOBODY - 1) : A_ANY));
			}
			w.reg(arr, r(2) != 0);
		} else {
			std::vector<uint32_t> d;
			for (uint32_t k = 1 + r(3); k; --k) d.push_back(w.all[r(w.all.size())]);
			w.del(d);
		}
	}
}

void test_random(uint64_t seed)
{
	std::mt19937_64 rng(seed);
	{
		World w;
		w.what = "random small";
		random_steps(w, rng, 600, 24, 0);
	}
	{ // a host that is cut while the sequence runs: 2040 plain listeners, then chains and new keys across the 2048 line
		World w;
		w.what = "random cut";
		w.reg(plain(2040));
		random_steps(w, rng, 150, 16, 2040);
		CHECK(w.hl.sub.size() >= 2 && !w.hl.overflow, "random cut: %zu parts, overflow %d", w.hl.sub.size(), (int)w.hl.overflow);
	}
	{ // a host that overflows for want of descriptors: two parts fill up, the cut into four is refused
		World w;
		w.what = "random overflow";
		w.desc_cap = 2;
		w.reg(plain(2100));
		w.reg({listener(100, 8000, A_V4_1), listener(100, 8000, A_V4_2), listener(100, 8001, A_ANY)});
		CHECK(w.hl.sub.size() == 2 && !w.hl.overflow, "random overflow: %zu parts before the overflow", w.hl.sub.size());
		w.reg(plain(2100, 2100));
		CHECK(w.hl.overflow && w.desc_used == 2, "random overflow: overflow %d, %u descriptors", (int)w.hl.overflow, w.desc_used);
		random_steps(w, rng, 150, 16, 4200);
	}
}

// --tables FILE: the registry calls of tests/lstkeys.py's scenarios ("host" / "reg n" + n x "netns(hex) port slot address-kind" / "del n" + n slots / "dump"
// / "end") through host_lst_insert and host_lst_remove + host_rebuild; every "dump" prints the host's sub-tables, local -> slot lists and candidate records
// (tests/test_hostlst_cpu.py compares them entry for entry with the Python restatement's prediction)
int tables_mode(const char *path)
{
	FILE *f = fopen(path, "r");
	if (!f) {
		printf("cannot read %s\n", path);
		return 2;
	}
	HostListeners hl;
	uint32_t desc_used = 0;
	std::vector<uint64_t> key_of_slot;
	char op[16];
	unsigned n = 0;
	while (fscanf(f, "%15s", op) == 1 && strcmp(op, "end") != 0) {
		if (!strcmp(op, "host")) {
			hl = HostListeners{};
			hl.tbl.assign(16, GYS_HOST_TBL_EMPTY); // (as gys_register_host leaves a new host)
			desc_used = 0;
			key_of_slot.clear();
			printf("host\n");
		} else if (!strcmp(op, "reg") && fscanf(f, "%u", &n) == 1) {
			std::vector<gys_listener_info> arr;
			std::vector<uint32_t> sl;
			for (unsigned i = 0; i < n; ++i) {
				unsigned netns, port, slot, kind;
				if (fscanf(f, "%x %u %u %u", &netns, &port, &slot, &kind) != 4 || kind >= A_KINDS) return 2;
				arr.push_back(listener(netns, (uint16_t)port, (int)kind));
				sl.push_back(slot);
				if (key_of_slot.size() <= slot) key_of_slot.resize(slot + 1, 0);
				key_of_slot[slot] = host_key48(netns, (uint16_t)port);
			}
			host_lst_insert(hl, arr.data(), n, sl.data(), desc_used, 1000);
		} else if (!strcmp(op, "del") && fscanf(f, "%u", &n) == 1) {
			std::unordered_set<uint32_t> dead;
			for (unsigned i = 0; i < n; ++i) {
				unsigned slot;
				if (fscanf(f, "%u", &slot) != 1) return 2;
				dead.insert(slot);
			}
			std::vector<uint64_t> gone;
			host_lst_remove(hl, dead, key_of_slot.data(), gone);
			CHECK(gone.size() == n, "%zu keys gone after %u plain listeners were deleted", gone.size(), n);
		} else if (!strcmp(op, "dump")) {
			if (hl.dirty) host_rebuild(hl); // (the engine's flush, before it uploads the tables)
			CHECK(!hl.overflow, "the host overflowed");
			const size_t np = hl.sub.empty() ? 1 : hl.sub.size();
			printf("tables %zu\n", np);
			for (size_t p = 0; p < np; ++p) {
				const HostListeners &t = hl.sub.empty() ? hl : hl.sub[p];
				printf("part %zu %zu %zu\n", p, t.tbl.size(), t.slots.size());
				for (uint64_t e : t.tbl) printf("%llx ", (unsigned long long)e);
				printf("\n");
				for (uint32_t s : t.slots) printf("%u ", s);
				printf("\n");
			}
			printf("cands %zu\n", hl.cands.size());
			for (const ListenerCand &cd : hl.cands) printf("%u %u %u %u\n", cd.ip32, cd.flags, cd.local, cd.slot);
		} else {
			printf("bad line '%s'\n", op);
			return 2;
		}
	}
	fclose(f);
	if (fails) return 1;
	printf("host listener tables ok\n");
	return 0;
}
} // namespace

int main(int argc, char **argv)
{
	if (argc > 2 && !strcmp(argv[1], "--tables")) return tables_mode(argv[2]);
	const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
	setvbuf(stdout, nullptr, _IOLBF, 0); // (a sanitizer abort must not take the lines of the failed checks with it)
	test_sizes();
	test_equal_part();
	test_chains();
	test_dirty_recovery();
	test_random(seed);
	if (fails) {
		printf("%d checks failed\n", fails);
		return 1;
	}
	printf("host listeners ok (seed %llu)\n", (unsigned long long)seed);
	return 0;
}
