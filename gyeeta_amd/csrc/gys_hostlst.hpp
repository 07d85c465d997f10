// gys_hostlst.hpp -- the host mirror of one host's listeners as pure host code: the open-addressing sub-tables k_resp_host probes, the cut of
// a many-listener host into parts, the chains of the keys that need the server address, the overflow fallback and the dirty / rebuild
// protocol.  No HIP call and no gys_ctx in here: the engine uploads what these build into its device pools (host_lst_flush in
// gys_engine.hip) and hands in the part-descriptor allocator as two numbers; tests/cpp/test_hostlst.cc checks the mirror on the CPU.
// Needs GYS_HOST_TBL_EMPTY (gys_kernels.hpp) declared before it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "gys_device.hpp"

namespace gys {

// host mirror of one host's listener sub-table (the device copy lives in the table / list pools, see k_resp_host)
struct HostListeners {
	std::vector<uint64_t> tbl;   // open addressing, entries (netns:32|port:16) << 16 | local index, ~0 = free
	std::vector<uint32_t> slots; // local index -> service slot
	std::vector<uint32_t> all_slots; // every service slot ever registered for the host (queries)
	std::vector<uint64_t> keys;  // local index -> (netns:32|port:16)
	uint32_t tbl_off = 0, tbl_cap = 0, lst_off = 0;
	bool on_device = false;
	bool overflow = false;       // more listeners than the LDS path supports (or pools exhausted): general pipeline only
	// A host with more than GYS_HOST_MAX_LOCAL listeners is cut into `sub.size()` PARTS (a power of two): a listener belongs to part
	// host_part_of(key48), every part has a sub-table of its own (the members above are then unused) and its own descriptor
	// hdesc[sub_desc + part]; k_resp_host runs one workgroup per (segment, part), each resolving only its part's events.
	std::vector<HostListeners> sub;
	uint32_t sub_desc = 0;
	// Keys with CANDIDATES (host level; a part's sub-table only holds the entries): a (netns, port) key whose listener is bound to an address, or
	// that has more than one listener.  chain[key48] = its listeners in registration order; `cands` = the device records of all chains
	// (a region of the candidate pool, rebuilt when a chain changes); a key that is not in `chain` has ONE any-address listener and its
	// sub-table entry names the local index directly, as before.
	struct LAddr {
		uint32_t ip32 = 0;
		uint32_t ip128[4] = {0, 0, 0, 0};
		bool any = true;
	};
	struct ChainEnt {
		uint32_t slot;
		LAddr a;
	};
	std::unordered_map<uint64_t, std::vector<ChainEnt>> chain;
	std::vector<ListenerCand> cands;
	std::unordered_map<uint64_t, uint32_t> cand_first; // key48 -> first record of its chain in `cands`
	uint32_t cand_off = 0, cand_cap = 0;
	bool dirty = false;                                 // a chain changed: tables and candidate region are rebuilt at the end of the registration call
	std::unordered_map<uint64_t, uint32_t> okey;        // overflow hosts (no sub-tables): key48 -> slot of the key's one any-address listener
};

#define GYS_HOST_MAX_LOCAL 2048u // listeners per sub-table the LDS path supports (32 KB LDS table + 48 KB per-key areas + the tile image)
#define GYS_HOST_MAX_PARTS 16u   // ... and parts per host: up to 32768 listeners per host on the host-local path

inline uint32_t next_pow2(uint64_t v)
{
	uint64_t p = 1;
	while (p < v) p <<= 1;
	return (uint32_t)p;
}

inline uint64_t host_key48(uint32_t netns, uint16_t port) { return ((uint64_t)netns << 16) | (uint64_t)port; }

inline int64_t host_tbl_find(const HostListeners &hl, uint64_t key48)
{
	if (hl.tbl.empty()) return -1;
	const uint32_t mask = (uint32_t)hl.tbl.size() - 1;
	uint32_t h = host_tbl_slot(host_tbl_hash(key48), mask);
	for (uint32_t probes = 0; probes <= mask; ++probes) {
		const uint64_t e = hl.tbl[h];
		if (e == GYS_HOST_TBL_EMPTY) return -1;
		if ((e >> 16) == key48) return (int64_t)h;
		h = (h + 1) & mask;
	}
	return -1;
}

// `local`: a local index, or GYS_LOCAL_GROUP | first candidate of the key's chain
inline void host_tbl_put(HostListeners &hl, uint64_t key48, uint32_t local)
{
	const uint32_t mask = (uint32_t)hl.tbl.size() - 1;
	uint32_t h = host_tbl_slot(host_tbl_hash(key48), mask);
	while (hl.tbl[h] != GYS_HOST_TBL_EMPTY) h = (h + 1) & mask;
	hl.tbl[h] = (key48 << 16) | (uint64_t)local;
}

inline uint32_t host_part_of(uint64_t key48, uint32_t nparts) { return host_tbl_part(host_tbl_hash(key48), nparts - 1u); }

// capacity of a sub-table of n listeners: a QUARTER full while that is at most GYS_HOST_TBL_SPARSE entries (32 KiB of LDS; 97 % of the
// events then find their listener in the two entries k_resp_host reads at once), half full above (up to 8192 entries for 4096 listeners)
#define GYS_HOST_TBL_SPARSE 4096u
inline uint32_t host_tbl_capacity(size_t n)
{
	const uint32_t c4 = next_pow2(std::max<uint64_t>(16, (uint64_t)n * 4));
	return c4 <= GYS_HOST_TBL_SPARSE ? c4 : std::max<uint32_t>(GYS_HOST_TBL_SPARSE, next_pow2(std::max<uint64_t>(16, (uint64_t)n * 2)));
}

// one listener into one sub-table (grown and rehashed at half full).  `top`: the host (holder of the chains): with chains around, a
// rehash has to know which keys' entries name a candidate region -- the whole host is rebuilt at the end of the registration call instead
inline void host_tbl_insert(HostListeners &top, HostListeners &t, uint64_t key48, uint32_t slot)
{
	const uint32_t local = (uint32_t)t.slots.size();
	t.slots.push_back(slot);
	t.keys.push_back(key48);
	// (the plain entries are kept current in any case -- later listeners of the same call look their key up in them; entries of keys with
	// candidates are put right by host_rebuild at the end of the call)
	if (host_tbl_capacity(t.slots.size()) > t.tbl.size()) {
		t.tbl.assign(host_tbl_capacity(t.slots.size()), GYS_HOST_TBL_EMPTY);
		for (uint32_t l = 0; l < t.keys.size(); ++l) host_tbl_put(t, t.keys[l], l);
		if (!top.chain.empty()) top.dirty = true;
	} else {
		host_tbl_put(t, key48, local);
	}
}

// the device record of entry k of a chain (`local`: its local index in the key's sub-table; an overflow host has none)
inline ListenerCand host_cand_record(const std::vector<HostListeners::ChainEnt> &ch, size_t k, uint32_t local)
{
	ListenerCand cd{};
	cd.ip32 = ch[k].a.ip32;
	cd.flags = (ch[k].a.any ? 1u : 0u) | (k + 1 == ch.size() ? 2u : 0u);
	cd.local = local;
	cd.slot = ch[k].slot;
	memcpy(cd.ip128, ch[k].a.ip128, 16);
	return cd;
}

// all tables of a host and its candidate records from the locals and the chains (after a chain changed)
inline void host_rebuild(HostListeners &hl)
{
	hl.cands.clear();
	hl.cand_first.clear();
	auto one = [&](HostListeners &t) {
		t.tbl.assign(std::max<size_t>(t.tbl.size(), host_tbl_capacity(t.slots.size())), GYS_HOST_TBL_EMPTY);
		std::unordered_map<uint32_t, uint32_t> local_of; // slot -> local, for the locals of keys with candidates
		for (uint32_t l = 0; l < t.keys.size(); ++l)
			if (hl.chain.count(t.keys[l])) local_of[t.slots[l]] = l;
		for (uint32_t l = 0; l < t.keys.size(); ++l) {
			const uint64_t key48 = t.keys[l];
			auto ch = hl.chain.find(key48);
			if (ch == hl.chain.end()) {
				host_tbl_put(t, key48, l);
				continue;
			}
			if (hl.cand_first.count(key48)) continue; // (the key's entry was made when its first local came by)
			const uint32_t first = (uint32_t)hl.cands.size();
			hl.cand_first[key48] = first;
			for (size_t k = 0; k < ch->second.size(); ++k) {
				auto lo = local_of.find(ch->second[k].slot);
				hl.cands.push_back(host_cand_record(ch->second, k, lo != local_of.end() ? lo->second : 0u));
			}
			host_tbl_put(t, key48, GYS_LOCAL_GROUP | first);
		}
	};
	if (hl.overflow) { // (no sub-tables: only the records, for the global table)
		for (auto &kv : hl.chain) {
			hl.cand_first[kv.first] = (uint32_t)hl.cands.size();
			for (size_t k = 0; k < kv.second.size(); ++k) hl.cands.push_back(host_cand_record(kv.second, k, 0u));
		}
	} else if (hl.sub.empty()) {
		one(hl);
	} else {
		for (HostListeners &t : hl.sub) one(t);
	}
	hl.dirty = false;
}

// cuts the host's listeners into nparts sub-tables (from one table, or from fewer parts); false: no descriptor room / too many parts.
// desc_used / desc_cap: the allocator of the part descriptors (the descriptors of the previous cut are abandoned, like outgrown table regions)
inline bool host_lst_repartition(HostListeners &hl, uint32_t nparts, uint32_t &desc_used, uint32_t desc_cap)
{
	if (nparts > GYS_HOST_MAX_PARTS || desc_used + nparts > desc_cap) return false;
	std::vector<std::pair<uint64_t, uint32_t>> all;
	if (hl.sub.empty()) {
		for (uint32_t l = 0; l < hl.keys.size(); ++l) all.emplace_back(hl.keys[l], hl.slots[l]);
	} else {
		for (const HostListeners &t : hl.sub)
			for (uint32_t l = 0; l < t.keys.size(); ++l) all.emplace_back(t.keys[l], t.slots[l]);
	}
	hl.tbl.clear();
	hl.slots.clear();
	hl.keys.clear();
	hl.sub.assign(nparts, HostListeners{});
	hl.sub_desc = desc_used;
	desc_used += nparts;
	for (const auto &kv : all) host_tbl_insert(hl, hl.sub[host_part_of(kv.first, nparts)], kv.first, kv.second);
	for (HostListeners &t : hl.sub)
		if (t.tbl.empty()) t.tbl.assign(16, GYS_HOST_TBL_EMPTY);
	if (!hl.chain.empty()) hl.dirty = true;
	return true;
}

// GY_IP_ADDR of a registered listener (set_ip(uint32_t) / set_ip(unsigned __int128), common/gy_common_inc.h:10673-10692)
inline HostListeners::LAddr listener_addr(const gys_listener_info &li)
{
	HostListeners::LAddr a;
	a.any = li.is_any_ip != 0;
	if (a.any) return a;
	if (li.addr_is_v6) {
		memcpy(a.ip128, li.addr, 16);
		a.ip32 = ip6_embedded_v4(a.ip128);
	} else {
		memcpy(&a.ip32, li.addr, 4);
	}
	return a;
}
inline bool laddr_equal(const HostListeners::LAddr &x, const HostListeners::LAddr &y) // GY_IP_ADDR::operator== (common/gy_common_inc.h:10629-10636)
{
	return (x.ip32 | y.ip32) ? x.ip32 == y.ip32 : memcmp(x.ip128, y.ip128, 16) == 0;
}

// the table a key's listeners live in: the host's own one, or the key's part
inline HostListeners &host_tbl_of(HostListeners &hl, uint64_t key48) { return hl.sub.empty() ? hl : hl.sub[host_part_of(key48, (uint32_t)hl.sub.size())]; }

// the local index that holds `slot` in the table of key48 gets `new_slot` (a listener replaced in place)
inline void host_rebind_local(HostListeners &hl, uint64_t key48, uint32_t slot, uint32_t new_slot)
{
	if (hl.overflow) return;
	HostListeners &t = host_tbl_of(hl, key48);
	for (uint32_t l = 0; l < t.slots.size(); ++l)
		if (t.slots[l] == slot && t.keys[l] == key48) {
			t.slots[l] = new_slot;
			return;
		}
}

// a new local (key48, slot); false: the host left the LDS path
inline bool host_new_local(HostListeners &hl, uint64_t key48, uint32_t slot, uint32_t &desc_used, uint32_t desc_cap)
{
	if (hl.overflow) return false;
	while (host_tbl_of(hl, key48).slots.size() >= GYS_HOST_MAX_LOCAL) { // the (part of the) host is full: twice the parts
		if (host_lst_repartition(hl, hl.sub.empty() ? 2u : (uint32_t)hl.sub.size() * 2u, desc_used, desc_cap)) continue;
		// beyond what the LDS sub-tables take: batches with this host use the general pipeline.  The keys of its any-address
		// listeners move to a flat map (what a later registration on the same key has to find)
		hl.overflow = true;
		auto take = [&](const HostListeners &s) {
			for (uint32_t l = 0; l < s.keys.size(); ++l)
				if (!hl.chain.count(s.keys[l])) hl.okey[s.keys[l]] = s.slots[l];
		};
		if (hl.sub.empty()) take(hl);
		else for (const HostListeners &s : hl.sub) take(s);
		return false;
	}
	host_tbl_insert(hl, host_tbl_of(hl, key48), key48, slot);
	return true;
}

// n listeners of the host into its mirror, arr[i] as service slot slot_of[i] (the device copy follows by host_lst_flush)
inline void host_lst_insert(HostListeners &hl, const gys_listener_info *arr, uint32_t n, const uint32_t *slot_of, uint32_t &desc_used, uint32_t desc_cap)
{
	// (a flush that failed after gys_delete_listeners compacted keys / slots left the tables behind the locals: the lookups below need them)
	if (hl.dirty) host_rebuild(hl);
	for (uint32_t i = 0; i < n; ++i) {
		const uint64_t key48 = host_key48(arr[i].netns, arr[i].port);
		const uint32_t slot = slot_of[i];
		const HostListeners::LAddr a = listener_addr(arr[i]);
		auto ch = hl.chain.find(key48);
		if (ch != hl.chain.end()) {
			// insert_or_replace (common/gy_socket_stat.cc:1372, :7779) under operator==(listener, NS_IP_PORT) (gy_socket_stat.h:708-714): the first
			// listener of the key that is any-address or bound to the new one's address is replaced in place, else the new one goes last
			bool replaced = false;
			for (HostListeners::ChainEnt &e : ch->second) {
				if (e.a.any || laddr_equal(e.a, a)) {
					host_rebind_local(hl, key48, e.slot, slot);
					e.slot = slot;
					e.a = a;
					replaced = true;
					break;
				}
			}
			if (!replaced) {
				ch->second.push_back(HostListeners::ChainEnt{slot, a});
				host_new_local(hl, key48, slot, desc_used, desc_cap);
			}
			hl.dirty = true;
			continue;
		}
		// the key has no candidates: no listener yet, or one any-address listener (which every new listener of the key replaces)
		uint32_t old_slot = GYS_NOSLOT;
		if (hl.overflow) {
			auto it = hl.okey.find(key48);
			if (it != hl.okey.end()) old_slot = it->second;
		} else {
			HostListeners &t = host_tbl_of(hl, key48);
			const int64_t pos = host_tbl_find(t, key48);
			if (pos >= 0) {
				uint32_t &ls = t.slots[(uint32_t)(t.tbl[(size_t)pos] & (GYS_LOCAL_GROUP - 1u))];
				old_slot = ls;
				ls = slot; // (re-registration of a listener tuple rebinds it to the newest slot)
			}
		}
		if (old_slot != GYS_NOSLOT) {
			if (hl.overflow && a.any) hl.okey[key48] = slot;
		} else if (!hl.overflow) {
			host_new_local(hl, key48, slot, desc_used, desc_cap);
			if (hl.overflow && a.any) hl.okey[key48] = slot; // (the host left the LDS path with this very listener)
		} else if (a.any) {
			hl.okey[key48] = slot;
		}
		if (!a.any) { // bound to an address: the key gets candidates
			hl.okey.erase(key48);
			hl.chain[key48].push_back(HostListeners::ChainEnt{slot, a});
			hl.dirty = true;
		}
	}
}

// the listeners in service slots `dead` leave the host's chains, okey, all_slots and sub-tables (key_of_slot[s]: the key48 slot s was
// registered under); the mirror is left dirty.  keys_gone += the (netns, port) keys that lost their last listener
inline void host_lst_remove(HostListeners &hl, const std::unordered_set<uint32_t> &dead, const uint64_t *key_of_slot, std::vector<uint64_t> &keys_gone)
{
	std::unordered_set<uint64_t> touched; // keys a deleted listener was registered under
	for (uint32_t s : dead) {
		const uint64_t key48 = key_of_slot[s];
		touched.insert(key48);
		auto ch = hl.chain.find(key48);
		if (ch != hl.chain.end()) {
			auto &v = ch->second;
			v.erase(std::remove_if(v.begin(), v.end(), [&](const HostListeners::ChainEnt &e) { return e.slot == s; }), v.end());
			if (v.empty()) hl.chain.erase(ch);
		}
		auto ok = hl.okey.find(key48);
		if (ok != hl.okey.end() && ok->second == s) hl.okey.erase(ok);
	}
	hl.all_slots.erase(std::remove_if(hl.all_slots.begin(), hl.all_slots.end(), [&](uint32_t s) { return dead.count(s) != 0; }), hl.all_slots.end());
	std::unordered_set<uint64_t> live; // touched keys that still have a listener bound
	if (hl.overflow) {
		for (uint64_t k : touched)
			if (hl.chain.count(k) || hl.okey.count(k)) live.insert(k);
	} else {
		// the locals (key, slot) of the deleted listeners go; the survivors close up and the tables are rebuilt from them, hole-free
		auto compact = [&](HostListeners &t) {
			size_t w = 0;
			for (size_t l = 0; l < t.slots.size(); ++l) {
				if (dead.count(t.slots[l])) continue;
				if (touched.count(t.keys[l])) live.insert(t.keys[l]);
				t.slots[w] = t.slots[l];
				t.keys[w] = t.keys[l];
				++w;
			}
			t.slots.resize(w);
			t.keys.resize(w);
		};
		if (hl.sub.empty()) compact(hl);
		else for (HostListeners &t : hl.sub) compact(t);
	}
	for (uint64_t k : touched)
		if (!live.count(k)) keys_gone.push_back(k);
	hl.dirty = true;
}

} // namespace gys
