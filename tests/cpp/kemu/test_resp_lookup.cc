// TEST INFRASTRUCTURE (CPU): k_resp_host's listener lookup on the key sets of tests/lstkeys.py, under the CPU stand-in of the device model.
// The file named on the command line holds WORLDS: per host its listeners (in the order of their oracle slots), the sub-table(s) and
// local -> slot lists the Python builder predicts (pinned to gys_hostlst.hpp by tests/test_hostlst_cpu.py) and one segment of events.
// The keys are searched so that runs wrap around the table's end (the copy of entry 0 behind the last entry, the wrap of the walk),
// grow long, collide in one 32-bit half of the packed compare, or equal the key bits of a free entry (the all-ones key); a host in two
// parts runs one workgroup per part.  Every world is one launch of k_resp_host<16 or 8, false, false, false, 0 or 1> over all its hosts -- tables
// of different sizes share one LDS layout -- and is compared with the oracle's sequential engine fed the same bytes: the three counters,
// HLL registers, the all-service histogram, every key's buffered values (as multisets) and digest.
// A world whose hosts have keys with candidates (listeners bound to an address: the entry names a candidate record) runs the MODE 1
// instance over the predicted candidate records; the IPv6 instance (MODE 2) is left to the GPU tests.
// Built plain and with -fsanitize=address by tests/test_kernel_logic_resp_lookup_cpu.py.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../../gyeeta_amd/csrc/gys_kernels.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>

#include "../../../oracle/gy_oracle.h"

extern "C" {
struct gyo_engine;
gyo_engine *gyo_engine_new_cap(uint32_t max_services, int enable_td, uint32_t td_cap);
void gyo_engine_free(gyo_engine *e);
int gyo_engine_register(gyo_engine *e, uint32_t host_slot, uint64_t glob_id, uint32_t netns, uint16_t port);
int gyo_engine_register_addr(gyo_engine *e, uint32_t host_slot, uint64_t glob_id, uint32_t netns, uint16_t port, const uint8_t *ip, int is_v6, int is_any);
void gyo_engine_resp_batch(gyo_engine *e, const uint8_t *ev24, uint64_t n, const uint32_t *seg_host, const uint64_t *seg_first, uint32_t nsegs);
const uint8_t *gyo_engine_hll(const gyo_engine *e);
const gyo_hist_serial *gyo_engine_ghist(const gyo_engine *e);
int64_t gyo_engine_gmax(const gyo_engine *e);
const gyo_td_buffered *gyo_engine_td(const gyo_engine *e, uint32_t slot);
const uint64_t *gyo_engine_counters(const gyo_engine *e);
}

#include <string.h>
#include <utility>
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

struct HostIn {
	char name[64];
	uint32_t nlst = 0, nparts = 0, nev = 0, ncand = 0;
	std::vector<std::pair<uint32_t, uint32_t>> keys; // (netns, port) in oracle slot order
	std::vector<uint32_t> kind;                      // address kind: 0 any address, k: bound to 10.0.0.k
	std::vector<ListenerCand> cands;                 // (slot: service slot of the world)
	std::vector<std::vector<uint64_t>> tbl;          // per part
	std::vector<std::vector<uint32_t>> slots;        // per part: local index -> service slot of the world
	std::vector<uint32_t> ev;                        // 6 words per event
};

bool read_host(FILE *f, HostIn &h)
{
	if (fscanf(f, " host %63s %u %u %u %u", h.name, &h.nlst, &h.nparts, &h.nev, &h.ncand) != 5) return false;
	for (uint32_t i = 0; i < h.nlst; ++i) {
		unsigned ns, pt, kind;
		if (fscanf(f, "%x %u %u", &ns, &pt, &kind) != 3) return false;
		h.keys.emplace_back(ns, pt);
		h.kind.push_back(kind);
	}
	for (uint32_t i = 0; i < h.ncand; ++i) {
		ListenerCand cd{};
		if (fscanf(f, "%u %u %u %u", &cd.ip32, &cd.flags, &cd.local, &cd.slot) != 4) return false;
		h.cands.push_back(cd);
	}
	for (uint32_t p = 0; p < h.nparts; ++p) {
		unsigned cap, nl;
		if (fscanf(f, " part %u %u", &cap, &nl) != 2) return false;
		h.tbl.emplace_back(cap);
		h.slots.emplace_back(nl);
		for (auto &e : h.tbl.back()) {
			unsigned long long v;
			if (fscanf(f, "%llx", &v) != 1) return false;
			e = v;
		}
		for (auto &s : h.slots.back())
			if (fscanf(f, "%u", &s) != 1) return false;
	}
	h.ev.resize((size_t)h.nev * 6);
	for (auto &w : h.ev)
		if (fscanf(f, "%x", &w) != 1) return false;
	return true;
}

template <int TPT, int MODE>
void launch_resp(uint32_t nwg, size_t dyn, const RespHostP &hp)
{
	kemu::launch(nwg, GYS_RESP_THREADS(TPT), dyn, [&] { k_resp_host<TPT, false, false, false, MODE>(hp); });
}

uint64_t run_world(const char *wname, uint32_t tpt, uint32_t mode, std::vector<HostIn> &hosts)
{
	const uint32_t NH = (uint32_t)hosts.size(), TILE = tpt * GYS_RESP_THREADS(16);
	const uint32_t pend_cap = GYS_TD_PEND_CAP, fast = 1024u, pcap = fast + 128u;
	uint32_t nsvc = 0;
	for (const HostIn &h : hosts) nsvc += h.nlst;

	// ---- registration: oracle engine + the host-local structures k_resp_host reads (descriptors of the hosts first, then of the parts)
	gyo_engine *orc = gyo_engine_new_cap(nsvc + 8, 1, pend_cap);
	std::vector<HostDesc> hdesc(NH);
	std::vector<uint64_t> htbl;
	std::vector<uint32_t> hlst, svc_host(nsvc);
	std::vector<gys_resp_seg> segs;
	std::vector<uint32_t> seg_host;
	std::vector<uint64_t> seg_first;
	std::vector<uint8_t> ev;
	std::vector<ListenerCand> cand(1); // (never empty: the pointer is handed over in any case)
	uint32_t max_tbl = 0, max_l = 0, slot0 = 0;
	for (uint32_t h = 0; h < NH; ++h) {
		const HostIn &in = hosts[h];
		for (uint32_t s = 0; s < in.nlst; ++s) {
			const uint8_t ip[16] = {10, 0, 0, (uint8_t)in.kind[s]};
			const int slot = gyo_engine_register_addr(orc, h, 0x100000ull * (h + 1) + s, in.keys[s].first, (uint16_t)in.keys[s].second, ip, 0, in.kind[s] == 0);
			CHECK(mode == 1 || in.kind[s] == 0, "%s %s: a bound listener in a MODE 0 world", wname, in.name);
			CHECK(slot == (int)(slot0 + s), "%s: oracle slot %d", wname, slot);
			svc_host[slot0 + s] = h;
		}
		slot0 += in.nlst;
		CHECK(in.nev > 0 && in.nev < TILE, "%s %s: %u events (a host's events stay under one tile)", wname, in.name, in.nev);
		seg_host.push_back(h);
		seg_first.push_back(ev.size() / 24);
		const uint32_t cand_off = (uint32_t)cand.size();
		cand.insert(cand.end(), in.cands.begin(), in.cands.end());
		for (uint32_t p = 0; p < in.nparts; ++p) {
			const uint32_t cap = (uint32_t)in.tbl[p].size();
			HostDesc d{(uint32_t)htbl.size(), cap - 1, (uint32_t)in.slots[p].size(), (uint32_t)hlst.size(), p, in.nparts - 1, cand_off, 0};
			htbl.insert(htbl.end(), in.tbl[p].begin(), in.tbl[p].end());
			hlst.insert(hlst.end(), in.slots[p].begin(), in.slots[p].end());
			for (uint32_t s : in.slots[p]) CHECK(s < nsvc && svc_host[s] == h, "%s %s: local list names slot %u", wname, in.name, s);
			max_tbl = std::max(max_tbl, cap);
			max_l = std::max(max_l, d.nlst);
			if (in.nparts == 1) {
				hdesc[h] = d;
				segs.push_back(gys_resp_seg{h, 0u, ev.size() / 24});
			} else { // one workgroup per (segment, part): gys_resp_seg.reserved = descriptor index + 1
				hdesc.push_back(d);
				segs.push_back(gys_resp_seg{h, (uint32_t)hdesc.size(), ev.size() / 24});
			}
		}
		const size_t at = ev.size();
		ev.resize(at + (size_t)in.nev * 24);
		memcpy(&ev[at], in.ev.data(), (size_t)in.nev * 24);
	}
	const uint64_t n = ev.size() / 24;
	// (exactly 3 n words on the heap: the kernel may not address a byte at or beyond 24 n)
	uint64_t *ev64 = (uint64_t *)malloc(n * 24);
	memcpy(ev64, ev.data(), n * 24);
	gyo_engine_resp_batch(orc, ev.data(), n, seg_host.data(), seg_first.data(), NH);

	// ---- engine state
	std::vector<int64_t> td_sum((size_t)nsvc * GYS_TD_NB, 0);
	std::vector<uint32_t> td_cnt((size_t)nsvc * GYS_TD_NB, 0), td_pend((size_t)nsvc * pcap, 0), td_cur(nsvc + 64, 0), td_run(nsvc, 0), staged(1u << 20, 0), bitmap((size_t)nsvc * GYS_BM_WORDS, 0),
		hll32(1u << GYS_HLL_P, 0), resp_win(nsvc, 0), host_spill(NH, 0), counts(16, 0);
	std::vector<TdMeta> meta(nsvc, TdMeta{0, 0, 0, 0, 0});
	std::vector<int2> minmax(nsvc, make_int2(INT32_MAX, INT32_MIN));
	std::vector<gys_hist_rec> hist_all(nsvc), hist_win(nsvc);
	for (auto *hv : {&hist_all, &hist_win})
		for (auto &r : *hv) {
			memset(&r, 0, sizeof(r));
			r.max_val_seen = INT64_MIN;
		}
	std::vector<MergeEnt> list0(nsvc + 1), list1(nsvc + 1), list2(nsvc + 1), listh(nsvc + 1), slow(nsvc + 1);
	std::vector<uint64_t> counters(CTR_NUM, 0);
	std::vector<unsigned long long> ghist(32, 0);
	long long gmax = INT64_MIN;

	// ---- the engine's side (what run_resp_batch sets up for the fused host-local form)
	FinP fin{};
	fin.td_cur = td_cur.data();
	fin.td_meta = meta.data();
	fin.nsvc = nsvc;
	fin.pcap = pcap;
	fin.pend_cap = pend_cap;
	fin.merge_fast = fast;
	fin.epoch = 1;
	fin.resp_win = resp_win.data();
	fin.list[FIN_CLASS0] = list0.data();
	fin.list[FIN_CLASS1] = list1.data();
	fin.list[FIN_CLASS2] = list2.data();
	fin.list[FIN_HUGE] = listh.data();
	fin.counts = counts.data();
	fin.td_run = td_run.data();
	fin.svc_host = svc_host.data();
	fin.host_spill = host_spill.data();
	fin.spill_stamp = 1;
	fin.counters = counters.data();
	RespHostP hp{};
	hp.ev = ev64;
	hp.n = n;
	hp.segs = segs.data();
	hp.nsegs = (uint32_t)segs.size();
	hp.hdesc = hdesc.data();
	hp.htbl = htbl.data();
	hp.hlst = hlst.data();
	hp.cand = cand.data();
	hp.hll32 = hll32.data();
	hp.td_cur = td_cur.data();
	hp.td_pend = td_pend.data();
	hp.pcap = pcap;
	hp.td_run = td_run.data();
	hp.staged = staged.data();
	hp.host_spill = host_spill.data();
	hp.spill_stamp = 1;
	hp.counters = counters.data();
	hp.ghist = ghist.data();
	hp.gmax = &gmax;
	hp.lds_tbl_entries = max_tbl;
	hp.lds_key_entries = (max_l + 1u) & ~1u;
	hp.fin = fin;
	const size_t dyn = resp_host_lds_bytes(max_tbl, hp.lds_key_entries, TILE);
	if (mode == 1) launch_resp<16, 1>(hp.nsegs, dyn, hp);
	else if (tpt == 16) launch_resp<16, 0>(hp.nsegs, dyn, hp);
	else launch_resp<8, 0>(hp.nsegs, dyn, hp);
	free(ev64);
	CHECK(counts[FIN_HUGE] == 0 && counts[FIN_RUN_ALLOC] == 0 && counts[FIN_CLASS2] == 0 && counts[FIN_CLASS0] == 0 && counts[FIN_CLASS1] == 0,
	      "%s: merges queued (the worlds keep every key inside its buffer)", wname);

	// ---- compare with the oracle
	const uint64_t *oc = gyo_engine_counters(orc);
	CHECK(counters[CTR_RESP_EVENTS] == oc[0] && counters[CTR_RESP_DROP_RANGE] == oc[1] && counters[CTR_RESP_DROP_NOLISTENER] == oc[2],
	      "%s counters {%llu, %llu, %llu} want {%llu, %llu, %llu}", wname, (unsigned long long)counters[CTR_RESP_EVENTS], (unsigned long long)counters[CTR_RESP_DROP_RANGE],
	      (unsigned long long)counters[CTR_RESP_DROP_NOLISTENER], (unsigned long long)oc[0], (unsigned long long)oc[1], (unsigned long long)oc[2]);
	CHECK(oc[2] > 0 && oc[1] > 0, "%s: no event without a listener / out of range", wname);
	const uint8_t *ohll = gyo_engine_hll(orc);
	for (uint32_t i = 0; i < (1u << GYS_HLL_P); ++i) CHECK(hll32[i] == ohll[i], "%s HLL register %u: %u want %u", wname, i, hll32[i], ohll[i]);
	const gyo_hist_serial *og = gyo_engine_ghist(orc);
	for (int b = 0; b < 15; ++b)
		CHECK(ghist[2 * b] == og[b].count && (int64_t)ghist[2 * b + 1] == og[b].sum, "%s all-service bucket %d: {%llu, %lld} want {%llu, %lld}", wname, b, ghist[2 * b],
		      (long long)ghist[2 * b + 1], (unsigned long long)og[b].count, (long long)og[b].sum);
	CHECK(ghist[30] == og[15].count && gmax == gyo_engine_gmax(orc), "%s all-service total %llu / max %lld", wname, ghist[30], gmax);
	for (uint32_t s = 0; s < nsvc; ++s) {
		const gyo_td_buffered *ot = gyo_engine_td(orc, s);
		CHECK(ot->npend >= 3, "%s key %u: %u events (every listener gets at least three)", wname, s, ot->npend);
		CHECK(meta[s].npend == ot->npend && (td_cur[s] & ~GYS_SPILL_BIT) == ot->npend, "%s key %u buffered %u (cur %u) want %u", wname, s, meta[s].npend, td_cur[s], ot->npend);
		if (meta[s].npend == ot->npend) {
			std::vector<int32_t> a(ot->npend), b(gyo_tdb_values(ot), gyo_tdb_values(ot) + ot->npend);
			for (uint32_t i = 0; i < ot->npend; ++i) a[i] = (int32_t)(td_pend[(size_t)s * pcap + i] >> GYS_ROW_BITS);
			std::sort(a.begin(), a.end());
			std::sort(b.begin(), b.end());
			CHECK(a == b, "%s key %u: buffered values differ", wname, s);
		}
		for (int j = 0; j < GYS_TD_NB; ++j)
			CHECK(td_sum[(size_t)s * GYS_TD_NB + j] == ot->d.sum[j] && td_cnt[(size_t)s * GYS_TD_NB + j] == ot->d.cnt[j], "%s key %u cluster %d", wname, s, j);
	}
	gyo_engine_free(orc);
	return n;
}
} // namespace

int main(int argc, char **argv)
{
	if (!kemu::can_run(1024u)) {
		printf("kemu: this process cannot have 1024 threads\n");
		return 77;
	}
	FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
	if (!f) {
		printf("usage: test_resp_lookup WORLDS (written by tests/lstkeys.py, write_standin)\n");
		return 2;
	}
	setvbuf(stdout, nullptr, _IOLBF, 0); // (a sanitizer abort must not take the lines of the worlds before it with it)
	const char *only = argc > 2 ? argv[2] : nullptr; // (one world by name)
	char word[64], wname[64];
	unsigned tpt, mode, nh, worlds = 0;
	uint64_t events = 0;
	while (fscanf(f, "%63s", word) == 1 && strcmp(word, "end") != 0) {
		if (strcmp(word, "world") != 0 || fscanf(f, "%63s %u %u %u", wname, &tpt, &mode, &nh) != 4 || (tpt != 16 && tpt != 8) || mode > 1 || (mode && tpt != 16)) {
			printf("bad world line at '%s'\n", word);
			return 2;
		}
		std::vector<HostIn> hosts(nh);
		for (HostIn &h : hosts)
			if (!read_host(f, h)) {
				printf("world %s: bad host\n", wname);
				return 2;
			}
		if (only && strcmp(only, wname) != 0) continue;
		printf("world %s ...\n", wname);
		events += run_world(wname, tpt, mode, hosts);
		++worlds;
	}
	fclose(f);
	if (fails) {
		printf("%d checks failed\n", fails);
		return 1;
	}
	printf("kemu resp lookup ok (%u worlds, %llu events)\n", worlds, (unsigned long long)events);
	return 0;
}
