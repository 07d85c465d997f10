// TEST INFRASTRUCTURE (CPU): the LOGIC of the selection kernels of the filtered roll-ups (gyeeta_amd/csrc/gys_rollsel.hpp: k_rollsel_count,
// k_rollsel_scan, k_rollsel_scatter, k_rollsel_chunks, k_rollsel_labels) under the CPU stand-in of the device model, against a plain loop
// that applies the oracle's criteria walk (gyo_svc_filter_match, the currency rule of gyo_svcstate_scan) and the grouping.  Synthetic state
// records as tests/cpp/kemu/test_svcquery.cc makes them (stale / deleted / foreign records, negative `int` views), random filters, host
// subsets and named listeners; all four group_by values with and without GYS_RF_ANY_STATE; an empty result; a group of more than 3 x 1024
// members (several chunks); maxrows below the number of rows; a label domain larger than one workgroup's LDS table (the wave-joined global
// atomics, a heavy label among many light ones, several tiles of the scan); several grid sizes.  Checked: the rows, the member SET of every
// row, the chunk lists and the totals; and the chunk lists, fed to k_hll_union as the engine feeds them, give gyo_hll_merge of the members
// byte for byte.
// Build + run: tests/test_kernel_logic_rollsel_cpu.py.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../../gyeeta_amd/csrc/gys_rollup.hpp"
#include "../../../gyeeta_amd/csrc/gys_hllroll.hpp"
#include "../../../gyeeta_amd/csrc/gys_svcquery.hpp"
#include "../../../gyeeta_amd/csrc/gys_rollsel.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
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

constexpr uint32_t PER = 1024u; // members per chunk (GYS_RB_CHUNK_SERVICES of the engine)

struct World {
	uint32_t NH, NSVC, EPOCH, NCL;
	std::vector<uint8_t> state;
	std::vector<uint32_t> svc_host, host_cluster, labels;
	std::vector<uint64_t> svc_gid;
};

struct Selection { // what the kernels leave
	uint32_t tot[RS_TOT_WORDS];
	std::vector<gys_rollup_row> rows;
	std::vector<uint2> rowoff;
	std::vector<uint32_t> members;
	std::vector<RollupChunk> chunks, gchunks;
};

// the launches of gys_rollup_filtered_dev
void run(RollSelP p, uint32_t maxrows, uint32_t grid, Selection &s)
{
	std::vector<uint32_t> item_group(p.nitems + 1, 0xABABABABu), counts(p.ndomain + 4, 0u), members(p.nitems + 1, 0xCDCDCDCDu);
	const uint32_t nscan = (p.ndomain + GYS_RS_SCAN_TILE - 1u) / GYS_RS_SCAN_TILE, rowcap = std::min(maxrows, p.ndomain);
	std::vector<uint32_t> tiles(3u * nscan + 1u, 0u);
	s.rows.assign(rowcap + 1, gys_rollup_row{0xEEEEEEEEu, 0xEEEEEEEEu});
	s.rowoff.assign(rowcap + 1, uint2{0, 0});
	memset(s.tot, 0xEE, sizeof(s.tot));
	p.ntiles = (p.nitems + GYS_RS_TILE - 1u) / GYS_RS_TILE;
	p.item_group = item_group.data();
	p.counts = counts.data();
	p.tot = s.tot;
	p.members = members.data();
	kemu::launch(std::max(1u, std::min(grid, p.ntiles)), GYS_RS_THREADS, 0, [&] { k_rollsel_count(p); });
	CHECK(item_group[p.nitems] == 0xABABABABu, "the count kernel wrote past item_group");
	RollScanP sp{};
	sp.counts = counts.data();
	sp.ndomain = p.ndomain;
	sp.ntiles = nscan;
	sp.per = PER;
	sp.maxrows = maxrows;
	sp.tiles = tiles.data();
	sp.tot = s.tot;
	sp.rows = s.rows.data();
	sp.rowoff = s.rowoff.data();
	for (uint32_t phase = 0; phase < 3u; ++phase) {
		sp.phase = phase;
		kemu::launch(phase == 1u ? 1u : std::min(grid, nscan), GYS_RS_THREADS, 0, [&] { k_rollsel_scan(sp); });
	}
	CHECK(s.rows[rowcap].group == 0xEEEEEEEEu, "the scan wrote past its rows");
	const uint32_t nr = std::min(s.tot[RS_TOT_ROWS], maxrows);
	s.chunks.assign(s.tot[RS_TOT_CHUNKS] + 1, RollupChunk{0xEEEEEEEEu, 0, 0, 0});
	s.gchunks.assign(nr + 1, RollupChunk{0xEEEEEEEEu, 0, 0, 0});
	if (nr) {
		kemu::launch(std::max(1u, std::min(grid, p.ntiles)), GYS_RS_THREADS, 0, [&] { k_rollsel_scatter(p); });
		RollChunksP cp{};
		cp.rows = s.rows.data();
		cp.rowoff = s.rowoff.data();
		cp.tot = s.tot;
		cp.maxrows = maxrows;
		cp.per = PER;
		cp.chunks = s.chunks.data();
		cp.gchunks = s.gchunks.data();
		kemu::launch(std::min(grid, (nr + 3u) / 4u), GYS_RS_THREADS, 0, [&] { k_rollsel_chunks(cp); });
	}
	CHECK(s.chunks.back().group == 0xEEEEEEEEu && s.gchunks.back().group == 0xEEEEEEEEu, "the chunk kernel wrote past its lists");
	for (uint32_t i = s.tot[RS_TOT_MEMBERS]; i <= p.nitems; ++i)
		if (members[i] != 0xCDCDCDCDu) {
			CHECK(false, "the scatter wrote member %u, past the %u members of the rows", i, s.tot[RS_TOT_MEMBERS]);
			break;
		}
	s.members = members;
}

struct Query {
	std::vector<gyo_svc_term> ot;
	std::vector<int64_t> osetv;
	std::vector<int32_t> setv;
	uint8_t goper[8];
	int top_oper;
	std::vector<uint8_t> host_in; // empty: every host
	std::vector<uint32_t> mask;
	std::vector<uint32_t> slot_list;
	bool named = false;
};

void random_query(std::mt19937 &rng, const World &w, uint32_t q, Query &Q, RollSelP &p)
{
	p = RollSelP{};
	p.svc_state = w.state.data();
	p.svc_host = w.svc_host.data();
	p.svc_gid = w.svc_gid.data();
	p.nsvc = w.NSVC;
	p.epoch = w.EPOCH;
	const uint32_t nterms = q % 3u == 0 ? 0u : 1u + rng() % 4u;
	Q.ot.assign(nterms, gyo_svc_term{});
	Q.osetv.clear();
	Q.setv.clear();
	for (int g = 0; g < 8; ++g) Q.goper[g] = rng() % 2u;
	Q.top_oper = rng() % 2u;
	for (uint32_t i = 0; i < nterms; ++i) {
		static const uint8_t comps[] = {0, 1, 2, 3, 4, 5, 6, 7, 12, 13};
		gyo_svc_term &t = Q.ot[i];
		memset(&t, 0, sizeof(t));
		t.col = (uint8_t)(rng() % SVC_NCOLS);
		t.comp = comps[rng() % 10u];
		t.group = (uint8_t)(rng() % 2u);
		t.value = (int64_t)(rng() % 40u) - (rng() % 8u == 0 ? 20 : 0);
		if (t.comp >= 12) {
			t.set_first = (uint32_t)Q.osetv.size();
			t.nvalues = rng() % 5u;
			for (uint32_t k = 0; k < t.nvalues; ++k) Q.osetv.push_back((int64_t)(rng() % 40u));
		}
		SvcTerm &d = p.terms[i];
		d.col = t.col;
		d.comp = t.comp;
		d.group = t.group;
		d.pad = 0;
		d.nvalues = t.nvalues;
		d.set_first = t.set_first;
		d.value = t.col == SVC_COL_ISSUE ? (int32_t)(int16_t)t.value : (int32_t)t.value;
		p.ngroups = std::max<uint32_t>(p.ngroups, t.group + 1u);
	}
	for (size_t k = 0; k < Q.osetv.size(); ++k) Q.setv.push_back((int32_t)Q.osetv[k]);
	p.nterms = nterms;
	p.set_values = Q.setv.empty() ? nullptr : Q.setv.data();
	memcpy(p.group_oper, Q.goper, 8);
	p.top_oper = (uint32_t)Q.top_oper;
	Q.host_in.clear();
	Q.mask.assign((w.NH + 31) / 32 + 1, 0);
	if (q % 4u == 2u) {
		Q.host_in.assign(w.NH, 0);
		for (uint32_t h = 0; h < w.NH; ++h) {
			Q.host_in[h] = rng() % 3u != 0;
			if (Q.host_in[h]) Q.mask[h >> 5] |= 1u << (h & 31u);
		}
		p.host_mask = Q.mask.data();
	}
	Q.slot_list.clear();
	Q.named = q % 5u == 4u;
	if (Q.named) {
		for (uint32_t s2 = 0; s2 < w.NSVC; ++s2)
			if (rng() % 3u == 0) Q.slot_list.push_back(s2);
		p.slot_list = Q.slot_list.data();
	}
	p.nitems = Q.named ? (uint32_t)Q.slot_list.size() : w.NSVC;
	p.host_cluster = w.host_cluster.data();
	p.labels = w.labels.data();
}

// the plain loop: group -> member slots
std::map<uint32_t, std::vector<uint32_t>> reference(const World &w, const Query &Q, bool any_state, uint32_t group_by, uint32_t ndomain)
{
	std::map<uint32_t, std::vector<uint32_t>> want;
	const uint32_t n = Q.named ? (uint32_t)Q.slot_list.size() : w.NSVC;
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t slot = Q.named ? Q.slot_list[i] : i;
		const uint8_t *r = &w.state[(size_t)slot * 96];
		uint32_t ep, tag;
		uint64_t gid;
		memcpy(&gid, r, 8);
		memcpy(&ep, r + 88, 4);
		memcpy(&tag, r + 92, 4);
		const uint32_t host = w.svc_host[slot];
		if (!any_state && (ep == 0 || ep + 1 < w.EPOCH || tag != host || gid != w.svc_gid[slot])) continue; // (the currency rule of gyo_svcstate_scan)
		if (!Q.host_in.empty() && !Q.host_in[host]) continue;
		if (!gyo_svc_filter_match(r, Q.ot.data(), (uint32_t)Q.ot.size(), Q.osetv.data(), Q.goper, Q.top_oper)) continue;
		const uint32_t g = group_by == GYS_GROUP_NONE ? 0u : group_by == GYS_GROUP_HOST ? host : group_by == GYS_GROUP_CLUSTER ? w.host_cluster[host] : w.labels[slot];
		if (g == GYS_NO_GROUP || g >= ndomain) continue;
		want[g].push_back(slot);
	}
	return want;
}

void compare(const char *what, const std::map<uint32_t, std::vector<uint32_t>> &want, const Selection &s, uint32_t maxrows)
{
	CHECK(s.tot[RS_TOT_ROWS] == want.size(), "%s: %u rows, the loop has %zu", what, s.tot[RS_TOT_ROWS], want.size());
	if (s.tot[RS_TOT_ROWS] != want.size()) return;
	const uint32_t nr = std::min<uint32_t>((uint32_t)want.size(), maxrows);
	uint32_t r = 0, moff = 0, coff = 0;
	for (auto it = want.begin(); it != want.end() && r < nr; ++it, ++r) {
		const std::vector<uint32_t> &mem = it->second;
		CHECK(s.rows[r].group == it->first && s.rows[r].nmembers == mem.size(), "%s: row %u is {%u, %u}, the loop has {%u, %zu}", what, r, s.rows[r].group, s.rows[r].nmembers, it->first,
		      mem.size());
		if (s.rows[r].group != it->first || s.rows[r].nmembers != mem.size()) return;
		CHECK(s.rowoff[r].x == moff && s.rowoff[r].y == coff, "%s: row %u starts at member %u chunk %u, expected %u / %u", what, r, s.rowoff[r].x, s.rowoff[r].y, moff, coff);
		std::vector<uint32_t> got(s.members.begin() + moff, s.members.begin() + moff + mem.size()), ref(mem);
		std::sort(got.begin(), got.end());
		std::sort(ref.begin(), ref.end());
		CHECK(got == ref, "%s: the members of row %u (group %u, %zu of them) differ from the loop's", what, r, it->first, mem.size());
		const uint32_t nch = ((uint32_t)mem.size() + PER - 1u) / PER;
		CHECK(s.gchunks[r].group == r && s.gchunks[r].m0 == coff && s.gchunks[r].m1 == coff + nch, "%s: row %u names chunks [%u, %u), expected [%u, %u)", what, r, s.gchunks[r].m0,
		      s.gchunks[r].m1, coff, coff + nch);
		for (uint32_t j = 0; j < nch && coff + j < s.chunks.size(); ++j) {
			const RollupChunk &ck = s.chunks[coff + j];
			CHECK(ck.group == r && ck.m0 == moff + j * PER && ck.m1 == moff + std::min<uint32_t>((uint32_t)mem.size(), (j + 1u) * PER), "%s: chunk %u of row %u is {%u, %u, %u}", what, j,
			      r, ck.group, ck.m0, ck.m1);
		}
		moff += (uint32_t)mem.size();
		coff += nch;
	}
	CHECK(s.tot[RS_TOT_MEMBERS] == moff && s.tot[RS_TOT_CHUNKS] == coff, "%s: totals %u members / %u chunks, expected %u / %u", what, s.tot[RS_TOT_MEMBERS], s.tot[RS_TOT_CHUNKS], moff,
	      coff);
}

// the chunk lists through k_hll_union, as the engine launches them: row files == gyo_hll_merge of the members
void check_union(const char *what, const World &w, const std::vector<uint8_t> &files, int hp, const std::map<uint32_t, std::vector<uint32_t>> &want, const Selection &s,
		 uint32_t maxrows)
{
	const uint32_t m = 1u << hp, nr = std::min<uint32_t>((uint32_t)want.size(), maxrows), nchunks = s.tot[RS_TOT_CHUNKS];
	if (!nr) return;
	std::vector<uint8_t> parts((size_t)nchunks * m + 16, 0xEE), out((size_t)nr * m + 16, 0xEE);
	const HllUnionP q1{files.data(), parts.data(), s.chunks.data(), s.members.data(), nchunks, 0u, 0u, (uint32_t)hp};
	const HllUnionP q2{parts.data(), out.data(), s.gchunks.data(), nullptr, nr, 0u, 0u, (uint32_t)hp};
	kemu::launch(std::min(nchunks, 3u), GYS_HLL_NT, 0, [=] { k_hll_union(q1); });
	kemu::launch(std::min(nr, 3u), GYS_HLL_NT, 0, [=] { k_hll_union(q2); });
	uint32_t r = 0;
	for (auto it = want.begin(); it != want.end() && r < nr; ++it, ++r) {
		std::vector<uint8_t> ref(m, 0);
		for (uint32_t slot : it->second) gyo_hll_merge(ref.data(), files.data() + (size_t)slot * m, hp);
		CHECK(memcmp(ref.data(), out.data() + (size_t)r * m, m) == 0, "%s: the file of row %u (group %u) differs from gyo_hll_merge of its %zu members", what, r, it->first,
		      it->second.size());
	}
	CHECK(out[(size_t)nr * m] == 0xEE && parts[(size_t)nchunks * m] == 0xEE, "%s: the union wrote past its output", what);
}
} // namespace

int main(int argc, char **argv)
{
	if (!kemu::can_run(GYS_RS_THREADS)) {
		printf("kemu: this process cannot have %u threads\n", GYS_RS_THREADS);
		return 77;
	}
	std::mt19937 rng(argc > 1 ? (unsigned)atoi(argv[1]) : 5u);
	std::mt19937_64 rng64(rng());
	World w;
	w.NH = 37;
	w.NSVC = 4200 + rng() % 200u; // (more than four tiles of 1024 items: the group of all services has more than 3 x 1024 members)
	w.EPOCH = 9;
	w.NCL = 4;
	const uint32_t NLABEL = 9000; // more than GYS_RS_LDS_GROUPS labels and more than two tiles of the scan
	w.state.assign((size_t)w.NSVC * 96, 0);
	w.svc_host.resize(w.NSVC);
	w.svc_gid.resize(w.NSVC);
	w.host_cluster.resize(w.NH);
	w.labels.assign(w.NSVC, GYS_NO_GROUP);
	for (uint32_t h = 0; h < w.NH; ++h) w.host_cluster[h] = h == 5 ? 3u : rng() % 3u; // (cluster 3: one host)
	// labels through the kernel that sets them: a heavy label (a third of the services), runs of equal labels, scattered ones, some unlabelled
	{
		std::vector<uint32_t> slots, groups;
		for (uint32_t s = 0; s < w.NSVC; ++s) {
			const uint32_t k = rng() % 10u;
			if (k == 0) continue;
			slots.push_back(s);
			groups.push_back(k <= 3 ? 4321u : k <= 5 ? (s / 7u) % NLABEL : k == 6 ? NLABEL - 1u - rng() % 3u : rng() % NLABEL);
		}
		const uint32_t *ps = slots.data(), *pg = groups.data();
		uint32_t *pl = w.labels.data();
		const uint32_t n = (uint32_t)slots.size();
		kemu::launch(3, 256, 0, [=] { k_rollsel_labels(ps, pg, n, pl); });
		for (uint32_t i = 0; i < n; ++i) CHECK(w.labels[slots[i]] == groups[i], "k_rollsel_labels: slot %u", slots[i]);
	}
	for (uint32_t s = 0; s < w.NSVC; ++s) {
		w.svc_host[s] = (uint32_t)((uint64_t)s * w.NH / w.NSVC); // contiguous runs of slots per host
		if (w.svc_host[s] == 11u) w.svc_host[s] = 12u;           // (host 11 has no service: no row)
		w.svc_gid[s] = 0x5000000000000000ull + 977ull * s;
		uint8_t *r = &w.state[(size_t)s * 96];
		if (rng() % 9u == 0) continue; // never reported: all zero
		for (int k = 8; k < 88; ++k) r[k] = (uint8_t)rng();
		if (rng() % 5u) {
			for (int off = 8; off < 76; off += 4) {
				const uint32_t v = rng() % 40u;
				memcpy(r + off, &v, 4);
			}
			r[78] = rng() % 2u;
			r[79] = rng() % 7u;
			r[80] = rng() % 12u;
		}
		memcpy(r, &w.svc_gid[s], 8);
		uint32_t ep = w.EPOCH - (rng() % 3u == 0 ? 1u : 0u), host = w.svc_host[s];
		const uint32_t kind = rng() % 20u;
		if (kind == 0) ep = w.EPOCH - 2u;             // stale
		else if (kind == 1) ep = 0;                    // deleted
		else if (kind == 2) host = (host + 1) % w.NH; // tagged with another host
		else if (kind == 3) r[3] ^= 0x40;              // another listener's record in the slot
		memcpy(r + 88, &ep, 4);
		memcpy(r + 92, &host, 4);
	}
	const int hp = 4 + 2 * (int)(rng() % 2u);
	std::vector<uint8_t> files((size_t)w.NSVC << hp, 0);
	for (uint32_t s = 0; s < w.NSVC; ++s) {
		if (s % 11u == 0) continue;
		for (uint32_t i = 0, n = 1u + rng() % 40u; i < n; ++i) gyo_hll_add(files.data() + ((size_t)s << hp), hp, rng64());
	}

	uint32_t ncases = 0, big = 0, cut = 0, empty = 0;
	for (uint32_t q = 0; q < 5; ++q) {
		Query Q;
		RollSelP p;
		random_query(rng, w, q, Q, p);
		for (uint32_t group_by = GYS_GROUP_NONE; group_by <= GYS_GROUP_LABEL; ++group_by) {
			for (uint32_t any_state = 0; any_state < 2u; ++any_state) {
				const uint32_t ndomain = group_by == GYS_GROUP_NONE ? 1u : group_by == GYS_GROUP_HOST ? w.NH : group_by == GYS_GROUP_CLUSTER ? w.NCL : NLABEL;
				p.group_by = group_by;
				p.any_state = any_state;
				p.ndomain = ndomain;
				const auto want = reference(w, Q, any_state != 0, group_by, ndomain);
				char what[96];
				snprintf(what, sizeof(what), "query %u group_by %u any_state %u", q, group_by, any_state);
				const uint32_t nrows = (uint32_t)want.size();
				const uint32_t grids[] = {1u, 3u, 64u};
				const uint32_t grid = grids[(q + group_by + any_state) % 3u];
				Selection s;
				run(p, ndomain, grid, s);
				compare(what, want, s, ndomain);
				if ((q + group_by) % 2u == 0) check_union(what, w, files, hp, want, s, ndomain);
				for (const auto &kv : want) big += kv.second.size() > 3u * PER;
				empty += nrows == 0;
				++ncases;
				if (nrows >= 2u && (q + group_by + any_state) % 2u == 0) { // maxrows below the number of rows: the first groups only, the total reported
					const uint32_t maxrows = 1u + rng() % (nrows - 1u);
					Selection s2;
					run(p, maxrows, grids[(q + 1u) % 3u], s2);
					snprintf(what, sizeof(what), "query %u group_by %u any_state %u maxrows %u", q, group_by, any_state, maxrows);
					compare(what, want, s2, maxrows);
					auto it = want.begin();
					std::advance(it, maxrows);
					CHECK(s2.tot[RS_TOT_GCUT] == it->first, "%s: the cut is at group %u, expected %u", what, s2.tot[RS_TOT_GCUT], it->first);
					if (q % 3u == 0) check_union(what, w, files, hp, want, s2, maxrows);
					++cut;
					++ncases;
				}
			}
		}
	}
	// a filter that matches nothing, every grouping: no row, nothing written
	{
		Query Q;
		RollSelP p;
		random_query(rng, w, 0, Q, p);
		Q.ot.assign(1, gyo_svc_term{});
		Q.ot[0].col = SVC_COL_NQRY5S;
		Q.ot[0].comp = SVC_COMP_IN; // (IN of an empty set)
		p.terms[0] = SvcTerm{SVC_COL_NQRY5S, SVC_COMP_IN, 0, 0, 0, 0, 0};
		p.nterms = 1;
		p.ngroups = 1;
		for (uint32_t group_by = GYS_GROUP_NONE; group_by <= GYS_GROUP_LABEL; ++group_by) {
			const uint32_t ndomain = group_by == GYS_GROUP_NONE ? 1u : group_by == GYS_GROUP_HOST ? w.NH : group_by == GYS_GROUP_CLUSTER ? w.NCL : NLABEL;
			p.group_by = group_by;
			p.any_state = group_by & 1u;
			p.ndomain = ndomain;
			const auto want = reference(w, Q, p.any_state != 0, group_by, ndomain);
			CHECK(want.empty(), "the empty filter matched in the loop");
			Selection s;
			run(p, ndomain, 2, s);
			compare("empty filter", want, s, ndomain);
			CHECK(s.tot[RS_TOT_ROWS] == 0 && s.tot[RS_TOT_MEMBERS] == 0 && s.tot[RS_TOT_CHUNKS] == 0 && s.tot[RS_TOT_GCUT] == GYS_NO_GROUP, "empty filter: totals");
			++empty;
			++ncases;
		}
	}
	CHECK(big >= 2, "only %u groups of more than three chunks", big);
	CHECK(cut >= 5 && empty >= 4, "%u cut and %u empty cases", cut, empty);
	if (fails) {
		printf("kemu rollsel: %d FAILURES\n", fails);
		return 1;
	}
	printf("kemu rollsel ok: %u selections over %u services (%u groups of more than three chunks, %u with maxrows below the rows, %u empty)\n", ncases, w.NSVC, big, cut, empty);
	return 0;
}
