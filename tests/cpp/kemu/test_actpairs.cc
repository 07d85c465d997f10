// TEST INFRASTRUCTURE (CPU): the LOGIC of the live active-connection row table (gyeeta_amd/csrc/gys_actpairs.hpp: k_actp_find / _keep /
// _add, the fused k_actp_all, k_actp_rebuild, k_actp_list, k_actp_svc_accum / _convert) under the CPU stand-in of the device model, against
// a std::map written here from the definition ("Live active-connection rows" in include/gysketch.h):
//   * calls of 1, 63, 64, 65, 257 (fused and three-pass form) and 2 048 rows; 300 rows of one key in one call (sums, the last row's fields);
//   * keys found by search to share a home entry of a 16-entry table, a chain that wraps the table's end; one listener with several
//     clients, one client with several listeners, keys that differ in kind only; an id equal to the free marker;
//   * the window rule: two calls in a window add, a report of window w is seen through w + 3 and gone at w + 4, a report in w and again
//     in w + 2 replaces; negative and NaN round-trip times count as 0;
//   * cap 128 with 32 fresh keys per window over 40 windows: no drop (fails without the rebuild); one call with more distinct keys than
//     entries: every key present has exact figures, the dropped rows are exactly the rows of the absent keys;
//   * the selection flags of k_actp_list, the cap, and the per-service sums.
// The host's room rule (gys_actpairs_host.hpp) is restated in Table::ingest.  Build + run: tests/test_kernel_logic_actpairs_cpu.py.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../../gyeeta_amd/csrc/gys_actpairs.hpp"

#include <stdio.h>
#include <stdlib.h>

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

using Key = std::tuple<uint64_t, uint64_t, uint32_t>;
inline Key K(uint64_t l, uint64_t c, uint32_t kind) { return Key(l, c, kind); }
struct Model {
	uint32_t window = 0, act = 0, nrows = 0, cdel = 0, sdel = 0, flags = 0;
	uint64_t sent = 0, rcvd = 0;
	float rtt = 0.0f;
	Row last{};
};

Row make_row(std::mt19937_64 &rng, uint64_t lid, uint64_t cid, uint32_t kind)
{
	Row r{};
	r.lid = lid;
	r.cid = cid;
	snprintf(r.ser_comm, sizeof(r.ser_comm), "s%llu", (unsigned long long)(rng() % 100000));
	snprintf(r.cli_comm, sizeof(r.cli_comm), "c%llu", (unsigned long long)(rng() % 100000));
	r.rmid[0] = rng();
	r.rmid[1] = rng();
	r.rmad = rng();
	r.sent = rng() % 100000;
	r.rcvd = rng() % 3 ? rng() % 100000 : 0;
	r.cdel = (uint32_t)(rng() % 50);
	r.sdel = (uint32_t)(rng() % 50);
	const uint32_t f = (uint32_t)(rng() % 16);
	r.rtt = f == 0 ? -1.5f : f == 1 ? NAN : (float)(rng() % 20000) / 1000.0f;
	r.act = (uint16_t)(rng() % 200);
	r.flags = (uint8_t)((kind ? 2u : 0u) | (rng() % 4 == 0 ? 1u : 0u) | (rng() % 8 == 0 ? 4u : 0u));
	return r;
}

struct Table {
	uint32_t cap, entries, cur = 0, rebuild_epoch = 0;
	uint64_t bound = 0, rebuilds = 0;
	bool no_rebuild = false;
	std::vector<ActPairKey> key[2];
	std::vector<ActPairEnt> ent[2];
	std::vector<unsigned long long> ctr;
	std::map<Key, Model> model;
	explicit Table(uint32_t cap_) : cap(cap_), ctr(APC_NUM, 0)
	{
		entries = 16;
		while (entries < 2 * cap) entries *= 2;
		for (int b = 0; b < 2; ++b) {
			key[b].resize(entries);
			memset(key[b].data(), 0xFF, entries * sizeof(ActPairKey));
			ent[b].assign(entries, ActPairEnt{});
		}
	}
	ActPairTbl view(uint32_t b) { return ActPairTbl{key[b].data(), ent[b].data(), entries - 1}; }
	void rebuild(uint32_t epoch)
	{
		const uint32_t to = cur ^ 1u;
		memset(key[to].data(), 0xFF, entries * sizeof(ActPairKey));
		ent[to].assign(entries, ActPairEnt{});
		ctr[APC_OCCUPIED] = 0;
		const ActPairTbl f = view(cur), t = view(to);
		unsigned long long *cp = ctr.data();
		kemu::launch(2, 256, 0, [=] { k_actp_rebuild(f, t, epoch, cp); });
		cur = to;
		rebuilds++;
		bound = ctr[APC_OCCUPIED];
	}
	// one call: the table (the host's room rule, then the passes) and the model
	void ingest(const std::vector<Row> &rows, uint32_t epoch, bool fused, bool track_model = true)
	{
		const uint32_t n = (uint32_t)rows.size();
		if (!no_rebuild && bound + n > entries / 2) {
			bound = ctr[APC_OCCUPIED];
			if (bound + n > entries / 2 && bound && rebuild_epoch != epoch) {
				rebuild(epoch);
				rebuild_epoch = epoch;
			}
		}
		std::vector<uint32_t> row_ent(n, 0xABABABABu);
		ActPairP p{};
		p.batch = (const uint8_t *)rows.data();
		p.n = n;
		p.t = view(cur);
		p.epoch = epoch;
		p.row_ent = row_ent.data();
		p.ctr = ctr.data();
		if (fused && n <= GYS_ACTP_FUSED_MAX) {
			p.row_ent = nullptr;
			kemu::launch(1, GYS_ACTP_FUSED_MAX, 0, [=] { k_actp_all(p); });
		} else {
			const uint32_t grid = (n + 255) / 256;
			kemu::launch(grid, 256, 0, [=] { k_actp_find(p); });
			kemu::launch(grid, 256, 0, [=] { k_actp_keep(p); });
			kemu::launch(grid, 256, 0, [=] { k_actp_add(p); });
		}
		bound = std::min<uint64_t>(bound + n, entries);
		if (!track_model) return;
		for (uint32_t i = 0; i < n; ++i) {
			const Row &r = rows[i];
			if (r.lid == ~0ull || r.cid == ~0ull) continue;
			const Key k{r.lid, r.cid, (r.flags >> 1) & 1u};
			Model &m = model[k];
			if (m.window != epoch) {
				m = Model{};
				m.window = epoch;
			}
			m.act += r.act;
			m.nrows += 1;
			m.sent += r.sent;
			m.rcvd += r.rcvd;
			m.cdel = std::max(m.cdel, r.cdel);
			m.sdel = std::max(m.sdel, r.sdel);
			const float f = (r.rtt >= 0.0f) ? r.rtt : 0.0f; // (false for a NaN)
			m.rtt = std::max(m.rtt, f);
			m.flags |= r.flags;
			m.last = r; // (rows in index order: the highest index of the last call stays)
		}
	}
	std::vector<gys_actconn_row> list(uint32_t epoch, const gys_actconn_sel &sel, uint32_t lcap, uint64_t *nmatch, DevTable gid = DevTable{nullptr, 0}, const uint32_t *svc_host = nullptr,
					  uint32_t nsvc = 0)
	{
		static TblEnt none[1] = {{GYS_EMPTY_KEY, 0, 0}};
		if (!gid.ent) gid = DevTable{none, 0};
		std::vector<gys_actconn_row> out(lcap + 1);
		memset(out.data(), 0x5A, out.size() * sizeof(gys_actconn_row));
		unsigned long long cnt = 0;
		ActPairListP p{};
		p.t = view(cur);
		p.epoch = epoch;
		p.gid = gid;
		p.svc_host = svc_host;
		p.nsvc = nsvc;
		p.sel = sel;
		p.out = out.data();
		p.cap = lcap;
		p.count = &cnt;
		kemu::launch(2, 256, 0, [=] { k_actp_list(p); });
		*nmatch = cnt;
		const uint8_t *guard = (const uint8_t *)&out[lcap];
		for (size_t b = 0; b < sizeof(gys_actconn_row); ++b) CHECK(guard[b] == 0x5A, "list wrote beyond its cap");
		out.resize(std::min<uint64_t>(lcap, cnt));
		return out;
	}
	// every live key of the model is listed with its exact figures, and nothing else is
	void verify(uint32_t epoch, const char *what, bool allow_absent = false)
	{
		gys_actconn_sel all{};
		all.struct_size = sizeof(all);
		uint64_t nm = 0;
		const std::vector<gys_actconn_row> got = list(epoch, all, entries, &nm);
		CHECK(nm == got.size(), "%s: %llu matches for %u entries", what, (unsigned long long)nm, entries);
		std::map<Key, const gys_actconn_row *> by_key;
		for (const gys_actconn_row &r : got) {
			const Key k{r.listener_glob_id, r.cli_aggr_task_id, r.kind};
			CHECK(!by_key.count(k), "%s: key %llx/%llx/%u listed twice", what, (unsigned long long)r.listener_glob_id, (unsigned long long)r.cli_aggr_task_id, r.kind);
			by_key[k] = &r;
		}
		size_t live = 0;
		uint64_t rows_absent = 0;
		for (const auto &kv : model) {
			const Model &m = kv.second;
			if (!(epoch - m.window <= 3u)) continue;
			auto it = by_key.find(kv.first);
			if (it == by_key.end()) {
				if (allow_absent) rows_absent += m.nrows;
				else CHECK(false, "%s: live key %llx/%llx/%u is not listed", what, (unsigned long long)std::get<0>(kv.first), (unsigned long long)std::get<1>(kv.first), std::get<2>(kv.first));
				continue;
			}
			++live;
			const gys_actconn_row &r = *it->second;
			uint32_t rb, mb;
			memcpy(&rb, &r.max_rtt_msec, 4);
			memcpy(&mb, &m.rtt, 4);
			CHECK(r.window == m.window && r.active_conns == m.act && r.nrows == m.nrows && r.bytes_sent == m.sent && r.bytes_received == m.rcvd, "%s: sums of %llx/%llx: window %u/%u act %u/%u rows %u/%u",
			      what, (unsigned long long)r.listener_glob_id, (unsigned long long)r.cli_aggr_task_id, r.window, m.window, r.active_conns, m.act, r.nrows, m.nrows);
			CHECK(r.cli_delay_msec == m.cdel && r.ser_delay_msec == m.sdel && rb == mb && r.flags == m.flags, "%s: maxima / flags of %llx/%llx", what, (unsigned long long)r.listener_glob_id,
			      (unsigned long long)r.cli_aggr_task_id);
			CHECK(!memcmp(r.ser_comm, m.last.ser_comm, 16) && !memcmp(r.cli_comm, m.last.cli_comm, 16) && !memcmp(r.remote_machine_id, m.last.rmid, 16) && r.remote_madhava_id == m.last.rmad,
			      "%s: the descriptive fields of %llx/%llx are not the last row's", what, (unsigned long long)r.listener_glob_id, (unsigned long long)r.cli_aggr_task_id);
			CHECK(r.slot == GYS_NOSLOT && r.pad[0] == 0 && r.pad[1] == 0 && r.reserved == 0, "%s: slot / padding", what);
		}
		CHECK(by_key.size() == live, "%s: %zu keys listed, %zu live in the model", what, by_key.size(), live);
		if (allow_absent) CHECK(ctr[APC_DROPPED] == rows_absent, "%s: %llu rows dropped, the absent keys had %llu", what, ctr[APC_DROPPED], (unsigned long long)rows_absent);
		else CHECK(ctr[APC_DROPPED] == 0, "%s: %llu rows dropped", what, ctr[APC_DROPPED]);
		for (uint32_t b = 0; b < 2; ++b)
			for (const ActPairEnt &e : ent[b]) CHECK(e.claim == 0, "%s: a claim word is left set", what);
	}
};

std::vector<Row> random_call(std::mt19937_64 &rng, uint32_t n, uint32_t nlid, uint32_t ncid)
{
	std::vector<Row> rows;
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t kind = (uint32_t)(rng() % 4 == 0);
		rows.push_back(make_row(rng, 0x1000 + rng() % nlid, 0x9000 + rng() % ncid, kind));
	}
	return rows;
}

void test_sizes(uint64_t seed)
{
	std::mt19937_64 rng(seed);
	Table tb(4096);
	uint32_t epoch = 5;
	for (uint32_t n : {1u, 63u, 64u, 65u, 257u})
		for (bool fused : {true, false}) {
			tb.ingest(random_call(rng, n, 9, 7), epoch, fused); // (63 (listener, client) pairs x 2 kinds: many repeats)
			tb.verify(epoch, "sizes");
		}
	tb.ingest(random_call(rng, 2048u, 40, 40), epoch, false);
	tb.verify(epoch, "sizes 2048");
	// 300 rows of one key in one call, both forms
	for (bool fused : {true, false}) {
		std::vector<Row> rows;
		for (int i = 0; i < 300; ++i) rows.push_back(make_row(rng, 0x77, 0x88, 0));
		++epoch;
		tb.ingest(rows, epoch, fused);
		const Model &m = tb.model[K(0x77, 0x88, 0)];
		CHECK(m.nrows == 300 && !memcmp(m.last.cli_comm, rows[299].cli_comm, 16), "one key: the model itself");
		tb.verify(epoch, "one key x 300");
	}
}

void test_collisions(uint64_t seed)
{
	std::mt19937_64 rng(seed);
	const uint32_t mask = 15;
	// five keys whose home is entry 14 of a 16-entry table: the chain is 14, 15, 0, 1, 2
	std::vector<std::pair<uint64_t, uint64_t>> same;
	while (same.size() < 5) {
		const uint64_t l = rng() >> 1, c = rng() >> 1;
		if (actp_home(l, c, 0, mask) == 14) same.push_back({l, c});
	}
	for (int pass = 0; pass < 2; ++pass) { // all in one call (the threads race for the entries) / one call each
		Table tb(8);
		CHECK(tb.entries == 16, "16 entries for cap 8");
		std::vector<Row> rows;
		for (auto &k : same)
			for (int r = 0; r < 3; ++r) rows.push_back(make_row(rng, k.first, k.second, 0));
		if (pass == 0) {
			tb.ingest(rows, 2, true);
		} else {
			for (size_t i = 0; i < rows.size(); i += 3) tb.ingest(std::vector<Row>(rows.begin() + i, rows.begin() + i + 3), 2, i % 2 == 0);
		}
		tb.verify(2, "chain");
		std::set<uint32_t> used;
		for (uint32_t h = 0; h < 16; ++h)
			if (tb.key[tb.cur][h].lid != GYS_EMPTY_KEY) used.insert(h);
		CHECK((used == std::set<uint32_t>{14, 15, 0, 1, 2}), "chain: the five keys do not occupy entries 14, 15, 0, 1, 2");
		CHECK(tb.ctr[APC_OCCUPIED] == 5, "chain: %llu entries counted", tb.ctr[APC_OCCUPIED]);
	}
	// one listener with several clients, one client with several listeners, keys that differ in kind only -- in one call, interleaved
	Table tb(64);
	std::vector<Row> rows;
	for (int rep = 0; rep < 4; ++rep) {
		for (uint64_t c = 1; c <= 6; ++c) rows.push_back(make_row(rng, 0xAAAA, c, 0));
		for (uint64_t l = 1; l <= 6; ++l) rows.push_back(make_row(rng, l, 0xBBBB, 0));
		for (uint32_t kind = 0; kind < 2; ++kind) rows.push_back(make_row(rng, 0xCCCC, 0xDDDD, kind));
		rows.push_back(make_row(rng, 0xDDDD, 0xCCCC, 1)); // (the ids swapped)
	}
	tb.ingest(rows, 3, true);
	tb.verify(3, "shared ids");
	CHECK(tb.model.size() == 15, "shared ids: %zu keys in the model", tb.model.size());
	tb.ingest(rows, 3, false);
	tb.verify(3, "shared ids, second call");
	// an id equal to the free marker
	std::vector<Row> bad = {make_row(rng, ~0ull, 5, 0), make_row(rng, 5, ~0ull, 0), make_row(rng, ~0ull, ~0ull, 1), make_row(rng, 5, 5, 0)};
	tb.ingest(bad, 3, true);
	tb.ingest(bad, 3, false);
	tb.verify(3, "free marker");
	CHECK(tb.ctr[APC_BADKEY] == 6, "free marker: %llu rows counted as bad", tb.ctr[APC_BADKEY]);
	CHECK(tb.model.count(K(5, 5, 0)) == 1 && tb.model.size() == 16, "free marker: the good row is there");
}

void test_windows(uint64_t seed)
{
	std::mt19937_64 rng(seed);
	Table tb(64);
	const uint32_t w = 10;
	std::vector<Row> a = {make_row(rng, 1, 2, 0), make_row(rng, 1, 3, 0), make_row(rng, 1, 2, 1)};
	tb.ingest(a, w, true);
	std::vector<Row> b = {make_row(rng, 1, 2, 0), make_row(rng, 1, 2, 0)};
	tb.ingest(b, w, false); // two calls in one window add
	CHECK(tb.model[K(1, 2, 0)].nrows == 3, "windows: the model adds within a window");
	for (uint32_t e = w; e <= w + 3; ++e) tb.verify(e, "visible through w + 3");
	gys_actconn_sel all{};
	all.struct_size = sizeof(all);
	uint64_t nm = 7;
	tb.list(w + 4, all, 64, &nm);
	CHECK(nm == 0, "windows: %llu rows at w + 4", (unsigned long long)nm);
	tb.verify(w + 4, "gone at w + 4");
	// a report in w + 2 replaces; the key not named again keeps its window-w report until w + 3
	std::vector<Row> c2 = {make_row(rng, 1, 2, 0)};
	tb.ingest(c2, w + 2, true);
	const Model &m = tb.model[K(1, 2, 0)];
	CHECK(m.nrows == 1 && m.window == w + 2 && m.sent == c2[0].sent, "windows: the model replaces");
	tb.verify(w + 2, "replaced at w + 2");
	tb.verify(w + 3, "w + 3");
	tb.list(w + 4, all, 64, &nm);
	CHECK(nm == 1, "windows: %llu rows at w + 4 after the second report", (unsigned long long)nm);
	tb.verify(w + 5, "w + 5");
	tb.list(w + 6, all, 64, &nm);
	CHECK(nm == 0, "windows: the second report is gone at w + 6");
	// a dead entry that is named again starts from zero
	tb.ingest(a, w + 20, false);
	tb.verify(w + 20, "named again");
}

void test_rebuild(uint64_t seed)
{
	std::mt19937_64 rng(seed);
	for (int with = 1; with >= 0; --with) {
		Table tb(128);
		tb.no_rebuild = !with;
		CHECK(tb.entries == 256, "256 entries for cap 128");
		uint64_t next = 1;
		for (uint32_t w = 1; w <= 40; ++w) {
			std::vector<Row> rows;
			for (int k = 0; k < 32; ++k, ++next) rows.push_back(make_row(rng, next * 0x9E3779B97F4A7C15ull >> 1, next, (uint32_t)(next % 5 == 0)));
			tb.ingest(rows, w, w % 2 == 0);
			if (with) tb.verify(w, "40 windows");
		}
		if (with) {
			CHECK(tb.ctr[APC_DROPPED] == 0 && tb.rebuilds > 0 && tb.rebuilds <= 40, "rebuild: %llu drops, %llu rebuilds", tb.ctr[APC_DROPPED], (unsigned long long)tb.rebuilds);
			CHECK(tb.ctr[APC_OCCUPIED] <= 128, "rebuild: %llu occupied entries", tb.ctr[APC_OCCUPIED]); // (at most 4 x 32 live keys)
		} else {
			CHECK(tb.ctr[APC_DROPPED] == 40u * 32u - 256u, "without the rebuild %llu rows are dropped, expected %u", tb.ctr[APC_DROPPED], 40u * 32u - 256u);
		}
	}
	// more distinct keys in one call than there are entries
	for (bool fused : {true, false}) {
		Table tb(8);
		std::vector<Row> rows;
		for (int rep = 0; rep < 2; ++rep)
			for (uint64_t k = 1; k <= 40; ++k) rows.push_back(make_row(rng, k << 20, k, (uint32_t)(k % 3 == 0)));
		tb.ingest(rows, 4, fused);
		tb.verify(4, "overflow", true);
		CHECK(tb.ctr[APC_OCCUPIED] == 16 && tb.ctr[APC_DROPPED] == 2u * (40u - 16u), "overflow: %llu occupied, %llu dropped", tb.ctr[APC_OCCUPIED], tb.ctr[APC_DROPPED]);
	}
}

void test_queries(uint64_t seed)
{
	std::mt19937_64 rng(seed);
	// listeners 0x100 .. 0x10B registered as slots 0 .. 11 (slot s on host s / 4), 0x10C .. not registered
	const uint32_t nsvc = 12;
	std::vector<TblEnt> gent(32, TblEnt{GYS_EMPTY_KEY, 0xFFFFFFFFu, 0xFFFFFFFFu});
	DevTable gid{gent.data(), 31};
	std::vector<uint32_t> svc_host(nsvc);
	for (uint32_t s = 0; s < nsvc; ++s) {
		uint32_t h = get_uint64_hash(0x100 + s) & 31u;
		while (gent[h].key != GYS_EMPTY_KEY) h = (h + 1) & 31u;
		gent[h] = TblEnt{0x100ull + s, s, 0};
		svc_host[s] = s / 4;
	}
	Table tb(512);
	std::vector<Row> rows;
	for (int i = 0; i < 400; ++i) rows.push_back(make_row(rng, 0x100 + rng() % 15, 0x9000 + rng() % 11, (uint32_t)(rng() % 4 == 0)));
	tb.ingest(rows, 8, true);
	tb.verify(8, "queries");
	auto want = [&](const gys_actconn_sel &s) {
		std::set<Key> w;
		for (const auto &kv : tb.model) {
			const uint64_t l = std::get<0>(kv.first), c = std::get<1>(kv.first);
			const uint32_t kind = std::get<2>(kv.first);
			const Model &m = kv.second;
			if ((s.flags & GYS_ACS_BY_LISTENER) && l != s.listener_glob_id) continue;
			if ((s.flags & GYS_ACS_BY_CLIENT) && c != s.cli_aggr_task_id) continue;
			if ((s.flags & (GYS_ACS_KIND_LOCAL | GYS_ACS_KIND_REMOTE)) && !(s.flags & (kind ? GYS_ACS_KIND_REMOTE : GYS_ACS_KIND_LOCAL))) continue;
			if (m.sent + m.rcvd < s.min_bytes || m.act < s.min_active_conns) continue;
			if ((s.flags & GYS_ACS_BY_HOST) && (kind || l >= 0x100 + nsvc || (l - 0x100) / 4 != s.host_slot)) continue;
			w.insert(kv.first);
		}
		return w;
	};
	std::vector<gys_actconn_sel> sels;
	auto sel = [&](uint32_t flags, uint64_t l, uint64_t c, uint32_t host, uint64_t minb, uint32_t mina) {
		gys_actconn_sel s{};
		s.struct_size = sizeof(s);
		s.flags = flags;
		s.listener_glob_id = l;
		s.cli_aggr_task_id = c;
		s.host_slot = host;
		s.min_bytes = minb;
		s.min_active_conns = mina;
		sels.push_back(s);
	};
	sel(0, 0, 0, 0, 0, 0);
	sel(GYS_ACS_BY_LISTENER, 0x103, 0, 0, 0, 0);
	sel(GYS_ACS_BY_LISTENER, 0x10D, 0, 0, 0, 0);
	sel(GYS_ACS_BY_CLIENT, 0, 0x9004, 0, 0, 0);
	sel(GYS_ACS_BY_LISTENER | GYS_ACS_BY_CLIENT, 0x103, 0x9004, 0, 0, 0);
	sel(GYS_ACS_BY_HOST, 0, 0, 1, 0, 0);
	sel(GYS_ACS_BY_HOST, 0, 0, 7, 0, 0);
	sel(GYS_ACS_KIND_LOCAL, 0, 0, 0, 0, 0);
	sel(GYS_ACS_KIND_REMOTE, 0, 0, 0, 0, 0);
	sel(GYS_ACS_KIND_LOCAL | GYS_ACS_KIND_REMOTE, 0, 0, 0, 0, 0);
	sel(0, 0, 0, 0, 150000, 0);
	sel(0, 0, 0, 0, 0, 300);
	sel(GYS_ACS_BY_HOST | GYS_ACS_BY_CLIENT, 0, 0x9001, 2, 1000, 10);
	for (size_t i = 0; i < sels.size(); ++i) {
		const std::set<Key> w = want(sels[i]);
		for (uint32_t lcap : {1024u, (uint32_t)w.size(), (uint32_t)w.size() / 2u, 0u}) {
			uint64_t nm = 0;
			const std::vector<gys_actconn_row> got = tb.list(8, sels[i], lcap, &nm, gid, svc_host.data(), nsvc);
			CHECK(nm == w.size(), "selection %zu cap %u: %llu matches, expected %zu", i, lcap, (unsigned long long)nm, w.size());
			std::set<Key> g;
			for (const gys_actconn_row &r : got) {
				g.insert(K(r.listener_glob_id, r.cli_aggr_task_id, r.kind));
				const uint32_t ws = (!r.kind && r.listener_glob_id < 0x100 + nsvc) ? (uint32_t)(r.listener_glob_id - 0x100) : GYS_NOSLOT;
				CHECK(r.slot == ws, "selection %zu: slot %u of listener %llx, expected %u", i, r.slot, (unsigned long long)r.listener_glob_id, ws);
			}
			CHECK(g.size() == got.size() && got.size() == std::min<size_t>(lcap, w.size()), "selection %zu cap %u: %zu rows", i, lcap, got.size());
			for (const Key &k : g) CHECK(w.count(k) == 1, "selection %zu: a row that does not match", i);
		}
		if (i >= 1 && i != 9) CHECK(w.size() < tb.model.size(), "selection %zu selects everything: the case is trivial", i);
	}
	CHECK(!want(sels[1]).empty() && !want(sels[5]).empty() && !want(sels[8]).empty() && !want(sels[10]).empty() && !want(sels[12]).empty() && want(sels[6]).empty(), "selections: trivial cases");
	// per-service sums
	for (uint32_t epoch : {8u, 11u, 12u}) {
		std::vector<unsigned long long> acc((size_t)nsvc * 4, 0);
		std::vector<double> out((size_t)nsvc * 4 + 1, -1.0);
		const ActPairTbl t = tb.view(tb.cur);
		unsigned long long *ap = acc.data();
		double *op = out.data();
		kemu::launch(2, 256, 0, [=] { k_actp_svc_accum(t, epoch, gid, nsvc, ap); });
		kemu::launch(1, 256, 0, [=] { k_actp_svc_convert(ap, (uint64_t)nsvc * 4, op); });
		std::vector<double> w((size_t)nsvc * 4, 0.0);
		for (const auto &kv : tb.model) {
			const uint64_t l = std::get<0>(kv.first);
			if (std::get<2>(kv.first) || l >= 0x100 + nsvc || !(epoch - kv.second.window <= 3u)) continue;
			double *a = &w[(l - 0x100) * 4];
			a[0] += 1;
			a[1] += kv.second.act;
			a[2] += (double)(kv.second.sent + kv.second.rcvd);
			a[3] += kv.second.nrows;
		}
		for (size_t i = 0; i < w.size(); ++i) CHECK(out[i] == w[i], "service sums at window %u: [%zu] = %f, expected %f", epoch, i, out[i], w[i]);
		CHECK(out[w.size()] == -1.0, "service sums: written beyond the services");
		CHECK((epoch == 12) == (w[1] == 0.0 && w[0] == 0.0), "service sums at window %u: the case is trivial", epoch);
	}
}

} // namespace

int main(int argc, char **argv)
{
	const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
	if (!kemu::can_run(GYS_ACTP_FUSED_MAX)) {
		printf("cannot start %u threads here\n", GYS_ACTP_FUSED_MAX);
		return 77;
	}
	test_sizes(seed);
	test_collisions(seed + 1);
	test_windows(seed + 2);
	test_rebuild(seed + 3);
	test_queries(seed + 4);
	if (fails) {
		printf("kemu actpairs: %d failures\n", fails);
		return 1;
	}
	printf("kemu actpairs ok\n");
	return 0;
}
