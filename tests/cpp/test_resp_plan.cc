// TEST INFRASTRUCTURE (CPU): the plan of a response batch, gyeeta_amd/csrc/gys_resp_plan.hpp, against the plain statement of its rules, over
// seeded random segment lists: 1 .. 64 segments, lengths 0 .. 3 x GYS_SPLIT_PART (0, exact multiples and their neighbours included), hosts
// with 0 .. 5 listener parts, split on and off.
//   * the virtual segments of each (segment, listener part) tile the segment's event range exactly once, first_event never decreases, a
//     zero-length segment produces none; the listener parts of one piece are adjacent, reserved = max_hosts + sub_desc + part + 1 (a host
//     without parts: 0); the count the builder reports is the number of entries it writes (the buffer has exactly that many: ASan);
//   * front end: a host in two segments, an overflowed table, a part that is not on the device and resp_path 1 each force the general
//     path; resp_path 3 splits whenever a segment is longer than GYS_SPLIT_PART; resp_path 0 splits exactly when the estimate says so;
//   * tile form: mode 1 / 2 never take the 6144-event form; mode 0 takes it exactly when two workgroups' LDS fit one CU.
// Build (g++ -fsanitize=address,undefined) + run: tests/test_resp_plan_cpu.py.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../gyeeta_amd/csrc/gys_resp_plan.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <memory>
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

constexpr uint64_t SP = GYS_SPLIT_PART;
constexpr uint32_t MAX_HOSTS = 100;

struct Batch {
	std::vector<RespSegView> sv;
	std::vector<RespPartView> pv;
	uint64_t n = 0;
	bool twice = false, overflow = false, off_device = false;
};

// `clean`: no duplicate host, no overflow, every part on the device (the batches whose split choice is looked at); `many`: 40 .. 64
// segments of about GYS_SPLIT_PART events -- enough workgroups to fill a chip, where the estimate is close to the line between the forms
Batch random_batch(std::mt19937_64 &rng, bool clean, bool many)
{
	auto r = [&](uint64_t m) { return (uint64_t)(rng() % m); };
	Batch b;
	const uint32_t nsegs = many ? 40 + (uint32_t)r(25) : 1 + (uint32_t)r(r(4) ? 6 : 64); // (few long segments are what the split form is for)
	std::vector<uint32_t> seen(MAX_HOSTS, 0);
	uint32_t desc = 0;
	for (uint32_t s = 0; s < nsegs; ++s) {
		uint32_t host = (uint32_t)r(MAX_HOSTS);
		if (clean || r(40)) while (seen[host]) host = (host + 1) % MAX_HOSTS;
		static const uint64_t lens[] = {0, 1, SP - 1, SP, SP + 1, 2 * SP, 2 * SP + 1, 3 * SP};
		const uint64_t len = many ? (r(100) ? SP - 1 + r(3) : 2 * SP) : r(3) ? lens[r(8)] : r(3 * SP + 1);
		RespSegView v{};
		v.host_slot = host;
		v.first_event = b.n;
		v.len = len;
		v.seen_twice = seen[host] != 0;
		v.overflow = !clean && r(60) == 0;
		v.chains = r(8) == 0;
		v.nparts = r(2) ? 0u : (uint32_t)r(6);
		v.part0 = (uint32_t)b.pv.size();
		v.sub_desc = v.nparts ? desc : 0u;
		desc += v.nparts + (uint32_t)r(3);
		for (uint32_t p = 0; p < std::max<uint32_t>(v.nparts, 1); ++p) {
			const uint32_t tbl = 16u << r(10);
			b.pv.push_back(RespPartView{tbl, 1u + (uint32_t)r(tbl / 2), clean || r(80) != 0});
			b.off_device = b.off_device || !b.pv.back().on_device;
		}
		seen[host] = 1;
		b.twice = b.twice || v.seen_twice;
		b.overflow = b.overflow || v.overflow;
		b.n += len;
		b.sv.push_back(v);
	}
	return b;
}

void check_virtual_segments(const Batch &b, bool split)
{
	const uint32_t nsegs = (uint32_t)b.sv.size();
	const uint64_t count = resp_virtual_segments(b.sv.data(), nsegs, split, MAX_HOSTS, nullptr);
	std::unique_ptr<gys_resp_seg[]> out(new gys_resp_seg[count]); // exactly `count` entries: one write more is a heap overflow under ASan
	const uint64_t written = resp_virtual_segments(b.sv.data(), nsegs, split, MAX_HOSTS, out.get());
	CHECK(written == count, "split %d: %llu entries counted, %llu written", (int)split, (unsigned long long)count, (unsigned long long)written);
	if (written != count) return;
	// the list, read from the side of the event ranges: segment after segment, piece after piece from the segment's first event to its end
	uint64_t at = 0;
	for (uint32_t s = 0; s < nsegs; ++s) {
		const RespSegView &v = b.sv[s];
		const uint64_t end = v.first_event + v.len;
		for (uint64_t fe = v.first_event; fe < end; fe += split ? SP : v.len) {
			for (uint32_t lp = 0; lp < std::max<uint32_t>(v.nparts, 1); ++lp, ++at) { // the listener parts of one piece: adjacent, in order
				if (at >= count) break;
				const uint32_t want = v.nparts ? MAX_HOSTS + v.sub_desc + lp + 1u : 0u;
				CHECK(out[at].host_slot == v.host_slot && out[at].reserved == want && out[at].first_event == fe,
				      "split %d seg %u part %u: entry %llu = {%u, %u, %llu}, want {%u, %u, %llu}", (int)split, s, lp, (unsigned long long)at, out[at].host_slot,
				      out[at].reserved, (unsigned long long)out[at].first_event, v.host_slot, want, (unsigned long long)fe);
			}
		}
	}
	CHECK(at == count, "split %d: the segments' pieces are %llu entries, the builder made %llu", (int)split, (unsigned long long)at, (unsigned long long)count);
	for (uint64_t i = 1; i < count; ++i) CHECK(out[i].first_event >= out[i - 1].first_event, "split %d: first_event decreases at entry %llu", (int)split, (unsigned long long)i);
	// every piece ends where the next piece of the same listener part (or the segment) does: none is longer than a part of the split form
	if (split)
		for (uint64_t i = 0; i + 1 < count; ++i) CHECK(out[i + 1].first_event - out[i].first_event <= SP, "a piece of more than GYS_SPLIT_PART events at entry %llu", (unsigned long long)i);
}

int n_split[2] = {0, 0};

void check_front(const Batch &b, int ncu, uint32_t resp_path)
{
	const uint32_t nsegs = (uint32_t)b.sv.size();
	const RespFront f = resp_front_choice(b.sv.data(), nsegs, b.pv.data(), b.n, ncu, resp_path);
	const bool general = b.twice || b.overflow || b.off_device || resp_path == 1;
	CHECK(f.host_local == !general, "resp_path %u (twice %d overflow %d off-device %d): host_local %d", resp_path, (int)b.twice, (int)b.overflow, (int)b.off_device, (int)f.host_local);
	if (general) {
		CHECK(!f.host_split && !f.host_parts, "general front end with split %d parts %d", (int)f.host_split, (int)f.host_parts);
		return;
	}
	uint64_t max_len = 0, nwg = 0;
	uint32_t max_tbl = 16, max_l = 1;
	bool parts = false, cands = false;
	for (const RespSegView &v : b.sv) {
		max_len = std::max(max_len, v.len);
		nwg += std::max<uint32_t>(v.nparts, 1);
		parts = parts || v.nparts != 0;
		cands = cands || v.chains;
		for (uint32_t p = 0; p < std::max<uint32_t>(v.nparts, 1); ++p) {
			max_tbl = std::max(max_tbl, b.pv[v.part0 + p].tbl_entries);
			max_l = std::max(max_l, b.pv[v.part0 + p].listeners);
		}
	}
	CHECK(f.max_len == max_len && f.nwg == nwg && f.max_tbl == max_tbl && f.max_l == max_l, "maxima: len %llu workgroups %llu table %u listeners %u",
	      (unsigned long long)f.max_len, (unsigned long long)f.nwg, f.max_tbl, f.max_l);
	CHECK(f.host_parts == parts && f.cands == cands, "parts %d (want %d) cands %d (want %d)", (int)f.host_parts, (int)parts, (int)f.cands, (int)cands);
	// the estimate as run_resp_batch had it in line (gys_engine.hip:1173-1175 of commit ffbe5ed)
	const double t_host = (double)((nwg + ncu - 1) / ncu) * (double)max_len / 0.35e9;
	const double t_split = (double)b.n * (double)std::max<uint64_t>(nwg, 1) / (double)std::max<uint32_t>(nsegs, 1) / 40.0e9 + 20e-6;
	const bool want = max_len > SP && (resp_path == 3 || (resp_path == 0 && t_split < t_host));
	CHECK(f.host_split == want, "resp_path %u ncu %d: split %d, want %d (t_split %g t_host %g max_len %llu)", resp_path, ncu, (int)f.host_split, (int)want, t_split, t_host,
	      (unsigned long long)max_len);
	if (resp_path == 3) CHECK(f.host_split == (max_len > SP), "resp_path 3: split %d with max_len %llu", (int)f.host_split, (unsigned long long)max_len);
	if (resp_path == 0 && max_len > SP) n_split[f.host_split]++;
}

int n_tile[3] = {0, 0, 0};

void check_tile(std::mt19937_64 &rng)
{
	const uint32_t max_tbl = 16u << (rng() % 10), keys = 2u * (1u + (uint32_t)(rng() % 2048));
	const uint32_t dyn_max = (160u * 1024u - (uint32_t)(rng() % 3 ? 5656u : rng() % 16384)) & ~255u; // (5656: the largest static part of today's instances)
	for (int mode = 0; mode < 3; ++mode) {
		const uint32_t tile = resp_tile_events(mode, max_tbl, keys, dyn_max);
		const bool two = resp_host_lds_bytes(max_tbl, keys, 6144u) + 160u * 1024u - dyn_max <= 80u * 1024u;
		CHECK(mode == 0 || tile != 6144u, "mode %d in the 6144-event form", mode);
		CHECK((tile == 6144u) == (mode == 0 && two), "mode %d table %u keys %u room %u: tile %u, two workgroups fit: %d", mode, max_tbl, keys, dyn_max, tile, (int)two);
		if (tile != 6144u) CHECK((tile == 16384u) == (resp_host_lds_bytes(max_tbl, keys, 16384u) <= dyn_max) && (tile == 16384u || tile == 8192u), "mode %d: tile %u", mode, tile);
		n_tile[tile == 6144u ? 0 : tile == 16384u ? 1 : 2]++;
	}
}
} // namespace

int main(int argc, char **argv)
{
	std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
	const int ncus[] = {1, 8, 256};
	for (int it = 0; it < 1500; ++it) {
		const bool many = it % 5 == 4;
		const Batch b = random_batch(rng, it % 3 != 0, many);
		check_virtual_segments(b, false);
		check_virtual_segments(b, true);
		for (uint32_t path = 0; path < 4; ++path) check_front(b, many ? 256 : ncus[rng() % 3], path);
		check_tile(rng);
	}
	{ // a zero-length segment produces no virtual segment, with or without listener parts
		Batch z;
		z.sv.push_back(RespSegView{3, 0, 0, false, false, false, 4, 0, 7});
		z.sv.push_back(RespSegView{4, 0, 0, false, false, false, 0, 4, 0});
		for (int p = 0; p < 5; ++p) z.pv.push_back(RespPartView{16, 1, true});
		CHECK(resp_virtual_segments(z.sv.data(), 2, true, MAX_HOSTS, nullptr) == 0 && resp_virtual_segments(z.sv.data(), 2, false, MAX_HOSTS, nullptr) == 0, "zero-length segments made entries");
	}
	CHECK(n_split[0] > 20 && n_split[1] > 20, "resp_path 0 with long segments: %d unsplit, %d split -- the inputs do not reach both", n_split[0], n_split[1]);
	CHECK(n_tile[0] > 20 && n_tile[1] > 20 && n_tile[2] > 20, "tile forms reached: %d / %d / %d", n_tile[0], n_tile[1], n_tile[2]);
	if (fails) {
		printf("%d checks failed\n", fails);
		return 1;
	}
	printf("resp plan ok (%d / %d unsplit / split, tiles %d / %d / %d)\n", n_split[0], n_split[1], n_tile[0], n_tile[1], n_tile[2]);
	return 0;
}
