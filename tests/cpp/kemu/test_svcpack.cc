// TEST INFRASTRUCTURE (CPU): the LOGIC of the service-record kernels (gyeeta_amd/csrc/gys_svcpack.hpp) under the CPU stand-in of the device
// model.  A synthetic segment list -- carried segments of 2, 4, 8, 24, 32, 96 (the kept state: host word), 256, 16 (an HLL file at p = 4) and
// 1 024 bytes, the cursor word, two "reset" segments, a "kept" one and a carried array the context has not allocated -- over per-byte
// patterns that differ per service; value buffers at a stride of cap + 65 words, so services sit at all four residues from a 16-byte
// boundary, with cursors 0, 1, 3, 4, 5, cap - 1 and cap.
//   * pack -> k_svc_clear -> unpack into ANOTHER context (other slots: a different permutation, other host slots, more services) is the
//     identity on every carried byte; the reset segments hold their initial value, the kept one is untouched, the host word holds the
//     destination's host slot (an all-zero state entry stays all zero), the buffer words behind the cursor keep their poison;
//   * the same through the source itself (pack, clear the slots, unpack): every array equals its snapshot;
//   * every byte of a record is written by the pack (pads and the words behind the cursor are zero); slots that are not listed and ids
//     marked as not registered are untouched; n = 0, 1 and more services than the grid has workgroups.
// Build + run: tests/test_kernel_logic_svcpack_cpu.py (plain, and with -fsanitize=address,undefined).
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../../gyeeta_amd/csrc/gys_rollup.hpp"
#include "../../../gyeeta_amd/csrc/gys_hllroll.hpp"
#include "../../../gyeeta_amd/csrc/gys_svcquery.hpp"
#include "../../../gyeeta_amd/csrc/gys_rollsel.hpp"
#include "../../../gyeeta_amd/csrc/gys_svcdel.hpp"
#include "../../../gyeeta_amd/csrc/gys_svcpack.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>

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

constexpr uint32_t CAP = 40, PCAP = CAP + 65;
const uint4 FILL = make_uint4(0x11111111u, 0x22222222u, 0x33333333u, 0x44444444u), LAST = make_uint4(1u, 2u, 3u, 4u);

struct SegDef {
	uint64_t bytes;
	uint32_t kind;
	bool absent, cursor;
};
const SegDef DEFS[] = {{8, GYS_SVCSEG_KEEP, false, false},  {2, GYS_SVCSEG_CARRY, false, false},   {4, GYS_SVCSEG_CARRY, false, false},
		       {8, GYS_SVCSEG_CARRY, false, false}, {24, GYS_SVCSEG_CARRY, false, false},  {32, GYS_SVCSEG_CARRY, false, false},
		       {96, GYS_SVCSEG_CARRY_HOST, false, false}, {256, GYS_SVCSEG_CARRY, false, false}, {8, GYS_SVCSEG_RESET, false, false},
		       {16, GYS_SVCSEG_CARRY, false, false}, {1024, GYS_SVCSEG_CARRY, false, false}, {4, GYS_SVCSEG_CARRY, false, true},
		       {4, GYS_SVCSEG_RESET, false, false}, {4, GYS_SVCSEG_CARRY, true, false},   {16, GYS_SVCSEG_CARRY, true, false}};
constexpr size_t NDEF = sizeof(DEFS) / sizeof(DEFS[0]);

inline bool carried(uint32_t kind) { return kind == GYS_SVCSEG_CARRY || kind == GYS_SVCSEG_CARRY_HOST; }

// a context: the arrays of S services (16-byte aligned bases), the value buffers
struct Ctx {
	uint32_t S;
	std::vector<std::vector<uint8_t>> arr;
	std::vector<SvcClearSeg> segs;
	std::vector<uint32_t> pend; // [S * PCAP + 4], the service buffers from an odd word on
	uint32_t *pend_base;
	SvcPackP p{};
	explicit Ctx(uint32_t S_) : S(S_), pend((size_t)S_ * PCAP + 8, 0xDEADBEEFu)
	{
		uint64_t off = 0;
		for (const SegDef &d : DEFS) arr.emplace_back((size_t)S * d.bytes + 16, (uint8_t)0x5A);
		for (size_t i = 0; i < NDEF; ++i) {
			uint8_t *base = DEFS[i].absent ? nullptr : (uint8_t *)(((uintptr_t)arr[i].data() + 15) & ~(uintptr_t)15);
			segs.push_back(SvcClearSeg{base, DEFS[i].bytes, FILL, LAST, DEFS[i].kind, 0u});
		}
		for (int pass = 0; pass < 2; ++pass) // the record layout rule of the library: multiples of 16 first, then the rest rounded to 4 bytes
			for (size_t i = 0; i < NDEF; ++i) {
				if (!carried(DEFS[i].kind) || ((DEFS[i].bytes & 15) == 0) != (pass == 0)) continue;
				segs[i].rec_off = (uint32_t)off;
				if (DEFS[i].cursor) p.cur_off = (uint32_t)off;
				off += (DEFS[i].bytes + 3) & ~3ull;
			}
		pend_base = (uint32_t *)(((uintptr_t)pend.data() + 15) & ~(uintptr_t)15) + 1; // service 0 one word behind a boundary
		p.nsegs = (uint32_t)NDEF;
		p.max_services = S;
		p.pad_off = (uint32_t)off;
		p.pend_off = (uint32_t)((off + 15) & ~15ull);
		p.stride = (p.pend_off + 4u * CAP + 15u) & ~15u;
		p.td_pend = pend_base;
		p.pcap = PCAP;
		p.pend_cap = CAP;
		for (size_t i = 0; i < NDEF; ++i)
			if (DEFS[i].cursor) p.td_cur = (const uint32_t *)segs[i].base;
	}
	uint8_t *at(size_t i, uint32_t slot) { return segs[i].base + (size_t)slot * DEFS[i].bytes; }
	uint32_t &cursor(uint32_t slot) { return ((uint32_t *)p.td_cur)[slot]; }
	uint32_t *buf(uint32_t slot) { return pend_base + (size_t)slot * PCAP; }
	void clear(const std::vector<uint32_t> &slots) // k_svc_clear over the arrays the context has
	{
		std::vector<SvcClearSeg> have;
		for (const SvcClearSeg &sg : segs)
			if (sg.base) have.push_back(sg);
		const SvcClearSeg *sp = have.data();
		const uint32_t *lp = slots.data();
		const uint32_t ns = (uint32_t)have.size(), nl = (uint32_t)slots.size(), ms = S;
		if (nl) kemu::launch(2, GYS_SVCCLEAR_NT, 0, [=] { k_svc_clear(sp, ns, lp, nl, ms); });
	}
};

inline uint8_t pat(size_t seg, uint32_t ident, uint64_t b) { return (uint8_t)(1u + ((seg * 131u + ident * 29u + b * 7u + (b >> 8)) % 251u)); }
const uint32_t CURSORS[] = {0, 1, 3, 4, 5, CAP - 1, CAP};

// the initial contents of byte b of a segment (what k_svc_clear stores)
uint8_t initial(uint64_t bytes, uint64_t b)
{
	const uint32_t f[4] = {FILL.x, FILL.y, FILL.z, FILL.w}, l[4] = {LAST.x, LAST.y, LAST.z, LAST.w};
	const bool last = bytes % 16 == 0 && b >= bytes - 16;
	const uint32_t w = (uint32_t)(b / 4) & 3u;
	return (uint8_t)((last ? l[w] : f[w]) >> (8 * (b & 3)));
}

void run_case(uint64_t seed, uint32_t n, uint32_t grid)
{
	std::mt19937_64 rng(seed * 1000 + n * 10 + grid);
	const uint32_t SA = 37, SB = 50;
	Ctx A(SA), B(SB);
	std::vector<uint32_t> pa(SA), pb(SB);
	for (uint32_t i = 0; i < SA; ++i) pa[i] = i;
	for (uint32_t i = 0; i < SB; ++i) pb[i] = i;
	std::shuffle(pa.begin(), pa.end(), rng);
	std::shuffle(pb.begin(), pb.end(), rng);
	// service k (k < n) lives in slot pa[k] of A and goes to slot pb[k] of B; k == 2 is not registered in B; every slot of A holds a pattern
	std::vector<uint32_t> ident_of(SA);
	for (uint32_t k = 0; k < SA; ++k) ident_of[pa[k]] = k;
	for (uint32_t s = 0; s < SA; ++s) {
		const uint32_t k = ident_of[s];
		for (size_t i = 0; i < NDEF; ++i) {
			if (DEFS[i].absent) continue;
			for (uint64_t b = 0; b < DEFS[i].bytes; ++b) A.at(i, s)[b] = pat(i, k, b);
			if (DEFS[i].kind == GYS_SVCSEG_CARRY_HOST) {
				if (k % 5 == 4) memset(A.at(i, s), 0, 96); // a service that never reported state
				else ((uint32_t *)A.at(i, s))[23] = 1000u + k; // A's host slot
			}
		}
		A.cursor(s) = CURSORS[k % 7];
		for (uint32_t w = 0; w < PCAP; ++w) A.buf(s)[w] = w < A.cursor(s) ? 0x10000u * (k + 1) + w : 0xDEADBEEFu;
	}
	std::vector<uint32_t> sa(n), sb(n), hb(n);
	for (uint32_t k = 0; k < n; ++k) {
		sa[k] = pa[k];
		sb[k] = k == 2 ? GYS_NOSLOT : pb[k];
		hb[k] = 7000u + k;
	}
	const Ctx A0 = A; // (vectors copied; the pointers of the copy still name A's memory: only its arr / pend contents are used below)
	std::vector<uint8_t> recs_mem((size_t)n * A.p.stride + 32, (uint8_t)0xEE);
	uint8_t *recs = (uint8_t *)(((uintptr_t)recs_mem.data() + 15) & ~(uintptr_t)15);
	CHECK(A.p.stride == B.p.stride && A.p.stride % 16 == 0, "stride");
	{
		SvcPackP p = A.p;
		p.segs = A.segs.data();
		p.n = n;
		p.slots = sa.data();
		p.recs = recs;
		if (n) kemu::launch(grid, GYS_SVCPACK_NT, 0, [=] { k_svc_pack(p); });
	}
	CHECK(A.arr == A0.arr && A.pend == A0.pend, "n %u: the pack modified its source", n);
	// every record byte is defined: carried bytes, zero pads, zero behind the cursor
	for (uint32_t k = 0; k < n; ++k) {
		std::vector<uint8_t> want(A.p.stride, 0);
		for (size_t i = 0; i < NDEF; ++i) {
			if (!carried(DEFS[i].kind)) continue;
			for (uint64_t b = 0; b < DEFS[i].bytes; ++b) want[A.segs[i].rec_off + b] = DEFS[i].absent ? initial(DEFS[i].bytes, b) : A.at(i, sa[k])[b];
		}
		memcpy(&want[A.p.pend_off], A.buf(sa[k]), 4u * A.cursor(sa[k]));
		for (uint32_t b = 0; b < A.p.stride; ++b)
			if (recs[(size_t)k * A.p.stride + b] != want[b]) {
				CHECK(false, "n %u grid %u: record %u byte %u is %02x, expected %02x", n, grid, k, b, recs[(size_t)k * A.p.stride + b], want[b]);
				break;
			}
	}
	CHECK(recs[(size_t)n * A.p.stride] == 0xEE, "the pack wrote behind the last record");

	// ---- into B: cleared slots, junk in the reset segments, poison in the buffers
	std::vector<uint32_t> listed_b;
	for (uint32_t k = 0; k < n; ++k)
		if (sb[k] != GYS_NOSLOT) listed_b.push_back(sb[k]);
	B.clear(listed_b);
	for (size_t i = 0; i < NDEF; ++i)
		if (DEFS[i].kind == GYS_SVCSEG_RESET || DEFS[i].kind == GYS_SVCSEG_KEEP)
			for (uint32_t s : listed_b) memset(B.at(i, s), 0x77, DEFS[i].bytes);
	const Ctx B0 = B;
	{
		SvcPackP p = B.p;
		p.segs = B.segs.data();
		p.n = n;
		p.slots = sb.data();
		p.hosts = hb.data();
		p.recs = recs;
		if (n) kemu::launch(grid, GYS_SVCPACK_NT, 0, [=] { k_svc_unpack(p); });
	}
	std::vector<int> k_of(SB, -1);
	for (uint32_t k = 0; k < n; ++k)
		if (sb[k] != GYS_NOSLOT) k_of[sb[k]] = (int)k;
	for (uint32_t s = 0; s < SB; ++s)
		for (size_t i = 0; i < NDEF; ++i) {
			if (DEFS[i].absent) continue;
			const int k = k_of[s];
			for (uint64_t b = 0; b < DEFS[i].bytes; ++b) {
				uint8_t want;
				const uint8_t before = B0.arr[i][(size_t)(B.at(i, s) - B.arr[i].data()) + b];
				if (k < 0 || DEFS[i].kind == GYS_SVCSEG_KEEP) want = before;
				else if (DEFS[i].kind == GYS_SVCSEG_RESET) want = initial(DEFS[i].bytes, b);
				else {
					want = A.at(i, sa[k])[b];
					const uint32_t *st = (const uint32_t *)A.at(i, sa[k]);
					if (DEFS[i].kind == GYS_SVCSEG_CARRY_HOST && b >= 92 && (st[0] | st[1])) want = (uint8_t)(hb[k] >> (8 * (b - 92)));
				}
				if (B.at(i, s)[b] != want) {
					CHECK(false, "n %u grid %u: B slot %u segment %zu (%llu bytes) byte %llu is %02x, expected %02x", n, grid, s, i,
					      (unsigned long long)DEFS[i].bytes, (unsigned long long)b, B.at(i, s)[b], want);
					break;
				}
			}
		}
	for (uint32_t s = 0; s < SB; ++s) {
		const int k = k_of[s];
		const uint32_t cur = k < 0 ? 0u : A.cursor(sa[k]);
		for (uint32_t w = 0; w < PCAP; ++w) {
			const uint32_t want = w < cur ? A.buf(sa[k])[w] : 0xDEADBEEFu;
			if (B.buf(s)[w] != want) {
				CHECK(false, "n %u grid %u: B slot %u buffer word %u is %08x, expected %08x (cursor %u)", n, grid, s, w, B.buf(s)[w], want, cur);
				break;
			}
		}
	}
	CHECK(B.pend.front() == 0xDEADBEEFu && B.pend.back() == 0xDEADBEEFu, "the unpack wrote outside the buffers");

	// ---- through the source itself: pack, clear, unpack = what it was (the host word: A's own host slots)
	std::vector<uint32_t> ha(n);
	for (uint32_t k = 0; k < n; ++k) ha[k] = 1000u + k;
	A.clear(sa);
	if (n) CHECK(A.arr != A0.arr, "the clear changed nothing");
	{
		SvcPackP p = A.p;
		p.segs = A.segs.data();
		p.n = n;
		p.slots = sa.data();
		p.hosts = ha.data();
		p.recs = recs;
		if (n) kemu::launch(grid, GYS_SVCPACK_NT, 0, [=] { k_svc_unpack(p); });
	}
	for (size_t i = 0; i < NDEF; ++i) {
		if (DEFS[i].absent) continue;
		if (carried(DEFS[i].kind)) CHECK(A.arr[i] == A0.arr[i], "n %u grid %u: segment %zu differs after pack, clear, unpack", n, grid, i);
	}
	CHECK(A.pend == A0.pend, "n %u grid %u: the buffers differ after pack, clear, unpack", n, grid);
}

} // namespace

int main(int argc, char **argv)
{
	const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
	if (!kemu::can_run(GYS_SVCPACK_NT)) {
		printf("cannot start %u threads here\n", GYS_SVCPACK_NT);
		return 77;
	}
	for (uint32_t n : {0u, 1u, 29u})
		for (uint32_t grid : {2u, 4u}) run_case(seed, n, grid);
	if (fails) {
		printf("kemu svcpack: %d failures\n", fails);
		return 1;
	}
	printf("kemu svcpack ok\n");
	return 0;
}
