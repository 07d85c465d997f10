// TEST INFRASTRUCTURE (CPU): the LOGIC of the distinct-count kernels k_hll_estimate / k_hll_union (gyeeta_amd/csrc/gys_hllroll.hpp) under the
// CPU stand-in of the device model, for p = 4, 6, 8, 10 (1, 4, 16 and 64 lanes per register file):
//   * estimates of random files (sparse: linear counting; dense: the raw estimator), of all-zero files and of files with every register at
//     the largest rank 64 - p + 1, against gyo_hll_estimate within 1e-12 relative (both add at most 1024 positive terms, the oracle with
//     one rounding each, the kernel exactly: 2 x 1023 x 1.1e-16 = 2.3e-13, plus a few ulp for the division and the logarithm);
//   * the estimate is a function of the file alone: the same bits with one, three and seven workgroups, with the file at another position
//     of the array (other lanes of the wave, another wave, another workgroup) and alone in a launch of its own (gys_query_distinct's form);
//   * group files: groups of 0, 1, 3, 1024, 1500 and 2500 members (one, two and three chunks of 1024) out of shuffled member lists with
//     repeats, files with byte values above 127 among them, first pass per chunk + second pass per group as the engine runs them, and the
//     list-free form (a contiguous array cut into equal chunks: the cluster-free paths), byte for byte against gyo_hll_merge applied
//     member by member.
// Build + run: tests/test_kernel_logic_hll_cpu.py.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../../gyeeta_amd/csrc/gys_rollup.hpp"
#include "../../../gyeeta_amd/csrc/gys_hllroll.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

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

uint64_t bits(double d)
{
	uint64_t u;
	memcpy(&u, &d, 8);
	return u;
}

// a file as `nflows` random 64-bit hashes leave it
void fill(std::mt19937_64 &rng, uint8_t *f, int p, uint32_t nflows)
{
	memset(f, 0, (size_t)1 << p);
	for (uint32_t i = 0; i < nflows; ++i) gyo_hll_add(f, p, rng());
}

std::vector<double> estimate(const std::vector<uint8_t> &files, uint32_t n, int p, uint32_t grid)
{
	std::vector<double> out(n + 1, -1.0);
	const uint8_t *d = files.data();
	double *o = out.data();
	kemu::launch(grid, GYS_HLL_NT, 0, [=] { k_hll_estimate(d, n, (uint32_t)p, o); });
	CHECK(out[n] == -1.0, "p %d: the estimate kernel wrote past its %u outputs", p, n);
	out.resize(n);
	return out;
}

void test_estimates(std::mt19937_64 &rng, int p)
{
	const uint32_t m = 1u << p, n = 41; // (41: the last wave of the pass is ragged for every p)
	std::vector<uint8_t> files((size_t)n * m + 16, 0);
	const uint32_t flows[] = {0, 1, 2, m / 8, m / 2, m, 2 * m, 3 * m, 5 * m, 20 * m, 100 * m, 400 * m};
	for (uint32_t f = 0; f < n; ++f) {
		uint8_t *r = files.data() + (size_t)f * m;
		if (f == 3 || f == n - 1) continue;                                 // all zero
		if (f == 5 || f == n - 2) { memset(r, 64 - p + 1, m); continue; }   // every register at the largest rank
		if (f == 7) { memset(r, 1, m); continue; }
		fill(rng, r, p, flows[f % (sizeof(flows) / sizeof(flows[0]))]);
	}
	const std::vector<double> e1 = estimate(files, n, p, 1);
	int lin = 0, raw = 0;
	for (uint32_t f = 0; f < n; ++f) {
		const double want = gyo_hll_estimate(files.data() + (size_t)f * m, p);
		const double rel = want == 0.0 ? fabs(e1[f]) : fabs(e1[f] - want) / want;
		CHECK(rel <= 1e-12, "p %d file %u: estimate %.17g, oracle %.17g", p, f, e1[f], want);
		uint32_t z = 0;
		for (uint32_t i = 0; i < m; ++i) z += files[(size_t)f * m + i] == 0;
		if (z == m) CHECK(bits(e1[f]) == 0, "p %d file %u: the all-zero file gives %.17g", p, f, e1[f]);
		(want <= 2.5 * m && z ? lin : raw)++;
	}
	CHECK(lin >= 5 && raw >= 5, "p %d: %d linear-counting and %d raw cases", p, lin, raw);
	// other launch shapes
	for (uint32_t grid : {3u, 7u}) {
		const std::vector<double> e = estimate(files, n, p, grid);
		for (uint32_t f = 0; f < n; ++f) CHECK(bits(e[f]) == bits(e1[f]), "p %d file %u: %.17g with %u workgroups, %.17g with one", p, f, e[f], grid, e1[f]);
	}
	// other positions: the files rotated by 1 .. and reversed
	for (uint32_t rot : {1u, 5u, 17u}) {
		std::vector<uint8_t> moved((size_t)n * m + 16, 0);
		for (uint32_t f = 0; f < n; ++f) memcpy(moved.data() + (size_t)((f * 3 + rot) % n) * m, files.data() + (size_t)f * m, m);
		const std::vector<double> e = estimate(moved, n, p, 2);
		for (uint32_t f = 0; f < n; ++f)
			CHECK(bits(e[(f * 3 + rot) % n]) == bits(e1[f]), "p %d file %u at position %u: %.17g, at its own %.17g", p, f, (f * 3 + rot) % n, e[(f * 3 + rot) % n], e1[f]);
	}
	// alone in a launch (one slot)
	for (uint32_t f = 0; f < n; f += 4) {
		std::vector<uint8_t> one(files.begin() + (size_t)f * m, files.begin() + (size_t)(f + 1) * m);
		one.resize(m + 16);
		const std::vector<double> e = estimate(one, 1, p, 1);
		CHECK(bits(e[0]) == bits(e1[f]), "p %d file %u alone: %.17g, in the scan %.17g", p, f, e[0], e1[f]);
	}
}

void launch_union(HllUnionP q, uint32_t grid)
{
	kemu::launch(grid, GYS_HLL_NT, 0, [=] { k_hll_union(q); });
}

void test_unions(std::mt19937_64 &rng, int p)
{
	const uint32_t m = 1u << p, nfiles = 300;
	std::vector<uint8_t> files((size_t)nfiles * m);
	for (uint32_t f = 0; f < nfiles; ++f) {
		uint8_t *r = files.data() + (size_t)f * m;
		if (f % 11 == 0) memset(r, 0, m);
		else if (f % 13 == 0) for (uint32_t i = 0; i < m; ++i) r[i] = (uint8_t)rng(); // any byte values (a caller's files)
		else fill(rng, r, p, (uint32_t)(rng() % (8 * m)) + 1);
	}
	const uint32_t sizes[] = {0, 1, 3, 1024, 0, 1500, 2500, 2, 1025};
	const uint32_t ng = sizeof(sizes) / sizeof(sizes[0]);
	std::vector<uint32_t> off(ng + 1, 0), members;
	for (uint32_t g = 0; g < ng; ++g) {
		for (uint32_t i = 0; i < sizes[g]; ++i) members.push_back(sizes[g] <= 3 ? (uint32_t)(rng() % nfiles) : (g == 3 ? 1u + (uint32_t)(rng() % 10) : (uint32_t)(rng() % nfiles)));
		off[g + 1] = (uint32_t)members.size();
	}
	std::vector<RollupChunk> chunks, gchunks;
	for (uint32_t g = 0; g < ng; ++g) {
		const uint32_t c0 = (uint32_t)chunks.size();
		for (uint32_t a = off[g]; a < off[g + 1]; a += 1024u) chunks.push_back(RollupChunk{g, a, std::min(off[g + 1], a + 1024u), 0u});
		gchunks.push_back(RollupChunk{g, c0, (uint32_t)chunks.size(), 0u});
	}
	std::vector<uint8_t> part(chunks.size() * m + 16, 0xEE), out((size_t)ng * m + 16, 0xEE);
	for (uint32_t grid : {1u, 4u}) {
		std::fill(part.begin(), part.end(), 0xEE);
		std::fill(out.begin(), out.end(), 0xEE); // (no pre-zeroed output needed)
		launch_union(HllUnionP{files.data(), part.data(), chunks.data(), members.data(), (uint32_t)chunks.size(), 0u, 0u, (uint32_t)p}, grid);
		launch_union(HllUnionP{part.data(), out.data(), gchunks.data(), nullptr, ng, 0u, 0u, (uint32_t)p}, grid);
		for (uint32_t g = 0; g < ng; ++g) {
			std::vector<uint8_t> want(m, 0);
			for (uint32_t a = off[g]; a < off[g + 1]; ++a) gyo_hll_merge(want.data(), files.data() + (size_t)members[a] * m, p);
			CHECK(memcmp(want.data(), out.data() + (size_t)g * m, m) == 0, "p %d group %u (%u members, grid %u): file differs from gyo_hll_merge", p, g, sizes[g], grid);
		}
		for (size_t i = 0; i < 16; ++i) CHECK(part[chunks.size() * m + i] == 0xEE && out[(size_t)ng * m + i] == 0xEE, "p %d: the union kernel wrote past its output", p);
	}
	// a contiguous array without lists: equal chunks, then the chunks' files
	for (uint32_t n : {1u, 3u, 300u}) {
		for (uint32_t per : {1024u, 128u, 7u}) {
			const uint32_t nch = (n + per - 1) / per;
			std::vector<uint8_t> p1((size_t)nch * m + 16, 0xEE), res(m + 16, 0xEE);
			launch_union(HllUnionP{files.data(), p1.data(), nullptr, nullptr, nch, n, per, (uint32_t)p}, 2);
			launch_union(HllUnionP{p1.data(), res.data(), nullptr, nullptr, 1u, nch, nch, (uint32_t)p}, 1);
			std::vector<uint8_t> want(m, 0);
			for (uint32_t f = 0; f < n; ++f) gyo_hll_merge(want.data(), files.data() + (size_t)f * m, p);
			CHECK(memcmp(want.data(), res.data(), m) == 0, "p %d: union of the first %u files in chunks of %u differs", p, n, per);
			CHECK(res[m] == 0xEE && p1[(size_t)nch * m] == 0xEE, "p %d: wrote past the output (n %u per %u)", p, n, per);
		}
	}
}
} // namespace

int main(int argc, char **argv)
{
	if (!kemu::can_run(GYS_HLL_NT)) {
		printf("kemu: this process cannot have 256 threads\n");
		return 77;
	}
	std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
	// hll_max4 on its own: every pair of byte values in every byte position
	for (uint32_t a = 0; a < 256; ++a)
		for (uint32_t b = 0; b < 256; ++b) {
			const uint32_t x = a | (b << 8) | (a << 16) | (b << 24), y = b | (a << 8) | ((255u - a) << 16) | (b << 24);
			const uint32_t mx = std::max(a, b), want = mx | (mx << 8) | (std::max(a, 255u - a) << 16) | (b << 24);
			CHECK(hll_max4(x, y) == want, "hll_max4(%08x, %08x) = %08x, want %08x", x, y, hll_max4(x, y), want);
		}
	for (int p : {4, 6, 8, 10}) {
		test_estimates(rng, p);
		test_unions(rng, p);
	}
	if (fails) {
		printf("kemu hllroll: %d failures\n", fails);
		return 1;
	}
	printf("kemu hllroll ok\n");
	return 0;
}
