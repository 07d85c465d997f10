// TEST INFRASTRUCTURE (CPU): the group-list builders of gyeeta_amd/csrc/gys_groups.hpp against their plain definitions, over seeded random
// inputs: group sizes 0, 1, per - 1, per, per + 1 and 3 * per for per in {1, 32, 1024}, in a shuffled order of groups.
//   * every member appears exactly once, inside its group's off range and in the stated order (lists: as given; keys: ascending item);
//   * a group's chunks tile [off[g], off[g + 1]) in order, none empty, none longer than per;
//   * gchunks[g] names exactly that group's chunk range (an empty group: an empty range);
//   * the key builder leaves out the items whose key is outside the domain and is stable; the single-group builder with n = 0 yields one
//     empty group.
// Build (g++ -fsanitize=address,undefined) + run: tests/test_groups_cpu.py.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../gyeeta_amd/csrc/gys_rollup.hpp"
#include "../../gyeeta_amd/csrc/gys_groups.hpp"

#include <stdio.h>
#include <stdlib.h>

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

// g's off / members hold exactly `want` (group by group, in order); its chunks and gchunks are those of `per`
void check_lists(const GroupLists &g, const std::vector<std::vector<uint32_t>> &want, uint32_t per, const char *what)
{
	const uint32_t ng = (uint32_t)want.size();
	CHECK(g.ngroups() == ng && g.off.size() == (size_t)ng + 1 && g.off[0] == 0, "%s per %u: %u groups, %zu offsets", what, per, g.ngroups(), g.off.size());
	if (g.off.size() != (size_t)ng + 1) return;
	size_t total = 0;
	for (uint32_t k = 0; k < ng; ++k) {
		total += want[k].size();
		CHECK(g.off[k + 1] == total, "%s per %u: off[%u] = %u, want %zu", what, per, k + 1, g.off[k + 1], total);
	}
	CHECK(g.members.size() == total, "%s per %u: %zu members, want %zu", what, per, g.members.size(), total);
	if (g.members.size() != total || g.off[ng] != total) return;
	for (uint32_t k = 0; k < ng; ++k)
		for (size_t i = 0; i < want[k].size(); ++i)
			CHECK(g.members[g.off[k] + i] == want[k][i], "%s per %u: group %u member %zu = %u, want %u", what, per, k, i, g.members[g.off[k] + i], want[k][i]);
	// chunks: group after group, tiling the group's range in order
	CHECK(g.gchunks.size() == ng, "%s per %u: %zu gchunks", what, per, g.gchunks.size());
	if (g.gchunks.size() != ng) return;
	uint32_t ci = 0;
	for (uint32_t k = 0; k < ng; ++k) {
		const RollupChunk gc = g.gchunks[k];
		CHECK(gc.group == k && gc.m0 == ci, "%s per %u: gchunks[%u] = {%u, %u, %u}, its chunks start at %u", what, per, k, gc.group, gc.m0, gc.m1, ci);
		uint32_t at = g.off[k];
		while (ci < g.chunks.size() && g.chunks[ci].group == k) {
			const RollupChunk ck = g.chunks[ci];
			CHECK(ck.m0 == at && ck.m1 > ck.m0 && ck.m1 - ck.m0 <= per && ck.m1 <= g.off[k + 1], "%s per %u: chunk %u of group %u = [%u, %u), at %u of [%u, %u)", what, per, ci,
			      k, ck.m0, ck.m1, at, g.off[k], g.off[k + 1]);
			at = ck.m1;
			++ci;
		}
		CHECK(at == g.off[k + 1], "%s per %u: the chunks of group %u end at %u, the group at %u", what, per, k, at, g.off[k + 1]);
		CHECK(gc.m1 == ci, "%s per %u: gchunks[%u] ends at chunk %u, the group's chunks at %u", what, per, k, gc.m1, ci);
		CHECK((g.off[k] == g.off[k + 1]) == (gc.m0 == gc.m1), "%s per %u: group %u of %u members has %u chunks", what, per, k, g.off[k + 1] - g.off[k], gc.m1 - gc.m0);
		CHECK(gc.m1 - gc.m0 == (g.off[k + 1] - g.off[k] + per - 1) / per, "%s per %u: group %u of %u members has %u chunks", what, per, k, g.off[k + 1] - g.off[k], gc.m1 - gc.m0);
	}
	CHECK(ci == g.chunks.size(), "%s per %u: %zu chunks, %u belong to a group", what, per, g.chunks.size(), ci);
}
} // namespace

int main(int argc, char **argv)
{
	std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
	for (uint32_t per : {1u, 32u, 1024u}) {
		std::vector<uint32_t> sizes = {0u, 1u, per - 1u, per, per + 1u, 3u * per, 0u, per};
		std::shuffle(sizes.begin(), sizes.end(), rng);
		const uint32_t ng = (uint32_t)sizes.size();
		// ---- lists: any member values (slots out of order, as after slot reuse), kept as given
		std::vector<std::vector<uint32_t>> lists(ng);
		for (uint32_t k = 0; k < ng; ++k)
			for (uint32_t i = 0; i < sizes[k]; ++i) lists[k].push_back((uint32_t)rng());
		GroupLists g = groups_from_lists(lists);
		groups_chunk(g, per);
		check_lists(g, lists, per, "lists");
		groups_chunk(g, per); // (cut again: the lists are replaced, not appended to)
		check_lists(g, lists, per, "lists, cut twice");
		// ---- keys: the items of every group scattered among each other and among items without a group (key >= ng)
		std::vector<uint32_t> key;
		for (uint32_t k = 0; k < ng; ++k) key.insert(key.end(), sizes[k], k);
		for (uint32_t i = 0; i < 100; ++i) key.push_back(i & 1u ? ng + (uint32_t)(rng() % 5) : ~0u - (uint32_t)(rng() % 3));
		std::shuffle(key.begin(), key.end(), rng);
		std::vector<std::vector<uint32_t>> want(ng);
		for (uint32_t i = 0; i < (uint32_t)key.size(); ++i)
			if (key[i] < ng) want[key[i]].push_back(i); // the plain definition: ascending item inside a group
		g = groups_from_keys(key, ng);
		groups_chunk(g, per);
		check_lists(g, want, per, "keys");
		// ---- one group of 0 .. n-1
		for (uint32_t n : {0u, 1u, per - 1u, per, per + 1u, 3u * per}) {
			std::vector<std::vector<uint32_t>> one(1);
			for (uint32_t i = 0; i < n; ++i) one[0].push_back(i);
			g = groups_single(n);
			groups_chunk(g, per);
			check_lists(g, one, per, "single");
		}
	}
	{ // no group at all, no item at all
		GroupLists g = groups_from_lists({});
		groups_chunk(g, 32);
		check_lists(g, {}, 32, "no lists");
		g = groups_from_keys({}, 3);
		groups_chunk(g, 32);
		check_lists(g, std::vector<std::vector<uint32_t>>(3), 32, "no keys");
		g = groups_from_keys({0u, 1u}, 0);
		groups_chunk(g, 32);
		check_lists(g, {}, 32, "no domain");
	}
	if (fails) {
		printf("kemu groups: %d checks failed\n", fails);
		return 1;
	}
	printf("kemu groups ok\n");
	return 0;
}
