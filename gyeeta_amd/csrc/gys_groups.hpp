// gys_groups.hpp -- the member lists of the roll-ups as pure host functions: which members a group has (off / members, CSR) and how a
// workgroup-sized pass walks them (chunks of at most `per` members, and per group the range of its chunks as the members of a second pass).
// No HIP call in here: the engine uploads what these build (DeviceGroups in gys_engine.hip), tests/cpp/test_groups.cc checks them on the CPU.
// Needs RollupChunk (gys_rollup.hpp) declared before it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace gys {

struct GroupLists {
	std::vector<uint32_t> off;     // [groups + 1]: members[off[g], off[g + 1]) belong to group g
	std::vector<uint32_t> members;
	std::vector<RollupChunk> chunks;  // groups_chunk(): {group, m0, m1}, group after group
	std::vector<RollupChunk> gchunks; // groups_chunk(): [groups] {group, first chunk, end chunk} of `chunks`
	uint32_t ngroups() const { return off.empty() ? 0u : (uint32_t)off.size() - 1u; }
};

inline void rollup_chunks(const std::vector<uint32_t> &off, uint32_t per, std::vector<RollupChunk> &chunks)
{
	for (uint32_t g = 0; g + 1 < (uint32_t)off.size(); ++g)
		for (uint32_t m = off[g]; m < off[g + 1]; m += per) chunks.push_back(RollupChunk{g, m, std::min(off[g + 1], m + per), 0u});
}

// the chunks of group g (rollup_chunks lays them out group after group) as ONE chunk of a second pass: {g, first chunk, end chunk}
inline void rollup_group_chunks(const std::vector<RollupChunk> &chunks, uint32_t ngroups, std::vector<RollupChunk> &gchunks)
{
	size_t i = 0;
	for (uint32_t g = 0; g < ngroups; ++g) {
		const uint32_t c0 = (uint32_t)i;
		while (i < chunks.size() && chunks[i].group == g) ++i;
		gchunks.push_back(RollupChunk{g, c0, (uint32_t)i, 0u});
	}
}

// (re)cuts g's groups into chunks of at most `per` members (per >= 1)
inline void groups_chunk(GroupLists &g, uint32_t per)
{
	g.chunks.clear();
	g.gchunks.clear();
	rollup_chunks(g.off, per, g.chunks);
	rollup_group_chunks(g.chunks, g.ngroups(), g.gchunks);
}

// group g = lists[g], in the order given
inline GroupLists groups_from_lists(const std::vector<std::vector<uint32_t>> &lists)
{
	GroupLists g;
	g.off.assign(lists.size() + 1, 0u);
	for (size_t i = 0; i < lists.size(); ++i) {
		g.members.insert(g.members.end(), lists[i].begin(), lists[i].end());
		g.off[i + 1] = (uint32_t)g.members.size();
	}
	return g;
}

// group k = the items i with key[i] == k, in ascending i (a stable counting sort); an item whose key is not below ngroups is in no group
inline GroupLists groups_from_keys(const std::vector<uint32_t> &key, uint32_t ngroups)
{
	GroupLists g;
	g.off.assign((size_t)ngroups + 1, 0u);
	for (uint32_t k : key)
		if (k < ngroups) g.off[k + 1]++;
	for (uint32_t k = 0; k < ngroups; ++k) g.off[k + 1] += g.off[k];
	g.members.resize(g.off[ngroups]);
	std::vector<uint32_t> at(g.off.begin(), g.off.end() - 1);
	for (uint32_t i = 0; i < (uint32_t)key.size(); ++i)
		if (key[i] < ngroups) g.members[at[key[i]]++] = i;
	return g;
}

// one group: 0 .. n-1
inline GroupLists groups_single(uint32_t n)
{
	GroupLists g;
	g.off = {0u, n};
	g.members.resize(n);
	for (uint32_t i = 0; i < n; ++i) g.members[i] = i;
	return g;
}

} // namespace gys
