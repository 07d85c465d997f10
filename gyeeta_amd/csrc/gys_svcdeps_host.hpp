// gys_svcdeps_host.hpp -- the task -> services list of the service dependency graph as a pure host function: from the per-slot bindings
// (gys_set_listener_tasks; 0 = unbound) the distinct task ids in ascending order, and per task the slots bound to it in ascending order (off /
// slots, CSR).  No HIP call in here: the engine uploads what this builds (gys_svcdeps_engine.hpp), the kernels read it (gys_svcdeps.hpp:
// a binary search over `ids`), tests/cpp/test_svcdeps_host.cc checks it on the CPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace gys {

struct TaskLists {
	std::vector<uint64_t> ids;   // [ntasks] ascending, distinct, never 0
	std::vector<uint32_t> off;   // [ntasks + 1]: slots[off[t], off[t + 1]) are bound to ids[t]
	std::vector<uint32_t> slots; // [bound services]
	uint32_t ntasks() const { return (uint32_t)ids.size(); }
	uint32_t nbound() const { return (uint32_t)slots.size(); }
	uint32_t longest() const
	{
		uint32_t m = 0;
		for (size_t t = 0; t + 1 < off.size(); ++t) m = std::max(m, off[t + 1] - off[t]);
		return m;
	}
};

// task[s] = the binding of slot s (0: none); host[s] == free_host marks a free slot, which is in no list whatever its binding says
// (host may be nullptr: every slot counts)
inline TaskLists task_lists_build(const uint64_t *task, const uint32_t *host, uint32_t free_host, uint32_t nsvc)
{
	std::vector<std::pair<uint64_t, uint32_t>> kv;
	for (uint32_t s = 0; s < nsvc; ++s)
		if (task[s] != 0 && !(host && host[s] == free_host)) kv.emplace_back(task[s], s);
	std::sort(kv.begin(), kv.end());
	TaskLists tl;
	tl.off.push_back(0u);
	tl.slots.reserve(kv.size());
	for (size_t i = 0; i < kv.size(); ++i) {
		if (i && kv[i].first != kv[i - 1].first) tl.off.push_back((uint32_t)i);
		if (!i || kv[i].first != kv[i - 1].first) tl.ids.push_back(kv[i].first);
		tl.slots.push_back(kv[i].second);
	}
	if (!kv.empty()) tl.off.push_back((uint32_t)kv.size());
	return tl;
}

} // namespace gys
