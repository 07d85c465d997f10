// TEST INFRASTRUCTURE (CPU): the task -> services list of the service dependency graph (gyeeta_amd/csrc/gys_svcdeps_host.hpp,
// task_lists_build) and the kernels' lookup over it (dep_task_find, gyeeta_amd/csrc/gys_svcdeps.hpp) against a std::map: empty input, every
// slot unbound (id 0), equal ids, one task with 70 slots, free slots with a stale binding, ids at both ends of the 64-bit range, random
// bindings.  A stand-alone program; build + run (plain and with AddressSanitizer): tests/test_kernel_logic_svcdeps_cpu.py.
#define GYS_OPAQUE_VGPR(x) asm volatile("" : "+r"(x))
#define GYS_OPAQUE_LOADED4(a) asm volatile("" : "+r"(a[0]), "+r"(a[1]), "+r"(a[2]), "+r"(a[3]))
#define GYS_DYN_LDS(type, name) type *name = (type *)kemu::dyn_lds()
#include "../../gyeeta_amd/csrc/gys_kernels.hpp"
#include "../../gyeeta_amd/csrc/gys_actpairs.hpp"
#include "../../gyeeta_amd/csrc/gys_svcdeps.hpp"
#include "../../gyeeta_amd/csrc/gys_svcdeps_host.hpp"

#include <stdio.h>

#include <map>
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

const uint32_t FREE = 0xFFFFFFFFu;

void check(const std::vector<uint64_t> &task, const std::vector<uint32_t> *host, const char *what)
{
	const uint32_t n = (uint32_t)task.size();
	std::map<uint64_t, std::vector<uint32_t>> want;
	for (uint32_t s = 0; s < n; ++s)
		if (task[s] && !(host && (*host)[s] == FREE)) want[task[s]].push_back(s); // (ascending s)
	const TaskLists tl = task_lists_build(task.data(), host ? host->data() : nullptr, FREE, n);
	CHECK(tl.ids.size() == want.size() && tl.off.size() == want.size() + 1 && tl.off[0] == 0, "%s: %zu ids, %zu offsets for %zu tasks", what, tl.ids.size(), tl.off.size(), want.size());
	if (tl.ids.size() != want.size() || tl.off.size() != want.size() + 1) return;
	uint32_t t = 0, nb = 0, longest = 0;
	for (const auto &kv : want) {
		CHECK(tl.ids[t] == kv.first, "%s: ids[%u]", what, t);
		CHECK(tl.off[t + 1] - tl.off[t] == kv.second.size() && tl.off[t + 1] <= tl.slots.size(), "%s: the list of task %u", what, t);
		if (tl.off[t + 1] - tl.off[t] == kv.second.size() && tl.off[t + 1] <= tl.slots.size())
			for (size_t j = 0; j < kv.second.size(); ++j) CHECK(tl.slots[tl.off[t] + j] == kv.second[j], "%s: member %zu of task %u", what, j, t);
		CHECK(dep_task_find(tl.ids.data(), tl.ntasks(), kv.first) == t, "%s: the lookup of ids[%u]", what, t);
		CHECK(dep_task_find(tl.ids.data(), tl.ntasks(), kv.first + 1) == (want.count(kv.first + 1) ? t + 1 : GYS_DEP_NOTASK), "%s: the lookup behind ids[%u]", what, t);
		nb += (uint32_t)kv.second.size();
		longest = std::max<uint32_t>(longest, (uint32_t)kv.second.size());
		++t;
	}
	CHECK(tl.nbound() == nb && tl.slots.size() == nb && tl.longest() == longest, "%s: %u bound, longest %u", what, tl.nbound(), tl.longest());
	CHECK(dep_task_find(tl.ids.data(), tl.ntasks(), 0) == GYS_DEP_NOTASK, "%s: id 0 is found", what);
}
} // namespace

int main()
{
	check({}, nullptr, "empty");
	check(std::vector<uint64_t>(9, 0), nullptr, "all unbound");
	check(std::vector<uint64_t>(9, 5), nullptr, "equal ids");
	check({7}, nullptr, "one");
	check({0, 3, 0, 3, 1, 0xFFFFFFFFFFFFFFFFull, 1, 0x8000000000000000ull, 0}, nullptr, "both ends of the range");
	{
		std::vector<uint64_t> task(200, 0);
		for (uint32_t s = 0; s < 200; ++s) task[s] = s % 2 ? 0x7070 : (s % 6 == 0 ? 0 : 0x100 + s); // 100 slots of one task
		check(task, nullptr, "one large task");
		std::vector<uint64_t> t70(90, 0);
		for (uint32_t s = 10; s < 80; ++s) t70[s] = 42;
		check(t70, nullptr, "70 slots of one task");
		std::vector<uint32_t> host(200, 0);
		for (uint32_t s = 0; s < 200; s += 7) host[s] = FREE; // stale bindings of free slots
		check(task, &host, "free slots");
		std::vector<uint32_t> all_free(200, FREE);
		check(task, &all_free, "every slot free");
	}
	std::mt19937_64 rng(7);
	for (int rep = 0; rep < 50; ++rep) {
		const uint32_t n = (uint32_t)(rng() % 300);
		std::vector<uint64_t> task(n);
		std::vector<uint32_t> host(n);
		for (uint32_t s = 0; s < n; ++s) {
			task[s] = rng() % 4 == 0 ? 0 : 1 + rng() % (rep % 2 ? 5 : 1000);
			host[s] = rng() % 9 == 0 ? FREE : (uint32_t)(rng() % 4);
		}
		check(task, &host, "random");
	}
	if (fails) {
		printf("svcdeps host: %d failures\n", fails);
		return 1;
	}
	printf("svcdeps host ok\n");
	return 0;
}
