// TEST INFRASTRUCTURE (CPU): the LOGIC of the level kernels k_hll_level_roll / k_hll_level_view (gyeeta_amd/csrc/gys_hllroll.hpp) under the CPU
// stand-in of the device model, for p = 4, 6, 8, 10 and 1, 63, 64, 65 and 1000 services, over a schedule of 64 window closes that crosses
// 30-s boundaries, wraps the 300-s ring, skips more than 300 s (the whole ring expires), crosses 43 200-s boundaries, skips more than
// 5 days, repeats a close time and goes backwards once (clamped).  The driver below does on the host what the engine's close and query do
// (include/gysketch.h, "distinct-flow counts of the closed windows": the clear masks, the current buckets, the live-bucket mask).
// After every close and at several query times, for every level:
//   the files of k_hll_level_view == the RING MODEL (the definition applied per service with gyo_hll_merge on plain arrays)
//                                 == the CLOSED FORM (the union of the windows with t_k / w > tq / w - 10; level 0: the last window for 5 s;
//                                    level 3: every window), byte for byte;
//   estimates within 1e-12 relative of gyo_hll_estimate (the bound tests/test_gpu_hll_rollup.py derives), exactly 0 for the all-zero file,
//   and the same bits from a one-slot launch (gys_query_distinct_level's form);
//   the open files are zero after the close, `last` is the closing window, a cleared current bucket holds exactly the closing window,
//   the slots above nsvc (the arrays are sized to max_services) are never written, and a view modifies no state.
// Build + run: tests/test_kernel_logic_hll_levels_cpu.py.
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

constexpr int64_t DUR[3] = {5, 300, 432000};
constexpr uint32_t RING = GYS_LEVEL_RING;
static_assert(GYS_LEVEL_RING == 10 && GYS_HLL_LVL_FILES == 22, "the issue's state: last + 2 x 10 + all");

int64_t bucket_start(int64_t t, int64_t dur, uint32_t j)
{
	const int64_t s = (t / dur) * dur + (int64_t)j * (dur / RING);
	return s <= t ? s : s - dur;
}
uint32_t bucket_idx(int64_t t, int64_t dur) { return (uint32_t)((t % dur) * RING / dur); }

struct Sim {
	int p;
	uint32_t m, nsvc, S; // S = max_services > nsvc
	std::vector<uint8_t> open, lvl; // [S] files; [22][S] files
	int64_t t_last = -1;
	// the ring model
	std::vector<uint8_t> m_last, m_all, m_ring[2][RING];
	int64_t mt_last = -1;
	// the closed form: every closed window
	std::vector<int64_t> wt;
	std::vector<std::vector<uint8_t>> wf;

	Sim(int p_, uint32_t n) : p(p_), m(1u << p_), nsvc(n), S(n + 3)
	{
		open.assign((size_t)S * m, 0);
		lvl.assign((size_t)GYS_HLL_LVL_FILES * S * m, 0);
		for (uint32_t f = 0; f < GYS_HLL_LVL_FILES; ++f) memset(arr(f) + (size_t)nsvc * m, 0xEE, (size_t)(S - nsvc) * m); // never to be touched
		memset(open.data() + (size_t)nsvc * m, 0xEE, (size_t)(S - nsvc) * m);
		m_last.assign((size_t)nsvc * m, 0);
		m_all = m_last;
		for (auto &l : m_ring)
			for (auto &b : l) b = m_last;
	}
	uint8_t *arr(uint32_t f) { return lvl.data() + (size_t)f * S * m; }

	void close(int64_t tsec, uint32_t grid)
	{
		// ---- the engine's side: masks + memsets on the host, one kernel
		const std::vector<uint8_t> closing(open.begin(), open.begin() + (size_t)nsvc * m);
		{
			const int64_t tnow = std::max(tsec, t_last);
			uint32_t mask[2] = {0, 0}, cur[2];
			for (int li = 0; li < 2; ++li) {
				for (uint32_t j = 0; j < RING; ++j)
					if (t_last >= 0 && bucket_start(tnow, DUR[li + 1], j) > t_last) mask[li] |= 1u << j;
				cur[li] = bucket_idx(tnow, DUR[li + 1]);
				for (uint32_t j = 0; j < RING; ++j)
					if (((mask[li] >> j) & 1u) && j != cur[li]) memset(arr(GYS_HLL_LVL_RING + li * RING + j), 0, (size_t)nsvc * m);
			}
			t_last = tnow;
			HllLevelRollP q{};
			q.open = (uint4 *)open.data();
			q.last = (uint4 *)arr(GYS_HLL_LVL_LAST);
			q.ring1 = (uint4 *)arr(GYS_HLL_LVL_RING + cur[0]);
			q.ring2 = (uint4 *)arr(GYS_HLL_LVL_RING + RING + cur[1]);
			q.all = (uint4 *)arr(GYS_HLL_LVL_ALL);
			q.npieces = (uint64_t)nsvc << (p - 4);
			q.fresh1 = (mask[0] >> cur[0]) & 1u;
			q.fresh2 = (mask[1] >> cur[1]) & 1u;
			kemu::launch(grid, GYS_HLL_NT, 0, [=] { k_hll_level_roll(q); });
			for (size_t i = 0; i < (size_t)nsvc * m; ++i)
				if (open[i]) {
					CHECK(false, "p %d nsvc %u: the open files are not zero after the close", p, nsvc);
					break;
				}
			CHECK(memcmp(arr(GYS_HLL_LVL_LAST), closing.data(), closing.size()) == 0, "p %d nsvc %u: `last` is not the closing window", p, nsvc);
			if (q.fresh1) CHECK(memcmp(q.ring1, closing.data(), closing.size()) == 0, "p %d nsvc %u t %lld: the cleared current 300-s bucket is not exactly the closing window", p, nsvc, (long long)tnow);
			if (q.fresh2) CHECK(memcmp(q.ring2, closing.data(), closing.size()) == 0, "p %d nsvc %u t %lld: the cleared current 5-day bucket is not exactly the closing window", p, nsvc, (long long)tnow);
			check_guard();
		}
		// ---- the ring model: the definition, file by file
		{
			const int64_t tnow = std::max(tsec, mt_last);
			for (int li = 0; li < 2; ++li) {
				for (uint32_t j = 0; j < RING; ++j)
					if (mt_last >= 0 && bucket_start(tnow, DUR[li + 1], j) > mt_last) std::fill(m_ring[li][j].begin(), m_ring[li][j].end(), 0);
				std::vector<uint8_t> &b = m_ring[li][bucket_idx(tnow, DUR[li + 1])];
				for (uint32_t s = 0; s < nsvc; ++s) gyo_hll_merge(b.data() + (size_t)s * m, closing.data() + (size_t)s * m, p);
			}
			for (uint32_t s = 0; s < nsvc; ++s) gyo_hll_merge(m_all.data() + (size_t)s * m, closing.data() + (size_t)s * m, p);
			m_last = closing;
			mt_last = tnow;
			// ---- the closed form's record
			wt.push_back(tnow);
			wf.push_back(closing);
		}
	}

	void check_guard()
	{
		bool ok = true;
		for (uint32_t f = 0; f < GYS_HLL_LVL_FILES && ok; ++f)
			for (size_t i = (size_t)nsvc * m; i < (size_t)S * m; ++i) ok = ok && arr(f)[i] == 0xEE;
		for (size_t i = (size_t)nsvc * m; i < (size_t)S * m; ++i) ok = ok && open[i] == 0xEE;
		CHECK(ok, "p %d nsvc %u: a slot above nsvc was written", p, nsvc);
	}

	std::vector<uint8_t> model_ring(int level, int64_t tq) const
	{
		std::vector<uint8_t> out((size_t)nsvc * m, 0);
		if (level == 0) {
			if (mt_last >= 0 && tq - mt_last < DUR[0]) out = m_last;
		} else if (level == 3) {
			out = m_all;
		} else {
			for (uint32_t j = 0; j < RING; ++j)
				if (mt_last >= 0 && !(bucket_start(tq, DUR[level], j) > mt_last))
					for (uint32_t s = 0; s < nsvc; ++s) gyo_hll_merge(out.data() + (size_t)s * m, m_ring[level - 1][j].data() + (size_t)s * m, p);
		}
		return out;
	}

	// (of every `step`-th service and the last one: the large cases check the closed form on a sample, the ring model on everything)
	std::vector<uint8_t> model_closed(int level, int64_t tq, uint32_t step) const
	{
		std::vector<uint8_t> out((size_t)nsvc * m, 0);
		for (size_t k = 0; k < wt.size(); ++k) {
			bool in;
			if (level == 0) in = k + 1 == wt.size() && tq - wt[k] < DUR[0];
			else if (level == 3) in = true;
			else {
				const int64_t w = DUR[level] / RING;
				in = wt[k] / w > tq / w - (int64_t)RING;
			}
			if (!in) continue;
			for (uint32_t s = 0; s < nsvc; s += step) gyo_hll_merge(out.data() + (size_t)s * m, wf[k].data() + (size_t)s * m, p);
			gyo_hll_merge(out.data() + (size_t)(nsvc - 1) * m, wf[k].data() + (size_t)(nsvc - 1) * m, p);
		}
		return out;
	}

	// the engine's query: the live mask on the host, then k_hll_level_view on slots [first, first + n)
	HllLevelViewP view_params(int level, int64_t tq_in, uint32_t first, uint32_t n, uint8_t *files, double *est)
	{
		const int64_t tq = std::max(tq_in, t_last);
		HllLevelViewP q{};
		uint32_t farr = GYS_HLL_LVL_LAST;
		if (level == 0) q.mask = t_last >= 0 && tq - t_last < DUR[0] ? 1u : 0u;
		else if (level == 3) {
			farr = GYS_HLL_LVL_ALL;
			q.mask = 1u;
		} else {
			farr = GYS_HLL_LVL_RING + (uint32_t)(level - 1) * RING;
			for (uint32_t j = 0; j < RING; ++j)
				if (t_last >= 0 && !(bucket_start(tq, DUR[level], j) > t_last)) q.mask |= 1u << j;
		}
		q.base = arr(farr);
		q.stride = (uint64_t)S * m;
		q.first = first;
		q.n = n;
		q.p = (uint32_t)p;
		q.files = files;
		q.est = est;
		return q;
	}

	struct Job {
		int level;
		int64_t tq;
		uint32_t first, n;
		bool files, est;
		std::vector<uint8_t> f;
		std::vector<double> e;
	};

	// every level at every query time of `tqs`; estimates at the first query time when with_est, and then also without files and on single
	// slots (gys_query_distinct_level's form).  The stand-in starts 256 host threads per workgroup, so all views of one check run one
	// after the other inside ONE launch.
	void check_queries(const std::vector<int64_t> &tqs, bool with_est, uint32_t grid, uint32_t closed_step)
	{
		const std::vector<uint8_t> state_before = lvl;
		std::vector<Job> jobs;
		for (size_t ti = 0; ti < tqs.size(); ++ti)
			for (int level = 0; level < 4; ++level) {
				jobs.push_back(Job{level, tqs[ti], 0u, nsvc, true, with_est && ti == 0, {}, {}});
				if (with_est && ti == 0) {
					jobs.push_back(Job{level, tqs[ti], 0u, nsvc, false, true, {}, {}});
					for (uint32_t s : {0u, nsvc / 2, nsvc - 1}) jobs.push_back(Job{level, tqs[ti], s, 1u, true, true, {}, {}});
				}
			}
		std::vector<HllLevelViewP> qs;
		for (Job &j : jobs) {
			j.f.assign((size_t)j.n * m + 16, 0xEE);
			j.e.assign(j.n + 1, -1.0);
			qs.push_back(view_params(j.level, j.tq, j.first, j.n, j.files ? j.f.data() : nullptr, j.est ? j.e.data() : nullptr));
		}
		const HllLevelViewP *qp = qs.data();
		const size_t nq = qs.size();
		kemu::launch(grid, GYS_HLL_NT, 0, [=] {
			for (size_t i = 0; i < nq; ++i) k_hll_level_view(qp[i]);
		});
		const Job *full = nullptr; // the whole-array job with files and estimates of the level at hand
		std::vector<uint8_t> a;
		for (const Job &j : jobs) {
			const int64_t tqc = std::max(j.tq, mt_last);
			for (int i = 0; i < 16; ++i) CHECK(j.f[(size_t)j.n * m + i] == 0xEE, "p %d: the view kernel wrote past its files", p);
			CHECK(j.e[j.n] == -1.0 && (j.est || j.e[0] == -1.0), "p %d: the view kernel wrote past its estimates, or estimates nobody asked for", p);
			if (j.n == nsvc && j.files) {
				a = model_ring(j.level, tqc);
				const std::vector<uint8_t> b = model_closed(j.level, tqc, closed_step);
				for (uint32_t s = 0; s < nsvc; s = s + closed_step < nsvc || s == nsvc - 1 ? s + closed_step : nsvc - 1)
					CHECK(memcmp(a.data() + (size_t)s * m, b.data() + (size_t)s * m, m) == 0, "p %d nsvc %u level %d tq %lld service %u: the ring model and the closed form differ", p, nsvc, j.level, (long long)tqc, s);
				CHECK(memcmp(j.f.data(), a.data(), a.size()) == 0, "p %d nsvc %u level %d tq %lld (close %zu): the kernel's files differ from the ring model", p, nsvc, j.level, (long long)tqc, wt.size());
				full = &j;
				if (!j.est) continue;
				for (uint32_t s = 0; s < nsvc; ++s) {
					const double want = gyo_hll_estimate(a.data() + (size_t)s * m, p);
					const double rel = want == 0.0 ? fabs(j.e[s]) : fabs(j.e[s] - want) / want;
					CHECK(rel <= 1e-12, "p %d level %d service %u: estimate %.17g, oracle %.17g", p, j.level, s, j.e[s], want);
					if (want == 0.0) CHECK(bits(j.e[s]) == 0, "p %d level %d service %u: the all-zero file gives %.17g", p, j.level, s, j.e[s]);
				}
			} else if (j.n == nsvc) {
				CHECK(full && memcmp(j.e.data(), full->e.data(), (size_t)nsvc * 8) == 0, "p %d level %d: estimates without files differ", p, j.level);
			} else {
				CHECK(full && bits(j.e[0]) == bits(full->e[j.first]), "p %d level %d slot %u alone: %.17g, in the scan %.17g", p, j.level, j.first, j.e[0], full->e[j.first]);
				CHECK(memcmp(j.f.data(), a.data() + (size_t)j.first * m, m) == 0, "p %d level %d slot %u alone: file differs", p, j.level, j.first);
			}
		}
		CHECK(lvl == state_before, "p %d nsvc %u: a view modified the state", p, nsvc);
	}
};

// the open window of one close: idle services, services with a few flows, busy ones
void fill_open(std::mt19937_64 &rng, Sim &s)
{
	for (uint32_t i = 0; i < s.nsvc; ++i) {
		uint8_t *f = s.open.data() + (size_t)i * s.m;
		const uint32_t kind = (uint32_t)(rng() % 8);
		const uint32_t nflows = kind < 2 ? 0u : (kind < 5 ? 1u + (uint32_t)(rng() % 4) : (kind < 7 ? (uint32_t)(rng() % (s.m / 2 + 2)) : (uint32_t)(rng() % (6 * s.m))));
		for (uint32_t k = 0; k < nflows; ++k) gyo_hll_add(f, s.p, rng());
	}
}

std::vector<int64_t> schedule(std::mt19937_64 &rng)
{
	std::vector<int64_t> st;
	auto rpt = [&](int64_t v, int n) { for (int i = 0; i < n; ++i) st.push_back(v); };
	rpt(5, 8);                 // crosses a 30-s boundary
	st.push_back(0);           // a repeated close time
	st.push_back(-7);          // backwards: clamped
	rpt(30, 12);               // wraps the 300-s ring
	for (int64_t v : {29, 31, 1, 301 /* the whole 300-s ring expires */, 5, 5, 299, 1, 43199, 43201, 5}) st.push_back(v);
	rpt(43200, 11);            // wraps the 5-day ring
	for (int64_t v : {5, 432001 /* more than 5 days */, 5, 5, 2 * 432000 + 7, 5}) st.push_back(v);
	const int64_t pick[] = {0, 1, 5, 29, 30, 31, 299, 300, 301, 43199, 43200, 43201};
	while (st.size() < 64) st.push_back(pick[rng() % 12]);
	return st;
}

void run(std::mt19937_64 &rng, int p, uint32_t nsvc)
{
	Sim s(p, nsvc);
	const bool big = nsvc > 100;
	const uint32_t cstep = big ? 37u : 1u;
	s.check_queries({1000000}, true, 1, cstep); // before the first close: everything empty
	int64_t t = 1700000000 + (int64_t)(rng() % 432000);
	const std::vector<int64_t> steps = schedule(rng);
	for (size_t k = 0; k < steps.size(); ++k) {
		fill_open(rng, s);
		const int64_t tcall = t + steps[k];
		s.close(tcall, 1 + (uint32_t)(k % 3));
		if (steps[k] > 0) t = tcall;
		// query times: at once, then inside and just outside the 5 s, around the 30-s / 300-s / 43 200-s / 5-day marks, and an earlier time (clamped)
		const int64_t all[] = {4, 5, 29, 31, 299, 301, 43201, 431999, 432001, -100};
		std::vector<int64_t> tqs = {t};
		if (big) {
			tqs.push_back(t + all[k % 10]);
			tqs.push_back(t + all[(k * 7 + 3) % 10]);
		} else {
			for (int64_t d : all) tqs.push_back(t + d);
		}
		s.check_queries(tqs, big || p >= 8 ? k % 16 == 3 : k % 4 == 3 || steps[k] > 31, // (estimates of wide files: 12 wave exchanges per piece, slow in the stand-in)
		                 1 + (uint32_t)(k % 2), cstep);
		if (fails) return;
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
	for (int p : {4, 6, 8, 10})
		for (uint32_t nsvc : {1u, 63u, 64u, 65u, 1000u})
			if (argc < 4 || (atoi(argv[2]) == p && (uint32_t)atoi(argv[3]) == nsvc)) run(rng, p, nsvc); // (argv[2], argv[3]: one case alone)
	if (fails) {
		printf("kemu hlllevels: %d failures\n", fails);
		return 1;
	}
	printf("kemu hlllevels ok\n");
	return 0;
}
