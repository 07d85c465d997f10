// gys_svccomp.hpp -- service components: the weakly connected components of the service dependency graph, which services form one
// application (gys_svc_components / _dev, gys_label_service_components).  The reference merges service groups that share a related
// listener into one cluster id with a serial two-pass hash walk (SHCONN_HANDLER::coalesce_svc_mesh_locked,
// server/gy_shconnhdlr.cc:4827-4912).  The definition is frozen in include/gysketch.h ("Service components").  Needs gys_svcdeps.hpp
// (the pair array of k_dep_edges<false>, DepEdgeP, dep_join) in front of it.
//
// The partition is a lock-free union-find over the pair array whose parent never points upwards -- a FIXED number of launches whatever
// the graph's diameter (a level-synchronous search, k_dep_level, needs one per hop):
//   k_cc_init     parent[s] = s for a registered slot, GYS_NOSLOT for a free one.
//   k_cc_hook     edge-parallel: the roots of an edge's two ends are joined by a compare-and-swap that hangs the HIGHER root below the lower.
//   k_cc_flatten  comp[s] = the root of s.  A launch of its own: nothing hooks while it runs.
// and the figures:
//   k_cc_sizes    size[comp[s]] += 1 (one root per tile of 256 slots is summed in LDS first: a component may hold most services).
//   k_cc_roots    counts the components, those with two members or more and those with >= min_services members; compacts the latter as
//                 (root, size) with k_dep_collect's tile cursor and writes index[root] = the root's place in that list.
//   k_cc_rows     k_dep_edges' walk of the row table: an entry that gives m > 0 edges adds (1, m, active_conns, bytes_sent,
//                 bytes_received) to the listed component of its listener slot -- once per ENTRY, not per edge (summed per tile as the sizes).
//   k_cc_labels   labels[s] = comp[s] where the component has >= min_services members, GYS_NO_GROUP elsewhere.  The only kernel in here
//                 that writes engine state.
#pragma once

namespace gys {

// counter words of the component calls (unsigned long long each)
enum { CCC_NCOMP = 0, CCC_NLINKED, CCC_NMATCH, CCC_CURSOR, CCC_CAPPED, CCC_NUM = 8 };
#define GYS_CC_ACC 5u // words a listed component accumulates: entries, edges, active_conns, bytes_sent, bytes_received

__global__ __launch_bounds__(256) void k_cc_init(uint32_t *parent, const uint32_t *svc_host, uint32_t nsvc)
{
	for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nsvc; s += gridDim.x * blockDim.x) parent[s] = svc_host[s] != GYS_NOSLOT ? s : GYS_NOSLOT;
}

// The root of x as this thread can see it, halving the path on the way: parent[x] = min(parent[x], grandparent).  GYS_NOSLOT for a free
// slot.  The reads go through a volatile pointer: every step and every retry loads anew.  A read may still be stale; parents only ever
// decrease and stay inside the set, so a stale value is a lower-or-equal member of x's set and the minimum is always safe -- the walk
// merely ends at a slot that was a root a moment ago, and the caller's compare-and-swap settles whether it still is.  Every step
// moves to a strictly lower slot: at most nsvc steps.  The cap on top of that argument must never trigger (*capped is raised if it does).
__device__ __forceinline__ uint32_t cc_find(uint32_t *parent, uint32_t x, uint32_t nsvc, unsigned long long *capped)
{
	const volatile uint32_t *vp = parent;
#pragma unroll 1
	for (uint32_t steps = 0; steps < nsvc; ++steps) {
		const uint32_t p = vp[x];
		if (p == x) return x;
		if (p > x) return GYS_NOSLOT; // (a free slot: no pair the join emits names one)
		const uint32_t g = vp[p];
		if (g > p) return GYS_NOSLOT;
		if (g != p) atomicMin(&parent[x], g);
		x = g;
	}
	atomicAdd(capped, 1ull);
	return x;
}

// INVARIANTS.  (1) parent[x] <= x always: init writes x, a hook writes lo < hi over hi, a halving writes a minimum.  (2) A non-root never
// becomes a root again: the only store that can write x into parent[x] is init.  (3) Only a slot that IS a root at that moment is hooked
// (the compare-and-swap expects parent[hi] == hi), and it is hung below a lower slot of ANOTHER set (were lo in hi's set, its walk up
// would end at the root hi > lo, against (1)): the trees stay trees, and two sets are joined exactly when an edge joins them.  (4) The
// lowest slot of a component has no lower slot to be hung below: it is never hooked and is the final root, whatever order the hooks
// took -- comp[] is a function of the graph alone.
// An edge is done when both ends show one root, or when its hook went in.  A failed compare-and-swap means parent[hi] went down in the
// meantime: the edge goes on from the value it returned (hi's new parent, in hi's set) and lo.  At most nsvc hooks ever succeed and
// every failure follows another thread's progress: the loop ends; the cap is there so that a wrong loop ends, too.
// (nsvc bounds every index, whatever the pair array holds, as in k_dep_level)
__global__ __launch_bounds__(256) void k_cc_hook(const uint2 *pairs, uint64_t nedges, uint32_t *parent, uint32_t nsvc, unsigned long long *capped)
{
	for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nedges; e += (uint64_t)gridDim.x * blockDim.x) {
		const uint2 pr = pairs[e];
		if (pr.x >= nsvc || pr.y >= nsvc || pr.x == pr.y) continue;
		uint32_t u = pr.x, v = pr.y, tries = 0;
#pragma unroll 1
		for (;;) {
			const uint32_t ru = cc_find(parent, u, nsvc, capped), rv = cc_find(parent, v, nsvc, capped);
			if (ru == rv || ru == GYS_NOSLOT || rv == GYS_NOSLOT) break;
			const uint32_t hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
			const uint32_t was = atomicCAS(&parent[hi], hi, lo);
			if (was == hi) break;
			if (++tries >= nsvc) {
				atomicAdd(capped, 1ull);
				break;
			}
			u = was;
			v = lo;
		}
	}
}

__global__ __launch_bounds__(256) void k_cc_flatten(uint32_t *parent, uint32_t *comp, uint32_t nsvc, unsigned long long *capped)
{
	for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nsvc; s += gridDim.x * blockDim.x) comp[s] = cc_find(parent, s, nsvc, capped);
}

// size[] was cleared before.  ONE application may hold most services: 10^5 slots of one component were 10^5 atomics on one word, 1.1 ms
// for a kernel that otherwise takes microseconds.  So a tile of 256 slots sums ONE root in LDS -- the first that claims the tile's key
// word -- and adds it with one global atomic; slots of any other root add directly.  Thread 0 alone clears and flushes the two words, on
// either side of the tile's two barriers: one set of words is enough.
__global__ __launch_bounds__(256) void k_cc_sizes(const uint32_t *comp, uint32_t *size, uint32_t nsvc)
{
	__shared__ uint32_t s_key, s_cnt;
	for (uint32_t base = blockIdx.x * blockDim.x; base < nsvc; base += gridDim.x * blockDim.x) {
		if (threadIdx.x == 0u) {
			s_key = GYS_NOSLOT;
			s_cnt = 0u;
		}
		__syncthreads();
		const uint32_t s = base + threadIdx.x;
		const uint32_t r = s < nsvc ? comp[s] : GYS_NOSLOT;
		if (r < nsvc) {
			uint32_t key = atomicCAS(&s_key, GYS_NOSLOT, r);
			if (key == GYS_NOSLOT) key = r;
			if (key == r) atomicAdd(&s_cnt, 1u);
			else atomicAdd(&size[r], 1u);
		}
		__syncthreads();
		if (threadIdx.x == 0u && s_cnt) atomicAdd(&size[s_key], s_cnt);
	}
}

struct CcRootsP {
	const uint32_t *comp, *size; // [nsvc]
	uint32_t nsvc, min_services;
	uint2 *list;                 // [nsvc] (root, size) of the components with size >= min_services, any order; nullptr: only the counts
	uint32_t *index;             // [nsvc] a listed root's place in `list`, GYS_NOSLOT elsewhere (with `list`)
	unsigned long long *ctr;     // [CCC_NUM]
};

// (the three counts stay in registers until the end -- a ballot per tile, three atomics per wave and launch: k_dep_edges' row counters)
__global__ __launch_bounds__(256) void k_cc_roots(CcRootsP p)
{
	__shared__ uint32_t s_wcnt[2][4];
	__shared__ unsigned long long s_base[2];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t par = 0, n_comp = 0, n_linked = 0, n_match = 0;
	for (uint32_t base = blockIdx.x * blockDim.x; base < p.nsvc; base += gridDim.x * blockDim.x, par ^= 1u) {
		const uint32_t s = base + threadIdx.x;
		const bool root = s < p.nsvc && p.comp[s] == s;
		const uint32_t sz = root ? p.size[s] : 0u;
		const bool hit = root && sz >= p.min_services;
		const unsigned long long b = __ballot(hit);
		n_comp += (uint32_t)__popcll(__ballot(root));
		n_linked += (uint32_t)__popcll(__ballot(root && sz >= 2u));
		n_match += (uint32_t)__popcll(b);
		if (!p.list) continue; // (uniform)
		if (lane == 0u) s_wcnt[par][wave] = (uint32_t)__popcll(b);
		__syncthreads();
		if (threadIdx.x == 0u) {
			const uint32_t tot = s_wcnt[par][0] + s_wcnt[par][1] + s_wcnt[par][2] + s_wcnt[par][3];
			s_base[par] = tot ? atomicAdd(&p.ctr[CCC_CURSOR], (unsigned long long)tot) : 0ull;
		}
		__syncthreads();
		unsigned long long at = s_base[par] + (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
		for (uint32_t w = 0; w < wave; ++w) at += s_wcnt[par][w];
		// (a root is its own slot: the roots are at most nsvc, so is `at`)
		if (hit && at < p.nsvc) p.list[at] = make_uint2(s, sz);
		if (s < p.nsvc) p.index[s] = hit && at < p.nsvc ? (uint32_t)at : GYS_NOSLOT;
	}
	if (lane == 0u) {
		if (n_comp) atomicAdd(&p.ctr[CCC_NCOMP], (unsigned long long)n_comp);
		if (n_linked) atomicAdd(&p.ctr[CCC_NLINKED], (unsigned long long)n_linked);
		if (n_match) atomicAdd(&p.ctr[CCC_NMATCH], (unsigned long long)n_match);
	}
}

// p: the join's inputs as for k_dep_edges (no selection; out / cap / ctr are not used); acc[nlisted][GYS_CC_ACC] was cleared before.
// The sums of a tile's entries go the way of k_cc_sizes -- the component that claims the tile's key word is summed in LDS and added with
// five global atomics per tile, the others add directly: the 10^5 entries of one path were 5 x 10^5 atomics on five words, 6.0 ms.
__global__ __launch_bounds__(256) void k_cc_rows(DepEdgeP p, const uint32_t *comp, const uint32_t *index, uint32_t nlisted, unsigned long long *acc)
{
	__shared__ uint32_t s_key;
	__shared__ unsigned long long s_sum[GYS_CC_ACC];
	const uint32_t n = p.t.mask + 1u;
	for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
		if (threadIdx.x == 0u) {
			s_key = GYS_NOSLOT;
			for (uint32_t f = 0; f < GYS_CC_ACC; ++f) s_sum[f] = 0ull;
		}
		__syncthreads();
		const uint32_t h = base + threadIdx.x;
		ActPairKey k;
		ActPairEnt v;
		uint32_t ci = GYS_NOSLOT, m = 0;
		if (h < n && actp_entry(p.t, h, p.epoch, k, v)) {
			uint32_t dst, t0;
			(void)dep_join(p, k, dst, t0, m);
			if (m) {
				const uint32_t r = comp[dst];
				if (r < p.nsvc) ci = index[r];
			}
		}
		if (ci < nlisted) {
			uint32_t key = atomicCAS(&s_key, GYS_NOSLOT, ci);
			if (key == GYS_NOSLOT) key = ci;
			if (key == ci) {
				atomicAdd(&s_sum[0], 1ull);
				atomicAdd(&s_sum[1], (unsigned long long)m);
				atomicAdd(&s_sum[2], (unsigned long long)v.active_conns);
				atomicAdd(&s_sum[3], v.bytes_sent);
				atomicAdd(&s_sum[4], v.bytes_received);
			} else {
				unsigned long long *a = acc + (uint64_t)ci * GYS_CC_ACC;
				atomicAdd(&a[0], 1ull);
				atomicAdd(&a[1], (unsigned long long)m);
				atomicAdd(&a[2], (unsigned long long)v.active_conns);
				atomicAdd(&a[3], v.bytes_sent);
				atomicAdd(&a[4], v.bytes_received);
			}
		}
		__syncthreads();
		if (threadIdx.x == 0u && s_key != GYS_NOSLOT) {
			unsigned long long *a = acc + (uint64_t)s_key * GYS_CC_ACC;
			for (uint32_t f = 0; f < GYS_CC_ACC; ++f) atomicAdd(&a[f], s_sum[f]);
		}
	}
}

__global__ __launch_bounds__(256) void k_cc_labels(const uint32_t *comp, const uint32_t *size, uint32_t nsvc, uint32_t min_services, uint32_t *labels)
{
	for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nsvc; s += gridDim.x * blockDim.x) {
		const uint32_t r = comp[s];
		labels[s] = (r < nsvc && size[r] >= min_services) ? r : GYS_NO_GROUP;
	}
}

} // namespace gys
