// gys_svcdeps.hpp -- the service dependency graph from the live active-connection rows: which service calls which, and what lies within N
// hops of a set of services (gys_set_listener_tasks, gys_svc_edges / _dev, gys_svcgraph_stats, gys_svc_deps / _dev).  The reference joins
// activeconn.cprocid to svcprocmap (json_db_svcprocmap_arr, common/gy_json_field_maps.h:1626-1633); a listener's process group arrives as
// NEW_LISTENER::ser_aggr_task_id_ (common/gy_comm_proto.h:1538).  The definition is frozen in include/gysketch.h ("Service dependency
// graph").  Needs gys_actpairs.hpp (the table and its liveness rule) in front of it.
//
// The join reads three things: the live entries (listener id L, client task group T, kind) of the row table, the glob_id -> slot table as
// it is NOW, and the task -> services list (gys_svcdeps_host.hpp builds it on the host: the bound task ids ascending, offsets, the member
// slots ascending inside a task).  The task lookup is a BINARY SEARCH over the sorted ids: the list is rebuilt whole whenever a binding or
// the registry changes, so there is nothing to insert into, and log2(tasks) dependent 8-byte loads sit beside the probe of the gid table.
//
//   k_dep_edges<FULL>  walks the table in tiles of 256 entries.  An entry whose listener is slot v and whose client group owns m services
//                      emits m edges u -> v, so the places in the output are taken by ONE returning atomic per tile on the SUM of the
//                      tile's m (k_actp_list's tile cursor with a wave scan in front of it), not one per row.  FULL = false writes
//                      (src, dst) pairs of 8 bytes for the traversal, FULL = true gys_svc_edge rows under a selection.  Edges beyond
//                      `cap` are counted and not written: the caller counts first (cap 0) and sizes its buffer from the count.
//   k_dep_seed         hops[slot] = 0 for a root, GYS_NOSLOT otherwise (the roots are a sorted slot list: a binary search per slot, so
//                      that no slot is written twice).
//   k_dep_level        one level of a level-synchronous search, edge-parallel over the pairs: an edge whose near end stands at `level` and
//                      whose far end is unreached claims the far end for level + 1 (compare-and-swap from GYS_NOSLOT) and raises the
//                      "changed" word.  A slot is claimed at most once, at the first level that reaches it: exact BFS distances.
//   k_dep_collect      the reached slots, compacted as (slot, hops) -- or only counted (out = nullptr).
#pragma once

namespace gys {

#define GYS_DEP_NOTASK 0xFFFFFFFFu

// counter words of the graph calls (unsigned long long each)
enum { DPC_EDGES = 0, DPC_LIVE, DPC_NOLISTENER, DPC_NOCLIENT, DPC_REACHED, DPC_CHANGED, DPC_NUM = 8 };

struct DepEdgeP {
	ActPairTbl t;
	uint32_t epoch;
	DevTable gid;               // glob_id -> service slot, as it is NOW
	const uint64_t *task_id;    // [ntask] the bound task ids, ascending
	const uint32_t *task_off;   // [ntask + 1]
	const uint32_t *task_slot;  // [task_off[ntask]] the services of a task, ascending slot
	uint32_t ntask, nsvc;
	const uint64_t *svc_gid;    // [nsvc] (FULL only)
	uint32_t sel_flags;         // GYS_SES_BY_SRC / _BY_DST, resolved by the host:
	uint32_t src_slot, dst_slot; // the selected ends' slots (GYS_NOSLOT: the id is not registered, nothing matches)
	uint64_t src_task;          // the task group src_slot is bound to (0: none, nothing matches)
	void *out;                  // [cap] uint2 pairs or gys_svc_edge rows; may be nullptr with cap 0
	uint32_t cap;
	unsigned long long *ctr;    // [DPC_NUM]: DPC_EDGES += the edges; with `stats` DPC_LIVE / _NOLISTENER / _NOCLIENT += the rows
	uint32_t stats;
};

// index of `id` in the ascending list, GYS_DEP_NOTASK if it is not there
__host__ __device__ __forceinline__ uint32_t dep_task_find(const uint64_t *ids, uint32_t n, uint64_t id)
{
	uint32_t lo = 0, hi = n;
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (ids[mid] < id) lo = mid + 1u;
		else hi = mid;
	}
	return (lo < n && ids[lo] == id) ? lo : GYS_DEP_NOTASK;
}

// the join of one live entry: dst = the listener's slot now (GYS_NOSLOT: not registered), the client group's services are
// task_slot[t0 .. t0 + m), m = the edges the entry gives (0 without a listener slot); returns "the client group owns no service"
// (k_dep_edges and k_cc_rows of gys_svccomp.hpp share it)
__device__ __forceinline__ bool dep_join(const DepEdgeP &p, const ActPairKey &k, uint32_t &dst, uint32_t &t0, uint32_t &m)
{
	dst = tbl_lookup(p.gid, k.lid);
	if (dst >= p.nsvc) dst = GYS_NOSLOT;
	t0 = m = 0u;
	const uint32_t ti = k.cid ? dep_task_find(p.task_id, p.ntask, k.cid) : GYS_DEP_NOTASK;
	if (ti != GYS_DEP_NOTASK) {
		t0 = p.task_off[ti];
		m = p.task_off[ti + 1u] - t0;
	}
	const bool nocli = m == 0u;
	if (dst == GYS_NOSLOT) m = 0u;
	return nocli;
}

template <bool FULL>
__global__ __launch_bounds__(256) void k_dep_edges(DepEdgeP p)
{
	__shared__ unsigned long long s_wsum[2][4];
	__shared__ unsigned long long s_base[2];
	const uint32_t n = p.t.mask + 1u, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t par = 0, n_live = 0, n_nol = 0, n_noc = 0;
	for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x, par ^= 1u) {
		const uint32_t h = base + threadIdx.x;
		ActPairKey k;
		ActPairEnt v;
		const bool live = h < n && actp_entry(p.t, h, p.epoch, k, v);
		uint32_t dst = GYS_NOSLOT, t0 = 0, m = 0;
		bool nocli = false, one = false;
		if (live) {
			nocli = dep_join(p, k, dst, t0, m);
			if (m && (p.sel_flags & GYS_SES_BY_DST) && dst != p.dst_slot) m = 0u;
			if (m && (p.sel_flags & GYS_SES_BY_SRC)) { // (src_slot is bound to src_task: it is one of the m callers exactly when the row's client is that task)
				one = true;
				m = (p.src_slot != GYS_NOSLOT && p.src_task != 0ull && k.cid == p.src_task) ? 1u : 0u;
			}
		}
		if (p.stats) { // (uniform; the wave's counts stay in registers until the end: three atomics per wave and launch, not per tile)
			n_live += (uint32_t)__popcll(__ballot(live));
			n_nol += (uint32_t)__popcll(__ballot(live && dst == GYS_NOSLOT));
			n_noc += (uint32_t)__popcll(__ballot(live && nocli));
		}
		// (a task owns at most nsvc services: 64 x nsvc stays below 2^32 for every max_services gys_create takes)
		const uint32_t incl = wave_incl_scan_u32(m);
		if (lane == 63u) s_wsum[par][wave] = incl;
		__syncthreads();
		if (threadIdx.x == 0u) {
			const unsigned long long tot = s_wsum[par][0] + s_wsum[par][1] + s_wsum[par][2] + s_wsum[par][3];
			s_base[par] = tot ? atomicAdd(&p.ctr[DPC_EDGES], tot) : 0ull;
		}
		__syncthreads();
		unsigned long long at = s_base[par] + (unsigned long long)(incl - m);
		for (uint32_t w = 0; w < wave; ++w) at += s_wsum[par][w];
		for (uint32_t j = 0; j < m && at + j < (unsigned long long)p.cap; ++j) {
			const uint32_t src = one ? p.src_slot : p.task_slot[t0 + j];
			if (!FULL) {
				((uint2 *)p.out)[at + j] = make_uint2(src, dst);
			} else {
				gys_svc_edge r;
				r.src_slot = src;
				r.dst_slot = dst;
				r.src_glob_id = p.svc_gid[src];
				r.dst_glob_id = k.lid;
				r.cli_aggr_task_id = k.cid;
				r.bytes_sent = v.bytes_sent;
				r.bytes_received = v.bytes_received;
				r.active_conns = v.active_conns;
				r.nrows = v.nrows;
				r.window = v.window;
				r.kind = (uint8_t)k.kind;
				r.flags = (uint8_t)v.flags;
				r.pad[0] = r.pad[1] = 0;
				((gys_svc_edge *)p.out)[at + j] = r;
			}
		}
	}
	if (p.stats && lane == 0u) {
		if (n_live) atomicAdd(&p.ctr[DPC_LIVE], (unsigned long long)n_live);
		if (n_nol) atomicAdd(&p.ctr[DPC_NOLISTENER], (unsigned long long)n_nol);
		if (n_noc) atomicAdd(&p.ctr[DPC_NOCLIENT], (unsigned long long)n_noc);
	}
}

__global__ __launch_bounds__(256) void k_dep_seed(uint32_t *hops, uint32_t nsvc, const uint32_t *roots /* ascending, distinct */, uint32_t nroots)
{
	for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nsvc; s += gridDim.x * blockDim.x) {
		uint32_t lo = 0, hi = nroots;
		while (lo < hi) {
			const uint32_t mid = lo + ((hi - lo) >> 1);
			if (roots[mid] < s) lo = mid + 1u;
			else hi = mid;
		}
		hops[s] = (lo < nroots && roots[lo] == s) ? 0u : GYS_NOSLOT;
	}
}

// (the plain reads of hops[] race with the claims of this launch, which only ever write level + 1 over GYS_NOSLOT: a stale read is "unreached"
// or "not at `level`", and the compare-and-swap settles the first; nsvc bounds every index, whatever the pair array holds)
__global__ __launch_bounds__(256) void k_dep_level(const uint2 *pairs, uint64_t nedges, uint32_t *hops, uint32_t nsvc, uint32_t level, uint32_t dir, unsigned long long *changed)
{
	for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nedges; e += (uint64_t)gridDim.x * blockDim.x) {
		const uint2 pr = pairs[e];
		if (pr.x >= nsvc || pr.y >= nsvc) continue;
		if ((dir & GYS_DEP_CALLEES) && hops[pr.x] == level && hops[pr.y] == GYS_NOSLOT && atomicCAS(&hops[pr.y], GYS_NOSLOT, level + 1u) == GYS_NOSLOT) *changed = 1ull;
		if ((dir & GYS_DEP_CALLERS) && hops[pr.y] == level && hops[pr.x] == GYS_NOSLOT && atomicCAS(&hops[pr.x], GYS_NOSLOT, level + 1u) == GYS_NOSLOT) *changed = 1ull;
	}
}

// the reached slots as (slot, hops) into out[0 .. cap) in any order (k_actp_list's tile cursor); *count += their number
__global__ __launch_bounds__(256) void k_dep_collect(const uint32_t *hops, uint32_t nsvc, uint2 *out, uint32_t cap, unsigned long long *count)
{
	__shared__ uint32_t s_wcnt[2][4];
	__shared__ unsigned long long s_base[2];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t par = 0;
	for (uint32_t base = blockIdx.x * blockDim.x; base < nsvc; base += gridDim.x * blockDim.x, par ^= 1u) {
		const uint32_t s = base + threadIdx.x;
		const uint32_t hp = s < nsvc ? hops[s] : GYS_NOSLOT;
		const bool hit = hp != GYS_NOSLOT;
		const unsigned long long b = __ballot(hit);
		if (lane == 0u) s_wcnt[par][wave] = (uint32_t)__popcll(b);
		__syncthreads();
		if (threadIdx.x == 0u) {
			const uint32_t tot = s_wcnt[par][0] + s_wcnt[par][1] + s_wcnt[par][2] + s_wcnt[par][3];
			s_base[par] = tot ? atomicAdd(count, (unsigned long long)tot) : 0ull;
		}
		__syncthreads();
		unsigned long long at = s_base[par] + (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
		for (uint32_t w = 0; w < wave; ++w) at += s_wcnt[par][w];
		if (hit && at < cap) out[at] = make_uint2(s, hp);
	}
}

} // namespace gys
