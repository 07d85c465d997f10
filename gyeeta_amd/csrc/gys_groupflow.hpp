// gys_groupflow.hpp -- the group flow map: the service dependency graph rolled up to hosts, clusters or labels -- which group calls which,
// with how many edges, entries, connections and bytes, and which groups lie within N hops of a set of groups (gys_group_edges / _dev,
// gys_group_deps / _dev).  The definition is frozen in include/gysketch.h ("Group flow map").  Needs gys_svcdeps.hpp (DepEdgeP, dep_join,
// and k_dep_seed / k_dep_level / k_dep_collect, which search the group pair array with the domain in place of nsvc) in front of it.
//
// The map is a GROUP BY (group(u), group(v)) over the edges of the join.  Its contention runs from "every edge hits one key" (two hosts)
// to "every edge its own key" (one label per service), so the keyed table is met in two steps:
//   k_gf_first_min / k_gf_first_flag
//                 first[j] for every member j of the task -> services list: "no EARLIER member of the same task has the same group".  An
//                 entry adds its figures once per DISTINCT (group(u), group(v)) of its edges: that is, at the members whose flag is set.
//                 A hash-minimum of the member position keyed (task index, group), then flag = (minimum == own position): linear in the
//                 bound members whatever a task's size, and the rows' walk looks at one byte per edge.  A task of one member (most are)
//                 needs no table entry.
//   k_gf_accum    k_dep_edges' walk of the row table, whole tiles of 256 entries.  A thread first joins the consecutive members of its
//                 entry that share a group in registers; then equal keys of the TILE are summed in an LDS table of GYS_GF_LDS_KEYS keys
//                 (64-bit key, edges, entries, connections, bytes sent / received, the latest window, the kind and flag bits), and one set
//                 of global atomics goes out per distinct key and tile.  A key that finds no room in the LDS table within
//                 GYS_GF_LDS_PROBES probes goes to the global table directly.
//   k_gf_rows     the occupied entries of the global table under a selection as gys_group_edge rows (k_actp_list's tile cursor), the
//                 counts of the group edges, and the (gu, gv) pairs with gu != gv for the search.
// The global table: open addressing, linear probing, the 64-bit key gu << 32 | gv claimed by compare-and-swap from all-ones
// (GYS_NO_GROUP never takes part, so the free marker cannot be a key); a set key never changes; every probe loop ends after `entries`
// steps and raises GFC_ERR, which the host turns into GYS_ERR_INTERNAL (the discipline of k_actp_find and k_cc_hook).  Every figure is
// an integer summed modulo 2^64, a maximum or an OR: no order of the atomics changes a bit of the result.
#pragma once

namespace gys {

#define GYS_GF_ACC 7u         // words of a key: GFA_*
#define GYS_GF_LDS_PROBES 16u // probes of the tile's LDS table before a key goes to the global table
#define GYS_GF_FIRST_YES 0xFFFFFFFEu
#define GYS_GF_FIRST_NO 0xFFFFFFFFu

static_assert((GYS_GF_LDS_KEYS & (GYS_GF_LDS_KEYS - 1u)) == 0u && GYS_GF_LDS_KEYS >= 256u, "the LDS table is a power of two, flushed by 256 threads");

// counter words of a group-flow call (unsigned long long each); GFC_GROUP_EDGES .. GFC_NPAIRS belong to k_gf_rows
enum { GFC_EDGES = 0, GFC_NOGROUP, GFC_ERR, GFC_GROUP_EDGES, GFC_SELF, GFC_NMATCH, GFC_NPAIRS, GFC_NUM = 8 };
enum { GFA_EDGES = 0, GFA_ROWS, GFA_CONNS, GFA_SENT, GFA_RCVD, GFA_WINDOW, GFA_BITS /* kinds | flags << 8 */ };

struct GfGroupP {
	uint32_t group_by, ndomain;   // GYS_GROUP_HOST / _CLUSTER / _LABEL; groups are < ndomain
	const uint32_t *svc_host;     // [nsvc]
	const uint32_t *host_cluster; // [hosts]
	const uint32_t *labels;       // [max_services], GYS_GROUP_LABEL only
	uint32_t nsvc;
};

// the group of a slot by the rule of the filtered roll-ups (rollsel_group_of); GYS_NO_GROUP for a free slot, a slot without a label and a
// group at or above the domain
__device__ __forceinline__ uint32_t gf_group(const GfGroupP &g, uint32_t slot)
{
	if (slot >= g.nsvc) return GYS_NO_GROUP;
	const uint32_t host = g.svc_host[slot];
	if (host == GYS_NOSLOT) return GYS_NO_GROUP;
	uint32_t v;
	switch (g.group_by) {
	case GYS_GROUP_HOST: v = host; break;
	case GYS_GROUP_CLUSTER: v = g.host_cluster[host]; break;
	default: v = g.labels[slot]; break;
	}
	return v < g.ndomain ? v : GYS_NO_GROUP;
}

// the entry of `key` in an open-addressing table of mask + 1 words (all-ones = free), claimed if it is not there; GYS_NOSLOT when
// mask + 1 probes found no place.  (a plain read first: a set word never changes, a stale "free" is put right by the compare-and-swap)
__device__ __forceinline__ uint32_t gf_claim(unsigned long long *keys, uint32_t mask, unsigned long long key)
{
	uint32_t h = get_uint64_hash(key) & mask;
#pragma unroll 1
	for (uint32_t probes = 0; probes <= mask; ++probes, h = (h + 1u) & mask) {
		unsigned long long k = ((const volatile unsigned long long *)keys)[h];
		if (k == GYS_EMPTY_KEY) {
			k = atomicCAS(&keys[h], (unsigned long long)GYS_EMPTY_KEY, key);
			if (k == GYS_EMPTY_KEY) k = key;
		}
		if (k == key) return h;
	}
	return GYS_NOSLOT;
}

// ---------------------------------------------------------------------------------------------------- first-of-group flags
struct GfFirstP {
	GfGroupP g;
	const uint32_t *task_off;  // [ntask + 1]
	const uint32_t *task_slot; // [nmem]
	uint32_t ntask, nmem;
	unsigned long long *hkey;  // [hmask + 1] all-ones; key = task index << 32 | group
	uint32_t *hmin;            // [hmask + 1] all-ones; the lowest member position of the key
	uint32_t hmask;
	uint32_t *first;           // [nmem] out: after k_gf_first_min the member's table entry or GYS_GF_FIRST_*, after k_gf_first_flag 1 / 0
	unsigned long long *ctr;   // [GFC_NUM]
};

__global__ __launch_bounds__(256) void k_gf_first_min(GfFirstP p)
{
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < p.nmem; j += gridDim.x * blockDim.x) {
		const uint32_t g = gf_group(p.g, p.task_slot[j]);
		if (g == GYS_NO_GROUP) {
			p.first[j] = GYS_GF_FIRST_NO;
			continue;
		}
		uint32_t lo = 0, hi = p.ntask; // the member's task: the last ti with task_off[ti] <= j
		while (lo + 1u < hi) {
			const uint32_t mid = lo + ((hi - lo) >> 1);
			if (p.task_off[mid] <= j) lo = mid;
			else hi = mid;
		}
		if (p.task_off[lo + 1u] - p.task_off[lo] == 1u) {
			p.first[j] = GYS_GF_FIRST_YES;
			continue;
		}
		const uint32_t h = gf_claim(p.hkey, p.hmask, ((unsigned long long)lo << 32) | g);
		if (h == GYS_NOSLOT) {
			atomicAdd(&p.ctr[GFC_ERR], 1ull);
			p.first[j] = GYS_GF_FIRST_NO;
			continue;
		}
		atomicMin(&p.hmin[h], j);
		p.first[j] = h;
	}
}

__global__ __launch_bounds__(256) void k_gf_first_flag(uint32_t *first, const uint32_t *hmin, uint32_t hmask, uint32_t nmem)
{
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < nmem; j += gridDim.x * blockDim.x) {
		const uint32_t f = first[j];
		first[j] = f == GYS_GF_FIRST_YES ? 1u : (f <= hmask && hmin[f] == j) ? 1u : 0u;
	}
}

// ---------------------------------------------------------------------------------------------------- the accumulation
struct GfAccP {
	DepEdgeP d;               // the join's inputs as for k_dep_edges (no selection; out / cap / ctr are not used)
	GfGroupP g;
	const uint32_t *first;    // [members] 1: the task's first member of its group
	unsigned long long *keys; // [mask + 1] all-ones
	unsigned long long *acc;  // [mask + 1][GYS_GF_ACC] zeroed
	uint32_t mask;
	unsigned long long *ctr;  // [GFC_NUM]: GFC_EDGES += the edges, GFC_NOGROUP += those with an end in no group
};

__device__ __forceinline__ void gf_global_add(const GfAccP &p, unsigned long long key, const unsigned long long *a)
{
	const uint32_t h = gf_claim(p.keys, p.mask, key);
	if (h == GYS_NOSLOT) {
		atomicAdd(&p.ctr[GFC_ERR], 1ull);
		return;
	}
	unsigned long long *d = p.acc + (uint64_t)h * GYS_GF_ACC;
#pragma unroll
	for (uint32_t f = 0; f <= GFA_RCVD; ++f)
		if (a[f]) atomicAdd(&d[f], a[f]);
	if (a[GFA_WINDOW]) atomicMax(&d[GFA_WINDOW], a[GFA_WINDOW]);
	if (a[GFA_BITS]) atomicOr(&d[GFA_BITS], a[GFA_BITS]);
}

__global__ __launch_bounds__(256) void k_gf_accum(GfAccP p)
{
	__shared__ unsigned long long s_key[GYS_GF_LDS_KEYS];
	__shared__ unsigned long long s_acc[GYS_GF_ACC][GYS_GF_LDS_KEYS];
	const uint32_t n = p.d.t.mask + 1u, lane = threadIdx.x & 63u;
	unsigned long long n_edges = 0, n_nogroup = 0;
	for (uint32_t s = threadIdx.x; s < GYS_GF_LDS_KEYS; s += blockDim.x) {
		s_key[s] = GYS_EMPTY_KEY;
#pragma unroll
		for (uint32_t f = 0; f < GYS_GF_ACC; ++f) s_acc[f][s] = 0ull;
	}
	__syncthreads();
	// a run's figures into the tile's table, or past it
	auto add = [&](unsigned long long key, const unsigned long long *a) {
		uint32_t h = get_uint64_hash(key) & (GYS_GF_LDS_KEYS - 1u);
#pragma unroll 1
		for (uint32_t probes = 0; probes < GYS_GF_LDS_PROBES; ++probes, h = (h + 1u) & (GYS_GF_LDS_KEYS - 1u)) {
			unsigned long long k = ((const volatile unsigned long long *)s_key)[h];
			if (k == GYS_EMPTY_KEY) {
				k = atomicCAS(&s_key[h], (unsigned long long)GYS_EMPTY_KEY, key);
				if (k == GYS_EMPTY_KEY) k = key;
			}
			if (k != key) continue;
#pragma unroll
			for (uint32_t f = 0; f <= GFA_RCVD; ++f)
				if (a[f]) atomicAdd(&s_acc[f][h], a[f]);
			if (a[GFA_WINDOW]) atomicMax(&s_acc[GFA_WINDOW][h], a[GFA_WINDOW]);
			if (a[GFA_BITS]) atomicOr(&s_acc[GFA_BITS][h], a[GFA_BITS]);
			return;
		}
		gf_global_add(p, key, a);
	};
	for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
		const uint32_t h = base + threadIdx.x;
		ActPairKey k;
		ActPairEnt v;
		if (h < n && actp_entry(p.d.t, h, p.d.epoch, k, v)) {
			uint32_t dst, t0, m;
			(void)dep_join(p.d, k, dst, t0, m);
			const uint32_t gv = m ? gf_group(p.g, dst) : GYS_NO_GROUP;
			n_edges += m;
			if (gv == GYS_NO_GROUP) {
				n_nogroup += m;
			} else {
				// (the members of a task ascend by slot: those of one host, cluster or application mostly lie side by side)
				uint32_t run_g = GYS_NO_GROUP, run_edges = 0, run_first = 0;
				for (uint32_t j = 0; j <= m; ++j) {
					const uint32_t gu = j < m ? gf_group(p.g, p.d.task_slot[t0 + j]) : GYS_NO_GROUP;
					if (gu != run_g || j == m) {
						if (run_edges) {
							unsigned long long a[GYS_GF_ACC] = {run_edges, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
							if (run_first) {
								a[GFA_ROWS] = 1ull;
								a[GFA_CONNS] = v.active_conns;
								a[GFA_SENT] = v.bytes_sent;
								a[GFA_RCVD] = v.bytes_received;
								a[GFA_WINDOW] = v.window;
								a[GFA_BITS] = (1ull << (k.kind & 1u)) | ((unsigned long long)(v.flags & 0xFFu) << 8);
							}
							add(((unsigned long long)run_g << 32) | gv, a);
						}
						run_g = gu;
						run_edges = run_first = 0;
					}
					if (j == m) break;
					if (gu == GYS_NO_GROUP) {
						n_nogroup++;
						continue;
					}
					run_edges++;
					run_first |= p.first[t0 + j];
				}
			}
		}
		__syncthreads();
		for (uint32_t s = threadIdx.x; s < GYS_GF_LDS_KEYS; s += blockDim.x) {
			const unsigned long long key = s_key[s];
			if (key == GYS_EMPTY_KEY) continue;
			unsigned long long a[GYS_GF_ACC];
#pragma unroll
			for (uint32_t f = 0; f < GYS_GF_ACC; ++f) {
				a[f] = s_acc[f][s];
				s_acc[f][s] = 0ull;
			}
			s_key[s] = GYS_EMPTY_KEY;
			gf_global_add(p, key, a);
		}
		__syncthreads();
	}
	// (the two counts stayed in registers: two atomics per wave and launch)
	n_edges = wave_incl_scan_u64(n_edges);
	n_nogroup = wave_incl_scan_u64(n_nogroup);
	if (lane == 63u) {
		if (n_edges) atomicAdd(&p.ctr[GFC_EDGES], n_edges);
		if (n_nogroup) atomicAdd(&p.ctr[GFC_NOGROUP], n_nogroup);
	}
}

// ---------------------------------------------------------------------------------------------------- rows and pairs
struct GfRowsP {
	const unsigned long long *keys, *acc;
	uint32_t mask;
	uint32_t sel_flags, src_group, dst_group; // GYS_GES_*
	gys_group_edge *out;                      // [cap]; may be nullptr with cap 0
	uint32_t cap;
	uint2 *pairs;                             // [pcap] (gu, gv) of every group edge with gu != gv, whatever the selection; nullptr: none
	uint32_t pcap;
	unsigned long long *ctr; // [GFC_NUM]: GFC_GROUP_EDGES, GFC_SELF += the map's; GFC_NMATCH += the selection's; GFC_NPAIRS += the pairs
};

__global__ __launch_bounds__(256) void k_gf_rows(GfRowsP p)
{
	__shared__ uint32_t s_wcnt[2][2][4];
	__shared__ unsigned long long s_base[2][2];
	const uint32_t n = p.mask + 1u, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t par = 0, n_ge = 0, n_self = 0;
	for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x, par ^= 1u) {
		const uint32_t h = base + threadIdx.x;
		const unsigned long long key = h < n ? p.keys[h] : GYS_EMPTY_KEY;
		const bool occ = key != GYS_EMPTY_KEY;
		const uint32_t gu = (uint32_t)(key >> 32), gv = (uint32_t)key;
		bool match = occ;
		if ((p.sel_flags & GYS_GES_BY_SRC) && gu != p.src_group) match = false;
		if ((p.sel_flags & GYS_GES_BY_DST) && gv != p.dst_group) match = false;
		if ((p.sel_flags & GYS_GES_NO_SELF) && gu == gv) match = false;
		const bool pr = occ && gu != gv && p.pairs != nullptr;
		const unsigned long long bm = __ballot(match), bp = __ballot(pr);
		n_ge += (uint32_t)__popcll(__ballot(occ));
		n_self += (uint32_t)__popcll(__ballot(occ && gu == gv));
		if (lane == 0u) {
			s_wcnt[par][0][wave] = (uint32_t)__popcll(bm);
			s_wcnt[par][1][wave] = (uint32_t)__popcll(bp);
		}
		__syncthreads();
		if (threadIdx.x < 2u) {
			const uint32_t *w = s_wcnt[par][threadIdx.x];
			const uint32_t tot = w[0] + w[1] + w[2] + w[3];
			s_base[par][threadIdx.x] = tot ? atomicAdd(&p.ctr[threadIdx.x ? GFC_NPAIRS : GFC_NMATCH], (unsigned long long)tot) : 0ull;
		}
		__syncthreads();
		const unsigned long long below = (1ull << lane) - 1ull;
		unsigned long long at = s_base[par][0] + (unsigned long long)__popcll(bm & below), pat = s_base[par][1] + (unsigned long long)__popcll(bp & below);
		for (uint32_t w = 0; w < wave; ++w) {
			at += s_wcnt[par][0][w];
			pat += s_wcnt[par][1][w];
		}
		if (pr && pat < p.pcap) p.pairs[pat] = make_uint2(gu, gv);
		if (!match || at >= p.cap) continue;
		const unsigned long long *a = p.acc + (uint64_t)h * GYS_GF_ACC;
		gys_group_edge r;
		r.src_group = gu;
		r.dst_group = gv;
		r.nedges = a[GFA_EDGES];
		r.nrows = a[GFA_ROWS];
		r.active_conns = a[GFA_CONNS];
		r.bytes_sent = a[GFA_SENT];
		r.bytes_received = a[GFA_RCVD];
		r.last_window = (uint32_t)a[GFA_WINDOW];
		r.kinds = (uint8_t)(a[GFA_BITS] & 3ull);
		r.flags = (uint8_t)(a[GFA_BITS] >> 8);
		r.pad[0] = r.pad[1] = 0;
		r.reserved = 0;
		p.out[at] = r;
	}
	if (lane == 0u) {
		if (n_ge) atomicAdd(&p.ctr[GFC_GROUP_EDGES], (unsigned long long)n_ge);
		if (n_self) atomicAdd(&p.ctr[GFC_SELF], (unsigned long long)n_self);
	}
}

} // namespace gys
