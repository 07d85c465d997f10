// gys_rollsel.hpp -- the device path from "the services a filter selects" to the member lists and chunks the roll-up kernels take
// (gys_rollup_filtered_dev): the WHERE and the GROUP BY of the aggregated percentile the reference leaves to Postgres,
// public.tdigest_percentile(col, 100, p) over a set of listeners' rows (common/gy_query_common.cc:1818-1855).  The arithmetic is that of
// gys_rollup.hpp (union by value bin) and gys_hllroll.hpp (byte-wise maximum): both are independent of the order of the members, so the
// members of a group may be placed with atomics and the results stay bit-reproducible.
//   k_rollsel_count    grid-stride over the candidate items in tiles of 1024 (the shape of k_svc_filter: four items per thread, a wave's lanes
//                      on consecutive items): svc_load_current / svc_load_any + svc_filter_match, the item's group (nothing / host / cluster /
//                      the caller's label) into item_group[item] -- 4 bytes instead of the 96-byte record for the second pass -- and the
//                      members of every group counted in counts[group].  A domain of up to GYS_RS_LDS_GROUPS groups is counted in LDS, one
//                      global atomic per group a workgroup has met; a larger one (labels, more hosts) goes to the global counters after
//                      the wave has joined its equal groups (rollsel_wave_join: ballots and lane reads, no LDS round trips).
//   k_rollsel_scan     the exclusive scan over the group domain in three launches whatever its size (tiles of 4096 groups: the tiles' totals, the
//                      scan of the totals by one workgroup, the tiles again): for every group with members its row index, the offset of its
//                      members and of its chunks; rows {group, nmembers} and their offsets for the first maxrows rows; counts[group] becomes
//                      the group's member cursor; the totals the host reads back.
//   k_rollsel_scatter  item_group again: every member's slot to members[cursor of its group ++] (LDS ranks + one global atomic per group and
//                      tile for a domain of up to GYS_RS_SCATTER_LDS_GROUPS groups, wave-joined global atomics for a larger one).  Order inside a group: arbitrary.
//   k_rollsel_chunks   a wave per row: its RollupChunk{row, m0, m1} list (chunks of `per` members) and the row's {row, first chunk, end chunk}
//                      for the second pass of k_hll_union.
//   k_rollsel_labels   labels[slot[i]] = group[i] (gys_set_service_groups).
#pragma once

namespace gys {

#define GYS_RS_THREADS 256u
#define GYS_RS_PER_THREAD 4u
#define GYS_RS_TILE (GYS_RS_THREADS * GYS_RS_PER_THREAD)
#define GYS_RS_LDS_GROUPS 4096u // group domains up to this size are counted in a workgroup's LDS (16 KB: four workgroups per CU keep theirs)
#define GYS_RS_SCATTER_LDS_GROUPS 1024u // ... and ranked in LDS by the scatter, which clears and walks its table once per tile of 1024 items (4 KB: a clear, a walk and
                                     // at most one global atomic per item); above it the wave-joined atomics cost less (a host's slots are neighbours: one or two groups per wave)
#define GYS_RS_ROUNDS 4u        // distinct groups a wave joins before the lanes left over add on their own
#define GYS_RS_SCAN_PER_THREAD 16u
#define GYS_RS_SCAN_TILE (GYS_RS_THREADS * GYS_RS_SCAN_PER_THREAD)

// device totals (u32 words) of a selection
enum { RS_TOT_ROWS = 0, RS_TOT_CHUNKS_ALL, RS_TOT_MEMBERS_ALL, RS_TOT_CHUNKS, RS_TOT_MEMBERS, RS_TOT_GCUT, RS_TOT_WORDS = 8 };

struct RollSelP {
	// the filter: the members q_fill_filter fills and svc_load_current / svc_filter_match read (as SvcFilterP)
	const uint8_t *svc_state;
	const uint32_t *svc_host;
	const uint64_t *svc_gid;
	uint32_t nsvc, epoch;
	const uint32_t *host_mask;
	const uint32_t *slot_list;
	uint32_t nitems;
	const int32_t *set_values;
	uint32_t nterms, ngroups;
	SvcTerm terms[GYS_SVCQ_MAX_TERMS];
	uint8_t group_oper[GYS_SVCQ_MAX_GROUPS];
	uint32_t top_oper;
	// the grouping
	uint32_t any_state;           // GYS_RF_ANY_STATE: the age of the state record does not matter
	uint32_t group_by;            // GYS_GROUP_*
	const uint32_t *host_cluster; // [hosts]
	const uint32_t *labels;       // [max_services], GYS_GROUP_LABEL only
	uint32_t ndomain;             // groups are < ndomain (a group outside: no member)
	uint32_t ntiles;              // ceil(nitems / GYS_RS_TILE)
	uint32_t *item_group;         // [nitems] out (count), in (scatter)
	uint32_t *counts;             // [ndomain] zeroed; members per group; after the scan: the group's cursor into members
	const uint32_t *tot;          // scatter: [RS_TOT_GCUT] = the first group that has no row (beyond maxrows)
	uint32_t *members;            // scatter: out
};

// the kept record of `slot` whatever its age (GYS_RF_ANY_STATE): all zero if the service never reported; its host is the one it was
// registered under.  false: the host is not part of the query, or the slot is free.
template <typename P>
__device__ __forceinline__ bool svc_load_any(const P &p, uint32_t slot, uint32_t *w, uint32_t *host_out)
{
	const uint4 *q = (const uint4 *)(p.svc_state + (size_t)slot * 96);
#pragma unroll
	for (int k = 0; k < 6; ++k) {
		const uint4 v = q[k];
		w[4 * k] = v.x;
		w[4 * k + 1] = v.y;
		w[4 * k + 2] = v.z;
		w[4 * k + 3] = v.w;
	}
	const uint32_t host = p.svc_host[slot];
	*host_out = host;
	if (host == GYS_NOSLOT) return false; // a free slot (gys_delete_listeners): no host, no group
	if (p.host_mask && !((p.host_mask[host >> 5] >> (host & 31u)) & 1u)) return false;
	return true;
}

// the value of `lane` (the same in every lane of the wave) in every lane
__device__ __forceinline__ uint32_t wave_read_lane_u32(uint32_t v, uint32_t lane)
{
#ifdef __HIP_DEVICE_COMPILE__
	return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
#else
	return (uint32_t)__shfl((int)v, (int)lane, 64);
#endif
}

// The lanes of a wave that hold the same group join: up to GYS_RS_ROUNDS times the first lane still open names its group, a ballot finds the
// lanes that hold it, and `leader_add(group, lanes)` -- called in the first of them only -- returns the base the others count from (or
// nothing that matters).  Returns in `base` / `rank` the lane's place: base + rank of a joined lane; a lane left over after the rounds has
// joined == false and acts on its own.  Every lane of the wave must call this (g == GYS_NO_GROUP: nothing to add).
template <typename F>
__device__ __forceinline__ bool rollsel_wave_join(uint32_t g, uint32_t lane, uint32_t &base, uint32_t &rank, F leader_add)
{
	bool joined = false;
	unsigned long long open = __ballot(g != GYS_NO_GROUP);
	base = 0;
	rank = 0;
#pragma unroll 1
	for (uint32_t r = 0; r < GYS_RS_ROUNDS && open; ++r) {
		const uint32_t first = (uint32_t)__ffsll((long long)open) - 1u;
		const uint32_t gl = wave_read_lane_u32(g, first);
		const unsigned long long same = __ballot(g == gl && g != GYS_NO_GROUP);
		uint32_t b = 0;
		if (lane == first) b = leader_add(gl, (uint32_t)__popcll(same));
		b = wave_read_lane_u32(b, first);
		if ((same >> lane) & 1ull) {
			joined = true;
			base = b;
			rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
		}
		open &= ~same;
	}
	return joined || g == GYS_NO_GROUP;
}

__device__ __forceinline__ uint32_t rollsel_group_of(const RollSelP &p, uint32_t slot, uint32_t host)
{
	uint32_t g;
	switch (p.group_by) {
	case GYS_GROUP_NONE: g = 0u; break;
	case GYS_GROUP_HOST: g = host; break;
	case GYS_GROUP_CLUSTER: g = p.host_cluster[host]; break;
	default: g = p.labels[slot]; break;
	}
	return g < p.ndomain ? g : GYS_NO_GROUP;
}

__global__ __launch_bounds__(GYS_RS_THREADS) void k_rollsel_count(RollSelP p)
{
	__shared__ uint32_t s_cnt[GYS_RS_LDS_GROUPS];
	const bool lds = p.ndomain <= GYS_RS_LDS_GROUPS;
	const uint32_t lane = threadIdx.x & 63u;
	if (lds) {
		for (uint32_t k = threadIdx.x; k < p.ndomain; k += GYS_RS_THREADS) s_cnt[k] = 0;
		__syncthreads();
	}
	for (uint32_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) { // (the same trips in every thread of the workgroup)
		const uint32_t first = tile * GYS_RS_TILE;
		uint32_t grp[GYS_RS_PER_THREAD];
#pragma unroll
		for (uint32_t k = 0; k < GYS_RS_PER_THREAD; ++k) {
			const uint32_t item = first + k * GYS_RS_THREADS + threadIdx.x;
			grp[k] = GYS_NO_GROUP;
			if (item < p.nitems) {
				const uint32_t slot = p.slot_list ? p.slot_list[item] : item;
				uint32_t w[24], host;
				const bool cand = p.any_state ? svc_load_any(p, slot, w, &host) : svc_load_current(p, slot, w, &host);
				if (cand && svc_filter_match(p, w)) grp[k] = rollsel_group_of(p, slot, host);
				p.item_group[item] = grp[k];
			}
		}
#pragma unroll
		for (uint32_t k = 0; k < GYS_RS_PER_THREAD; ++k) {
			const uint32_t g = grp[k];
			if (lds) {
				if (g != GYS_NO_GROUP) atomicAdd(&s_cnt[g], 1u);
			} else {
				uint32_t base, rank;
				const bool done = rollsel_wave_join(g, lane, base, rank, [&](uint32_t gl, uint32_t n) {
					atomicAdd(&p.counts[gl], n);
					return 0u;
				});
				if (!done) atomicAdd(&p.counts[g], 1u);
			}
		}
	}
	if (lds) {
		__syncthreads();
		for (uint32_t k = threadIdx.x; k < p.ndomain; k += GYS_RS_THREADS) {
			const uint32_t n = s_cnt[k];
			if (n) atomicAdd(&p.counts[k], n);
		}
	}
}

struct RollScanP {
	uint32_t *counts;  // [ndomain] in: members per group; phase 2 out: the group's cursor (offset of its members)
	uint32_t ndomain, ntiles; // ntiles = ceil(ndomain / GYS_RS_SCAN_TILE)
	uint32_t per;      // members per chunk
	uint32_t maxrows;
	uint32_t *tiles;   // [ntiles][3] {rows, members, chunks}: phase 0 the tile's totals, phase 1 their exclusive scan
	uint32_t *tot;     // [RS_TOT_WORDS]
	gys_rollup_row *rows; // [min(maxrows, ndomain)]
	uint2 *rowoff;     // ... {first member, first chunk}
	uint32_t phase;
};

// exclusive sums of (a, b, c) over the workgroup's threads in thread order; the workgroup's totals in ta, tb, tc
// (s_w: the workgroup's LDS words, one triple per wave)
__device__ __forceinline__ void rollsel_block_scan3(uint32_t (*s_w)[3], uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &ta, uint32_t &tb, uint32_t &tc)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t ia = wave_incl_scan_u32(a), ib = wave_incl_scan_u32(b), ic = wave_incl_scan_u32(c);
	__syncthreads(); // (s_w of an earlier call has been read)
	if (lane == 63u) {
		s_w[wave][0] = ia;
		s_w[wave][1] = ib;
		s_w[wave][2] = ic;
	}
	__syncthreads();
	uint32_t ba = 0, bb = 0, bc = 0;
	ta = tb = tc = 0;
#pragma unroll
	for (uint32_t k = 0; k < GYS_RS_THREADS / 64u; ++k) {
		if (k < wave) {
			ba += s_w[k][0];
			bb += s_w[k][1];
			bc += s_w[k][2];
		}
		ta += s_w[k][0];
		tb += s_w[k][1];
		tc += s_w[k][2];
	}
	a = ba + ia - a;
	b = bb + ib - b;
	c = bc + ic - c;
}

__global__ __launch_bounds__(GYS_RS_THREADS) void k_rollsel_scan(RollScanP q)
{
	__shared__ uint32_t s_w[GYS_RS_THREADS / 64u][3];
	if (q.phase == 1u) { // one workgroup: the tiles' totals -> their exclusive scan, the totals of the selection
		uint32_t ra = 0, rb = 0, rc = 0; // totals of the tiles before this round
		for (uint32_t t0 = 0; t0 < q.ntiles; t0 += GYS_RS_THREADS) { // (uniform trips)
			const uint32_t t = t0 + threadIdx.x;
			uint32_t a = 0, b = 0, c = 0, ta, tb, tc;
			if (t < q.ntiles) {
				a = q.tiles[3u * t];
				b = q.tiles[3u * t + 1u];
				c = q.tiles[3u * t + 2u];
			}
			rollsel_block_scan3(s_w, a, b, c, ta, tb, tc);
			if (t < q.ntiles) {
				q.tiles[3u * t] = ra + a;
				q.tiles[3u * t + 1u] = rb + b;
				q.tiles[3u * t + 2u] = rc + c;
			}
			ra += ta;
			rb += tb;
			rc += tc;
		}
		if (threadIdx.x == 0) {
			q.tot[RS_TOT_ROWS] = ra;
			q.tot[RS_TOT_MEMBERS_ALL] = rb;
			q.tot[RS_TOT_CHUNKS_ALL] = rc;
			// no row is cut off unless phase 2 finds row `maxrows`
			q.tot[RS_TOT_MEMBERS] = rb;
			q.tot[RS_TOT_CHUNKS] = rc;
			q.tot[RS_TOT_GCUT] = GYS_NO_GROUP;
		}
		return;
	}
	for (uint32_t tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
		// thread t: the GYS_RS_SCAN_PER_THREAD consecutive groups from g0
		const uint32_t g0 = tile * GYS_RS_SCAN_TILE + threadIdx.x * GYS_RS_SCAN_PER_THREAD;
		uint32_t cnt[GYS_RS_SCAN_PER_THREAD];
		uint32_t a = 0, b = 0, c = 0, ta, tb, tc;
#pragma unroll
		for (uint32_t k = 0; k < GYS_RS_SCAN_PER_THREAD; k += 4u) {
			uint4 v = make_uint4(0u, 0u, 0u, 0u);
			if (g0 + k + 3u < q.ndomain) { // (counts is 16-byte aligned and g0 + k a multiple of 4)
				v = *(const uint4 *)(q.counts + g0 + k);
			} else {
				if (g0 + k < q.ndomain) v.x = q.counts[g0 + k];
				if (g0 + k + 1u < q.ndomain) v.y = q.counts[g0 + k + 1u];
				if (g0 + k + 2u < q.ndomain) v.z = q.counts[g0 + k + 2u];
			}
			cnt[k] = v.x;
			cnt[k + 1u] = v.y;
			cnt[k + 2u] = v.z;
			cnt[k + 3u] = v.w;
		}
#pragma unroll
		for (uint32_t k = 0; k < GYS_RS_SCAN_PER_THREAD; ++k) {
			a += cnt[k] != 0u;
			b += cnt[k];
			c += (cnt[k] + q.per - 1u) / q.per;
		}
		rollsel_block_scan3(s_w, a, b, c, ta, tb, tc);
		if (q.phase == 0u) {
			if (threadIdx.x == 0) {
				q.tiles[3u * tile] = ta;
				q.tiles[3u * tile + 1u] = tb;
				q.tiles[3u * tile + 2u] = tc;
			}
			continue;
		}
		uint32_t row = q.tiles[3u * tile] + a, moff = q.tiles[3u * tile + 1u] + b, coff = q.tiles[3u * tile + 2u] + c;
#pragma unroll
		for (uint32_t k = 0; k < GYS_RS_SCAN_PER_THREAD; ++k) {
			const uint32_t n = cnt[k], g = g0 + k;
			if (!n) continue; // (a group without members: no row, its counter stays zero)
			if (row < q.maxrows) {
				q.rows[row].group = g;
				q.rows[row].nmembers = n;
				q.rowoff[row] = make_uint2(moff, coff);
			} else if (row == q.maxrows) { // the first row cut off: what lies before it is what the call computes
				q.tot[RS_TOT_MEMBERS] = moff;
				q.tot[RS_TOT_CHUNKS] = coff;
				q.tot[RS_TOT_GCUT] = g;
			}
			q.counts[g] = moff;
			++row;
			moff += n;
			coff += (n + q.per - 1u) / q.per;
		}
	}
}

__global__ __launch_bounds__(GYS_RS_THREADS) void k_rollsel_scatter(RollSelP p)
{
	__shared__ uint32_t s_cnt[GYS_RS_SCATTER_LDS_GROUPS];
	const bool lds = p.ndomain <= GYS_RS_SCATTER_LDS_GROUPS;
	const uint32_t lane = threadIdx.x & 63u, gcut = p.tot[RS_TOT_GCUT];
	for (uint32_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) { // (uniform trips)
		const uint32_t first = tile * GYS_RS_TILE;
		uint32_t grp[GYS_RS_PER_THREAD], slot[GYS_RS_PER_THREAD], at[GYS_RS_PER_THREAD];
#pragma unroll
		for (uint32_t k = 0; k < GYS_RS_PER_THREAD; ++k) {
			const uint32_t item = first + k * GYS_RS_THREADS + threadIdx.x;
			grp[k] = GYS_NO_GROUP;
			slot[k] = 0;
			at[k] = 0;
			if (item < p.nitems) {
				const uint32_t g = p.item_group[item];
				if (g < gcut) grp[k] = g; // (GYS_NO_GROUP is below no cut; a group at or past the cut has no row)
				slot[k] = p.slot_list ? p.slot_list[item] : item;
			}
		}
		if (lds) {
			// the member's rank among the tile's members of its group, then one global atomic per group the tile has met
			for (uint32_t k = threadIdx.x; k < p.ndomain; k += GYS_RS_THREADS) s_cnt[k] = 0;
			__syncthreads();
#pragma unroll
			for (uint32_t k = 0; k < GYS_RS_PER_THREAD; ++k)
				if (grp[k] != GYS_NO_GROUP) at[k] = atomicAdd(&s_cnt[grp[k]], 1u);
			__syncthreads();
			for (uint32_t k = threadIdx.x; k < p.ndomain; k += GYS_RS_THREADS) {
				const uint32_t n = s_cnt[k];
				if (n) s_cnt[k] = atomicAdd(&p.counts[k], n);
			}
			__syncthreads();
#pragma unroll
			for (uint32_t k = 0; k < GYS_RS_PER_THREAD; ++k)
				if (grp[k] != GYS_NO_GROUP) p.members[s_cnt[grp[k]] + at[k]] = slot[k];
			__syncthreads(); // (s_cnt is cleared again in the next trip)
		} else {
#pragma unroll
			for (uint32_t k = 0; k < GYS_RS_PER_THREAD; ++k) {
				const uint32_t g = grp[k];
				uint32_t base, rank;
				const bool done = rollsel_wave_join(g, lane, base, rank, [&](uint32_t gl, uint32_t n) { return atomicAdd(&p.counts[gl], n); });
				if (g == GYS_NO_GROUP) continue;
				p.members[done ? base + rank : atomicAdd(&p.counts[g], 1u)] = slot[k];
			}
		}
	}
}

struct RollChunksP {
	const gys_rollup_row *rows;
	const uint2 *rowoff;
	const uint32_t *tot;
	uint32_t maxrows, per;
	RollupChunk *chunks;  // [tot[RS_TOT_CHUNKS]]
	RollupChunk *gchunks; // [rows computed]
};

__global__ __launch_bounds__(GYS_RS_THREADS) void k_rollsel_chunks(RollChunksP q)
{
	const uint32_t lane = threadIdx.x & 63u, nrows = min(q.tot[RS_TOT_ROWS], q.maxrows);
	const uint32_t wave = (blockIdx.x * GYS_RS_THREADS + threadIdx.x) >> 6, nwaves = gridDim.x * (GYS_RS_THREADS / 64u);
	for (uint32_t r = wave; r < nrows; r += nwaves) {
		const uint32_t n = q.rows[r].nmembers;
		const uint2 off = q.rowoff[r];
		const uint32_t nch = (n + q.per - 1u) / q.per;
		for (uint32_t j = lane; j < nch; j += 64u) {
			RollupChunk ck;
			ck.group = r;
			ck.m0 = off.x + j * q.per;
			ck.m1 = off.x + min(n, (j + 1u) * q.per);
			ck.pad = 0u;
			q.chunks[off.y + j] = ck;
		}
		if (lane == 0u) {
			RollupChunk gk;
			gk.group = r;
			gk.m0 = off.y;
			gk.m1 = off.y + nch;
			gk.pad = 0u;
			q.gchunks[r] = gk;
		}
	}
}

__global__ __launch_bounds__(256) void k_rollsel_labels(const uint32_t *__restrict__ slots, const uint32_t *__restrict__ groups, uint32_t n, uint32_t *__restrict__ labels)
{
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) labels[slots[i]] = groups[i];
}

} // namespace gys
