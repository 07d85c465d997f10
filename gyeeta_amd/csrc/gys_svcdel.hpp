// Deleting listeners (gys_delete_listeners, gys_register_listeners_slots, gys_list_stale_listeners): the device side.
//
// The reference drops a listener on a LISTENER_STATE_NOTIFY record flagged LISTEN_FLAG_DELETE (server/gy_mconnhdlr.cc:11195-11248: the
// object leaves glob_listener_tbl_ and the partha's listen_tbl_, its histograms go with it) and synthesises such records for every
// listener whose state is older than 30 minutes (:16296-16343).  Here a deleted service gives its SLOT back: the slot leaves both key
// tables, its per-service state returns to what gys_create left (once at the delete, once more when the slot is handed out: window
// closes in between write for a free slot what they write for a service without data), and a later registration may take it.
//
//   k_table_erase        keys out of an open-addressing table (gys_device.hpp) by BACKWARD-SHIFT deletion: the entries of the probe run
//                        behind the hole move up as far as their home position allows, so the table is afterwards what inserting the
//                        remaining keys alone could have produced -- no tombstone, "no key behind an empty entry" (tbl_lookup,
//                        k_table_insert_vals and k_table_set rely on it) holds, and probe lengths are those of the live keys however many
//                        register / delete cycles have passed.  Two erases in overlapping runs would race, and a batch is at most a few
//                        hundred keys with runs of two or three entries at the table's load of <= 1/2: one thread walks the list.
//                        BATCH SIZE: the kernel is one lane, a few dependent global accesses per key -- right for the hundreds of ids
//                        of a delete message or a cleanup round (the shim deletes 512 per call), not for 10^5 ids in one call.
//   k_table_insert_vals  keys into a table, each with its value (the service slot: a reused one or one of the tail); a key that is
//                        already there is rebound to the new value.
//   k_svc_clear          per listed slot, every per-service array back to its initial contents.  The arrays are described by a segment
//                        list the host fills in (SvcClearSeg: base, bytes per service, fill words): a workgroup per slot, its four waves
//                        take the segments in turn, the lanes of a wave store 16 bytes each (segments of 4 or 8 bytes per service: dwords).
//                        512 deletions are one launch that writes 512 x ~12 KB instead of 512 x ~45 memsets.
//   k_svc_stale_mark / _scan / _emit   the inactivity walk: one pass over the id word and the epoch word of the 96-byte kept records
//                        (mark: a hit bit per slot, by wave ballot, and the hits per tile of 1024 slots), an exclusive scan of the tile
//                        counts (one workgroup, rollsel_block_scan3 of gys_rollsel.hpp), and the ordered emit of the first `cap` ids from the bits -- ascending slot order, no
//                        sort, and the records are read once.
#pragma once

namespace gys {

// ---------------------------------------------------------------------------------------------------- key tables
// true: the key was there.  One caller at a time per table.
__device__ __forceinline__ bool tbl_erase(const DevTable &t, uint64_t key)
{
	if (key == GYS_EMPTY_KEY) return false;
	uint32_t i = get_uint64_hash(key) & t.mask;
	uint32_t probes = 0;
	for (;; ++probes) {
		if (probes > t.mask) return false;
		const uint64_t k = t.ent[i].key;
		if (k == key) break;
		if (k == GYS_EMPTY_KEY) return false;
		i = (i + 1) & t.mask;
	}
	// i is the hole.  An entry at j behind it (same run) may move into the hole unless its home position lies cyclically in (i, j]:
	// then a lookup that starts at home would no longer pass the hole before it reaches j, i.e. the entry is still found where it is.
	uint32_t j = i;
	for (uint32_t steps = 0; steps <= t.mask; ++steps) {
		j = (j + 1) & t.mask;
		const TblEnt e = t.ent[j];
		if (e.key == GYS_EMPTY_KEY) break;
		const uint32_t home = get_uint64_hash(e.key) & t.mask;
		const bool stays = i <= j ? (i < home && home <= j) : (i < home || home <= j);
		if (stays) continue;
		t.ent[i] = e;
		i = j;
	}
	t.ent[i].key = GYS_EMPTY_KEY;
	t.ent[i].val = 0xFFFFFFFFu;
	t.ent[i].pad = 0xFFFFFFFFu;
	return true;
}

// nerased (may be nullptr) += the keys that were found
__global__ void k_table_erase(DevTable t, const uint64_t *keys, uint32_t n, uint32_t *nerased)
{
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	uint32_t hit = 0;
	for (uint32_t i = 0; i < n; ++i) hit += tbl_erase(t, keys[i]) ? 1u : 0u;
	if (nerased) *nerased += hit;
}

__global__ void k_table_insert_vals(DevTable t, const uint64_t *keys, const uint32_t *vals, uint32_t n, uint32_t *nfail)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint64_t key = keys[i];
	uint32_t h = get_uint64_hash(key) & t.mask;
	for (uint32_t probes = 0; probes <= t.mask; ++probes) {
		const unsigned long long prev = atomicCAS((unsigned long long *)&t.ent[h].key, (unsigned long long)GYS_EMPTY_KEY, (unsigned long long)key);
		if (prev == GYS_EMPTY_KEY || prev == key) {
			t.ent[h].val = vals[i];
			return;
		}
		h = (h + 1) & t.mask;
	}
	atomicAdd(nfail, 1u);
}

// out[i] = in[i] placed by slot: dst[slots[i]] = src[i] (svc_gid / svc_host of the services a registration puts into listed slots)
__global__ void k_scatter_u64(uint64_t *dst, const uint32_t *slots, const uint64_t *src, uint32_t n)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) dst[slots[i]] = src[i];
}
__global__ void k_scatter_const_u32(uint32_t *dst, const uint32_t *slots, uint32_t v, uint32_t n)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) dst[slots[i]] = v;
}

// ---------------------------------------------------------------------------------------------------- per-service state
// One per-service array: service s owns [base + s * bytes, base + (s + 1) * bytes).  bytes is a multiple of 16 with a 16-byte aligned
// base, or a smaller multiple of 4 (dword stores), or 2.  Every 16-byte piece is filled with `fill`, the LAST piece of the service's part with `last` (a
// histogram record is zero up to max_val_seen, its last 8 bytes); a dword segment takes the words of `fill` in turn.
// kind / rec_off: what a service record does with the array and where it holds it (gys_svcpack.hpp; k_svc_clear reads neither).
struct SvcClearSeg {
	uint8_t *base;
	uint64_t bytes;
	uint4 fill, last;
	uint32_t kind = 0, rec_off = 0;
};
#define GYS_SVCCLEAR_NT 256u
#define GYS_SVCCLEAR_MAXSEG 96u

__global__ __launch_bounds__(GYS_SVCCLEAR_NT) void k_svc_clear(const SvcClearSeg *segs, uint32_t nsegs, const uint32_t *slots, uint32_t nslots, uint32_t max_services)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	constexpr uint32_t nwaves = GYS_SVCCLEAR_NT / 64u;
	for (uint32_t it = blockIdx.x; it < nslots; it += gridDim.x) {
		const uint32_t slot = slots[it];
		if (slot >= max_services) continue; // (never: the host lists registered slots)
		for (uint32_t g = wave; g < nsegs; g += nwaves) {
			const SvcClearSeg sg = segs[g];
			uint8_t *dst = sg.base + (uint64_t)slot * sg.bytes;
			if (sg.bytes < 4ull) { // (the two history bytes of gys_decide_listener_state_dev)
				if (lane < sg.bytes / 2ull) ((uint16_t *)dst)[lane] = (uint16_t)sg.fill.x;
			} else if (sg.bytes & 15ull) {
				const uint32_t nw = (uint32_t)(sg.bytes >> 2);
				for (uint32_t w = lane; w < nw; w += 64u) ((uint32_t *)dst)[w] = (w & 1u) ? ((w & 2u) ? sg.fill.w : sg.fill.y) : ((w & 2u) ? sg.fill.z : sg.fill.x);
			} else {
				const uint64_t np = sg.bytes >> 4;
				for (uint64_t q = lane; q < np; q += 64u) ((uint4 *)dst)[q] = q + 1 == np ? sg.last : sg.fill;
			}
		}
	}
}

// ---------------------------------------------------------------------------------------------------- stale listeners
#define GYS_STALE_NT 256u
#define GYS_STALE_TILE 1024u // slots per tile: 16 ballot words

struct SvcStaleP {
	const uint8_t *svc_state; // [nsvc * 96]: words 0..1 the record's glob_id_, word 22 the window it was kept in (0: deleted / never)
	uint32_t nsvc, ntiles;
	uint32_t epoch;           // the open window
	uint32_t flags, max_age;  // GYS_STALE_DELETED: id != 0 and window word 0; GYS_STALE_AGED: window word != 0 and epoch - word > max_age
	unsigned long long *bits; // [ntiles * 16] a bit per slot
	uint32_t *tile_cnt;       // [ntiles + 1] hits per tile; after the scan: hits before the tile, [ntiles] = all
	uint64_t *ids;            // [cap]
	uint32_t cap;
};

__device__ __forceinline__ bool svc_stale_hit(const SvcStaleP &p, uint32_t slot)
{
	const uint32_t *r = (const uint32_t *)(p.svc_state + (size_t)slot * 96);
	const uint2 id = *(const uint2 *)r;
	const uint32_t ep = r[22];
	if (ep == 0u) return (p.flags & 1u) && (id.x | id.y) != 0u;
	return (p.flags & 2u) && p.epoch - ep > p.max_age;
}

__global__ __launch_bounds__(GYS_STALE_NT) void k_svc_stale_mark(SvcStaleP p)
{
	__shared__ uint32_t s_cnt[GYS_STALE_NT / 64u];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (uint32_t tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
		uint32_t cnt = 0;
#pragma unroll
		for (uint32_t k = 0; k < GYS_STALE_TILE / GYS_STALE_NT; ++k) {
			const uint32_t slot = tile * GYS_STALE_TILE + k * GYS_STALE_NT + threadIdx.x;
			const bool hit = slot < p.nsvc && svc_stale_hit(p, slot);
			const unsigned long long m = __ballot(hit);
			if (lane == 0u) p.bits[(size_t)tile * 16u + k * 4u + wave] = m;
			cnt += (uint32_t)__popcll(m);
		}
		if (lane == 0u) s_cnt[wave] = cnt;
		__syncthreads();
		if (threadIdx.x == 0) p.tile_cnt[tile] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
		__syncthreads();
	}
}

// one workgroup: tile_cnt -> exclusive prefix, tile_cnt[ntiles] = total
__global__ __launch_bounds__(GYS_STALE_NT) void k_svc_stale_scan(SvcStaleP p)
{
	// the workgroup scan of gys_rollsel.hpp (k_rollsel_scan, phase 1), a round of GYS_RS_THREADS tiles at a time; one of its three sums is used
	__shared__ uint32_t s_w[GYS_RS_THREADS / 64u][3];
	uint32_t run = 0; // hits of the tiles before this round
	for (uint32_t t0 = 0; t0 < p.ntiles; t0 += GYS_RS_THREADS) { // (uniform trips)
		const uint32_t t = t0 + threadIdx.x;
		uint32_t a = t < p.ntiles ? p.tile_cnt[t] : 0u, b = 0, c = 0, ta, tb, tc;
		rollsel_block_scan3(s_w, a, b, c, ta, tb, tc);
		if (t < p.ntiles) p.tile_cnt[t] = run + a;
		run += ta;
	}
	if (threadIdx.x == 0) p.tile_cnt[p.ntiles] = run;
}
static_assert(GYS_STALE_NT == GYS_RS_THREADS, "k_svc_stale_scan runs the rollsel workgroup scan");

// a thread per ballot word: its place = hits before the tile + hits of the tile's earlier words
__global__ __launch_bounds__(GYS_STALE_NT) void k_svc_stale_emit(SvcStaleP p)
{
	const uint64_t nwords = (uint64_t)p.ntiles * 16ull;
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += (uint64_t)gridDim.x * blockDim.x) {
		unsigned long long m = p.bits[w];
		if (!m) continue;
		const uint32_t tile = (uint32_t)(w >> 4), k = (uint32_t)(w & 15u);
		uint32_t at = p.tile_cnt[tile];
		for (uint32_t e = 0; e < k; ++e) at += (uint32_t)__popcll(p.bits[(size_t)tile * 16u + e]);
		// word k of a tile holds slots tile * 1024 + (k / 4) * 256 + (k % 4) * 64 + bit: ascending in k
		const uint32_t first = tile * GYS_STALE_TILE + k * 64u;
		for (; m && at < p.cap; m &= m - 1ull, ++at) {
			const uint32_t slot = first + (uint32_t)__ffsll((long long)m) - 1u;
			const uint2 id = *(const uint2 *)(p.svc_state + (size_t)slot * 96);
			p.ids[at] = (uint64_t)id.x | ((uint64_t)id.y << 32);
		}
	}
}

} // namespace gys
