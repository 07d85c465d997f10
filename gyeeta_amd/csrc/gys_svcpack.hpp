// Saving, restoring and moving per-service state (gys_pack_services*, gys_unpack_services*; "service records" in include/gysketch.h):
// the device side.
//
// A service RECORD is the service's part of every per-service array of the context, byte for byte, at a fixed offset per array.  The
// arrays are the segment list of k_svc_clear (gys_svcdel.hpp; the host builds it in svc_clear_segments(), the one place that names a
// per-service array), each with a KIND and, where it is carried, its offset in the record:
//   GYS_SVCSEG_CARRY       copied both ways.  An array the context has not allocated (base == nullptr: the history bytes before the first
//                          decision, td_prevm without predicted runs) packs as its initial contents and is skipped by the unpack.
//   GYS_SVCSEG_CARRY_HOST  the 96-byte kept listener state: carried, and the unpack rewrites word 23 (the host slot k_lstate_keep stored
//                          behind the 88-byte record) to the DESTINATION's host slot of the service -- in a record that was ever kept
//                          (id words non-zero); a service that never reported state has an all-zero entry here and keeps it.
//   GYS_SVCSEG_RESET       not in the record; the unpack writes the array's initial contents (the run cursors of an ingest call, the claim word).
//   GYS_SVCSEG_KEEP        not in the record and not touched (glob id, host, label: the destination's registration owns them).
// Behind the arrays a record holds the service's buffered t-digest values: the first td_cur[slot] words of its td_pend buffer (the words
// behind the cursor are never read and are not carried; the record reserves td_pend_cap words and the pack zeroes the rest, so a record
// is a function of the state alone).
//
//   k_svc_pack / k_svc_unpack   the walk of k_svc_clear with a load in front of the store: one 256-thread workgroup per listed service
//                          (grid-stride beyond the grid), the four waves take the segments in turn, 16-byte pieces where the segment
//                          allows (up to GYS_SVCPACK_VEC pieces per lane in flight: the 20 level snapshots, the 200 clusters, the
//                          buffer), dwords for the 4 / 8 / 24 / 32-byte segments, one 16-bit access for the two history bytes.  The
//                          buffer is the last "segment": a service's buffer starts at slot * td_buf_values words, 4-byte aligned only
//                          when that is odd, so the copy runs in three parts like k_huge_count's loads -- head words up to a 16-byte
//                          boundary of the BUFFER side, 16-byte pieces, tail words; the record side of a piece is one 16-byte access
//                          when the head is empty and four dwords otherwise.  No atomics, no LDS, no barrier.
#pragma once

namespace gys {

#define GYS_SVCSEG_CARRY 1u
#define GYS_SVCSEG_CARRY_HOST 2u
#define GYS_SVCSEG_RESET 3u
#define GYS_SVCSEG_KEEP 4u
#define GYS_SVCPACK_NT GYS_SVCCLEAR_NT
#define GYS_SVCPACK_VEC 4u // 16-byte pieces a lane requests before it stores them

struct SvcPackP {
	const SvcClearSeg *segs;  // the context's arrays (SvcClearSeg::kind / rec_off filled in)
	uint32_t nsegs;
	uint32_t n;               // records
	const uint32_t *slots;    // [n] the service slot of record i (unpack: GYS_NOSLOT = the id is not registered here, skipped)
	const uint32_t *hosts;    // [n] unpack: the destination's host slot of the service
	uint32_t max_services;
	uint32_t stride;          // bytes per record (a multiple of 16)
	uint8_t *recs;            // record i at recs + i * stride (16-byte aligned)
	uint32_t *td_pend;        // nullptr: no t-digest
	const uint32_t *td_cur;   // pack: the cursors of the source
	uint32_t pcap;            // words per service in td_pend
	uint32_t pend_cap;        // words the record reserves (<= pcap)
	uint32_t cur_off;         // unpack: record offset of the service's td_cur word
	uint32_t pad_off;         // record bytes [pad_off, pend_off) belong to no array: zeroed by the pack
	uint32_t pend_off;        // record offset of the buffered words (a multiple of 16); stride without t-digest
};

__device__ __forceinline__ uint32_t svcseg_fill_word(const SvcClearSeg &sg, uint32_t w)
{
	return (w & 1u) ? ((w & 2u) ? sg.fill.w : sg.fill.y) : ((w & 2u) ? sg.fill.z : sg.fill.x);
}

// np 16-byte pieces, both sides 16-byte aligned; HOSTW: the piece that holds word 23 of a kept state entry takes `host`
template <bool HOSTW>
__device__ __forceinline__ void svcpack_copy16(uint4 *dst, const uint4 *src, uint64_t np, uint32_t lane, uint32_t host, bool rewrite)
{
	for (uint64_t q0 = 0; q0 < np; q0 += 64u * GYS_SVCPACK_VEC) {
		uint4 w[GYS_SVCPACK_VEC];
#pragma unroll
		for (uint32_t u = 0; u < GYS_SVCPACK_VEC; ++u) {
			const uint64_t q = q0 + u * 64u + lane;
			w[u] = q < np ? src[q] : make_uint4(0u, 0u, 0u, 0u);
		}
#pragma unroll
		for (uint32_t u = 0; u < GYS_SVCPACK_VEC; ++u) {
			const uint64_t q = q0 + u * 64u + lane;
			if (q < np) {
				if (HOSTW && rewrite && q == 5u) w[u].w = host; // word 23 = the last word of piece 5
				dst[q] = w[u];
			}
		}
	}
}

// a segment's initial contents (k_svc_clear's stores) to dst
__device__ __forceinline__ void svcpack_fill(uint8_t *dst, const SvcClearSeg &sg, uint32_t lane, bool rec_side)
{
	if (sg.bytes < 4ull) {
		if (lane == 0u) {
			if (rec_side) *(uint32_t *)dst = sg.fill.x & 0xFFFFu; // (the record gives the two bytes a whole word)
			else *(uint16_t *)dst = (uint16_t)sg.fill.x;
		}
	} else if (sg.bytes & 15ull) {
		const uint32_t nw = (uint32_t)(sg.bytes >> 2);
		for (uint32_t w = lane; w < nw; w += 64u) ((uint32_t *)dst)[w] = svcseg_fill_word(sg, w);
	} else {
		const uint64_t np = sg.bytes >> 4;
		for (uint64_t q = lane; q < np; q += 64u) ((uint4 *)dst)[q] = q + 1 == np ? sg.last : sg.fill;
	}
}

__device__ __forceinline__ uint4 svcpack_ld4(const uint32_t *p, bool aligned)
{
	return aligned ? *(const uint4 *)p : make_uint4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void svcpack_st4(uint32_t *p, bool aligned, uint4 v)
{
	if (aligned) {
		*(uint4 *)p = v;
	} else {
		p[0] = v.x;
		p[1] = v.y;
		p[2] = v.z;
		p[3] = v.w;
	}
}

// n buffered words between a service's buffer (`buf`, 4-byte aligned) and its record (`rec`, 16-byte aligned): TO_REC = pack.
// The 16-byte pieces are cut on the buffer side; one wave.
template <bool TO_REC>
__device__ __forceinline__ void svcpack_pend(uint32_t *buf, uint32_t *rec, uint32_t n, uint32_t lane)
{
	const uint32_t head = min(n, (4u - ((uint32_t)((uintptr_t)buf >> 2) & 3u)) & 3u); // words in front of the buffer's first 16-byte boundary
	const bool al = head == 0u;
	if (lane < head) {
		if (TO_REC) rec[lane] = buf[lane];
		else buf[lane] = rec[lane];
	}
	const uint32_t nvec = (n - head) >> 2;
	uint32_t *bv = buf + head, *rv = rec + head;
	for (uint32_t j0 = 0; j0 < nvec; j0 += 64u * GYS_SVCPACK_VEC) {
		uint4 w[GYS_SVCPACK_VEC];
#pragma unroll
		for (uint32_t u = 0; u < GYS_SVCPACK_VEC; ++u) {
			const uint32_t j = j0 + u * 64u + lane;
			if (j < nvec) w[u] = TO_REC ? *(const uint4 *)(bv + 4u * j) : svcpack_ld4(rv + 4u * j, al);
			else w[u] = make_uint4(0u, 0u, 0u, 0u);
		}
#pragma unroll
		for (uint32_t u = 0; u < GYS_SVCPACK_VEC; ++u) {
			const uint32_t j = j0 + u * 64u + lane;
			if (j < nvec) {
				if (TO_REC) svcpack_st4(rv + 4u * j, al, w[u]);
				else *(uint4 *)(bv + 4u * j) = w[u];
			}
		}
	}
	const uint32_t t0 = head + 4u * nvec; // (at most three words behind the last whole piece)
	if (t0 + lane < n) {
		if (TO_REC) rec[t0 + lane] = buf[t0 + lane];
		else buf[t0 + lane] = rec[t0 + lane];
	}
}

__global__ __launch_bounds__(GYS_SVCPACK_NT) void k_svc_pack(SvcPackP p)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	constexpr uint32_t nwaves = GYS_SVCPACK_NT / 64u;
	for (uint32_t it = blockIdx.x; it < p.n; it += gridDim.x) {
		const uint32_t slot = p.slots[it];
		if (slot >= p.max_services) continue; // (never: the host lists registered slots)
		uint8_t *rec = p.recs + (uint64_t)it * p.stride;
		for (uint32_t g = wave; g <= p.nsegs; g += nwaves) {
			if (g == p.nsegs) { // the pad in front of the buffered words, the words, zeroes up to the record's end
				for (uint32_t b = p.pad_off + lane * 4u; b < p.pend_off; b += 256u) *(uint32_t *)(rec + b) = 0u;
				if (!p.td_pend) continue;
				const uint32_t npend = min(p.td_cur[slot], p.pend_cap);
				uint32_t *dst = (uint32_t *)(rec + p.pend_off);
				svcpack_pend<true>(p.td_pend + (uint64_t)slot * p.pcap, dst, npend, lane);
				const uint32_t nres = (p.stride - p.pend_off) >> 2;
				for (uint32_t w = npend + lane; w < nres; w += 64u) dst[w] = 0u;
				continue;
			}
			const SvcClearSeg sg = p.segs[g];
			if (sg.kind != GYS_SVCSEG_CARRY && sg.kind != GYS_SVCSEG_CARRY_HOST) continue;
			uint8_t *dst = rec + sg.rec_off;
			if (!sg.base) {
				svcpack_fill(dst, sg, lane, true);
				continue;
			}
			const uint8_t *src = sg.base + (uint64_t)slot * sg.bytes;
			if (sg.bytes < 4ull) {
				if (lane == 0u) *(uint32_t *)dst = (uint32_t)*(const uint16_t *)src;
			} else if (sg.bytes & 15ull) {
				const uint32_t nw = (uint32_t)(sg.bytes >> 2);
				for (uint32_t w = lane; w < nw; w += 64u) ((uint32_t *)dst)[w] = ((const uint32_t *)src)[w];
			} else {
				svcpack_copy16<false>((uint4 *)dst, (const uint4 *)src, sg.bytes >> 4, lane, 0u, false);
			}
		}
	}
}

__global__ __launch_bounds__(GYS_SVCPACK_NT) void k_svc_unpack(SvcPackP p)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	constexpr uint32_t nwaves = GYS_SVCPACK_NT / 64u;
	for (uint32_t it = blockIdx.x; it < p.n; it += gridDim.x) {
		const uint32_t slot = p.slots[it];
		if (slot >= p.max_services) continue; // GYS_NOSLOT: the id is not registered here
		const uint8_t *rec = p.recs + (uint64_t)it * p.stride;
		for (uint32_t g = wave; g <= p.nsegs; g += nwaves) {
			if (g == p.nsegs) {
				if (!p.td_pend) continue;
				const uint32_t npend = min(*(const uint32_t *)(rec + p.cur_off), p.pend_cap); // nothing is written past the cursor
				svcpack_pend<false>(p.td_pend + (uint64_t)slot * p.pcap, (uint32_t *)(rec + p.pend_off), npend, lane);
				continue;
			}
			const SvcClearSeg sg = p.segs[g];
			if (!sg.base || sg.kind == GYS_SVCSEG_KEEP) continue;
			uint8_t *dst = sg.base + (uint64_t)slot * sg.bytes;
			if (sg.kind == GYS_SVCSEG_RESET) {
				svcpack_fill(dst, sg, lane, false);
				continue;
			}
			if (sg.kind != GYS_SVCSEG_CARRY && sg.kind != GYS_SVCSEG_CARRY_HOST) continue;
			const uint8_t *src = rec + sg.rec_off;
			if (sg.bytes < 4ull) {
				if (lane == 0u) *(uint16_t *)dst = (uint16_t)*(const uint32_t *)src;
			} else if (sg.bytes & 15ull) {
				const uint32_t nw = (uint32_t)(sg.bytes >> 2);
				for (uint32_t w = lane; w < nw; w += 64u) ((uint32_t *)dst)[w] = ((const uint32_t *)src)[w];
			} else if (sg.kind == GYS_SVCSEG_CARRY_HOST) {
				const uint2 id = *(const uint2 *)src; // a record that was ever kept names its listener
				svcpack_copy16<true>((uint4 *)dst, (const uint4 *)src, sg.bytes >> 4, lane, p.hosts[it], (id.x | id.y) != 0u);
			} else {
				svcpack_copy16<false>((uint4 *)dst, (const uint4 *)src, sg.bytes >> 4, lane, 0u, false);
			}
		}
	}
}

} // namespace gys
