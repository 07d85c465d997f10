// Group response-time histograms: the GY_HISTOGRAM record of a GROUP of services (a host, a cluster, this rank, the rows of a filtered
// selection) at one of the four closed-window levels (5 s / 300 s / 5 days / all; "multi-level windows" in gys_kernels.hpp).  A group's record
// is the sum of its members' records, the reference's GY_HISTOGRAM::add_histogram (common/gy_statistics.h:625-660; oracle: gyo_hist_merge):
// per bucket count += count and sum += sum, total_count += total_count, max_val_seen = the larger one.  No member: the record gys_hist_init_dev
// leaves (all zero, max_val_seen = INT64_MIN).  The group's percentiles are the existing k_hist_percentiles on that record.
//
// One kernel, k_hist_level_union, launched twice (the shape of k_hll_union, over the same RollupChunk / member lists):
//   1. a workgroup per chunk of at most GYS_RB_CHUNK_SERVICES member services.  A record is 16 pairs of 16 bytes, pairs 0..14 {count, sum},
//      pair 15 {total_count, max_val_seen}: a group of 16 lanes owns one member at a time, lane k its pair k.  The member's record of the
//      level is never stored: the lanes work it out in registers by level_pair_load / level_pair_value, the rule k_level_view stores from
//      (one definition, gys_kernels.hpp), and add it to their running pair (pair_add: u64 adds, a signed maximum in pair 15's .y).  The loads
//      of GYS_HR_INFLIGHT members are requested before the first is used.  Which loads there are depends on the level's mode and on whether
//      meta / sub / last_tag exist: kernel arguments, the same in every lane.
//   2. "plain": the members are records as they stand (members == nullptr: member j = record j).  The chunks' partial records -> one record
//      per row (the rows' chunk ranges, gchunks); host records -> cluster records, host records -> the rank's record.
// Join: the 16 lane groups of the workgroup hold 16 partial records.  Pair k of a record lives in lane k of EVERY row of 16 lanes and the DPP
// row operations move data inside a row (row_bcast only carries lane 15 onwards), so DPP does not reach from one lane group to the next:
// lane groups and waves alike are joined by one LDS step -- every thread stores its pair (4 KB), one barrier, the first 16 threads add the 16
// pairs of their column (reads of 16 consecutive 16-byte words: no bank conflict) and store the chunk's 256-byte record.  No __shfl, no
// atomics, no pre-zeroed output: every chunk's record is written exactly once, whole.
//
// DETERMINISM: counts and sums are added as 64-bit integers (the sums in two's complement, i.e. as u64), and such adds commute and associate
// mod 2^64; so does the maximum.  Every path therefore gives the same BITS: any chunking, any grid size, any order of the members, services ->
// hosts -> cluster as well as services -> cluster directly.  tests/cpp/kemu/test_histroll.cc and tests/test_gpu_hist_rollup.py rely on it.
//
// Bytes per member service (first launch): 256 (cumulative) + 256 (snapshot, levels 1 and 2 / the last-window record, level 0, whose
// cumulative read shrinks to pair 15) + 16 (TdMeta, lazily folded records) + 4 (member index) + 256 (window record) only for a member whose
// open window is partly folded.  Written: 256 per chunk.
#pragma once

namespace gys {

#define GYS_HR_NT 256u     // threads of a workgroup: 16 lane groups
#define GYS_HR_INFLIGHT 4u // members per lane group whose loads are requested together

struct HistUnionP {
	LevelViewP v;              // plain == 0: the level's sources (first / n / out are not used); members are service slots
	const gys_hist_rec *src;   // plain == 1: the members' records
	gys_hist_rec *dst;         // one record per CHUNK: dst[chunk index]
	const RollupChunk *chunks; // nullptr: chunk i = members [i * per, min(n, (i + 1) * per))
	const uint32_t *members;   // slot (plain: record index) of a member; nullptr: member j = j
	uint32_t nchunks, n, per;
	int plain;
};

__global__ __launch_bounds__(GYS_HR_NT) void k_hist_level_union(HistUnionP q)
{
	__shared__ ulonglong2 red[GYS_HR_NT]; // 4 KB
	const uint32_t t = threadIdx.x, k = t & 15u, row = t >> 4;
	constexpr uint32_t rows = GYS_HR_NT / 16u;
	ulonglong2 ident;
	ident.x = 0ull;
	ident.y = k < 15u ? 0ull : (unsigned long long)INT64_MIN;
	for (uint32_t ch = blockIdx.x; ch < q.nchunks; ch += gridDim.x) {
		uint32_t m0, m1;
		if (q.chunks) {
			m0 = q.chunks[ch].m0;
			m1 = q.chunks[ch].m1;
		} else {
			m0 = ch * q.per;
			m1 = q.n - m0 < q.per ? q.n : m0 + q.per;
		}
		ulonglong2 acc = ident;
		uint32_t j = m0 + row;
		for (; j < m1 && m1 - j > (GYS_HR_INFLIGHT - 1u) * rows; j += GYS_HR_INFLIGHT * rows) { // the members' indices, then every load of theirs, then the adds
			uint32_t s[GYS_HR_INFLIGHT];
#pragma unroll
			for (uint32_t i = 0; i < GYS_HR_INFLIGHT; ++i) s[i] = q.members ? q.members[j + i * rows] : j + i * rows;
			if (q.plain) {
				ulonglong2 r[GYS_HR_INFLIGHT];
#pragma unroll
				for (uint32_t i = 0; i < GYS_HR_INFLIGHT; ++i) r[i] = ((const ulonglong2 *)q.src)[(uint64_t)s[i] * 16ull + k];
#pragma unroll
				for (uint32_t i = 0; i < GYS_HR_INFLIGHT; ++i) acc = pair_add(acc, r[i], k);
			} else {
				LevelPair in[GYS_HR_INFLIGHT];
#pragma unroll
				for (uint32_t i = 0; i < GYS_HR_INFLIGHT; ++i) in[i] = level_pair_load<true>(q.v, s[i], k);
#pragma unroll
				for (uint32_t i = 0; i < GYS_HR_INFLIGHT; ++i) acc = pair_add(acc, level_pair_value(q.v, in[i], k), k);
			}
		}
		for (; j < m1; j += rows) {
			const uint32_t s = q.members ? q.members[j] : j;
			if (q.plain) {
				acc = pair_add(acc, ((const ulonglong2 *)q.src)[(uint64_t)s * 16ull + k], k);
			} else {
				const LevelPair in = level_pair_load<true>(q.v, s, k);
				acc = pair_add(acc, level_pair_value(q.v, in, k), k);
			}
		}
		red[t] = acc;
		__syncthreads();
		if (t < 16u) {
			ulonglong2 r = red[t];
#pragma unroll
			for (uint32_t g = 1; g < rows; ++g) r = pair_add(r, red[g * 16u + t], k);
			((ulonglong2 *)q.dst)[(uint64_t)ch * 16ull + t] = r;
		}
		__syncthreads(); // (red is written again in the next turn)
	}
}

// ---------------------------------------------------------------------------------------------------- group records of a PERIOD
// The record of a group for the seconds [start, end) (gys_hist_rollup_period_dev): the sum of the members' records as k_level_period stores
// them.  A partly covered ring bucket is scaled in float and truncated per member and per ring bucket BEFORE anything is added (range_adjust),
// so the group record is not a function of the group's level records: the members are walked here, by the one period rule period_pair_load /
// period_pair_value (gys_kernels.hpp).  Shape, join and determinism are those of k_hist_level_union above: 16 lane groups of 16, lane k owns pair
// k, one workgroup per RollupChunk (grid-stride), the 4 KB LDS join, no atomics, no __shfl, no pre-zeroed output.  Pair 15's .x (total_count)
// costs nothing in the member loop: period_pair_value brings 0 there, and after the join it is the sum of the 15 joined counts -- the sum over
// the members of their totals, mod 2^64 the same value -- read back by thread 15 from the 15 joined pairs through LDS.
// The mode, nrb, whole_mask, the scales and the boundary pointers are kernel arguments: every branch on them is wave-uniform, and the
// boundary walk is unrolled under those scalar guards (no register array is indexed at run time).  All loads of GYS_HP_INFLIGHT members are
// requested before the first is used; in mode 0 a member asks for up to 13 sixteen-byte loads per lane (11 boundaries, cumulative, window).
// MEMBERS IN FLIGHT, from the register counts of the gfx950 code object (hipcc -O3; .vgpr_count of the kernel's metadata; the ~50 SGPRs of plan
// that do not fit the 102 are kept in VGPR lanes, no scratch either way): GYS_HP_INFLIGHT = 1 -> 78 VGPRs (allocated 80), 6 waves / SIMD;
// GYS_HP_INFLIGHT = 2 -> 134 VGPRs (allocated 136), 3 waves / SIMD.  Either way a SIMD has the same 6 x 13 = 3 x 26 = 78 sixteen-byte loads in
// flight in mode 0 (registers are allocated for the 11 boundaries whatever nrb is), so one member per lane group is kept: twice the waves to
// cover the dependent member index -> TdMeta -> window-record loads, half the live state.  (Two in flight would pay below 128 VGPRs, 4 waves.)
// Bytes per member service: 4 (member index) + 16 (TdMeta, lazily folded records) + 256 x (boundaries + cumulative [+ window, a member whose
// open window is partly folded]); modes 1 and 2 read pair 15 of the cumulative record only, mode 2 the last-window record, mode 3 first_sec.
#define GYS_HP_INFLIGHT 1u // members per lane group whose loads are requested together (see above)

struct HistPeriodUnionP {
	LevelPeriodP v;            // the period's sources and plan (first / n / out are not used)
	gys_hist_rec *dst;         // one record per CHUNK: dst[chunk index]
	const RollupChunk *chunks;
	const uint32_t *members;   // service slot of a member
	uint32_t nchunks;
};

__global__ __launch_bounds__(GYS_HR_NT) void k_hist_period_union(HistPeriodUnionP q)
{
	__shared__ ulonglong2 red[GYS_HR_NT]; // 4 KB
	const uint32_t t = threadIdx.x, k = t & 15u, row = t >> 4;
	constexpr uint32_t rows = GYS_HR_NT / 16u;
	ulonglong2 ident;
	ident.x = 0ull;
	ident.y = k < 15u ? 0ull : (unsigned long long)INT64_MIN;
	for (uint32_t ch = blockIdx.x; ch < q.nchunks; ch += gridDim.x) {
		const uint32_t m0 = q.chunks[ch].m0, m1 = q.chunks[ch].m1;
		ulonglong2 acc = ident;
		uint32_t j = m0 + row;
		for (; j < m1 && m1 - j > (GYS_HP_INFLIGHT - 1u) * rows; j += GYS_HP_INFLIGHT * rows) { // the members' indices, then every load of theirs, then the adds
			uint32_t s[GYS_HP_INFLIGHT];
#pragma unroll
			for (uint32_t i = 0; i < GYS_HP_INFLIGHT; ++i) s[i] = q.members[j + i * rows];
			PeriodPair in[GYS_HP_INFLIGHT];
#pragma unroll
			for (uint32_t i = 0; i < GYS_HP_INFLIGHT; ++i) in[i] = period_pair_load<true>(q.v, s[i], k);
#pragma unroll
			for (uint32_t i = 0; i < GYS_HP_INFLIGHT; ++i) acc = pair_add(acc, period_pair_value(q.v, in[i], k), k);
		}
		for (; j < m1; j += rows) {
			const PeriodPair in = period_pair_load<true>(q.v, q.members[j], k);
			acc = pair_add(acc, period_pair_value(q.v, in, k), k);
		}
		red[t] = acc;
		__syncthreads();
		ulonglong2 r = ident;
		if (t < 16u) {
			r = red[t];
#pragma unroll
			for (uint32_t g = 1; g < rows; ++g) r = pair_add(r, red[g * 16u + t], k);
		}
		__syncthreads(); // (every column is read: red takes the joined pairs)
		if (t < 15u) red[t] = r;
		__syncthreads();
		if (t == 15u) { // total_count = the sum of the 15 joined counts
#pragma unroll
			for (uint32_t b = 0; b < 15u; ++b) r.x += red[b].x;
		}
		if (t < 16u) ((ulonglong2 *)q.dst)[(uint64_t)ch * 16ull + t] = r;
		__syncthreads(); // (red is written again in the next turn)
	}
}

} // namespace gys
