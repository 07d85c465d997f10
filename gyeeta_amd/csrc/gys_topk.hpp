// gys_topk.hpp -- exact top-k of a column of doubles on the device (gys_topk_dev, gys_top_services): which services or groups a scan's
// results name.  The definition is frozen in include/gysketch.h ("Top-k"): NaNs are not eligible, -0.0 equals +0.0, larger (or smaller)
// value first, then the LOWER row number; the answer is a function of the set of rows alone.
//   k_topk_keys    grid-stride over tiles of 1024 rows in the shape of k_svc_filter (256 threads, four rows per thread, one list-cursor atomic
//                  per workgroup and tile): the row number, the strided value and the weight; the eligible rows go, compacted, into the
//                  candidate list as {key, row}.  key = the 64-bit order-preserving image of the value (-0.0 first mapped to +0.0; sign bit
//                  set for the non-negative values, all bits flipped for the negative ones), complemented for "smallest": largest key first
//                  is the order either way.
//   k_svc_hist / k_svc_pick (gys_svcquery.hpp), unchanged: six rounds on the keys when more rows are eligible than k.  They leave the threshold
//                  image T and `want`, the number of rows with image T still to be taken.
//   k_topk_ties    the keys are not unique: the rows with image T become a second key list, 0xFFFFFFFF - row (unique), on which three more
//                  rounds of the same pair (11 + 11 + 10 bits) find the `want` lowest row numbers.  Linear in the number of ties.
//   k_topk_gather  the candidates above T and the tie rows at or above the tie threshold, compacted as {row, value bits, weight} for the host
//                  to order.
//   k_top_metric   gys_top_services: the metric column and the weight column from the scans' outputs.
#pragma once

namespace gys {

enum { TOPK_LARGEST = 0, TOPK_SMALLEST = 1 };

struct TopkEntry { // gys_topk_entry
	uint32_t row, reserved;
	unsigned long long vbits; // the column's stored bits
	unsigned long long weight;
};

// the stored bits of a double that is no NaN -> a key that orders as the real numbers do (-0.0 == +0.0), largest key first for either order
__host__ __device__ __forceinline__ unsigned long long topk_key(unsigned long long bits, uint32_t smallest)
{
	if (bits == 0x8000000000000000ull) bits = 0ull;
	const unsigned long long img = (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
	return smallest ? ~img : img;
}
__host__ __device__ __forceinline__ bool topk_is_nan(unsigned long long bits) { return (bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }

struct TopkKeysP {
	const unsigned long long *col; // the column as stored bits
	uint32_t stride, nrows;
	const uint32_t *rows;            // nullptr: rows 0 .. nrows - 1
	const unsigned long long *weight; // by row number; may be nullptr
	unsigned long long min_weight;
	uint32_t smallest;
	unsigned long long *cand_key; // [nrows]
	uint32_t *cand_row;           // [nrows]
	uint32_t *cursor;             // [0] candidates so far
};

__global__ __launch_bounds__(GYS_SVCQ_THREADS) void k_topk_keys(TopkKeysP p)
{
	__shared__ uint32_t s_wave[GYS_SVCQ_THREADS / 64u];
	__shared__ uint32_t s_base;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	constexpr uint32_t TILE = GYS_SVCQ_THREADS * GYS_SVCQ_PER_THREAD;
	const uint32_t ntiles = p.nrows / TILE + (p.nrows % TILE ? 1u : 0u);
	for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (uniform trip count per workgroup)
		const uint32_t first = tile * TILE; // (first < nrows)
		unsigned long long keys[GYS_SVCQ_PER_THREAD];
		uint32_t rws[GYS_SVCQ_PER_THREAD];
		uint32_t mine = 0; // bit k: row k of this thread is eligible
#pragma unroll
		for (uint32_t k = 0; k < GYS_SVCQ_PER_THREAD; ++k) {
			const uint32_t off = k * GYS_SVCQ_THREADS + threadIdx.x;
			keys[k] = 0;
			rws[k] = 0;
			if (off < p.nrows - first) {
				const uint32_t row = p.rows ? p.rows[first + off] : first + off;
				const unsigned long long bits = p.col[(size_t)row * p.stride];
				const bool heavy = !p.weight || p.weight[row] >= p.min_weight;
				rws[k] = row;
				if (heavy && !topk_is_nan(bits)) {
					keys[k] = topk_key(bits, p.smallest);
					mine |= 1u << k;
				}
			}
		}
		const uint32_t cnt = (uint32_t)__popc(mine);
		uint32_t incl = cnt;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
			if ((int)lane >= d) incl += o;
		}
		if (lane == 63u) s_wave[wave] = incl;
		__syncthreads();
		if (threadIdx.x == 0) {
			uint32_t tot = 0;
			for (uint32_t k = 0; k < GYS_SVCQ_THREADS / 64u; ++k) {
				const uint32_t c = s_wave[k];
				s_wave[k] = tot;
				tot += c;
			}
			s_base = tot ? atomicAdd(p.cursor, tot) : 0u;
		}
		__syncthreads();
		uint32_t at = s_base + s_wave[wave] + incl - cnt; // (at most nrows rows are eligible: inside the lists)
#pragma unroll
		for (uint32_t k = 0; k < GYS_SVCQ_PER_THREAD; ++k) {
			if (mine & (1u << k)) {
				p.cand_key[at] = keys[k];
				p.cand_row[at] = rws[k];
				++at;
			}
		}
		__syncthreads(); // (s_wave / s_base are rewritten by the next trip)
	}
}

// the place of the lanes of a workgroup of 256 that have `take` set in a list with the cursor `cursor`: one atomic per workgroup and call.
// Every thread of the workgroup calls; two barriers.
__device__ __forceinline__ uint32_t topk_wg_place(bool take, uint32_t *cursor, uint32_t *s_wave, uint32_t *s_base)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const unsigned long long b = __ballot(take);
	const uint32_t before = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
	if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(b);
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t tot = 0;
		for (uint32_t k = 0; k < 4u; ++k) {
			const uint32_t c = s_wave[k];
			s_wave[k] = tot;
			tot += c;
		}
		*s_base = tot ? atomicAdd(cursor, tot) : 0u;
	}
	__syncthreads();
	return *s_base + s_wave[wave] + before;
}

struct TopkTiesP {
	const unsigned long long *cand_key;
	const uint32_t *cand_row;
	const uint32_t *ncand;
	const unsigned long long *threshold; // T
	unsigned long long *tie_key;         // [candidates]: 0xFFFFFFFF - row of the candidates with key T
	uint32_t *ntie;                      // [0] cursor
};

__global__ __launch_bounds__(256) void k_topk_ties(TopkTiesP p)
{
	__shared__ uint32_t s_wave[4];
	__shared__ uint32_t s_base;
	const uint32_t n = *p.ncand;
	const unsigned long long thr = *p.threshold;
	for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n; i0 += (uint64_t)gridDim.x * blockDim.x) { // (uniform trip count per workgroup)
		const uint64_t i = i0 + threadIdx.x;
		const bool take = i < n && p.cand_key[i] == thr;
		const uint32_t at = topk_wg_place(take, p.ntie, s_wave, &s_base);
		if (take) p.tie_key[at] = (unsigned long long)(0xFFFFFFFFu - p.cand_row[i]); // (at < the number of ties <= n)
		__syncthreads();
	}
}

struct TopkGatherP {
	const unsigned long long *col;
	uint32_t stride;
	const unsigned long long *weight;
	const unsigned long long *cand_key;
	const uint32_t *cand_row;
	const uint32_t *ncand;
	const unsigned long long *threshold;     // T: keys above it are taken; nullptr = every candidate
	const unsigned long long *tie_threshold; // ... and of the keys equal to T the rows with 0xFFFFFFFF - row >= *tie_threshold
	uint32_t maxout;
	uint32_t *out_count;
	TopkEntry *out; // [maxout]
};

__global__ __launch_bounds__(256) void k_topk_gather(TopkGatherP p)
{
	__shared__ uint32_t s_wave[4];
	__shared__ uint32_t s_base;
	const uint32_t n = *p.ncand;
	const unsigned long long thr = p.threshold ? *p.threshold : 0ull, tthr = p.threshold ? *p.tie_threshold : 0ull;
	for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n; i0 += (uint64_t)gridDim.x * blockDim.x) { // (uniform trip count per workgroup)
		const uint64_t i = i0 + threadIdx.x;
		bool take = false;
		uint32_t row = 0;
		if (i < n) {
			const unsigned long long key = p.cand_key[i];
			row = p.cand_row[i];
			take = !p.threshold || key > thr || (key == thr && (unsigned long long)(0xFFFFFFFFu - row) >= tthr);
		}
		const uint32_t at = topk_wg_place(take, p.out_count, s_wave, &s_base);
		if (take && at < p.maxout) {
			TopkEntry e;
			e.row = row;
			e.reserved = 0;
			e.vbits = p.col[(size_t)row * p.stride];
			e.weight = p.weight ? p.weight[row] : 0ull;
			p.out[at] = e;
		}
		__syncthreads();
	}
}

// gys_top_services: the metric column and the eligibility weight of every service slot from the scans' outputs (in place)
enum { TOP_QUANTILE = 0, TOP_SHARE_WITHIN = 1, TOP_MISSES = 2, TOP_DISTINCT = 3 };

struct TopMetricP {
	int metric;               // TOP_SHARE_WITHIN / TOP_MISSES: col = below / total, total - below; TOP_DISTINCT: weight = the slot is not free
	uint32_t nsvc;
	const double *below;      // [nsvc] (the rank metrics)
	const uint32_t *svc_host; // [nsvc] (TOP_DISTINCT; GYS_NOSLOT: a free slot)
	double *col;              // [nsvc] out (the rank metrics)
	unsigned long long *weight; // [nsvc] in: the totals (the rank metrics); out (TOP_DISTINCT)
};

__global__ __launch_bounds__(256) void k_top_metric(TopMetricP p)
{
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < p.nsvc; i += gridDim.x * blockDim.x) {
		if (p.metric == TOP_DISTINCT) {
			p.weight[i] = p.svc_host[i] != GYS_NOSLOT ? 1ull : 0ull;
		} else {
			const double total = (double)p.weight[i], below = p.below[i];
			p.col[i] = p.metric == TOP_SHARE_WITHIN ? below / total : total - below; // (total 0: not eligible, whatever stands here)
		}
	}
}

} // namespace gys
