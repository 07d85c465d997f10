// Ranks: how many of a digest's recorded values are <= x, for every service slot or for any slabs -- the inverse of the quantile calls
// (gys_query_ranks, gys_scan_ranks_dev, gys_tdigest_slab_ranks_dev).  Builder-defined, parity unpinned like the t-digest itself; the
// definition is frozen in include/gysketch.h ("Ranks") and DESIGN.md section 4:
//   below(x) = r(x) + nb(x): nb = the buffered values <= x, counted EXACTLY; r = the clusters' share, 0 below the overall minimum, N at and
//   above the overall maximum, otherwise ONE interpolation between the centres c = W + cnt / 2 of the two non-empty clusters whose means
//   enclose x + 1/2 (minimum - 1/2 / maximum + 1/2 at the ends) -- the inverse of td_quantile_interp and its half-up rounding.  Which clusters
//   these are is decided in exact integers (sum - floor(cnt / 2) <= x cnt), the weight before a cluster is an exact integer, and the few
//   double operations happen once, in one lane, in a fixed order:
//   the answer does not depend on the launch shape and a restatement in any language gives the same bits.
// One kernel, k_td_ranks: a wave per member, grid-stride, nothing but loads, wave operations and the member's output row -- no LDS, no atomics,
// no scratch buffer of the engine, no write-back, outputs need not be zeroed (the service instances spill a few registers: 0 - 28 B of private
// scratch per lane, profiles/td_ranks_timing.txt).  The load pattern is k_rollup_accum's (gys_rollup.hpp): the member's buffer fill is
// read one member ahead and the first 16-byte pieces of its buffered values are requested before its clusters are looked at.
//   clusters   lane l holds clusters l, l + 64, l + 128, l + 192 and their inclusive weight prefix (four 64-bit DPP scans); per threshold four
//              ballots of "non-empty and mean <= x + 1/2" give the greatest such cluster j (highest bit) and, with the ballots of "non-empty", the
//              next non-empty cluster n (lowest bit above): lane t keeps the pair of threshold t.  After the last threshold every lane < nt
//              fetches its two clusters' {sum, cnt, prefix} from the lanes that hold them and does the arithmetic of its threshold.
//   buffered   each lane counts the values <= x_t it sees, two thresholds to a 32-bit counter (a buffer holds fewer than 2^16 values), and takes
//              their minimum / maximum on the way; DPP reductions join the lanes.  Staged words are value << GYS_ROW_BITS | ...: the value counts.
//              No fold is needed: td_minmax without it lies between the overall and the merged extreme (k_fold and the merges only ever widen
//              it by values of the buffer), so min(td_minmax.x, min P) is the overall minimum either way.
// And the quantile direction for slabs, k_td_slab_quantiles (gys_tdigest_slab_quantiles_dev), at the end of this file: the same shape, the
// arithmetic of the one-slab host call gys_tdigest_slab_quantiles.
#pragma once

#include <type_traits>

namespace gys {

#define GYS_TR_NT 256u   // threads of a workgroup: four waves, each walks members of its own
#define GYS_TR_MAXT 16u  // thresholds per call at most
#define GYS_TR_AHEAD 2u  // 16-byte pieces per lane of a member's buffered values requested before its clusters (as GYS_RB_AHEAD)
#define GYS_TR_ROWS ((GYS_TD_NB + 63u) / 64u)

struct TdRankP {
	DigestP d;                  // KIND 0: members are service slots
	const gys_tdigest_slab *in; // KIND 1: members are slabs
	uint32_t first, n;          // members [first, first + n); member m writes row m - first
	uint32_t nt;
	int64_t thr[GYS_TR_MAXT];
	double *below;              // [n][nt]
	unsigned long long *total;  // [n], may be nullptr
};

// sum - floor(cnt / 2) <= x cnt in exact integers (the mean is at most x + 1/2), x = (xneg ? -xabs : xabs), cnt != 0: sign and magnitude on
// both sides -- the left one has at most 64 bits of magnitude, the right one is a 128-bit product
template <class CNT>
__device__ __forceinline__ bool tr_mean_le(int64_t sum, CNT cnt, bool xneg, uint64_t xabs)
{
	const uint64_t hi = __umul64hi(xabs, (uint64_t)cnt), lo = xabs * (uint64_t)cnt, half = (uint64_t)cnt >> 1;
	const bool sneg = sum < (int64_t)half; // (half < 2^63)
	const uint64_t smag = sum < 0 ? (0ull - (uint64_t)sum) + half : (sneg ? half - (uint64_t)sum : (uint64_t)sum - half);
	if (!xneg) return sneg || hi != 0ull || smag <= lo;
	return sneg && hi == 0ull && smag >= lo;
}

// lane 63's value (after an inclusive scan: the wave's total) in every lane
__device__ __forceinline__ uint64_t tr_last_u64(uint64_t v)
{
#ifdef __HIP_DEVICE_COMPILE__
	return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63) | ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63) << 32);
#else
	return __shfl(v, 63, 64);
#endif
}

// r[idx / 64] of lane idx % 64, idx a value of the calling lane's own (every lane of the wave calls)
__device__ __forceinline__ uint32_t tr_fetch(const uint32_t (&r)[GYS_TR_ROWS], uint32_t idx)
{
	uint32_t out = 0;
#pragma unroll
	for (uint32_t k = 0; k < GYS_TR_ROWS; ++k) {
		const uint32_t v = (uint32_t)__shfl((int)r[k], (int)(idx & 63u), 64);
		if ((idx >> 6) == k) out = v;
	}
	return out;
}
__device__ __forceinline__ uint64_t tr_fetch(const uint64_t (&r)[GYS_TR_ROWS], uint32_t idx)
{
	uint32_t lo[GYS_TR_ROWS], hi[GYS_TR_ROWS];
#pragma unroll
	for (uint32_t k = 0; k < GYS_TR_ROWS; ++k) {
		lo[k] = (uint32_t)r[k];
		hi[k] = (uint32_t)(r[k] >> 32);
	}
	return (uint64_t)tr_fetch(lo, idx) | ((uint64_t)tr_fetch(hi, idx) << 32);
}

// KIND 0: service slots (32-bit counts, buffered values), 1: slabs (64-bit counts).  TP: the pairs of thresholds the buffered values are
// counted for (1, 2, 4 or 8 >= nt / 2; slabs: 1, unused)
template <int KIND, uint32_t TP>
__global__ __launch_bounds__(GYS_TR_NT, TP >= 8u ? 5 : (TP >= 4u ? 6 : 8)) void k_td_ranks(TdRankP q)
{
	typedef typename std::conditional<KIND == 0, uint32_t, uint64_t>::type cnt_t;
	const DigestP &p = q.d;
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	constexpr uint32_t NW = GYS_TR_NT / 64u;
	const uint32_t stride = gridDim.x * NW, end = q.first + q.n;
	const bool quads = KIND == 0 && (p.pcap & 3u) == 0u; // 16 bytes per lane and request

	// the buffered values are compared as 32-bit integers (a value has 26 bits): thresholds below -1 / above INT32_MAX count none / all alike
	int32_t xs[2u * TP];
#pragma unroll
	for (uint32_t t = 0; t < 2u * TP; ++t) {
		const int64_t x = t < q.nt ? q.thr[t] : -1ll;
		xs[t] = x < -1ll ? -1 : (x > (int64_t)INT32_MAX ? INT32_MAX : (int32_t)x);
	}

	uint32_t mem_n = q.first + blockIdx.x * NW + wave, npend_n = 0;
	if (KIND == 0 && mem_n < end) npend_n = min(p.td_meta[mem_n].npend, p.pend_cap); // (between batches a buffer holds at most pend_cap values)
	while (mem_n < end) {
		const uint32_t mem = mem_n, npend = npend_n;
		mem_n += stride;
		if (KIND == 0 && mem_n < end) npend_n = min(p.td_meta[mem_n].npend, p.pend_cap);
		const uint32_t *pend = p.td_pend + (size_t)mem * p.pcap;
		uint4 va[GYS_TR_AHEAD];
#pragma unroll
		for (uint32_t k = 0; k < GYS_TR_AHEAD; ++k) {
			va[k] = make_uint4(0, 0, 0, 0);
			if (quads && 4u * lane + 256u * k < npend) va[k] = ((const uint4 *)pend)[lane + 64u * k];
		}
		// ---- the member's clusters: lane l holds l + 64 k
		cnt_t cn[GYS_TR_ROWS];
		uint64_t sm[GYS_TR_ROWS];
#pragma unroll
		for (uint32_t k = 0; k < GYS_TR_ROWS; ++k) {
			const uint32_t j = lane + 64u * k;
			cn[k] = 0;
			sm[k] = 0;
			if (j < GYS_TD_NB) {
				if (KIND == 0) {
					cn[k] = (cnt_t)p.td_cnt[(size_t)mem * GYS_TD_NB + j];
					sm[k] = (uint64_t)p.td_sum[(size_t)mem * GYS_TD_NB + j];
				} else {
					cn[k] = (cnt_t)q.in[mem].cnt[j];
					sm[k] = (uint64_t)q.in[mem].sum[j];
				}
			}
		}
		long long vmn, vmx;
		if (KIND == 0) {
			const int2 mm = p.td_minmax[mem];
			vmn = mm.x;
			vmx = mm.y;
		} else {
			vmn = q.in[mem].vmin;
			vmx = q.in[mem].vmax;
		}
		// ---- a service's buffered values, while the clusters are on their way: how many are <= each threshold, their minimum and maximum
		uint32_t nb = 0;
		int32_t pmin = INT32_MAX, pmax = INT32_MIN;
		if (KIND == 0 && npend) {
			uint32_t cpk[TP];
#pragma unroll
			for (uint32_t k = 0; k < TP; ++k) cpk[k] = 0;
			auto one = [&](uint32_t word) {
				const int32_t v = (int32_t)(word >> GYS_ROW_BITS);
				pmin = min(pmin, v);
				pmax = max(pmax, v);
#pragma unroll
				for (uint32_t k = 0; k < TP; ++k) cpk[k] += (v <= xs[2u * k] ? 1u : 0u) + (v <= xs[2u * k + 1u] ? 0x10000u : 0u);
			};
			auto quad = [&](const uint4 w4, uint32_t i) {
				if (i + 3u < npend) { // (all but the buffer's last quad)
					one(w4.x);
					one(w4.y);
					one(w4.z);
					one(w4.w);
				} else {
					if (i < npend) one(w4.x);
					if (i + 1u < npend) one(w4.y);
					if (i + 2u < npend) one(w4.z);
				}
			};
			if (quads) {
#pragma unroll
				for (uint32_t k = 0; k < GYS_TR_AHEAD; ++k) quad(va[k], 4u * lane + 256u * k);
#pragma unroll 2
				for (uint32_t i = 4u * lane + 256u * GYS_TR_AHEAD; i < npend; i += 256u) quad(((const uint4 *)pend)[i >> 2], i);
			} else {
#pragma unroll 4
				for (uint32_t i = lane; i < npend; i += 64u) one(pend[i]);
			}
			pmin = wave_min_i32(pmin);
			pmax = wave_max_i32(pmax);
#pragma unroll
			for (uint32_t k = 0; k < TP; ++k) {
				const uint32_t s = wave_sum_u32(cpk[k]);
				if (lane == 2u * k) nb = s & 0xFFFFu;
				if (lane == 2u * k + 1u) nb = s >> 16;
			}
		}
		unsigned long long ne[GYS_TR_ROWS];
#pragma unroll
		for (uint32_t k = 0; k < GYS_TR_ROWS; ++k) ne[k] = __ballot(cn[k] != 0);
		// ---- per threshold: a = the greatest non-empty cluster whose mean is at most x + 1/2 (tr_mean_le; -1: none), b = the next non-empty one (-1: a is the last)
		int my_a = -1, my_b = -1;
		int64_t my_x = 0;
		for (uint32_t t = 0; t < q.nt; ++t) {
			const int64_t x = q.thr[t];
			const bool xneg = x < 0;
			const uint64_t xabs = xneg ? 0ull - (uint64_t)x : (uint64_t)x;
			int a = -1, b = -1;
#pragma unroll
			for (uint32_t k = 0; k < GYS_TR_ROWS; ++k) {
				const unsigned long long le = __ballot(cn[k] != 0 && tr_mean_le<cnt_t>((int64_t)sm[k], cn[k], xneg, xabs));
				if (le) a = (int)(64u * k) + 63 - __clzll((long long)le);
			}
#pragma unroll
			for (uint32_t k = 0; k < GYS_TR_ROWS; ++k) {
				const int base = (int)(64u * k);
				unsigned long long m = ne[k];
				if (a >= base + 63) m = 0ull;
				else if (a >= base) m &= ~0ull << (uint32_t)(a - base + 1);
				if (b < 0 && m) b = base + __ffsll((long long)m) - 1;
			}
			if (lane == t) {
				my_a = a;
				my_b = b;
				my_x = x;
			}
		}
		// ---- the weight up to and including every cluster, in index order (exact integers)
		uint64_t pfx[GYS_TR_ROWS], N = 0;
#pragma unroll
		for (uint32_t k = 0; k < GYS_TR_ROWS; ++k) {
			const uint64_t inc = wave_incl_scan_u64((uint64_t)cn[k]);
			pfx[k] = N + inc;
			N += tr_last_u64(inc);
		}
		// ---- lane t: its two clusters from the lanes that hold them, then the arithmetic of threshold t
		const uint32_t ia = my_a < 0 ? 0u : (uint32_t)my_a, ib = my_b < 0 ? 0u : (uint32_t)my_b;
		const uint64_t sa = tr_fetch(sm, ia), pa = tr_fetch(pfx, ia), sb = tr_fetch(sm, ib);
		const uint64_t ca = (uint64_t)tr_fetch(cn, ia), cb = (uint64_t)tr_fetch(cn, ib);
		if (lane < q.nt) {
			double r;
			const long long lo = KIND == 0 && (long long)pmin < vmn ? (long long)pmin : vmn, hi = KIND == 0 && (long long)pmax > vmx ? (long long)pmax : vmx;
			if (N == 0ull || my_x < lo) {
				r = 0.0;
			} else if (my_x >= hi) {
				r = (double)N;
			} else {
				const double y = (double)my_x + 0.5; // an integer value v stands for [v - 1/2, v + 1/2]
				if (my_a < 0) { // below the first mean: from the minimum to the first centre
					const double cf = (double)0ull + (double)cb * 0.5, mf = (double)(int64_t)sb / (double)cb, dlo = (double)lo - 0.5;
					r = cf * ((y - dlo) / (mf - dlo));
				} else {
					const double cj = (double)(pa - ca) + (double)ca * 0.5, mj = (double)(int64_t)sa / (double)ca;
					if (my_b < 0) { // at or above the last mean: from the last centre to the maximum
						const double dhi = (double)hi + 0.5;
						r = cj + ((double)N - cj) * ((y - mj) / (dhi - mj));
					} else {
						const double cnx = (double)pa + (double)cb * 0.5, mn = (double)(int64_t)sb / (double)cb;
						r = cj + (cnx - cj) * ((y - mj) / (mn - mj));
					}
				}
			}
			q.below[(size_t)(mem - q.first) * q.nt + lane] = N == 0ull ? (double)nb : r + (double)nb;
		}
		if (q.total && lane == 0u) q.total[mem - q.first] = N + npend;
	}
}

// ---- quantiles of any number of slabs (gys_tdigest_slab_quantiles_dev): k_td_ranks<1, .>'s shape the other way round.  A wave per slab,
// grid-stride; lane l holds clusters l + 64 k and their exact integer weight prefix; the centres c_k = (double)W_k + (double)cnt_k * 0.5 are
// those of the one-slab host call (gys_tdigest_slab_quantiles), which adds the weights up in doubles: the same numbers while a slab weighs
// less than 2^53.  Per quantile the ballots of "non-empty and t < c_k" give the first such cluster f (lowest bit) and, with the ballots of
// "non-empty", the last non-empty cluster before it (highest bit below f; the last of all when there is no f): lane t keeps the pair of
// quantile t, fetches the two clusters from the lanes that hold them and does the host call's double operations in its order.  Loads, wave
// operations and the slab's output row only: no LDS, no atomics, outputs need not be zeroed.
struct TdSlabQP {
	const gys_tdigest_slab *in;
	uint32_t n, nq;         // slab i writes out[i * nq .. + nq)
	double q[GYS_TR_MAXT];
	double *out;
};

__global__ __launch_bounds__(GYS_TR_NT) void k_td_slab_quantiles(TdSlabQP q)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
	constexpr uint32_t NW = GYS_TR_NT / 64u;
	const uint32_t stride = gridDim.x * NW;
	for (uint32_t mem = blockIdx.x * NW + wave; mem < q.n; mem += stride) {
		uint64_t cn[GYS_TR_ROWS], sm[GYS_TR_ROWS];
#pragma unroll
		for (uint32_t k = 0; k < GYS_TR_ROWS; ++k) {
			const uint32_t j = lane + 64u * k;
			cn[k] = 0;
			sm[k] = 0;
			if (j < GYS_TD_NB) {
				cn[k] = q.in[mem].cnt[j];
				sm[k] = (uint64_t)q.in[mem].sum[j];
			}
		}
		const long long vmn = q.in[mem].vmin, vmx = q.in[mem].vmax;
		unsigned long long ne[GYS_TR_ROWS];
		uint64_t pfx[GYS_TR_ROWS], N = 0;
		double cc[GYS_TR_ROWS];
#pragma unroll
		for (uint32_t k = 0; k < GYS_TR_ROWS; ++k) {
			ne[k] = __ballot(cn[k] != 0);
			const uint64_t inc = wave_incl_scan_u64(cn[k]);
			pfx[k] = N + inc;
			N += tr_last_u64(inc);
			cc[k] = (double)(pfx[k] - cn[k]) + (double)cn[k] * 0.5;
		}
		const double dN = (double)N;
		// ---- per quantile: f = the first non-empty cluster with t < c_f (-1: none), pv = the last non-empty cluster before it (-1: f is the first)
		int my_f = -1, my_p = -1;
		double my_t = 0.0;
		for (uint32_t t = 0; t < q.nq; ++t) {
			const double qv = q.q[t], qq = qv < 0.0 ? 0.0 : (qv > 1.0 ? 1.0 : qv), tq = qq * dN;
			int f = -1, pv = -1;
#pragma unroll
			for (uint32_t k = 0; k < GYS_TR_ROWS; ++k) {
				const unsigned long long lt = __ballot(cn[k] != 0 && tq < cc[k]);
				if (f < 0 && lt) f = (int)(64u * k) + __ffsll((long long)lt) - 1;
			}
#pragma unroll
			for (uint32_t k = 0; k < GYS_TR_ROWS; ++k) {
				const int base = (int)(64u * k);
				unsigned long long m = ne[k];
				if (f >= 0) {
					if (f < base) m = 0ull;
					else if (f < base + 64) m &= (1ull << (uint32_t)(f - base)) - 1ull;
				}
				if (m) pv = base + 63 - __clzll((long long)m);
			}
			if (lane == t) {
				my_f = f;
				my_p = pv;
				my_t = tq;
			}
		}
		// ---- lane t: its two clusters from the lanes that hold them, then the arithmetic of quantile t
		const uint32_t jf = my_f < 0 ? 0u : (uint32_t)my_f, jp = my_p < 0 ? 0u : (uint32_t)my_p;
		const uint64_t sf = tr_fetch(sm, jf), cf = tr_fetch(cn, jf), pf = tr_fetch(pfx, jf);
		const uint64_t sp = tr_fetch(sm, jp), cp = tr_fetch(cn, jp), pp = tr_fetch(pfx, jp);
		if (lane < q.nq) {
			double r = 0.0;
			if (N) {
				double prev_mean = 0.0, prev_c = 0.0;
				if (my_p >= 0) {
					prev_mean = (double)(int64_t)sp / (double)cp;
					prev_c = (double)(pp - cp) + (double)cp * 0.5;
				}
				if (my_f >= 0) {
					const double mean = (double)(int64_t)sf / (double)cf, cf_c = (double)(pf - cf) + (double)cf * 0.5;
					if (my_p < 0) {
						const double lo = (double)vmn;
						r = cf_c <= 0.0 ? mean : lo + (mean - lo) * (my_t / cf_c);
					} else {
						r = prev_mean + (mean - prev_mean) * ((my_t - prev_c) / (cf_c - prev_c));
					}
				} else {
					const double hi = (double)vmx, span = dN - prev_c;
					r = span <= 0.0 ? hi : prev_mean + (hi - prev_mean) * ((my_t - prev_c) / span);
				}
				r = floor(r + 0.5);
			}
			q.out[(size_t)mem * q.nq + lane] = r;
		}
	}
}

} // namespace gys
