// Distinct-flow counts from the per-service HyperLogLog registers (gys_config.svc_hll_p, written by svc_hll_update in the event kernels):
// the estimate of every service, and the register files + estimates of GROUPS of services (a host, a cluster, all hosts of this rank, any
// list of files).  Definitions (oracle/gy_oracle.h: gyo_hll_merge, gyo_hll_estimate):
//   a register FILE is m = 1 << p bytes, byte i = the largest rank seen for register i;
//   the file of a group is the byte-wise maximum of its members' files (order does not matter; no member: all zero);
//   the estimate of a file is Flajolet's raw estimator alpha m^2 / sum 2^-rank, and linear counting m ln(m / zeros) when the raw value is
//   <= 2.5 m and a register is zero.  The all-zero file gives exactly 0.
// ONE ESTIMATOR: sum 2^-rank is kept as exact integers -- ranks <= 32 in units of 2^-32, ranks above in units of 2^-64, the zero count in
// the spare high bits of the first word -- through every lane and every reduction step, and turned into a double at one place
// (hll_finish).  The estimate is therefore a pure function of the file's bytes: the same bits whichever lanes, workgroup or launch
// shape looked at it.
// Two kernels, both plain streaming kernels with one 16-byte load per lane:
//   k_hll_estimate  n files -> n doubles.  m / 16 lanes per file (p = 4: one lane, p = 10: a wave), partial sums joined by the DPP steps
//                   of gys_device.hpp cut off at the file's width.  Reads n m bytes, writes 8 n.
//   k_hll_union     a workgroup per chunk of members (RollupChunk, the lists the digest roll-up keeps), the running byte-wise maximum in
//                   registers, four files in flight per lane, the workgroup's rows joined through LDS; one file out per chunk.  Groups
//                   of several chunks: the chunks' files are the members of a second launch (maximum is idempotent and commutative:
//                   no atomics, no pre-zeroed output).  Reads (members) m bytes + 4 per listed member, writes (chunks) m.
#pragma once

namespace gys {

#define GYS_HLL_NT 256u          // threads of a workgroup of either kernel
#define GYS_HLL_ZSHIFT 48        // the zero count sits above the low word's sum (at most 1024 * 2^32 = 2^42)

// the 16 registers of one 16-byte piece: lo += 2^(32 - rank) for rank <= 32 (+ 1 << GYS_HLL_ZSHIFT for rank 0), hi += 2^(64 - rank) above.
// 1024 registers: lo's sum < 2^43, hi < 2^41, zeros <= 1024 -- no overflow, no carry into the zero count.  A byte above 64 (no hash has
// such a rank; a caller's file may hold anything) counts as 64.
__device__ __forceinline__ void hll_acc_word(uint32_t w, uint64_t &lo, uint64_t &hi)
{
#pragma unroll
	for (int b = 0; b < 4; ++b) {
		uint32_t r = (w >> (8 * b)) & 0xffu;
		r = r > 64u ? 64u : r;
		lo += r <= 32u ? ((1ull << ((32u - r) & 63u)) | (r == 0u ? 1ull << GYS_HLL_ZSHIFT : 0ull)) : 0ull;
		hi += r > 32u ? 1ull << ((64u - r) & 63u) : 0ull;
	}
}

// THE conversion to floating point (the only one): the same arithmetic as gyo_hll_estimate on an exactly known sum
__device__ __forceinline__ double hll_finish(uint64_t lo, uint64_t hi, uint32_t p)
{
	const uint32_t zeros = (uint32_t)(lo >> GYS_HLL_ZSHIFT);
	lo &= (1ull << GYS_HLL_ZSHIFT) - 1ull;
	const uint32_t m = 1u << p;
	const double sum = (double)lo * 0x1p-32 + (double)hi * 0x1p-64;
	const double alpha = m == 16 ? 0.673 : (m == 32 ? 0.697 : (m == 64 ? 0.709 : 0.7213 / (1.0 + 1.079 / (double)m)));
	double e = alpha * (double)m * (double)m / sum;
	if (e <= 2.5 * (double)m && zeros) e = (double)m * log((double)m / (double)zeros);
	return e;
}

// sums over aligned groups of 1 << lg lanes (lg <= 6, the same in every lane), valid in the LAST lane of each group.  Device: the first lg
// of the six DPP steps of GYS_DPP_STEP (row_shr 1 / 2 / 4 / 8 give every lane the sum of the 2 / 4 / 8 / 16 lanes ending at it, inside its row
// of 16; row_bcast:15 and :31 join the rows), on both halves of the 64-bit words.  All 64 lanes must be active.
__device__ __forceinline__ void hll_group_sum(uint64_t &lo, uint64_t &hi, uint32_t lg)
{
#ifdef __HIP_DEVICE_COMPILE__
#define GYS_HLL_DPP(ctrl, rmask)                                                                                                  \
	do {                                                                                                                      \
		const uint32_t a0_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)lo, ctrl, rmask, 0xf, false);         \
		const uint32_t a1_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(lo >> 32), ctrl, rmask, 0xf, false); \
		const uint32_t b0_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)hi, ctrl, rmask, 0xf, false);         \
		const uint32_t b1_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(hi >> 32), ctrl, rmask, 0xf, false); \
		lo += (uint64_t)a0_ | ((uint64_t)a1_ << 32);                                                                      \
		hi += (uint64_t)b0_ | ((uint64_t)b1_ << 32);                                                                      \
	} while (0)
	if (lg >= 1) GYS_HLL_DPP(0x111, 0xf); // row_shr:1
	if (lg >= 2) GYS_HLL_DPP(0x112, 0xf); // row_shr:2
	if (lg >= 3) GYS_HLL_DPP(0x114, 0xf); // row_shr:4
	if (lg >= 4) GYS_HLL_DPP(0x118, 0xf); // row_shr:8
	if (lg >= 5) GYS_HLL_DPP(0x142, 0xa); // row_bcast:15 -> rows 1, 3
	if (lg >= 6) GYS_HLL_DPP(0x143, 0xc); // row_bcast:31 -> rows 2, 3
#undef GYS_HLL_DPP
#else
	const uint32_t pos = threadIdx.x & ((1u << lg) - 1u);
	for (uint32_t d = 1; d < (1u << lg); d <<= 1) {
		const uint64_t a = __shfl_up(lo, d, 64), b = __shfl_up(hi, d, 64);
		if (pos >= d) {
			lo += a;
			hi += b;
		}
	}
#endif
}

// out[f] = estimate of file f, f < n.  files: 16-byte aligned, n << p bytes.  4 <= p <= 10.
__global__ __launch_bounds__(GYS_HLL_NT) void k_hll_estimate(const uint8_t *__restrict__ files, uint32_t n, uint32_t p, double *__restrict__ out)
{
	const uint32_t lg = p - 4u, lane = threadIdx.x & 63u;
	const uint64_t npieces = (uint64_t)n << lg, stride = (uint64_t)gridDim.x * GYS_HLL_NT;
	// the loop runs on the wave's first piece: every lane of a wave makes the same number of turns (the DPP steps need all 64), and a file
	// never straddles two waves (64 is a multiple of the lanes per file)
	for (uint64_t base = (uint64_t)blockIdx.x * GYS_HLL_NT + (threadIdx.x & ~63u); base < npieces; base += stride) {
		const uint64_t i = base + lane;
		uint64_t lo = 0, hi = 0;
		if (i < npieces) {
			const uint4 v = ((const uint4 *)files)[i];
			hll_acc_word(v.x, lo, hi);
			hll_acc_word(v.y, lo, hi);
			hll_acc_word(v.z, lo, hi);
			hll_acc_word(v.w, lo, hi);
		}
		hll_group_sum(lo, hi, lg);
		if (i < npieces && (i & ((1u << lg) - 1u)) == (1u << lg) - 1u) out[i >> lg] = hll_finish(lo, hi, p);
	}
}

// byte-wise unsigned maximum of two words of four bytes (any byte values)
__device__ __forceinline__ uint32_t hll_max4(uint32_t a, uint32_t b)
{
	const uint32_t H = 0x80808080u;
	const uint32_t ge7 = ((a | H) - (b & ~H)) & H;                       // per byte: low seven bits of a >= those of b
	const uint32_t ge = ((a & ~b) | (~(a ^ b) & ge7)) & H;                 // a's top bit alone set, or the top bits equal and the rest decides
	const uint32_t mask = (ge >> 7) * 0xffu;
	return (a & mask) | (b & ~mask);
}
__device__ __forceinline__ uint4 hll_max16(uint4 a, uint4 b)
{
	return make_uint4(hll_max4(a.x, b.x), hll_max4(a.y, b.y), hll_max4(a.z, b.z), hll_max4(a.w, b.w));
}

struct HllUnionP {
	const uint8_t *src;        // the members' files (16-byte aligned)
	uint8_t *dst;              // one file per CHUNK: dst[chunk index]
	const RollupChunk *chunks; // nullptr: chunk i = members [i * per, min(n, (i + 1) * per))
	const uint32_t *members;   // index of a member's file in src; nullptr: member j = file j
	uint32_t nchunks, n, per, p;
};

__global__ __launch_bounds__(GYS_HLL_NT) void k_hll_union(HllUnionP q)
{
	__shared__ uint4 red[GYS_HLL_NT];
	const uint32_t lg = q.p - 4u, L = 1u << lg, t = threadIdx.x, piece = t & (L - 1u), row = t >> lg, rows = GYS_HLL_NT >> lg;
	const uint4 *src = (const uint4 *)q.src + piece;
	for (uint32_t ch = blockIdx.x; ch < q.nchunks; ch += gridDim.x) {
		uint32_t m0, m1;
		if (q.chunks) {
			m0 = q.chunks[ch].m0;
			m1 = q.chunks[ch].m1;
		} else {
			m0 = ch * q.per;
			m1 = q.n - m0 < q.per ? q.n : m0 + q.per;
		}
		uint4 acc = make_uint4(0u, 0u, 0u, 0u);
		uint32_t j = m0 + row;
		for (; j < m1 && m1 - j > 3u * rows; j += 4u * rows) { // four members of this lane's row: their indices, then their pieces, all requested before the first is used
			uint32_t s0 = j, s1 = j + rows, s2 = j + 2u * rows, s3 = j + 3u * rows;
			if (q.members) {
				s0 = q.members[s0];
				s1 = q.members[s1];
				s2 = q.members[s2];
				s3 = q.members[s3];
			}
			const uint4 v0 = src[(uint64_t)s0 << lg], v1 = src[(uint64_t)s1 << lg], v2 = src[(uint64_t)s2 << lg], v3 = src[(uint64_t)s3 << lg];
			acc = hll_max16(hll_max16(acc, v0), hll_max16(hll_max16(v1, v2), v3));
		}
		for (; j < m1; j += rows) {
			const uint32_t s = q.members ? q.members[j] : j;
			acc = hll_max16(acc, src[(uint64_t)s << lg]);
		}
		red[t] = acc;
		__syncthreads();
		for (uint32_t s = GYS_HLL_NT / 2u; s >= L; s >>= 1) { // rows t and t + s hold the same piece (s is a multiple of L)
			if (t < s) red[t] = hll_max16(red[t], red[t + s]);
			__syncthreads();
		}
		if (t < L) ((uint4 *)q.dst)[((uint64_t)ch << lg) + t] = red[t];
		__syncthreads(); // (red is written again in the next turn)
	}
}

// ------------------------------------------------------------------------------------------------ levels (gys_config.svc_hll_levels)
// The registers of CLOSED windows for the four horizons of the histogram levels (5 s / 300 s / 5 days / all; the definition is in
// include/gysketch.h).  A byte-wise maximum cannot be subtracted, so the 300-s and the 5-day level keep real ring buckets.  State:
// GYS_HLL_LVL_FILES arrays of [max_services] files, bucket-major (a bucket of all services is one contiguous array):
//   array 0 = the window closed last, 1 .. 10 = the 300-s ring, 11 .. 20 = the 5-day ring, 21 = every closed window.
// Two more streaming kernels, 16 bytes per lane, no atomics, no LDS:
//   k_hll_level_roll  the window close.  Per 16-byte piece of every open file: the two current ring buckets and `all` take the maximum with
//                     it, `last` becomes it, the open file is cleared.  A piece that is all zero changes none of the three maxima and is
//                     already clear: only `last` is written for it (1 piece read, 1 written).  Otherwise 4 pieces read + 5 written
//                     (144 B per service at p = 4).  A current bucket whose ring slot has just expired (fresh) is written without being
//                     read.  The host clears the OTHER expired buckets with memsets before the launch.
//   k_hll_level_view  a level's files at query time: the byte-wise maximum of the buckets in `mask` (all their loads requested before the
//                     first is used; mask 0: all zero), stored as files and / or turned into estimates by the arithmetic of k_hll_estimate
//                     (hll_acc_word -> hll_group_sum -> hll_finish: the same bits for the same bytes).  Reads popcount(mask) m per service.
#define GYS_HLL_LVL_LAST 0u
#define GYS_HLL_LVL_RING 1u                                   // + (level - 1) * GYS_LEVEL_RING + bucket
#define GYS_HLL_LVL_ALL (1u + 2u * GYS_LEVEL_RING)
#define GYS_HLL_LVL_FILES (2u + 2u * GYS_LEVEL_RING)

struct HllLevelRollP {
	uint4 *open;                      // the open window's files, [npieces] pieces of 16 bytes (cleared)
	uint4 *last, *ring1, *ring2, *all; // the same pieces of `last`, of the two CURRENT ring buckets and of `all`
	uint64_t npieces;                 // nsvc << (p - 4)
	uint32_t fresh1, fresh2;          // the current bucket of the 300-s / 5-day ring is in the clear mask: written, not read
};

__global__ __launch_bounds__(GYS_HLL_NT) void k_hll_level_roll(HllLevelRollP q)
{
	const uint64_t stride = (uint64_t)gridDim.x * GYS_HLL_NT;
	const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
	for (uint64_t i = (uint64_t)blockIdx.x * GYS_HLL_NT + threadIdx.x; i < q.npieces; i += stride) {
		const uint4 o = q.open[i];
		const bool any = (o.x | o.y | o.z | o.w) != 0u;
		uint4 a = zero, b = zero, g = zero;
		if (any) { // (three loads in flight)
			if (!q.fresh1) a = q.ring1[i];
			if (!q.fresh2) b = q.ring2[i];
			g = q.all[i];
		}
		q.last[i] = o;
		if (any || q.fresh1) q.ring1[i] = hll_max16(a, o);
		if (any || q.fresh2) q.ring2[i] = hll_max16(b, o);
		if (any) {
			q.all[i] = hll_max16(g, o);
			q.open[i] = zero;
		}
	}
}

struct HllLevelViewP {
	const uint8_t *base; // bucket j of the level = the array at base + j * stride; the file of slot s sits at + (s << p) inside it
	uint64_t stride;     // bytes between two buckets (max_services << p)
	uint32_t mask;       // the live buckets (bit j, j < GYS_LEVEL_RING); levels 0 and 3: the one array, or nothing
	uint32_t first, n, p; // slots [first, first + n)
	uint8_t *files;      // [n] files (16-byte aligned), or nullptr
	double *est;         // [n] estimates, or nullptr
};

__global__ __launch_bounds__(GYS_HLL_NT) void k_hll_level_view(HllLevelViewP q)
{
	const uint32_t lg = q.p - 4u, lane = threadIdx.x & 63u;
	const uint64_t npieces = (uint64_t)q.n << lg, stride = (uint64_t)gridDim.x * GYS_HLL_NT, stride16 = q.stride / 16u;
	const uint4 *src = (const uint4 *)q.base + ((uint64_t)q.first << lg);
	// (the loop of k_hll_estimate: every lane of a wave makes the same number of turns, a file never straddles two waves)
	for (uint64_t base = (uint64_t)blockIdx.x * GYS_HLL_NT + (threadIdx.x & ~63u); base < npieces; base += stride) {
		const uint64_t i = base + lane;
		uint64_t lo = 0, hi = 0;
		if (i < npieces) {
			uint4 v[GYS_LEVEL_RING];
#pragma unroll
			for (uint32_t j = 0; j < GYS_LEVEL_RING; ++j) v[j] = (q.mask >> j) & 1u ? src[(uint64_t)j * stride16 + i] : make_uint4(0u, 0u, 0u, 0u);
			uint4 acc = v[0];
#pragma unroll
			for (uint32_t j = 1; j < GYS_LEVEL_RING; ++j) acc = hll_max16(acc, v[j]);
			if (q.files) ((uint4 *)q.files)[i] = acc;
			hll_acc_word(acc.x, lo, hi);
			hll_acc_word(acc.y, lo, hi);
			hll_acc_word(acc.z, lo, hi);
			hll_acc_word(acc.w, lo, hi);
		}
		if (!q.est) continue; // (the same in every lane)
		hll_group_sum(lo, hi, lg);
		if (i < npieces && (i & ((1u << lg) - 1u)) == (1u << lg) - 1u) q.est[i >> lg] = hll_finish(lo, hi, q.p);
	}
}

} // namespace gys
