// gys_svcresol.hpp -- issue resolution: which listener is the SOURCE of a dependent-listener issue, and what did each source take down
// (gys_svc_resolve_issues / _dev).  The reference resolves ISSUE_DEPENDENT_SERVER_LISTENER every 5 s with a serial recursive hash walk
// per source under RCU (MCONN_HANDLER::handle_dependency_issue, server/gy_mconnhdlr.cc:10866-10990, at most
// MM_LISTENER_ISSUE_RESOL::MAX_DOWNSTREAM_TIERS = 8 tiers).  The definition is frozen in include/gysketch.h ("Issue resolution").  Needs
// gys_svcdeps.hpp (the pair array of k_dep_edges<false>) in front of it.
//
// A labelled multi-source search over the pairs (u, v) = "u calls v": an issue travels from a callee v to its callers u.  Every level
// is TWO launches, so that the word a launch tests is never written in that launch -- there is no race to argue about, and the minimum
// of a slot is complete before anything reads it:
//   k_resol_seed    per slot: (state, issue) from the kept 96-byte state entry under the currency rule of svc_load_current
//                   (gys_svcquery.hpp), or from the caller's gys_listener_decision array; word[slot] = tier byte | class | state | issue
//                   (tier 0 for a SOURCE, RS_UNSET for a DEPENDENT or CARRIER, RS_BLOCKED for the rest), best[slot] = all-ones,
//                   nres[slot] = 0.
//   k_resol_level   per pair: the callee stands at `level`, the caller is RS_UNSET: atomicMin(best[caller], source(callee) << 32 | callee).
//                   The 64-bit minimum IS the tie rule (lowest source slot, then lowest via slot) whatever the order of the atomics.
//                   word[] is only read.  best[callee] is read, best[caller] is written: a callee is settled, a caller is not.
//   k_resol_settle  per slot: RS_UNSET with a best word becomes tier level + 1; a DEPENDENT adds 1 to nres[its source].  The count is
//                   taken here and not at the end, so that the record of a slot -- nresolved included -- leaves in one store.
//   k_resol_finish  per slot: the 16-byte gys_svc_resol as ONE 16-byte store, the impact column, the counters (a ballot per tile and
//                   counter, the sums in registers until the end as k_dep_edges keeps its row counters; then summed per workgroup in LDS).
//   k_resol_rows    the host form: the records whose role is in the mask as gys_svc_resol_row, compacted with k_dep_collect's tile cursor.
#pragma once

namespace gys {

// counter words of the resolution calls (unsigned long long each)
enum { RSC_WITH_STATE = 0, RSC_SOURCES, RSC_RESOLVED, RSC_UNRESOLVED, RSC_CARRIERS, RSC_TIER0 /* .. RSC_TIER0 + 7 */, RSC_CURSOR = RSC_TIER0 + 8, RSC_NUM = 16 };

// word[slot]: bits 0..7 the tier (0 .. 8, RS_UNSET, RS_BLOCKED), 8..15 the class, 16..23 the state, 24..31 the issue
#define RS_UNSET 0xFFu
#define RS_BLOCKED 0xFEu
enum { RS_CL_NOSTATE = 0, RS_CL_OPAQUE, RS_CL_SOURCE, RS_CL_DEPENDENT, RS_CL_CARRIER };
#define RS_NOBEST 0xFFFFFFFFFFFFFFFFull
#define RS_ISSUE_DEPENDENT 7u // ISSUE_DEPENDENT_SERVER_LISTENER

struct ResolSeedP {
	const uint8_t *svc_state;         // [nsvc * 96]
	const uint32_t *svc_host;         // [nsvc] (GYS_NOSLOT: a free slot)
	const uint64_t *svc_gid;          // [nsvc]
	const gys_listener_decision *dec; // [nsvc] or nullptr = the kept states
	uint32_t nsvc, epoch;
	uint32_t *word;                   // [nsvc]
	unsigned long long *best;         // [nsvc]
	uint32_t *nres;                   // [nsvc]
};

__host__ __device__ __forceinline__ uint32_t resol_class(bool has, uint32_t state, uint32_t issue)
{
	if (!has || state > 5u) return RS_CL_NOSTATE;
	if (state >= 3u) return issue == RS_ISSUE_DEPENDENT ? RS_CL_DEPENDENT : RS_CL_SOURCE;
	return state == 2u ? RS_CL_CARRIER : RS_CL_OPAQUE;
}

__global__ __launch_bounds__(256) void k_resol_seed(ResolSeedP p)
{
	for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < p.nsvc; s += gridDim.x * blockDim.x) {
		const uint32_t host = p.svc_host[s];
		bool has = host != GYS_NOSLOT;
		uint32_t state = 0, issue = 0;
		if (has && p.dec) {
			state = p.dec[s].state;
			issue = p.dec[s].issue;
		} else if (has) {
			// words 0..1 the record's id, 19 (byte 79) and 20 (byte 80), 22 the window it was kept in (0: deleted / never), 23 its host
			const uint4 *q = (const uint4 *)(p.svc_state + (size_t)s * 96);
			const uint4 a = q[0], e = q[4], f = q[5];
			const uint64_t gid = (uint64_t)a.x | ((uint64_t)a.y << 32);
			has = f.z != 0u && f.z + 1u >= p.epoch && f.w == host && gid == p.svc_gid[s];
			state = e.w >> 24;
			issue = f.x & 0xFFu;
		}
		const uint32_t cl = resol_class(has, state, issue);
		if (cl == RS_CL_NOSTATE) state = issue = 0u;
		const uint32_t tier = cl == RS_CL_SOURCE ? 0u : (cl == RS_CL_DEPENDENT || cl == RS_CL_CARRIER) ? RS_UNSET : RS_BLOCKED;
		p.word[s] = tier | (cl << 8) | (state << 16) | (issue << 24);
		p.best[s] = RS_NOBEST;
		p.nres[s] = 0u;
	}
}

// (nsvc bounds every index, whatever the pair array holds, as in k_dep_level; a self edge names one slot, which cannot both stand at
// `level` and be unset)
__global__ __launch_bounds__(256) void k_resol_level(const uint2 *pairs, uint64_t nedges, const uint32_t *word, unsigned long long *best, uint32_t nsvc, uint32_t level)
{
	for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nedges; e += (uint64_t)gridDim.x * blockDim.x) {
		const uint2 pr = pairs[e];
		if (pr.x >= nsvc || pr.y >= nsvc) continue;
		if ((word[pr.y] & 0xFFu) != level || (word[pr.x] & 0xFFu) != RS_UNSET) continue;
		const uint32_t src = level ? (uint32_t)(best[pr.y] >> 32) : pr.y;
		atomicMin(&best[pr.x], ((unsigned long long)src << 32) | (unsigned long long)pr.y);
	}
}

__global__ __launch_bounds__(256) void k_resol_settle(uint32_t *word, const unsigned long long *best, uint32_t *nres, uint32_t nsvc, uint32_t level)
{
	for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nsvc; s += gridDim.x * blockDim.x) {
		const uint32_t w = word[s];
		if ((w & 0xFFu) != RS_UNSET) continue;
		const unsigned long long b = best[s];
		if (b == RS_NOBEST) continue;
		word[s] = (w & ~0xFFu) | (level + 1u);
		const uint32_t src = (uint32_t)(b >> 32);
		if (((w >> 8) & 0xFFu) == RS_CL_DEPENDENT && src < nsvc) atomicAdd(&nres[src], 1u);
	}
}

struct ResolFinP {
	const uint32_t *word;           // [nsvc]
	const unsigned long long *best; // [nsvc]
	const uint32_t *nres;           // [nsvc]
	uint32_t nsvc;
	gys_svc_resol *out;             // [nsvc], 16-byte aligned
	double *impact;                 // [nsvc] or nullptr
	unsigned long long *ctr;        // [RSC_NUM]
};

// the record of a slot from its word, its best word and its count
__host__ __device__ __forceinline__ gys_svc_resol resol_record(uint32_t slot, uint32_t w, unsigned long long b, uint32_t nres)
{
	const uint32_t tier = w & 0xFFu, cl = (w >> 8) & 0xFFu;
	gys_svc_resol r;
	r.src_slot = r.via_slot = GYS_NOSLOT;
	r.role = GYS_RS_NONE;
	r.tier = 0;
	r.state = (uint8_t)(w >> 16);
	r.issue = (uint8_t)(w >> 24);
	r.nresolved = 0u;
	if (cl == RS_CL_SOURCE) {
		r.role = GYS_RS_SOURCE;
		r.src_slot = slot;
		r.nresolved = nres;
	} else if ((cl == RS_CL_DEPENDENT || cl == RS_CL_CARRIER) && tier <= GYS_RESOL_MAX_TIERS) {
		r.role = cl == RS_CL_DEPENDENT ? GYS_RS_RESOLVED : GYS_RS_CARRIER;
		r.tier = (uint8_t)tier;
		r.src_slot = (uint32_t)(b >> 32);
		r.via_slot = (uint32_t)b;
	} else if (cl == RS_CL_DEPENDENT) {
		r.role = GYS_RS_UNRESOLVED;
	}
	return r;
}

// The counters: 13 words that every wave of the launch adds to.  One atomic per WAVE and word, as k_dep_edges counts its rows, was
// 0.45 ms of a 1.7 ms call at 10^6 slots (8 192 waves on the same 13 words); the waves of a workgroup are summed in LDS first and the
// launch is half as wide as the other slot passes (the engine side), which leaves a few thousand atomics: 0.023 ms
// (profiles/svcresol_timing.txt).
__global__ __launch_bounds__(256) void k_resol_finish(ResolFinP p)
{
	__shared__ unsigned long long s_ctr[RSC_CURSOR];
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t n_state = 0, n_role[5] = {0, 0, 0, 0, 0}, n_tier[GYS_RESOL_MAX_TIERS] = {0, 0, 0, 0, 0, 0, 0, 0};
	if (threadIdx.x < RSC_CURSOR) s_ctr[threadIdx.x] = 0ull;
	__syncthreads();
	for (uint32_t base = blockIdx.x * blockDim.x; base < p.nsvc; base += gridDim.x * blockDim.x) {
		const uint32_t s = base + threadIdx.x;
		const bool in = s < p.nsvc;
		uint32_t w = RS_BLOCKED; // (class RS_CL_NOSTATE: counts nowhere)
		gys_svc_resol r;
		r.role = GYS_RS_NONE;
		r.tier = 0;
		if (in) {
			w = p.word[s];
			r = resol_record(s, w, p.best[s], p.nres[s]);
			uint4 q;
			q.x = r.src_slot;
			q.y = r.via_slot;
			q.z = (uint32_t)r.role | ((uint32_t)r.tier << 8) | ((uint32_t)r.state << 16) | ((uint32_t)r.issue << 24);
			q.w = r.nresolved;
			((uint4 *)p.out)[s] = q;
			if (p.impact) p.impact[s] = r.role == GYS_RS_SOURCE ? (double)r.nresolved : __builtin_nan("");
		}
		n_state += (uint32_t)__popcll(__ballot(((w >> 8) & 0xFFu) != RS_CL_NOSTATE));
#pragma unroll
		for (uint32_t k = 1; k <= 4; ++k) n_role[k] += (uint32_t)__popcll(__ballot(r.role == k));
#pragma unroll
		for (uint32_t t = 0; t < GYS_RESOL_MAX_TIERS; ++t) n_tier[t] += (uint32_t)__popcll(__ballot(r.role == GYS_RS_RESOLVED && r.tier == t + 1u));
	}
	if (lane == 0u) {
		if (n_state) atomicAdd(&s_ctr[RSC_WITH_STATE], (unsigned long long)n_state);
		if (n_role[GYS_RS_SOURCE]) atomicAdd(&s_ctr[RSC_SOURCES], (unsigned long long)n_role[GYS_RS_SOURCE]);
		if (n_role[GYS_RS_RESOLVED]) atomicAdd(&s_ctr[RSC_RESOLVED], (unsigned long long)n_role[GYS_RS_RESOLVED]);
		if (n_role[GYS_RS_UNRESOLVED]) atomicAdd(&s_ctr[RSC_UNRESOLVED], (unsigned long long)n_role[GYS_RS_UNRESOLVED]);
		if (n_role[GYS_RS_CARRIER]) atomicAdd(&s_ctr[RSC_CARRIERS], (unsigned long long)n_role[GYS_RS_CARRIER]);
#pragma unroll
		for (uint32_t t = 0; t < GYS_RESOL_MAX_TIERS; ++t)
			if (n_tier[t]) atomicAdd(&s_ctr[RSC_TIER0 + t], (unsigned long long)n_tier[t]);
	}
	__syncthreads();
	if (threadIdx.x < RSC_CURSOR && s_ctr[threadIdx.x]) atomicAdd(&p.ctr[threadIdx.x], s_ctr[threadIdx.x]);
}

struct ResolRowsP {
	const gys_svc_resol *rec; // [nsvc]
	const uint64_t *svc_gid;  // [nsvc]
	const uint32_t *svc_host; // [nsvc] (GYS_NOSLOT: a free slot, its id reads 0)
	uint32_t nsvc, role_mask;
	gys_svc_resol_row *out;   // [cap]
	uint32_t cap;
	unsigned long long *cursor;
};

// the records whose role is in the mask into out[0 .. cap) in any order (k_dep_collect's tile cursor); *cursor += their number
__global__ __launch_bounds__(256) void k_resol_rows(ResolRowsP p)
{
	__shared__ uint32_t s_wcnt[2][4];
	__shared__ unsigned long long s_base[2];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t par = 0;
	for (uint32_t base = blockIdx.x * blockDim.x; base < p.nsvc; base += gridDim.x * blockDim.x, par ^= 1u) {
		const uint32_t s = base + threadIdx.x;
		gys_svc_resol r;
		r.role = 0xFFu;
		if (s < p.nsvc) r = p.rec[s];
		const bool hit = r.role <= 4u && ((p.role_mask >> r.role) & 1u);
		const unsigned long long b = __ballot(hit);
		if (lane == 0u) s_wcnt[par][wave] = (uint32_t)__popcll(b);
		__syncthreads();
		if (threadIdx.x == 0u) {
			const uint32_t tot = s_wcnt[par][0] + s_wcnt[par][1] + s_wcnt[par][2] + s_wcnt[par][3];
			s_base[par] = tot ? atomicAdd(p.cursor, (unsigned long long)tot) : 0ull;
		}
		__syncthreads();
		unsigned long long at = s_base[par] + (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
		for (uint32_t w = 0; w < wave; ++w) at += s_wcnt[par][w];
		if (!hit || at >= p.cap) continue;
		gys_svc_resol_row o;
		o.glob_id = p.svc_host[s] != GYS_NOSLOT ? p.svc_gid[s] : 0ull;
		o.src_glob_id = o.via_glob_id = 0ull;
		o.slot = s;
		o.src_slot = r.src_slot;
		o.via_slot = r.via_slot;
		o.nresolved = r.nresolved;
		o.role = r.role;
		o.tier = r.tier;
		o.state = r.state;
		o.issue = r.issue;
		o.src_state = o.src_issue = 0;
		o.pad[0] = o.pad[1] = 0;
		if (r.src_slot < p.nsvc) { // (a source is a registered slot with a state)
			const gys_svc_resol sr = p.rec[r.src_slot];
			o.src_glob_id = p.svc_gid[r.src_slot];
			o.src_state = sr.state;
			o.src_issue = sr.issue;
		}
		if (r.via_slot < p.nsvc) o.via_glob_id = p.svc_gid[r.via_slot];
		p.out[at] = o;
	}
}

} // namespace gys
