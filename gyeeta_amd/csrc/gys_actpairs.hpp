// gys_actpairs.hpp -- the LIVE (listener, client task group) rows of ACTIVE_CONN_STATS as an exact keyed table on the device
// (gys_config.actconn_pair_cap; gys_actconn_list / _list_dev / _svc_stats_dev / _table_stats, gys_json_activeconn).  The reference keeps
// these rows in activeconntbl / remoteconntbl (insert_active_conns, server/gy_mconnhdlr.cc:7780-7928) and the Active Conn query reads the
// rows of the last 25 s (server/gy_mnodehandle.cc:3699-3735); the Count-Min pair of k_actconn_ingest can only be asked about a pair the
// caller already knows.  The definition of an entry is frozen in include/gysketch.h ("Live active-connection rows").
//
// Layout: open addressing on a power-of-two table of >= 2 x cap entries, linear probing.  A KEY is three words -- listener_glob_id_,
// cli_aggr_task_id_, kind (0 = local listener, 1 = is_remote_listen_) -- in an array of its own (all bits set = free); the entry's figures
// lie in a second array (all zero = never reported).  Home entry: jhash2_4w of the four id words, seeded by the kind.
//
// NO THREAD EVER WAITS FOR ANOTHER.  A key is claimed word by word with compare-and-swap from "free": listener id, then client id, then
// kind.  A word, once set, never changes while the table lives, so a thread that finds another value in any of the three moves on to the
// next entry for good; a thread that finds a word free sets it, a thread that finds its own value goes on to the next word.  An entry
// whose first word was set by one key and whose second by another (same listener, two clients racing) simply belongs to the second; the
// first key's thread moves on.  Whoever sets a word also attempts the next, so no entry is left half claimed at the end of a kernel, and
// all rows of one key end at the same entry (they walk the same probe sequence and pass only entries that can never become theirs).
// Every probe loop ends after `entries` steps; a row that finds no place is dropped and counted, never retried.
//
// A call's rows run three passes (a reset-then-add needs an order between the rows of a call):
//   find   k_actp_find   the row's entry (found or inserted) into row_ent[i]; atomicMax of i + 1 on the entry's claim word
//   keep   k_actp_keep   the row that holds the claim (the call's highest-index row of the key: the claim pattern of k_lstate_ingest /
//                        k_lstate_keep) clears the claim, resets the figures of an entry last reported in an OLDER window (a newer report
//                        replaces, it does not add), stamps the window and stores the descriptive fields of its own row, whole
//   add    k_actp_add    every row adds its counts (atomicAdd), raises the maxima (atomicMax; floats compared as non-negative bit patterns,
//                        a negative or NaN value counting as 0.0f) and ORs its flag bits
// k_actp_all is the three in one workgroup for calls of <= GYS_ACTP_FUSED_MAX rows (a partha's report is <= 2 048 rows, typically far
// fewer), the passes separated by workgroup barriers as in k_lstate_both.
//
// Dead entries are reclaimed by k_actp_rebuild: the live entries are re-inserted into the table's second buffer (distinct keys: the thread
// that inserts one owns the new entry) and counted; the host side decides when (gys_actpairs_host.hpp).
#pragma once

namespace gys {

#define GYS_ACTP_FUSED_MAX 1024u
#define GYS_ACTP_NOENT 0xFFFFFFFFu
#define GYS_ACTP_SEED 0x5bd1e995u
#define GYS_ACTP_NOKIND 0xFFFFFFFFu

struct ActPairKey { // 24 bytes; all bits set = free
	unsigned long long lid, cid;
	uint32_t kind, spare;
};

struct ActPairEnt { // 104 bytes; all zero = never reported
	uint32_t claim;  // i + 1 of the call's highest-index row of the key between the find and the keep pass, 0 otherwise
	uint32_t window; // the window of the latest report (0 = none)
	uint32_t active_conns, nrows;
	unsigned long long bytes_sent, bytes_received;
	uint32_t cli_delay_msec, ser_delay_msec, rtt_bits, flags;
	unsigned long long desc[7]; // row words 2 .. 8: ser_comm_, cli_comm_, remote_machine_id_, remote_madhava_id_
};

struct ActPairTbl {
	ActPairKey *key;
	ActPairEnt *ent;
	uint32_t mask; // entries - 1
};

// counter words of a table (unsigned long long each)
enum { APC_OCCUPIED = 0, APC_DROPPED, APC_BADKEY, APC_MATCH, APC_NUM = 8 };

__host__ __device__ __forceinline__ uint32_t actp_home(uint64_t lid, uint64_t cid, uint32_t kind, uint32_t mask)
{
	return jhash2_4w((uint32_t)lid, (uint32_t)(lid >> 32), (uint32_t)cid, (uint32_t)(cid >> 32), GYS_ACTP_SEED + kind) & mask;
}

// an entry is LIVE while epoch - window <= GYS_ACT_RING: the open window and the three closed before it (the "last report" rule of k_act_latch)
__host__ __device__ __forceinline__ bool actp_live(uint32_t window, uint32_t epoch) { return window != 0u && window <= epoch && epoch - window <= GYS_ACT_RING; }

// the key's entry, inserted if it is not there; GYS_ACTP_NOENT when `entries` probes found no place
__device__ __forceinline__ uint32_t actp_find_insert(const ActPairTbl &t, uint64_t lid, uint64_t cid, uint32_t kind, unsigned long long *ctr)
{
	uint32_t h = actp_home(lid, cid, kind, t.mask);
#pragma unroll 1
	for (uint32_t probes = 0; probes <= t.mask; ++probes, h = (h + 1u) & t.mask) {
		ActPairKey *k = &t.key[h];
		// (a plain read first: a set word never changes, so a value that is neither free nor ours settles it without an atomic; a stale
		// "free" is put right by the compare-and-swap)
		unsigned long long a = k->lid;
		if (a == GYS_EMPTY_KEY) {
			a = atomicCAS(&k->lid, (unsigned long long)GYS_EMPTY_KEY, (unsigned long long)lid);
			if (a == GYS_EMPTY_KEY) {
				atomicAdd(&ctr[APC_OCCUPIED], 1ull);
				a = lid;
			}
		}
		if (a != lid) continue;
		a = k->cid;
		if (a == GYS_EMPTY_KEY) {
			a = atomicCAS(&k->cid, (unsigned long long)GYS_EMPTY_KEY, (unsigned long long)cid);
			if (a == GYS_EMPTY_KEY) a = cid;
		}
		if (a != cid) continue;
		uint32_t b = k->kind;
		if (b == GYS_ACTP_NOKIND) {
			b = atomicCAS(&k->kind, GYS_ACTP_NOKIND, kind);
			if (b == GYS_ACTP_NOKIND) b = kind;
		}
		if (b != kind) continue;
		return h;
	}
	return GYS_ACTP_NOENT;
}

struct ActPairP {
	const uint8_t *batch; // 104-byte rows (comm::ACTIVE_CONN_STATS, layout at k_actconn_ingest)
	uint32_t n;
	ActPairTbl t;
	uint32_t epoch;     // the open window
	uint32_t *row_ent;  // [n] the rows' entries between the passes (the fused form keeps them in registers)
	unsigned long long *ctr; // [APC_NUM]
};

// a float's bits as a non-negative value: negative and NaN count as 0.0f
__host__ __device__ __forceinline__ uint32_t actp_rtt_bits(uint32_t bits) { return ((bits >> 31) || (bits & 0x7FFFFFFFu) > 0x7F800000u) ? 0u : bits; }

__device__ __forceinline__ uint32_t actp_find_one(const ActPairP &p, uint32_t i)
{
	const uint64_t *q = (const uint64_t *)(p.batch + (size_t)i * 104u);
	const uint64_t lid = q[0], cid = q[1];
	const uint32_t kind = (uint32_t)((q[12] >> 49) & 1ull); // flags byte @102, is_remote_listen_ = bit 1
	if (lid == GYS_EMPTY_KEY || cid == GYS_EMPTY_KEY) { // (the table's free marker cannot be a key)
		atomicAdd(&p.ctr[APC_BADKEY], 1ull);
		return GYS_ACTP_NOENT;
	}
	const uint32_t e = actp_find_insert(p.t, lid, cid, kind, p.ctr);
	if (e == GYS_ACTP_NOENT) {
		atomicAdd(&p.ctr[APC_DROPPED], 1ull);
		return e;
	}
	atomicMax(&p.t.ent[e].claim, i + 1u);
	return e;
}

__device__ __forceinline__ void actp_keep_one(const ActPairP &p, uint32_t i, uint32_t e)
{
	if (e == GYS_ACTP_NOENT) return;
	ActPairEnt *d = &p.t.ent[e];
	if (atomicMax(&d->claim, 0u) != i + 1u) return; // (read where the find pass's atomics landed)
	d->claim = 0u; // (no other row of the call matches i + 1, nor 0)
	if (d->window != p.epoch) {
		d->active_conns = 0u;
		d->nrows = 0u;
		d->bytes_sent = 0ull;
		d->bytes_received = 0ull;
		d->cli_delay_msec = 0u;
		d->ser_delay_msec = 0u;
		d->rtt_bits = 0u;
		d->flags = 0u;
		d->window = p.epoch;
	}
	const uint64_t *q = (const uint64_t *)(p.batch + (size_t)i * 104u);
#pragma unroll
	for (int k = 0; k < 7; ++k) d->desc[k] = q[2 + k];
}

__device__ __forceinline__ void actp_add_one(const ActPairP &p, uint32_t i, uint32_t e)
{
	if (e == GYS_ACTP_NOENT) return;
	ActPairEnt *d = &p.t.ent[e];
	const uint64_t *q = (const uint64_t *)(p.batch + (size_t)i * 104u);
	const uint64_t sent = q[9], rcvd = q[10], w11 = q[11], w12 = q[12];
	const uint32_t act = (uint32_t)((w12 >> 32) & 0xFFFFu), flags = (uint32_t)((w12 >> 48) & 0xFFu);
	const uint32_t cdel = (uint32_t)w11, sdel = (uint32_t)(w11 >> 32), rtt = actp_rtt_bits((uint32_t)w12);
	atomicAdd(&d->nrows, 1u);
	if (act) atomicAdd(&d->active_conns, act);
	if (sent) atomicAdd(&d->bytes_sent, (unsigned long long)sent);
	if (rcvd) atomicAdd(&d->bytes_received, (unsigned long long)rcvd);
	if (cdel) atomicMax(&d->cli_delay_msec, cdel);
	if (sdel) atomicMax(&d->ser_delay_msec, sdel);
	if (rtt) atomicMax(&d->rtt_bits, rtt);
	if (flags) atomicOr(&d->flags, flags);
}

__global__ __launch_bounds__(256) void k_actp_find(ActPairP p)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < p.n) p.row_ent[i] = actp_find_one(p, i);
}

__global__ __launch_bounds__(256) void k_actp_keep(ActPairP p)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < p.n) actp_keep_one(p, i, p.row_ent[i]);
}

__global__ __launch_bounds__(256) void k_actp_add(ActPairP p)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < p.n) actp_add_one(p, i, p.row_ent[i]);
}

// a call of <= GYS_ACTP_FUSED_MAX rows in ONE launch: the three passes by one workgroup (device-scope atomics and stores made visible by the
// fence in front of each barrier, read back by threads of the same workgroup)
__global__ __launch_bounds__(GYS_ACTP_FUSED_MAX) void k_actp_all(ActPairP p)
{
	const uint32_t i = threadIdx.x;
	uint32_t e = GYS_ACTP_NOENT;
	if (i < p.n) e = actp_find_one(p, i);
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
	__syncthreads();
	if (i < p.n) actp_keep_one(p, i, e);
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
	__syncthreads();
	if (i < p.n) actp_add_one(p, i, e);
}

// the live entries of `from` into `to` (cleared by the caller, as is to_ctr[APC_OCCUPIED], which ends as the number of live entries)
__global__ __launch_bounds__(256) void k_actp_rebuild(ActPairTbl from, ActPairTbl to, uint32_t epoch, unsigned long long *to_ctr)
{
	const uint32_t n = from.mask + 1u;
	for (uint32_t h = blockIdx.x * blockDim.x + threadIdx.x; h < n; h += gridDim.x * blockDim.x) {
		const ActPairKey k = from.key[h];
		if (k.lid == GYS_EMPTY_KEY || k.cid == GYS_EMPTY_KEY || k.kind == GYS_ACTP_NOKIND) continue;
		const ActPairEnt v = from.ent[h];
		if (!actp_live(v.window, epoch)) continue;
		const uint32_t e = actp_find_insert(to, k.lid, k.cid, k.kind, to_ctr);
		if (e == GYS_ACTP_NOENT) { // (cannot happen: `to` has as many entries as `from`)
			atomicAdd(&to_ctr[APC_DROPPED], 1ull);
			continue;
		}
		to.ent[e] = v;
	}
}

// ---------------------------------------------------------------------------------------------------- queries
struct ActPairListP {
	ActPairTbl t;
	uint32_t epoch;
	DevTable gid;             // glob_id -> service slot, as it is NOW
	const uint32_t *svc_host; // [nsvc]
	uint32_t nsvc;
	gys_actconn_sel sel;
	gys_actconn_row *out; // [cap]; may be nullptr with cap 0
	uint32_t cap;
	unsigned long long *count; // += the matches
};

__device__ __forceinline__ bool actp_entry(const ActPairTbl &t, uint32_t h, uint32_t epoch, ActPairKey &k, ActPairEnt &v)
{
	k = t.key[h];
	if (k.lid == GYS_EMPTY_KEY || k.cid == GYS_EMPTY_KEY || k.kind == GYS_ACTP_NOKIND) return false;
	v = t.ent[h];
	return actp_live(v.window, epoch);
}

// every workgroup walks whole tiles of 256 entries, so that its waves stay together: the matches of a TILE take their places in the output
// with ONE returning atomic on the count -- a million matches on one address, wave by wave, were 0.8 ms of serialised atomics.  The waves'
// counts and the tile's base go through LDS words that alternate between two sets from trip to trip (a wave two trips ahead cannot exist:
// it would have passed a barrier the slowest wave has not reached)
__global__ __launch_bounds__(256) void k_actp_list(ActPairListP p)
{
	__shared__ uint32_t s_wcnt[2][4];
	__shared__ unsigned long long s_base[2];
	const uint32_t n = p.t.mask + 1u, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t par = 0;
	for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x, par ^= 1u) {
		const uint32_t h = base + threadIdx.x;
		ActPairKey k;
		ActPairEnt v;
		uint32_t slot = GYS_NOSLOT;
		bool match = h < n && actp_entry(p.t, h, p.epoch, k, v);
		if (match) {
			const uint32_t f = p.sel.flags;
			if ((f & GYS_ACS_BY_LISTENER) && k.lid != p.sel.listener_glob_id) match = false;
			if ((f & GYS_ACS_BY_CLIENT) && k.cid != p.sel.cli_aggr_task_id) match = false;
			if ((f & (GYS_ACS_KIND_LOCAL | GYS_ACS_KIND_REMOTE)) && !(f & (k.kind ? GYS_ACS_KIND_REMOTE : GYS_ACS_KIND_LOCAL))) match = false;
			if (v.bytes_sent + v.bytes_received < p.sel.min_bytes || v.active_conns < p.sel.min_active_conns) match = false;
			if (match) {
				slot = k.kind ? GYS_NOSLOT : tbl_lookup(p.gid, k.lid);
				if ((f & GYS_ACS_BY_HOST) && (slot == GYS_NOSLOT || slot >= p.nsvc || p.svc_host[slot] != p.sel.host_slot)) match = false;
			}
		}
		const unsigned long long b = __ballot(match);
		if (lane == 0u) s_wcnt[par][wave] = (uint32_t)__popcll(b);
		__syncthreads();
		if (threadIdx.x == 0u) {
			const uint32_t tot = s_wcnt[par][0] + s_wcnt[par][1] + s_wcnt[par][2] + s_wcnt[par][3];
			s_base[par] = tot ? atomicAdd(p.count, (unsigned long long)tot) : 0ull;
		}
		__syncthreads();
		unsigned long long at = s_base[par] + (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
		for (uint32_t w = 0; w < wave; ++w) at += s_wcnt[par][w];
		if (!match || at >= p.cap) continue;
		gys_actconn_row r;
		r.listener_glob_id = k.lid;
		r.cli_aggr_task_id = k.cid;
		memcpy(r.ser_comm, v.desc, 56); // ser_comm, cli_comm, remote_machine_id, remote_madhava_id: 56 contiguous bytes
		r.bytes_sent = v.bytes_sent;
		r.bytes_received = v.bytes_received;
		r.cli_delay_msec = v.cli_delay_msec;
		r.ser_delay_msec = v.ser_delay_msec;
		memcpy(&r.max_rtt_msec, &v.rtt_bits, 4);
		r.active_conns = v.active_conns;
		r.nrows = v.nrows;
		r.window = v.window;
		r.slot = slot;
		r.flags = (uint8_t)v.flags;
		r.kind = (uint8_t)k.kind;
		r.pad[0] = r.pad[1] = 0;
		r.reserved = 0;
		p.out[at] = r;
	}
}

// per service slot {live client groups, active connections, bytes sent + received, rows} over the live local entries, in exact integers
__global__ __launch_bounds__(256) void k_actp_svc_accum(ActPairTbl t, uint32_t epoch, DevTable gid, uint32_t nsvc, unsigned long long *acc /* [nsvc * 4], zeroed */)
{
	const uint32_t n = t.mask + 1u;
	for (uint32_t h = blockIdx.x * blockDim.x + threadIdx.x; h < n; h += gridDim.x * blockDim.x) {
		ActPairKey k;
		ActPairEnt v;
		if (!actp_entry(t, h, epoch, k, v) || k.kind) continue;
		const uint32_t slot = tbl_lookup(gid, k.lid);
		if (slot == GYS_NOSLOT || slot >= nsvc) continue;
		unsigned long long *a = acc + (size_t)slot * 4;
		atomicAdd(&a[0], 1ull);
		if (v.active_conns) atomicAdd(&a[1], (unsigned long long)v.active_conns);
		if (v.bytes_sent + v.bytes_received) atomicAdd(&a[2], v.bytes_sent + v.bytes_received);
		atomicAdd(&a[3], (unsigned long long)v.nrows);
	}
}

__global__ __launch_bounds__(256) void k_actp_svc_convert(const unsigned long long *acc, uint64_t n, double *out)
{
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) out[i] = (double)acc[i];
}

} // namespace gys
