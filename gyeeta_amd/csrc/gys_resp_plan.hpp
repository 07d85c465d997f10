// gys_resp_plan.hpp -- the plan of one response batch as pure host arithmetic: which front end the batch takes (general, host-local, split,
// many-listener parts), which tile form k_resp_host runs in, and the "virtual" segment list of the split / parts forms.
// No HIP call and no gys_ctx in here: the engine describes the batch's segments as RespSegView (run_resp_batch in gys_engine.hip) and
// launches what these decide, tests/cpp/test_resp_plan.cc checks them on the CPU.
// Needs gys_resp_seg (gysketch.h), GYS_SPLIT_PART and resp_host_lds_bytes (gys_kernels.hpp) declared before it.
#pragma once

#include <algorithm>
#include <cstdint>

namespace gys {

// one listener sub-table: a host's own one, or one part of a many-listener host
struct RespPartView {
	uint32_t tbl_entries, listeners;
	bool on_device;
};

// one segment of the batch as the plan sees it
struct RespSegView {
	uint32_t host_slot;
	uint64_t first_event, len;
	bool seen_twice; // the host has an earlier segment in this batch
	bool overflow;   // more listeners than the LDS path supports: general pipeline only
	bool chains;     // the host has keys with candidates
	uint32_t nparts; // listener parts of a many-listener host; 0: the host's own sub-table, parts[part0]
	uint32_t part0;  // first of its max(nparts, 1) entries in the batch's RespPartView array
	uint32_t sub_desc; // nparts != 0: descriptor of part 0, relative to the part descriptors
};

struct RespFront {
	bool host_local = false; // one workgroup per (virtual) segment, LDS sub-table + tile-wise LDS counting sort straight into the value buffers
	bool host_split = false; // ... with the segments cut into parts of GYS_SPLIT_PART events (SHARED form)
	bool host_parts = false; // ... with one workgroup per listener part of a many-listener host
	bool cands = false;      // some host of the batch has keys with candidates: the instances that resolve them by the server address
	uint32_t max_tbl = 16, max_l = 1; // largest sub-table / listener count among the batch's parts
	uint64_t max_len = 0, nwg = 0;    // longest segment; workgroups of the unsplit form
};

// host-local when every segment is a distinct host whose listener tables are LDS-sized and on the device (resp_path 1: never); split
// when that leaves most of the chip idle (resp_path 3: whenever a segment is longer than a part).  `n`: events of the batch.
inline RespFront resp_front_choice(const RespSegView *sv, uint32_t nsegs, const RespPartView *parts, uint64_t n, int ncu, uint32_t resp_path)
{
	RespFront f;
	f.host_local = resp_path != 1;
	for (uint32_t s = 0; s < nsegs && f.host_local; ++s) {
		const RespSegView &v = sv[s];
		f.cands = f.cands || v.chains;
		if (v.seen_twice || v.overflow) f.host_local = false;
		f.max_len = std::max(f.max_len, v.len);
		f.host_parts = f.host_parts || v.nparts != 0;
		const uint32_t np = std::max<uint32_t>(v.nparts, 1);
		for (uint32_t p = 0; p < np; ++p) {
			const RespPartView &t = parts[v.part0 + p];
			if (!t.on_device) f.host_local = false;
			f.max_tbl = std::max(f.max_tbl, t.tbl_entries);
			f.max_l = std::max(f.max_l, t.listeners);
		}
		f.nwg += np;
	}
	if (!f.host_local) return RespFront{};
	// few hosts with long segments: one workgroup per segment would leave most of the chip idle, so the segments are cut into parts
	// of GYS_SPLIT_PART events (SHARED form: buffer space reserved with device atomics).  A workgroup walks ~0.35 G events/s.
	const double t_host = (double)((f.nwg + ncu - 1) / ncu) * (double)f.max_len / 0.35e9;
	const double t_split = (double)n * (double)std::max<uint64_t>(f.nwg, 1) / (double)std::max<uint32_t>(nsegs, 1) / 40.0e9 + 20e-6;
	f.host_split = f.max_len > GYS_SPLIT_PART && (resp_path == 3 || (resp_path == 0 && t_split < t_host));
	return f;
}

// MODE of the k_resp_host instance: 2 IPv6 events, 1 keys with candidates, 0 neither
inline int resp_mode(const RespFront &f, bool v6) { return v6 ? 2 : f.cands ? 1 : 0; }

// tile form (events per tile): 512 threads x 12 events (6144-event tiles) when the batch's tables leave room for TWO such workgroups per CU
// (hosts of up to ~500 listeners: one workgroup's load / scan / flush phases run under the other's event phase -- r3t: 1.59 against
// 1.79 ms at 480 listeners per host; r3u: 51.2 against 45.5 G events/s at 20 832 x 480); else 1024 threads x 16 events (16384-event
// tiles, one workgroup per CU: 1000-listener hosts -- there the two-workgroup form needs half-full tables and 6-value pieces and loses,
// r3l / r3n); else 1024 x 8.  The instances of mode 1 / 2 exist in the two 1024-thread forms.
// (two workgroups per CU: each gets half of the CU's LDS -- resp_dyn_max is 160 KiB minus ONE static part)
inline uint32_t resp_tile_events(int mode, uint32_t max_tbl, uint32_t key_entries, uint32_t resp_dyn_max)
{
	if (mode == 0 && resp_host_lds_bytes(max_tbl, key_entries, 6144u) + 160u * 1024u - resp_dyn_max <= 80u * 1024u) return 6144u;
	return resp_host_lds_bytes(max_tbl, key_entries, 16384u) <= resp_dyn_max ? 16384u : 8192u;
}

// virtual segments: every segment cut into parts of GYS_SPLIT_PART events (`split`) and, for a many-listener host, one entry per part
// of its listeners (reserved = descriptor index + 1: the part descriptors follow the max_hosts host descriptors), the listener parts of
// one piece next to each other.  Returns the number of entries; out == nullptr: counts only (the same loop, so that the size of the
// buffer and what is written into it cannot disagree).
inline uint64_t resp_virtual_segments(const RespSegView *sv, uint32_t nsegs, bool split, uint32_t max_hosts, gys_resp_seg *out)
{
	uint64_t v = 0;
	for (uint32_t s = 0; s < nsegs; ++s) {
		const uint64_t step = split ? (uint64_t)GYS_SPLIT_PART : std::max<uint64_t>(sv[s].len, 1);
		for (uint64_t q = 0; q * step < sv[s].len; ++q)
			for (uint32_t lp = 0; lp < std::max<uint32_t>(sv[s].nparts, 1); ++lp, ++v)
				if (out) out[v] = gys_resp_seg{sv[s].host_slot, sv[s].nparts ? max_hosts + sv[s].sub_desc + lp + 1u : 0u, sv[s].first_event + q * step};
	}
	return v;
}

} // namespace gys
