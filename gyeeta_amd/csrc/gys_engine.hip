// gys_engine.hip -- host side of libgysketch.so: context, registries, the C ABI of include/gysketch.h.
//
// C++17 host code + hand-written HIP kernels (gys_kernels.hpp) for gfx950.  There is no CPU fallback anywhere in this library:
// every ingest/query path runs on the GPU or fails with GYS_ERR_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <thread>
#include <condition_variable>
#include <mutex>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include <dlfcn.h>
#include <rccl/rccl.h>

#include "gys_devmem.hpp"
#include "gys_subq.hpp"
#include "gys_kernels.hpp"
#include "gys_rollup.hpp"
#include "gys_groups.hpp"
#include "gys_resp_plan.hpp"
#include "gys_hostlst.hpp"
#include "gys_hllroll.hpp"
#include "gys_histroll.hpp"
#include "gys_huge.hpp"
#include "gys_svcquery.hpp"
#include "gys_rollsel.hpp"
#include "gys_svcdel.hpp"
#include "gys_svcpack.hpp"
#include "gys_tdrank.hpp"
#include "gys_topk.hpp"
#include "gys_actpairs.hpp"
#include "gys_svcdeps.hpp"
#include "gys_svcdeps_host.hpp"
#include "gys_svccomp.hpp"
#include "gys_groupflow.hpp"
#include "gys_svcresol.hpp"

using namespace gys;

namespace {

// The member lists of one grouping (gys_groups.hpp) and their copy on the device, built at one generation of the registry
// (gys_ctx::registry_gen); ensure_host_groups() / ensure_cluster_groups() rebuild them when the registry has moved on.
struct DeviceGroups {
	GroupLists h;
	DevBuf<uint32_t> members, off; // (off: only where a kernel reads it -- the all-hosts top-N)
	DevBuf<RollupChunk> chunks, gchunks;
	uint32_t nchunks = 0;
	uint64_t gen = ~0ull;
};

struct MachId {
	uint64_t first, second;
	bool operator==(const MachId &o) const { return first == o.first && second == o.second; }
};
struct MachIdHash {
	// GY_MACHINE_ID::get_hash common/gy_sys_hardware.h:82-85
	size_t operator()(const MachId &m) const
	{
		uint32_t w[4];
		memcpy(w, &m.first, 8);
		memcpy(w + 2, &m.second, 8);
		uint32_t k[6] = {w[0], w[1], w[2], w[3], 0, 0};
		return jhash2<6>(k, 4, GYS_SEED);
	}
};

inline MachId to_machid(const uint8_t id[16])
{
	MachId m;
	memcpy(&m.first, id, 8);
	memcpy(&m.second, id + 8, 8);
	return m;
}

struct ProfEntry {
	double total_ms = 0;
	uint64_t launches = 0;
	std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

struct ArenaLayout {
	uint64_t off_hll8, off_u32, n_u32, off_i64sum, n_i64sum, off_i64max, n_i64max, total;
	uint64_t u32_cms, u32_cluster, u32_pair, u32_misc, u32_cpair; // element offsets inside the u32 section
	uint64_t i64_cms, i64_ghist, i64_pair, i64_cpair;             // element offsets inside the i64 SUM section
};

// u32_pair / i64_pair: Count-Min pair of the ACTIVE_CONN_STATS roll-up; u32_misc[0]: its local-listener rows of the window;
// u32_cpair / i64_cpair: the TCP_CONN_NOTIFY pair roll-up, present only with gys_config.conn_pair_cms (its own tables: the two feeds
// count different things -- a gauge of active connections vs. closed connections -- and must not share cells): two table pairs, the
// listener side (connlistenmap_: records of the accepting partha) and behind it the client side (connclientmap_: connect-only records)
ArenaLayout arena_layout(uint32_t max_clusters, bool conn_pair)
{
	ArenaLayout a;
	a.off_hll8 = 0;
	a.off_u32 = align_up((uint64_t)1 << GYS_HLL_P, 256);
	a.u32_cms = 0;
	a.u32_cluster = (uint64_t)GYS_CMS_D * GYS_CMS_W;
	a.u32_pair = a.u32_cluster + align_up((uint64_t)max_clusters * 12, 64); // Count-Min pair of the (listener, client task) roll-up
	a.u32_misc = a.u32_pair + 2ull * GYS_CMS_D * GYS_CMS_W; // (local-listener rows' table, then the remote-listener rows')
	a.u32_cpair = a.u32_misc + 64;
	a.n_u32 = a.u32_cpair + (conn_pair ? (uint64_t)2 * GYS_CMS_D * GYS_CMS_W : 0); // listener-side tables, then client-side tables
	a.off_i64sum = align_up(a.off_u32 + a.n_u32 * 4, 256);
	a.i64_cms = 0;
	a.i64_ghist = (uint64_t)GYS_CMS_D * GYS_CMS_W;
	a.i64_pair = a.i64_ghist + 32;
	a.i64_cpair = a.i64_pair + 2ull * GYS_CMS_D * GYS_CMS_W;
	a.n_i64sum = a.i64_cpair + (conn_pair ? (uint64_t)2 * GYS_CMS_D * GYS_CMS_W : 0);
	a.off_i64max = align_up(a.off_i64sum + a.n_i64sum * 8, 256);
	a.n_i64max = 8;
	a.total = align_up(a.off_i64max + a.n_i64max * 8, 256);
	return a;
}

} // namespace

#define GYS_SEG_RING 4

struct gys_ctx {
	gys_config cfg{};
	int device = 0;
	hipStream_t stream = nullptr;
	bool own_stream = false;
	hipStream_t copy_stream = nullptr; // H2D copies of the response submissions: the copy of submission k + 1 runs under the kernels of submission k
	int ncu = 256;

	// registries (host)
	std::unordered_map<MachId, uint32_t, MachIdHash> host_map;
	std::vector<MachId> hosts;
	std::vector<std::string> host_names;
	std::vector<std::array<char, 16>> svc_comm; // TASK_COMM_LEN process name per service slot (SvcStateFields "name")
	std::vector<uint64_t> svc_gid_h;
	std::vector<uint32_t> host_cluster_h;
	std::unordered_map<std::string, uint32_t> cluster_map;
	std::vector<std::string> cluster_names;
	std::unordered_map<uint64_t, uint32_t> gid_map_h; // glob_id -> slot (host mirror for single-key queries)
	uint32_t nsvc = 0; // high-water mark of the slots handed out: [0, nsvc) are registered or free
	// deleted listeners (gys_svcdel.hpp): the slots gys_delete_listeners gave back, lowest first, and per slot the host (GYS_NOSLOT: free)
	// and the (netns:32|port:16) key it was registered under
	std::set<uint32_t> free_slots;
	std::vector<uint32_t> svc_host_h;
	std::vector<uint64_t> svc_key_h;
	DevBuf<SvcClearSeg> clr_segs;     // k_svc_clear's segment list (rebuilt per call: hist_win and lvl_last change places)
	DevBuf<unsigned long long> stale_bits; // gys_list_stale_listeners scratch (grows)
	DevBuf<uint32_t> stale_tiles;
	DevBuf<uint64_t> stale_ids;
	std::vector<HostListeners> host_lst;
	std::vector<uint32_t> host_seen; // batch stamp per host (duplicate-host detection in a multi-segment batch)
	uint32_t batch_stamp = 0;
	uint64_t n_batches_host_local = 0, n_batches_general = 0, n_batches_host_split = 0;
	uint64_t htbl_used = 0, htbl_cap = 0, hlst_used = 0, hlst_cap = 0;
	uint32_t resp_dyn_max = 0; // dynamic LDS a k_resp_host launch may use (160 KiB minus the kernel's static part)
	DevBuf<uint64_t> htbl; // pool of per-host sub-tables
	DevBuf<uint32_t> hlst; // pool of per-host local index -> slot lists
	DevBuf<HostDesc> hdesc; // [max_hosts] by host slot, then hdesc_ext_cap descriptors of the parts of many-listener hosts
	DevBuf<ListenerCand> cand_pool; // candidate records of the keys that need the server address (allocated on first use)
	uint64_t cand_used = 0; // records handed out to the hosts' regions (cand_pool.cap: records allocated)
	uint32_t hdesc_ext_used = 0, hdesc_ext_cap = 0;

	// device state
	DevTable lk_tbl{}, gid_tbl{}; // (views, passed to the kernels by value: lk_ent / gid_ent own their entries)
	DevBuf<TblEnt> lk_ent, gid_ent;
	DevBuf<uint64_t> svc_gid;
	DevBuf<gys_hist_rec> hist_win, hist_all;
	DevBuf<uint32_t> bitmap;
	DevBuf<int64_t> td_sum;
	DevBuf<uint32_t> td_cnt;
	DevBuf<TdMeta> td_meta;
	DevBuf<int2> td_minmax;
	DevBuf<double> rank_row;      // gys_query_ranks: the one row k_td_ranks writes (GYS_TR_MAXT doubles, then the total); kept between calls
	DevBuf<uint32_t> td_pend;     // per service a buffer of pcap staged words ("per-key value buffers" in gys_kernels.hpp)
	DevBuf<uint32_t> td_cur;      // words in each buffer (== td_meta.npend between batches)
	DevBuf<uint32_t> td_run;      // spilled services: fill cursor of the run in `staged`
	DevBuf<uint32_t> svc_host;    // host slot of each service
	DevBuf<uint32_t> host_spill;  // per host: batch stamp of the last batch in which one of its services spilled
	// predicted runs (k_prespill): start / end of a service's predicted run, the values its last batch brought, "worth predicting" flags of
	// the previous / this batch, hosts of the running batch, keys whose run goes into the buffer after all
	DevBuf<uint32_t> td_run0, td_run1, td_prevm, pre_hot, host_batch;
	DevBuf<MergeEnt> append_list;
	uint32_t pre_seq = 0; // k_prespill launches so far (parity = which pre_hot word it reads)
	bool prespill = false;
	uint32_t spill_stamp = 0;
	uint32_t pcap = 0;
	uint32_t pend_cap = GYS_TD_PEND_CAP, merge_fast = GYS_TDIGEST_MERGE_FAST; // the t-digest rule's buffer size (gys_config.td_pend_cap) and its fast merge class
	DevBuf<MergeEnt> merge_list, merge_list_slow, merge_list1, merge_list2, huge_list, query_list;
	DevBuf<uint32_t> merge_count; // [FIN_*]: the words of the FIN_* enum (gys_kernels.hpp); [FIN_QUERY_ONE] = 1 (query list)
	DevBuf<uint32_t> resp_win;    // per service: response events of the open window (-> Count-Min rows at the window boundary)
	DevBuf<uint32_t> cms_partial; // [cms_nch][GYS_CMS_D][GYS_CMS_W] partial rows of k_cms_partial
	uint32_t cms_nch = 0;
	bool resp_dirty = false;
	DevBuf<int64_t> query_sum;    // scratch of the non-destructive merge behind gys_query_quantiles
	DevBuf<uint32_t> query_cnt;
	DevBuf<uint32_t> batch_cnt, batch_off, scan_block_sums;
	DevBuf<uint64_t> ev_kv;       // general front end: (slot, staged word) per event
	DevBuf<uint32_t> staged;      // runs of the general front end / of spilled services
	// the window boundary's fixed sequence of copies / clears, captured once per registry shape as a hipGraph and replayed
	hipGraph_t win_graph = nullptr;
	hipGraphExec_t win_graph_exec = nullptr;
	uint64_t win_graph_shape = 0; // (hosts, services) the graph was captured for
	int win_graph_state = 0;      // 0 not tried, 1 usable, -1 capture unavailable: plain launches
	uint64_t win_graph_launches = 0;
	int64_t i64min = INT64_MIN;   // stable host source of the graph's 8-byte copy
	DevBuf<uint32_t> huge_scratch;
	// several-workgroups-per-key path (gys_huge.hpp): per-entry accumulators, chunk prefix, global tail list, fallback list
	DevBuf<unsigned long long> huge_acc, huge_tail;
	DevBuf<uint32_t> huge_tb_list;
	DevBuf<uint32_t> huge_bm, huge_chunk_off;
	DevBuf<MergeEnt> huge_fb_list;
	uint32_t huge_maxent = 0;
	uint64_t huge_list_cap = 0;
	int huge_blocks = 0;
	DevBuf<uint32_t> hll32;
	DevBuf<unsigned long long> svc_ctr;
	DevBuf<unsigned long long> svc_act; // per listener: ACTIVE_CONN_STATS rows, bytes sent / received, active connections (cumulative)
	DevBuf<unsigned long long> svc_win; // per-service window accumulators of the connection path (k_conn_ingest / k_conn_fold)
	bool conn_dirty = false;
	DevBuf<uint8_t> svc_state;
	DevBuf<unsigned long long> svc_claim; // [S] k_lstate_ingest / k_lstate_keep: last record of a call per listener
	uint32_t lstate_launch = 0;
	DevBuf<uint8_t> svc_hll;
	DevBuf<int32_t> host_summ_win, host_summ_last;
	DevBuf<gys_host_state> host_state;
	DevBuf<uint32_t> host_state_epoch, host_cluster;
	DevBuf<uint64_t> counters;
	DevBuf<uint32_t> misc; // [0] table insert failures, [1] topn count
	// segment descriptors of the batches in flight: a caller's segs array is only valid during the call and several batches may be
	// queued on the stream, so each call copies it into one of GYS_SEG_RING pinned host buffers (+ its own device buffer); a slot is
	// reused only after the kernels that read it have finished (event)
	struct SegSlot {
		PinnedPair<gys_resp_seg> segs;
		hipEvent_t done = nullptr;
		PinnedPair<gys_resp_seg> vsegs; // long segments cut into parts, many-listener hosts: the virtual segments
	} seg_ring[GYS_SEG_RING];
	uint32_t seg_next = 0;
	std::vector<RespSegView> resp_sv; // the current batch as gys_resp_plan.hpp sees it (kept for their capacity)
	std::vector<RespPartView> resp_pv;

	// reduce arena + last-window results
	uint8_t *arena = nullptr; // (a view: the caller's gys_config.reduce_arena, or arena_own)
	DevBuf<uint8_t> arena_own;
	ArenaLayout al{};
	DevBuf<uint8_t> last; // copy of the reduced arena of the last finished window (queries read this)
	DevBuf<uint32_t> last_act32;           // ACTIVE_CONN_STATS Count-Min pair the queries read: per-cell maximum over the tables of the
	DevBuf<unsigned long long> last_act64; // last GYS_ACT_RING windows (a partha reports every 15 s, a window is 5 s; k_act_latch)
	DevBuf<uint32_t> ring_act32, act_live;
	DevBuf<unsigned long long> ring_act64;
	// live (listener, client task group) rows of ACTIVE_CONN_STATS (gys_actpairs.hpp, gys_actpairs_host.hpp; cfg.actconn_pair_cap, 0 = nothing
	// allocated): two buffers of keys and entries -- ap_cur is the one in use, the other takes the live entries at a rebuild
	DevBuf<ActPairKey> ap_key[2];
	DevBuf<ActPairEnt> ap_ent[2];
	DevBuf<unsigned long long> ap_ctr; // [APC_NUM]
	DevBuf<uint32_t> ap_row_ent;       // a call's row -> entry list between the passes (grows)
	DevBuf<gys_actconn_row> ap_rows;   // gys_actconn_list: the rows on the device (grows)
	DevBuf<unsigned long long> ap_acc; // gys_actconn_svc_stats_dev: the integer sums (grows)
	uint32_t ap_entries = 0, ap_cur = 0;
	uint64_t ap_occ_bound = 0; // upper bound of the occupied entries of the buffer in use (+ rows per call; exact after a read-back)
	uint64_t ap_rebuilds = 0;
	uint32_t ap_rebuild_epoch = 0; // the window of the last rebuild (entries only die at a window close: no second one before the next)
	// service dependency graph (gys_svcdeps.hpp, gys_svcdeps_engine.hpp): per slot the task group the listener is bound to (0 = none; identity,
	// like svc_comm: not part of a service record); task_gen counts the calls that can change the task -> services list (a binding, a delete,
	// a registration), dep_tasks / dep_task_* are the list built at dep_tasks_gen and its copy on the device; the rest is scratch (grows)
	std::vector<uint64_t> svc_task_h;
	uint64_t task_gen = 0, dep_tasks_gen = ~0ull;
	TaskLists dep_tasks;
	DevBuf<uint64_t> dep_task_id;
	DevBuf<uint32_t> dep_task_off, dep_task_slot, dep_roots, dep_hops;
	DevBuf<uint2> dep_pairs, dep_hits;
	DevBuf<gys_svc_edge> dep_rows;
	DevBuf<unsigned long long> dep_ctr; // [DPC_NUM] (allocated by the first graph call)
	// service components (gys_svccomp.hpp, gys_svccomp_engine.hpp): scratch of one call (grows) -- the union-find's parents, the flattened
	// partition, the components' sizes, a listed root's place in the list, the list itself, the listed components' sums, the counter words
	DevBuf<uint32_t> cc_parent, cc_comp, cc_size, cc_index;
	DevBuf<uint2> cc_list;
	DevBuf<unsigned long long> cc_acc, cc_ctr; // [listed][GYS_CC_ACC], [CCC_NUM]
	// group flow map (gys_groupflow.hpp, gys_groupflow_engine.hpp): scratch of one call (grows; nothing before the first call) -- the keyed
	// table (keys, GYS_GF_ACC words each), the first-of-group flags of the task -> services list and their hash-minimum table, the rows of
	// the host form, the group pairs and distances of the search, the counter words
	DevBuf<unsigned long long> gf_keys, gf_acc, gf_hkey, gf_ctr; // [entries], [entries][GYS_GF_ACC], [flag table], [GFC_NUM]
	DevBuf<uint32_t> gf_first, gf_hmin, gf_hops;
	DevBuf<uint2> gf_pairs;
	DevBuf<gys_group_edge> gf_rows;
	// issue resolution (gys_svcresol.hpp, gys_svcresol_engine.hpp): scratch of one call (grows; nothing before the first call) -- per slot the
	// search's word (tier, class, state, issue), the 64-bit minimum (source << 32 | via) and a source's count of resolved slots; the records
	// and the rows of the host form; the counter words
	DevBuf<uint32_t> ri_word, ri_nres;
	DevBuf<unsigned long long> ri_best, ri_ctr; // [nsvc], [RSC_NUM]
	DevBuf<gys_svc_resol> ri_rec;
	DevBuf<gys_svc_resol_row> ri_rows;
	uint32_t epoch = 1;      // current window number (0 = never)
	bool prepared = false;
	DevBuf<uint32_t> d_epoch; // device copy of `epoch` for the captured window graph
	// gys_window_close: the WHOLE single-rank window boundary as one hipGraph per (registry shape, which folds are due)
	struct CloseGraph {
		hipGraph_t g = nullptr;
		hipGraphExec_t x = nullptr;
		uint64_t shape = 0;
		int state = 0; // 0 not tried, 1 usable, -1 capture unavailable
	} close_graph[4];
	uint64_t close_graph_launches = 0;
	bool have_last = false;
	bool clock_adopted = false; // gys_unpack_services took a blob's window number and close times (a context that had not closed a window)

	// host-pointer boundary (gys_subq.hpp): the submission queues of gys_ingest_resp_events / _tcp_conn / _listener_state (indexed by
	// SubQ::Kind), the ring of pinned staging slots of the calls that go on their own, and what both use of this context (bound at gys_create)
	IngestEnv ingest;
	SubQ sq[3];
	StageRing ring;
	std::mutex enq_mu; // the enqueue of a concurrent host-pointer call: stream order, shared flags
	DevBuf<uint8_t> dev_staging; // device-pointer record calls: the records and their offsets (grow)
	DevBuf<uint32_t> dev_offsets;
	// which service belongs to which host, which host to which cluster: counted up by every call that changes either (services added or
	// deleted, a host registered or moved to another cluster, a cluster added).  The two cached groupings are rebuilt when it has moved:
	// host -> services (ascending slot inside a host, the tie-break order of the top-N; roll-ups, all-hosts top-N) and cluster -> hosts
	uint64_t registry_gen = 0;
	DeviceGroups host_groups, cluster_groups;
	std::vector<uint16_t> svc_port_h; // listener port per service slot (web_curr_top_listeners "port")
	DevBuf<uint32_t> topn_slot;
	DevBuf<uint64_t> topn_metric;
	// filtered multi-host listener-state query (gys_svcquery.hpp): scratch, grow-only
	DevBuf<unsigned long long> q_cand_key, q_out_keys, q_cnt;
	// rankings on sketch results (gys_topk.hpp): the tie rows' keys; gys_top_services' metric column, totals and below(x) (grow-only)
	DevBuf<unsigned long long> q_tie_key, top_weight;
	DevBuf<double> top_col, top_below;
	DevBuf<uint32_t> q_cand_slot, q_misc, q_host_mask, q_slot_list;
	DevBuf<int32_t> q_set;
	DevBuf<uint8_t> q_out_rows;
	DevBuf<long long> q_acc;
	DevBuf<float> dev_pcts;
	DevBuf<float> zipf_cdf;
	uint32_t zipf_n = 0, zipf_milli = 0;

	// wire front-end scratch (grow-only)
	uint64_t wire_slots_cap = 0; // slots the per-slot arrays hold; kept apart from their .cap: wire_bsums holds a word per scan tile, not per slot
	DevBuf<uint32_t> wire_jump[2], wire_cnt, wire_rank, wire_bsums, wire_status;
	DevBuf<uint8_t> wire_mark, wire_flags;
	DevBuf<WireMsg> wire_msgs;

	// multi-level windows (cfg.enable_levels; kernels: "multi-level windows" in gys_kernels.hpp)
	DevBuf<gys_hist_rec> lvl_snap; // [2][GYS_LEVEL_RING][max_services] cumulative records at the last start of every ring bucket
	DevBuf<gys_hist_rec> lvl_last; // [max_services] the window closed last (level 0)
	// lazily folded records (t-digest on): hist_win and lvl_last change places at every close instead of a copy; lvl_last[slot] then is the service's
	// record of window lvl_last_tag[slot] (written by the close's fold pass) and counts only when that is lvl_last_epoch, the window closed last
	DevBuf<uint32_t> lvl_last_tag;
	// roll-up digests (gys_rollup.hpp): the groups' value bins (GYS_RB_STRIDE words per group; grows)
	DevBuf<unsigned long long> rb_bins;
	// distinct counts (gys_hllroll.hpp): one scratch buffer (grows: a file per chunk, per host and per group -- first call / after a
	// registration only)
	DevBuf<uint8_t> hl_buf;
	// group histograms of the levels (gys_histroll.hpp): one scratch buffer (grows: a record per chunk and per host)
	DevBuf<gys_hist_rec> hr_buf;
	// distinct counts of the closed windows (cfg.svc_hll_levels; "levels" in gys_hllroll.hpp)
	DevBuf<uint8_t> hl_lvl;        // [GYS_HLL_LVL_FILES][max_services] files: last, the two rings, all
	DevBuf<uint8_t> hl_view;          // a level's files of every service, materialised for gys_hll_rollup_level_dev (nsvc files; grows)
	// filtered roll-ups (gys_rollsel.hpp): the services' labels (gys_set_service_groups; allocated on first use, GYS_NO_GROUP everywhere)
	// and the scratch of a selection (grows): the items' groups, the groups' counters / cursors, the members, the chunk lists,
	// the rows with their offsets, the scan's tile sums and the totals
	DevBuf<uint32_t> svc_label;
	uint32_t label_domain = 0; // every label set so far is below this
	DevBuf<uint32_t> rs_item_group, rs_counts, rs_members, rs_tiles, rs_tot;
	DevBuf<RollupChunk> rs_chunks, rs_gchunks;
	DevBuf<gys_rollup_row> rs_rows;
	DevBuf<uint2> rs_rowoff;
	int64_t hl_t_last = -1;           // close time (s) of the last window rolled into hl_lvl, -1: none yet
	uint32_t hl_roll_epoch = 0xFFFFFFFEu; // the window rolled last (a finish step that is retried after a failure further down must not roll twice)
	int64_t hl_close_t = 0;           // close time (s) the prepared window was given (gys_window_prepare; the roll runs in gys_window_finish)
	DevBuf<uint8_t> svc_bithist; // [max_services][2] TCP_LISTENER::issue_bit_hist_ / high_resp_bit_hist_ (gys_decide_listener_state_dev; allocated on first use)
	uint32_t lvl_last_epoch = 0;
	DevBuf<int64_t> lvl_first;     // [max_services] time (s) of the service's first window close (firstTime_ of its series), 0: none yet
	DevBuf<gys_hist_rec> qps_hist, act_hist; // per-service QPS_HISTOGRAM / ACTIVE_CONN_HISTOGRAM
	int64_t lvl_t_last = -1;          // close time (s) of the last window, -1: none yet

	bool profile = false;
	std::map<std::string, ProfEntry> prof;
};

namespace {

// ------------------------------------------------------------------------------------------------ launch + profiling
struct ProfScope {
	gys_ctx *c;
	ProfEntry *e = nullptr;
	hipEvent_t a = nullptr, b = nullptr;
	hipStream_t st;
	ProfScope(gys_ctx *ctx, const char *name, hipStream_t stream = nullptr) : c(ctx), st(stream ? stream : ctx->stream)
	{
		if (!c->profile) return;
		e = &c->prof[name];
		if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
			e = nullptr;
			return;
		}
		hipEventRecord(a, st);
	}
	~ProfScope()
	{
		if (!e) return;
		hipEventRecord(b, st);
		e->pending.emplace_back(a, b);
		e->launches++;
	}
};

void prof_resolve(gys_ctx *c)
{
	for (auto &kv : c->prof) {
		for (auto &pr : kv.second.pending) {
			float ms = 0;
			hipEventSynchronize(pr.second);
			if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) kv.second.total_ms += ms;
			hipEventDestroy(pr.first);
			hipEventDestroy(pr.second);
		}
		kv.second.pending.clear();
	}
}

inline uint32_t grid_for(uint64_t n, uint32_t block, uint32_t cap)
{
	uint64_t g = (n + block - 1) / block;
	if (g < 1) g = 1;
	if (g > cap) g = cap;
	return (uint32_t)g;
}

int ensure_staging(gys_ctx *c, uint64_t bytes, uint32_t nrec)
{
	int rc = GYS_OK;
	if (bytes > c->dev_staging.cap) rc = c->dev_staging.grow(align_up(std::max<uint64_t>(bytes, 1u << 20), 4096), c->stream);
	if (!rc && nrec > c->dev_offsets.cap) rc = c->dev_offsets.grow(std::max<uint32_t>(nrec, 4096), c->stream);
	return rc;
}

int lookup_host(gys_ctx *c, const uint8_t machine_id[16], uint32_t *slot)
{
	auto it = c->host_map.find(to_machid(machine_id));
	if (it == c->host_map.end()) {
		set_err("unknown machine id");
		return GYS_ERR_NOTFOUND;
	}
	*slot = it->second;
	return GYS_OK;
}

int check_owner(gys_ctx *c, const uint8_t machine_id[16])
{
	if (c->cfg.nranks > 1 && gys_shard_of(machine_id, c->cfg.nranks) != c->cfg.rank) {
		set_err("host belongs to rank %u", gys_shard_of(machine_id, c->cfg.nranks));
		return GYS_ERR_NOT_OWNER;
	}
	return GYS_OK;
}

// ---- per-host listener sub-tables: the device pools of the mirror in gys_hostlst.hpp, used by k_resp_host
// (re)uploads one sub-table, its slot list and its descriptor hdesc[desc]; regions only ever grow, an outgrown region is abandoned in
// the pool (geometric growth: the abandoned total stays below the final size, which is what the pool capacity accounts for).
// Returns false when the pools are exhausted.
int host_tbl_upload(gys_ctx *c, HostListeners &hl, uint32_t desc, uint32_t part, uint32_t nparts, uint32_t cand_off, bool *ok)
{
	*ok = true;
	if (!hl.on_device || hl.tbl.size() > hl.tbl_cap) {
		if (c->htbl_used + hl.tbl.size() > c->htbl_cap || c->hlst_used + hl.tbl.size() / 2 > c->hlst_cap) {
			*ok = false;
			return GYS_OK;
		}
		hl.tbl_off = (uint32_t)c->htbl_used;
		hl.tbl_cap = (uint32_t)hl.tbl.size();
		c->htbl_used += hl.tbl.size();
		hl.lst_off = (uint32_t)c->hlst_used;
		c->hlst_used += hl.tbl.size() / 2;
		hl.on_device = true;
	}
	HIPCHK(hipMemcpyAsync(c->htbl + hl.tbl_off, hl.tbl.data(), hl.tbl.size() * 8, hipMemcpyHostToDevice, c->stream));
	if (!hl.slots.empty()) HIPCHK(hipMemcpyAsync(c->hlst + hl.lst_off, hl.slots.data(), hl.slots.size() * 4, hipMemcpyHostToDevice, c->stream));
	const HostDesc hd{hl.tbl_off, (uint32_t)hl.tbl.size() - 1, (uint32_t)hl.slots.size(), hl.lst_off, part, nparts - 1u, cand_off, 0u};
	HIPCHK(hipMemcpyAsync(c->hdesc + desc, &hd, sizeof(hd), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream)); // hd is a stack object
	return GYS_OK;
}

// the host's candidate region: allocated in the pool on first use (the pool itself on the first listener that needs it: a context whose
// listeners are all alone on their key and any-address never pays for it), re-allocated (twice the size) when outgrown
int host_cands_upload(gys_ctx *c, HostListeners &hl)
{
	if (hl.cands.empty()) return GYS_OK;
	if (hl.cands.size() > hl.cand_cap) {
		const uint64_t want = std::max<uint64_t>(16, next_pow2(hl.cands.size()));
		// round 6: the pool grows geometrically from 4 096 records (128 KB) to its bound of 4 x max_services + 64 x max_hosts
		// records instead of taking all of that -- 1.3 GB at 10^7 services -- on the first bound-address listener.  Regions are offsets
		// into the pool: they survive the move; kernels take the pool's address at launch.
		const uint64_t bound = 4ull * c->cfg.max_services + 64ull * c->cfg.max_hosts;
		if (c->cand_used + want > bound) {
			set_err("listener candidate pool exhausted");
			return GYS_ERR_NOMEM;
		}
		if (c->cand_used + want > c->cand_pool.cap) {
			uint64_t ncap = std::max<uint64_t>(c->cand_pool.cap * 2, 4096);
			while (ncap < c->cand_used + want) ncap *= 2;
			const int rc = c->cand_pool.grow_keep(std::min(ncap, bound), c->cand_used, c->stream);
			if (rc) return rc;
		}
		hl.cand_off = (uint32_t)c->cand_used;
		hl.cand_cap = (uint32_t)want;
		c->cand_used += want;
	}
	HIPCHK(hipMemcpyAsync(c->cand_pool + hl.cand_off, hl.cands.data(), hl.cands.size() * sizeof(ListenerCand), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
}

int host_lst_upload(gys_ctx *c, uint32_t host)
{
	HostListeners &hl = c->host_lst[host];
	if (hl.overflow) return GYS_OK;
	bool ok = true;
	if (hl.sub.empty()) {
		const int rc = host_tbl_upload(c, hl, host, 0, 1, hl.cand_off, &ok);
		if (rc) return rc;
	} else {
		for (uint32_t p = 0; p < hl.sub.size() && ok; ++p) {
			const int rc = host_tbl_upload(c, hl.sub[p], c->cfg.max_hosts + hl.sub_desc + p, p, (uint32_t)hl.sub.size(), hl.cand_off, &ok);
			if (rc) return rc;
		}
	}
	if (!ok) hl.overflow = true; // pools exhausted: this host keeps working through the general pipeline
	return GYS_OK;
}

// after the host's mirror changed: rebuilds what a changed chain invalidated (tables, candidate records, the global table's entries of the
// keys with candidates) and uploads the sub-tables
int host_lst_flush(gys_ctx *c, uint32_t host)
{
	HostListeners &hl = c->host_lst[host];
	if (hl.dirty) {
		host_rebuild(hl);
		const int rc = host_cands_upload(c, hl);
		if (rc) return rc;
		// the global table (general pipeline): a key with candidates points at its chain's records
		std::vector<uint64_t> kv;
		for (const auto &cf : hl.cand_first) {
			kv.push_back(listener_key(host, (uint32_t)(cf.first >> 16), (uint16_t)(cf.first & 0xFFFFu)));
			kv.push_back((uint64_t)(GYS_SLOT_GROUP | (hl.cand_off + cf.second)));
		}
		if (!kv.empty()) {
			const uint32_t nk = (uint32_t)(kv.size() / 2);
			const int rs = ensure_staging(c, kv.size() * 8, 0);
			if (rs) return rs;
			HIPCHK(hipMemcpyAsync(c->dev_staging, kv.data(), kv.size() * 8, hipMemcpyHostToDevice, c->stream));
			hipLaunchKernelGGL(k_table_set, dim3((nk + 255) / 256), dim3(256), 0, c->stream, c->lk_tbl, (const uint64_t *)c->dev_staging.p, nk);
			HIPCHK(hipStreamSynchronize(c->stream));
		}
	}
	return host_lst_upload(c, host);
}

// the fresh listeners of one call into the host's mirror (slot_of[i]: the service slot of arr[i]) and on to the device
int host_lst_add(gys_ctx *c, uint32_t host, const gys_listener_info *arr, uint32_t n, const uint32_t *slot_of)
{
	host_lst_insert(c->host_lst[host], arr, n, slot_of, c->hdesc_ext_used, c->hdesc_ext_cap);
	return host_lst_flush(c, host);
}

inline DigestP digest_params(gys_ctx *c)
{
	DigestP d{};
	d.td_sum = c->td_sum;
	d.td_cnt = c->td_cnt;
	d.td_meta = c->td_meta;
	d.td_minmax = c->td_minmax;
	d.td_pend = c->td_pend;
	d.td_cur = c->td_cur;
	d.pcap = c->pcap;
	d.pend_cap = c->pend_cap;
	d.nsvc = c->nsvc;
	d.staged = c->staged;
	d.hist_win = c->hist_win;
	d.hist_all = c->hist_all;
	d.bitmap = c->bitmap;
	return d;
}

// lazy fold (t-digest on): the records of services [first, first + n) are brought up to date with their buffered values before
// anything reads them ("per-key value buffers" in gys_kernels.hpp)
int fold_range(gys_ctx *c, uint32_t first, uint32_t n)
{
	if (!c->cfg.enable_tdigest || !n) return GYS_OK;
	FoldP f{};
	f.d = digest_params(c);
	f.first = first;
	f.n = n;
	ProfScope ps(c, "fold");
	const uint32_t nchunks = (n + 63u) / 64u;
	hipLaunchKernelGGL(k_fold, dim3(std::min<uint32_t>((nchunks + 3u) / 4u, (uint32_t)c->ncu * 8)), dim3(256), 0, c->stream, f);
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

// window close with the 5-s level: every service's records are brought up to date; the same pass leaves the window each record in hist_win
// belongs to in lvl_last_tag and the services' first close time in lvl_first (level_roll then swaps hist_win and lvl_last)
int fold_close_levels(gys_ctx *c, int64_t tnow)
{
	FoldP f{};
	f.d = digest_params(c);
	f.first = 0;
	f.n = c->nsvc;
	f.last_tag = c->lvl_last_tag;
	f.first_sec = c->lvl_first;
	f.tnow = tnow;
	ProfScope ps(c, "fold");
	const uint32_t nchunks = (c->nsvc + 63u) / 64u;
	hipLaunchKernelGGL(k_fold, dim3(std::min<uint32_t>((nchunks + 3u) / 4u, (uint32_t)c->ncu * 8)), dim3(256), 0, c->stream, f);
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

template <int TPT, bool SHARED, bool SPILL, int MODE = 0>
void launch_resp_host(gys_ctx *c, uint32_t grid, size_t dyn, const RespHostP &hp)
{
	// (IPv6 events: every kept event takes the rolled general hash path anyway, so ONE instance -- the one with the per-service register code,
	// which checks svc_hll_p at run time there -- serves both configurations)
	if (!SPILL && (hp.svc_hll_p || MODE == 2)) hipLaunchKernelGGL((k_resp_host<TPT, SHARED, SPILL, !SPILL, MODE>), dim3(grid), dim3(GYS_RESP_THREADS(TPT)), dyn, c->stream, hp);
	else hipLaunchKernelGGL((k_resp_host<TPT, SHARED, SPILL, false, MODE>), dim3(grid), dim3(GYS_RESP_THREADS(TPT)), dyn, c->stream, hp);
}
// mode 1 / 2 (keys with candidates / IPv6 events) exist in the 1024-thread tile forms (16 384 or 8 192 events)
template <bool SHARED, bool SPILL>
void launch_resp_host_mode(gys_ctx *c, int mode, bool tpt16, uint32_t grid, size_t dyn, const RespHostP &hp)
{
	if (mode == 2) {
		if (tpt16) launch_resp_host<16, SHARED, SPILL, 2>(c, grid, dyn, hp);
		else launch_resp_host<8, SHARED, SPILL, 2>(c, grid, dyn, hp);
	} else {
		if (tpt16) launch_resp_host<16, SHARED, SPILL, 1>(c, grid, dyn, hp);
		else launch_resp_host<8, SHARED, SPILL, 1>(c, grid, dyn, hp);
	}
}

// dynamic LDS a k_resp_host launch may ask for: the CU's 160 KiB minus the instance's own static part (read from the code object, so that
// a kernel change cannot silently push a launch over the limit); *dyn_max ends as the smallest such room over the instances
template <int TPT, bool SHARED, bool SPILL, int MODE = 0>
hipError_t resp_host_lds_attr(uint32_t *dyn_max)
{
	for (int svchll = (MODE == 2 && !SPILL) ? 1 : 0; svchll < (SPILL ? 1 : 2); ++svchll) {
		const void *fn = svchll ? (const void *)k_resp_host<TPT, SHARED, SPILL, !SPILL, MODE> : (const void *)k_resp_host<TPT, SHARED, SPILL, false, MODE>;
		hipFuncAttributes fa{};
		hipError_t e = hipFuncGetAttributes(&fa, fn);
		if (e != hipSuccess) return e;
		const uint32_t room = (160u * 1024u - (uint32_t)fa.sharedSizeBytes) & ~255u;
		e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)room);
		if (e != hipSuccess) return e;
		*dyn_max = std::min(*dyn_max, room);
	}
	return hipSuccess;
}

// ---- the response pipeline on a device-resident batch: run_resp_batch (below) is the list of these stages
struct RespBatch {
	const gys_resp_seg *segs_host;
	uint32_t nsegs;
	const void *d_ev;
	uint64_t n;
	bool v6; // the events are 48-byte tcp_ipv6_resp_event_t (handle_ipv6_resp_event, common/gy_socket_stat.cc:1535-1551)
	bool td;
	gys_ctx::SegSlot *slot = nullptr;
	RespFront front;
	int mode = 0;      // host-local: MODE of the k_resp_host instances
	uint32_t tile = 0; // host-local: events per tile of the k_resp_host form (gys_resp_plan.hpp)
	bool pre = false;  // predicted runs: only for the host-local front end, and only when the batch is large enough for a key to overflow a buffer at all
	FinP fin{};
	RespHostP hp{};
	uint32_t hgrid = 0;
	size_t dyn = 0;
};

int resp_check_segments(gys_ctx *c, const RespBatch &b)
{
	if (b.nsegs == 0 || !b.segs_host || b.segs_host[0].first_event != 0) {
		set_err("resp batch needs >= 1 segment starting at event 0");
		return GYS_ERR_INVAL;
	}
	if (b.td && b.n > c->cfg.max_batch_events) {
		set_err("batch of %llu events exceeds max_batch_events %llu", (unsigned long long)b.n, (unsigned long long)c->cfg.max_batch_events);
		return GYS_ERR_NOMEM;
	}
	if (b.n >= (1ull << 31)) {
		set_err("batch too large (u32 offsets)");
		return GYS_ERR_INVAL;
	}
	for (uint32_t s = 0; s < b.nsegs; ++s) {
		if (b.segs_host[s].host_slot >= c->hosts.size() || b.segs_host[s].first_event > b.n || (s && b.segs_host[s].first_event < b.segs_host[s - 1].first_event)) {
			set_err("bad resp segment %u", s);
			return GYS_ERR_INVAL;
		}
	}
	return GYS_OK;
}

// the caller's segments into the next slot of the ring, and from there to the device
int resp_upload_segments(gys_ctx *c, RespBatch &b)
{
	gys_ctx::SegSlot &slot = c->seg_ring[c->seg_next];
	c->seg_next = (c->seg_next + 1) % GYS_SEG_RING;
	b.slot = &slot;
	if (!slot.done) HIPCHK(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
	HIPCHK(hipEventSynchronize(slot.done)); // the batch that used this slot GYS_SEG_RING calls ago has consumed it
	int rc = slot.segs.grow(b.nsegs, 1024);
	if (rc) return rc;
	memcpy(slot.segs.host, b.segs_host, (uint64_t)b.nsegs * sizeof(gys_resp_seg));
	// `reserved` is the engine's own part-descriptor index (descriptor + 1, written only into the engine-built virtual segments): whatever
	// the caller left in the field must never reach k_resp_host's hdesc[] lookup
	for (uint32_t s = 0; s < b.nsegs; ++s) slot.segs.host[s].reserved = 0;
	HIPCHK(hipMemcpyAsync(slot.segs.dev, slot.segs.host, (uint64_t)b.nsegs * sizeof(gys_resp_seg), hipMemcpyHostToDevice, c->stream));
	return GYS_OK;
}

// front end and tile form of the batch (gys_resp_plan.hpp decides; this describes the segments' hosts to it)
void resp_plan_front(gys_ctx *c, RespBatch &b)
{
	if (!b.td || c->nsvc == 0) return; // the general front end
	c->batch_stamp++;
	c->resp_sv.clear();
	c->resp_pv.clear();
	for (uint32_t s = 0; s < b.nsegs; ++s) {
		const uint32_t host = b.segs_host[s].host_slot;
		const HostListeners &hl = c->host_lst[host];
		const uint64_t first = b.segs_host[s].first_event;
		c->resp_sv.push_back(RespSegView{host, first, (s + 1 < b.nsegs ? b.segs_host[s + 1].first_event : b.n) - first, c->host_seen[host] == c->batch_stamp,
						 hl.overflow, !hl.chain.empty(), (uint32_t)hl.sub.size(), (uint32_t)c->resp_pv.size(), hl.sub_desc});
		c->host_seen[host] = c->batch_stamp;
		if (hl.sub.empty()) c->resp_pv.push_back(RespPartView{(uint32_t)hl.tbl.size(), (uint32_t)hl.slots.size(), hl.on_device});
		for (const HostListeners &t : hl.sub) c->resp_pv.push_back(RespPartView{(uint32_t)t.tbl.size(), (uint32_t)t.slots.size(), t.on_device});
	}
	b.front = resp_front_choice(c->resp_sv.data(), b.nsegs, c->resp_pv.data(), b.n, c->ncu, c->cfg.resp_path);
	if (!b.front.host_local) return;
	b.mode = resp_mode(b.front, b.v6);
	b.tile = resp_tile_events(b.mode, b.front.max_tbl, (uint32_t)align_up(b.front.max_l, 2), c->resp_dyn_max);
	b.dyn = resp_host_lds_bytes(b.front.max_tbl, (uint32_t)align_up(b.front.max_l, 2), b.tile);
	b.pre = c->prespill && b.n > (uint64_t)c->pcap - c->pend_cap;
}

// FinP (key finalize) and, for the host-local front end, RespHostP; clears the batch's words of merge_count
int resp_fill_params(gys_ctx *c, RespBatch &b)
{
	FinP &fin = b.fin;
	if (b.td) {
		HIPCHK(hipMemsetAsync(c->merge_count, 0, FIN_BATCH_CLEARED * 4, c->stream)); // merge / huge / fallback list lengths, run allocation cursor
		c->resp_dirty = true;
		fin.td_cur = c->td_cur;
		fin.td_meta = c->td_meta;
		fin.nsvc = c->nsvc;
		fin.pcap = c->pcap;
		fin.pend_cap = c->pend_cap;
		fin.merge_fast = c->merge_fast;
		fin.class2_max = GYS_MERGE_LDS_MAX; // merges of 4097 .. 16 384 values (size class 2) go through the streamed value-bin instance
		fin.epoch = c->epoch;
		fin.resp_win = c->resp_win;
		fin.list[FIN_CLASS0] = c->merge_list;
		fin.list[FIN_CLASS1] = c->merge_list1;
		fin.list[FIN_CLASS2] = c->merge_list2;
		fin.list[FIN_HUGE] = c->huge_list;
		fin.counts = c->merge_count;
		fin.td_run = c->td_run;
		fin.svc_host = c->svc_host;
		fin.host_spill = c->host_spill;
		fin.counters = c->counters;
		fin.staged_cap = (uint32_t)std::min<uint64_t>(c->staged.cap, 0xFFFFFFFFull);
	}
	if (b.td && c->prespill) {
		fin.td_run0 = c->td_run0;
		fin.td_run1 = c->td_run1;
		fin.td_prevm = c->td_prevm;
		fin.hot = c->pre_hot;
		fin.hot_wr = b.pre ? ((c->pre_seq & 1u) ^ 1u) : (c->pre_seq & 1u); // the word the NEXT k_prespill reads (this batch's own one, if any, reads the other)
		fin.append_list = c->append_list;
		fin.append_cap = (uint32_t)c->append_list.cap;
		fin.td_pend = c->td_pend;
		fin.staged = c->staged;
		HIPCHK(hipMemsetAsync(c->merge_count + FIN_APPEND, 0, (FIN_NWORDS - FIN_APPEND) * 4, c->stream)); // (the append list's length; the predicted runs' reservation counter)
	}
	if (!b.front.host_local) return GYS_OK;
	RespHostP &hp = b.hp;
	hp.ev = (const uint64_t *)b.d_ev;
	hp.n = b.n;
	hp.segs = b.slot->segs.dev;
	hp.nsegs = b.nsegs;
	hp.hdesc = c->hdesc;
	hp.htbl = c->htbl;
	hp.hlst = c->hlst;
	hp.cand = c->cand_pool;
	hp.hll32 = c->hll32;
	hp.td_cur = c->td_cur;
	hp.td_pend = c->td_pend;
	hp.pcap = c->pcap;
	hp.td_run = c->td_run;
	hp.td_run1 = c->td_run1;
	hp.run_delta = (long long)(((intptr_t)c->staged.p - (intptr_t)c->td_pend.p) / 4);
	hp.staged = c->staged;
	hp.host_spill = c->host_spill;
	hp.spill_stamp = ++c->spill_stamp;
	fin.spill_stamp = hp.spill_stamp;
	hp.fin = fin;
	static const uint32_t dbg = [] { const char *e = getenv("GYS_DBG"); return e ? (uint32_t)atoi(e) : 0u; }();
	hp.dbg = dbg;
	hp.counters = c->counters;
	hp.svc_hll = c->svc_hll;
	hp.svc_hll_p = c->cfg.svc_hll_p;
	hp.ghist = (unsigned long long *)(c->arena + c->al.off_i64sum) + c->al.i64_ghist;
	hp.gmax = (long long *)(c->arena + c->al.off_i64max);
	hp.lds_tbl_entries = b.front.max_tbl;
	hp.lds_key_entries = (uint32_t)align_up(b.front.max_l, 2);
	b.hgrid = b.nsegs;
	return GYS_OK;
}

// the mode-0 k_resp_host instance of the batch's tile form
template <bool SHARED, bool SPILL>
void launch_resp_host_tile(gys_ctx *c, const RespBatch &b)
{
	if (b.tile == 6144u) return launch_resp_host<12, SHARED, SPILL>(c, b.hgrid, b.dyn, b.hp);
	if (b.tile == 16384u) launch_resp_host<16, SHARED, SPILL>(c, b.hgrid, b.dyn, b.hp);
	else launch_resp_host<8, SHARED, SPILL>(c, b.hgrid, b.dyn, b.hp);
}

// host-local front end: the virtual segments of the split / parts forms, the predicted runs, k_resp_host
int resp_launch_host_local(gys_ctx *c, RespBatch &b)
{
	if (b.front.host_split || b.front.host_parts) {
		PinnedPair<gys_resp_seg> &vs = b.slot->vsegs;
		const uint64_t nv = resp_virtual_segments(c->resp_sv.data(), b.nsegs, b.front.host_split, c->cfg.max_hosts, nullptr);
		int rc = vs.grow(nv, (1u << 16) / sizeof(gys_resp_seg));
		if (rc) return rc;
		resp_virtual_segments(c->resp_sv.data(), b.nsegs, b.front.host_split, c->cfg.max_hosts, vs.host);
		HIPCHK(hipMemcpyAsync(vs.dev, vs.host, nv * sizeof(gys_resp_seg), hipMemcpyHostToDevice, c->stream));
		b.hp.segs = vs.dev;
		b.hp.nsegs = b.hgrid = (uint32_t)nv;
	}
	if (b.front.host_split) c->n_batches_host_split++;
	else c->n_batches_host_local++;
	if (b.pre) {
		// runs for the keys whose last batch, repeated, would overflow their buffer (nothing but a flag read when no key was that large)
		ProfScope ps(c, "prespill");
		PreSpillP pp{};
		pp.td_cur = c->td_cur;
		pp.td_prevm = c->td_prevm;
		pp.td_run = c->td_run;
		pp.td_run0 = c->td_run0;
		pp.td_run1 = c->td_run1;
		pp.counts = c->merge_count;
		pp.hot = c->pre_hot;
		pp.hot_rd = c->pre_seq & 1u;
		pp.svc_host = c->svc_host;
		pp.host_batch = c->host_batch;
		pp.batch_stamp = c->batch_stamp;
		pp.nsvc = c->nsvc;
		pp.pcap = c->pcap;
		pp.pend_cap = c->pend_cap;
		pp.resv = (unsigned long long *)(c->merge_count + FIN_PRE_RESV); // (cleared at the start of the batch)
		pp.run_limit = (uint32_t)std::min<uint64_t>(c->staged.cap - std::min<uint64_t>(b.n, c->staged.cap), 0xFFFFFFFFull); // the exact runs of the fall-back (<= n words) keep their room
		++c->pre_seq;
		hipLaunchKernelGGL(k_mark_hosts, dim3((b.nsegs + 255) / 256), dim3(256), 0, c->stream, b.slot->segs.dev, b.nsegs, c->host_batch, c->batch_stamp);
		hipLaunchKernelGGL(k_prespill, dim3((c->nsvc + 255) / 256), dim3(256), 0, c->stream, pp);
	}
	ProfScope ps(c, "resp_host");
	if (b.mode != 0) {
		if (b.front.host_split) launch_resp_host_mode<true, false>(c, b.mode, b.tile == 16384u, b.hgrid, b.dyn, b.hp);
		else launch_resp_host_mode<false, false>(c, b.mode, b.tile == 16384u, b.hgrid, b.dyn, b.hp);
	} else if (b.front.host_split) {
		launch_resp_host_tile<true, false>(c, b);
	} else {
		launch_resp_host_tile<false, false>(c, b);
	}
	return GYS_OK;
}

// general front end, first pass: the per-event sketches; with t-digests also the events' (key, value) pairs and the keys' counts
void resp_launch_pass1(gys_ctx *c, const RespBatch &b)
{
	c->n_batches_general++;
	RespP1 p{};
	p.ev = (const uint64_t *)b.d_ev;
	p.cand = c->cand_pool;
	p.n = b.n;
	p.segs = b.slot->segs.dev;
	p.nsegs = b.nsegs;
	p.lk = c->lk_tbl;
	p.svc_gid = c->svc_gid;
	p.hist_win = c->hist_win;
	p.bitmap = c->bitmap;
	p.hll32 = c->hll32;
	p.cms32 = (uint32_t *)(c->arena + c->al.off_u32) + c->al.u32_cms;
	p.batch_cnt = b.td ? c->batch_cnt : nullptr;
	p.ev_kv = b.td ? c->ev_kv : nullptr;
	p.counters = c->counters;
	p.svc_hll = c->svc_hll;
	p.svc_hll_p = c->cfg.svc_hll_p;
	p.ghist = (unsigned long long *)(c->arena + c->al.off_i64sum) + c->al.i64_ghist;
	p.gmax = (long long *)(c->arena + c->al.off_i64max);
	ProfScope ps(c, "resp_pass1");
	if (b.v6) hipLaunchKernelGGL(k_resp_pass1<true>, dim3(grid_for(b.n, 256, (uint32_t)c->ncu * 8)), dim3(256), 0, c->stream, p);
	else hipLaunchKernelGGL(k_resp_pass1<false>, dim3(grid_for(b.n, 256, (uint32_t)c->ncu * 8)), dim3(256), 0, c->stream, p);
}

// general front end, the rest: the values sorted by key into `staged`, the keys' runs appended to their buffers
void resp_launch_general(gys_ctx *c, const RespBatch &b)
{
	const uint32_t nsvc = c->nsvc, nblk = (nsvc + GYS_SCAN_TILE - 1) / GYS_SCAN_TILE;
	{
		ProfScope ps(c, "scan");
		hipLaunchKernelGGL(k_scan_block_sums, dim3(nblk), dim3(256), 0, c->stream, c->batch_cnt, nsvc, c->scan_block_sums);
		hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(256), 0, c->stream, c->scan_block_sums, nblk);
		hipLaunchKernelGGL(k_scan_final, dim3(nblk), dim3(256), 0, c->stream, c->batch_cnt, nsvc, c->scan_block_sums, c->batch_off);
	}
	{
		ProfScope ps(c, "scatter");
		hipLaunchKernelGGL(k_resp_scatter, dim3(grid_for(b.n, 256, (uint32_t)c->ncu * 8)), dim3(256), 0, c->stream, c->ev_kv, b.n, c->batch_off, c->staged);
	}
	ProfScope ps(c, "key_append");
	AppendP ap{};
	ap.batch_cnt = c->batch_cnt;
	ap.off_end = c->batch_off;
	ap.staged = c->staged;
	ap.td_cur = c->td_cur;
	ap.td_pend = c->td_pend;
	ap.pcap = c->pcap;
	ap.nsvc = nsvc;
	const uint32_t nchunks = (nsvc + 63u) / 64u;
	hipLaunchKernelGGL(k_key_append, dim3(std::min<uint32_t>((nchunks + 3u) / 4u, (uint32_t)c->ncu * 8)), dim3(256), 0, c->stream, ap);
}

// what follows either front end: the keys finalized (queued for their merges), predicted runs that fit after all, the second pass
void resp_launch_finalize(gys_ctx *c, RespBatch &b)
{
	const bool host_local = b.front.host_local;
	if (!host_local || b.front.host_split) { // (the fused host-local form finalizes its keys in the tail of k_resp_host)
		ProfScope ps(c, "key_finalize");
		b.fin.batch_off = host_local ? nullptr : c->batch_off;
		hipLaunchKernelGGL(k_key_finalize, dim3((c->nsvc + 255) / 256), dim3(256), 0, c->stream, b.fin);
	}
	if (b.pre) // keys whose predicted run fits their buffer after all: the run is copied behind the buffered values (before the merges read either)
		hipLaunchKernelGGL(k_run_append, dim3((uint32_t)c->ncu), dim3(256), 0, c->stream, c->append_list, c->merge_count + FIN_APPEND, c->staged, c->td_pend, c->pcap);
	// (a key spills / lands in a larger merge class only when THIS batch brought it more values than its buffer had room for: a small
	// batch -- a partha message of a few thousand events -- cannot, and the launches for those cases are not made)
	if (host_local && b.n > (uint64_t)c->pcap - c->pend_cap) {
		// second pass over the hosts that have spilled services (a workgroup of any other host returns at once): their events again,
		// only the spilled services' values, into the runs k_key_finalize allocated in `staged`
		ProfScope ps(c, "resp_spill");
		if (b.mode != 0) launch_resp_host_mode<true, true>(c, b.mode, b.tile == 16384u, b.hgrid, b.dyn, b.hp);
		else launch_resp_host_tile<true, true>(c, b);
	}
}

// the slow list through the general kernel, in the instance that holds the largest merge of size class `top`
void resp_launch_slow_pass(gys_ctx *c, const DigestP &d, uint32_t cap, int top)
{
	MergeP mp{};
	mp.d = d;
	mp.list = c->merge_list_slow;
	mp.count = c->merge_count + FIN_SLOW;
	const dim3 grid(std::max(1u, std::min<uint32_t>(cap, (uint32_t)c->ncu)));
	if (top == 2) hipLaunchKernelGGL((k_digest_merge<GYS_MERGE_LDS_MAX, 1024u>), grid, dim3(1024), 0, c->stream, mp);
	else if (top == 0 && c->merge_fast <= GYS_MERGE_CLASS0) hipLaunchKernelGGL((k_digest_merge<GYS_MERGE_CLASS0, 256u>), grid, dim3(256), 0, c->stream, mp);
	else hipLaunchKernelGGL((k_digest_merge<GYS_MERGE_CLASS1, 256u>), grid, dim3(256), 0, c->stream, mp);
}

// the merges of the keys the batch queued, by size class.  The value-bin launches run for the classes the batch can reach (a key lands in
// class 1 / 2 only when THIS batch brought it more values than the class below holds).  Then exactly ONE pass of the general kernel over the
// slow list -- what a value-bin launch handed over: entries whose total weight needs 64-bit arithmetic, or with more large values than the
// bin kernel's list holds (normally none) -- behind the last value-bin launch, so that an entry is merged once; its instance is the one
// of the highest class reached.  (Entries above class 2 take the several-workgroup path, resp_launch_huge.)
void resp_launch_merges(gys_ctx *c, const RespBatch &b)
{
	const uint32_t nsvc = c->nsvc, ncu = (uint32_t)c->ncu;
	const uint32_t cap = (uint32_t)std::min<uint64_t>(nsvc, b.n);
	const bool reach[3] = {true, c->merge_fast < GYS_MERGE_CLASS1 && b.n > c->merge_fast - c->pend_cap, b.n > GYS_MERGE_CLASS1 - c->pend_cap};
	const int top = reach[2] ? 2 : reach[1] ? 1 : 0;
	MergeEnt *const lists[3] = {c->merge_list, c->merge_list1, c->merge_list2};
	MergeBP bp{};
	bp.d = digest_params(c);
	bp.slow_list = c->merge_list_slow;
	bp.slow_count = c->merge_count + FIN_SLOW;
	for (int cls = 0; cls < 3; ++cls) {
		if (!reach[cls]) continue;
		ProfScope ps(c, cls ? "digest_merge_big" : "digest_merge");
		bp.list = lists[cls];
		bp.count = c->merge_count + FIN_CLASS0 + cls;
		if (cls == 0) {
			const dim3 bgrid(std::max(1u, std::min<uint32_t>(cap, ncu * 8)));
			if (c->merge_fast <= 1024u) hipLaunchKernelGGL((k_digest_bins<false, 4u>), bgrid, dim3(256), 0, c->stream, bp);
			else if (c->merge_fast <= 2048u) hipLaunchKernelGGL((k_digest_bins<false, 8u>), bgrid, dim3(256), 0, c->stream, bp);
			else hipLaunchKernelGGL((k_digest_bins<false, 16u>), bgrid, dim3(256), 0, c->stream, bp);
		} else if (cls == 1) { // up to 4096 values: the same exact-integer definition, bit-identical
			hipLaunchKernelGGL((k_digest_bins<false, 16u>), dim3(std::max(1u, std::min<uint32_t>(cap, ncu * GYS_MB_WAVES16))), dim3(256), 0, c->stream, bp);
		} else { // 4097 .. 16 384 values: the streamed instance
			const uint32_t cap2 = (uint32_t)std::min<uint64_t>(nsvc, b.n / (GYS_MERGE_CLASS1 - c->pend_cap) + 1);
			hipLaunchKernelGGL((k_digest_bins<false, 64u>), dim3(std::max(1u, std::min<uint32_t>(cap2, ncu * 8))), dim3(256), 0, c->stream, bp);
		}
		if (cls == top) resp_launch_slow_pass(c, bp.d, cap, top);
	}
}

// huge keys (> 16 384 values in this call): several workgroups per key (gys_huge.hpp); what that path cannot take -- entries beyond its
// pool, more than 4 096 values >= 16 384 in one key -- is handed to the one-workgroup kernel through a fallback list
void resp_launch_huge(gys_ctx *c, const RespBatch &b)
{
	ProfScope ps(c, "digest_huge");
	Huge2P q{};
	q.d = digest_params(c);
	q.list = c->huge_list;
	q.count = c->merge_count + FIN_HUGE;
	q.bins = c->huge_scratch;
	q.acc = c->huge_acc;
	q.bm = c->huge_bm;
	q.chunk_off = c->huge_chunk_off;
	q.tail = c->huge_tail;
	q.tail_count = c->merge_count + FIN_HUGE_TAIL;
	q.tail_cap = GYS_HB_TAIL_CAP;
	q.maxent = c->huge_maxent;
	q.fb_list = c->huge_fb_list;
	q.fb_count = c->merge_count + FIN_HUGE_FB;
	q.nent_used = c->merge_count + FIN_HUGE_NENT;
	q.tb_list = c->huge_tb_list;
	q.tb_count = c->merge_count + FIN_HUGE_TB;
#ifdef GYS_HUGE_TIMING
	q.dbg = (unsigned long long *)c->counters + 20;
#endif
	// the pool holds huge_maxent entries: the list is walked in rounds (a round beyond the list's end costs four empty launches)
	const uint64_t list_cap = std::min<uint64_t>(std::min<uint64_t>(c->nsvc, b.n / (GYS_MERGE_CLASS1 - c->pend_cap) + 1), c->huge_list_cap);
	for (uint64_t first = 0; first < list_cap; first += c->huge_maxent) {
		q.first = (uint32_t)first;
		hipLaunchKernelGGL(k_huge_plan, dim3(1), dim3(1024), 0, c->stream, q);
		hipLaunchKernelGGL(k_huge_clear, dim3((uint32_t)c->ncu * 8), dim3(256), 0, c->stream, q);
		hipLaunchKernelGGL(k_huge_count, dim3((uint32_t)c->ncu * 2), dim3(1024), GYS_HB_BINS * 4, c->stream, q);
		// tier A: two 512-thread workgroups per CU (79 KiB of LDS each); tier B: whatever tier A handed over (usually nothing)
		hipLaunchKernelGGL((k_huge_merge<512, GYS_HB_TAIL_A, false>), dim3((uint32_t)c->ncu * 2), dim3(512), (GYS_HB_BINS + GYS_HB_TAIL_A) * 4, c->stream, q);
		hipLaunchKernelGGL((k_huge_merge<1024, GYS_HB_TAIL_LDS, true>), dim3((uint32_t)c->ncu), dim3(1024), (GYS_HB_BINS + GYS_HB_TAIL_LDS) * 4, c->stream, q);
	}
	HugeP h{};
	h.d = q.d;
	h.scratch = c->huge_scratch;
	h.huge_list = c->huge_fb_list;
	h.huge_count = c->merge_count + FIN_HUGE_FB;
	hipLaunchKernelGGL(k_digest_huge, dim3(c->huge_blocks), dim3(256), 0, c->stream, h);
}

int run_resp_batch(gys_ctx *c, const gys_resp_seg *segs_host, uint32_t nsegs, const void *d_ev, uint64_t n, bool v6 = false)
{
	if (n == 0) return GYS_OK;
	RespBatch b{segs_host, nsegs, d_ev, n, v6, c->cfg.enable_tdigest != 0};
	int rc = resp_check_segments(c, b);
	if (rc) return rc;
	if ((rc = resp_upload_segments(c, b)) != GYS_OK) return rc;
	resp_plan_front(c, b);
	if ((rc = resp_fill_params(c, b)) != GYS_OK) return rc;
	if (b.front.host_local) {
		if ((rc = resp_launch_host_local(c, b)) != GYS_OK) return rc;
	} else {
		resp_launch_pass1(c, b);
		HIPCHK(hipGetLastError());
		if (!b.td || c->nsvc == 0) {
			HIPCHK(hipEventRecord(b.slot->done, c->stream));
			return GYS_OK;
		}
		resp_launch_general(c, b);
	}
	HIPCHK(hipGetLastError());
	resp_launch_finalize(c, b);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(b.slot->done, c->stream)); // the segment descriptors have been consumed once the stream gets here
	resp_launch_merges(c, b);
	if (n > GYS_MERGE_CLASS1 - c->pend_cap) resp_launch_huge(c, b);
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

// ------------------------------------------------------------------------------------------------ multi-level windows
constexpr int64_t LEVEL_SECS[GYS_NLEVELS] = {5, 300, 5 * 24 * 3600, 0}; // Level_5s_5min_5days_all common/gy_statistics.h:1545-1551

// most recent start (<= t) of ring bucket j of a level of `dur` seconds (folly BucketedTimeSeries::getBucketInfo; dur % ring == 0)
inline int64_t level_bucket_start(int64_t t, int64_t dur, uint32_t j)
{
	const int64_t s = (t / dur) * dur + (int64_t)j * (dur / GYS_LEVEL_RING);
	return s <= t ? s : s - dur;
}

inline uint32_t level_bucket_idx(int64_t t, int64_t dur) { return (uint32_t)((t % dur) * GYS_LEVEL_RING / dur); }

inline uint8_t *hll_level_array(gys_ctx *c, uint32_t f) { return c->hl_lvl + (((uint64_t)f * c->cfg.max_services) << c->cfg.svc_hll_p); }

// window close at c->hl_close_t: the open window's registers enter `last`, the two current ring buckets and `all`, and are cleared
// (k_hll_level_roll).  The ring arithmetic is level_roll's: a bucket whose start was crossed since the previous close expires.
int hll_level_roll(gys_ctx *c)
{
	if (c->hl_roll_epoch == c->epoch) return GYS_OK; // once per window
	c->hl_roll_epoch = c->epoch;
	const int64_t tnow = std::max(c->hl_close_t, c->hl_t_last); // time does not go backwards
	const uint32_t p = c->cfg.svc_hll_p;
	uint32_t mask[2] = {0, 0}, cur[2];
	for (int li = 0; li < 2; ++li) {
		const int64_t dur = LEVEL_SECS[li + 1];
		for (uint32_t j = 0; j < GYS_LEVEL_RING; ++j)
			if (c->hl_t_last >= 0 && level_bucket_start(tnow, dur, j) > c->hl_t_last) mask[li] |= 1u << j;
		cur[li] = level_bucket_idx(tnow, dur);
	}
	c->hl_t_last = tnow;
	if (!c->nsvc) return GYS_OK; // (slots above nsvc have never been written: nothing to clear)
	ProfScope ps(c, "hll_level_roll");
	for (int li = 0; li < 2; ++li)
		for (uint32_t j = 0; j < GYS_LEVEL_RING; ++j)
			if (((mask[li] >> j) & 1u) && j != cur[li])
				HIPCHK(hipMemsetAsync(hll_level_array(c, GYS_HLL_LVL_RING + (uint32_t)li * GYS_LEVEL_RING + j), 0, (uint64_t)c->nsvc << p, c->stream));
	HllLevelRollP q{};
	q.open = (uint4 *)c->svc_hll.p;
	q.last = (uint4 *)hll_level_array(c, GYS_HLL_LVL_LAST);
	q.ring1 = (uint4 *)hll_level_array(c, GYS_HLL_LVL_RING + cur[0]);
	q.ring2 = (uint4 *)hll_level_array(c, GYS_HLL_LVL_RING + GYS_LEVEL_RING + cur[1]);
	q.all = (uint4 *)hll_level_array(c, GYS_HLL_LVL_ALL);
	q.npieces = (uint64_t)c->nsvc << (p - 4u);
	q.fresh1 = (mask[0] >> cur[0]) & 1u;
	q.fresh2 = (mask[1] >> cur[1]) & 1u;
	hipLaunchKernelGGL(k_hll_level_roll, dim3(grid_for(q.npieces, GYS_HLL_NT, (uint32_t)c->ncu * 16)), dim3(GYS_HLL_NT), 0, c->stream, q);
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

// window close at tusec: remember the closing window as level 0 and snapshot the cumulative records into every ring bucket whose
// start was crossed since the previous close
int level_roll(gys_ctx *c, uint64_t tusec)
{
	int64_t tnow = (int64_t)(tusec / 1000000ull);
	if (tnow < c->lvl_t_last) tnow = c->lvl_t_last; // time does not go backwards (BucketedTimeSeries::update)
	LevelRollP p{};
	for (int li = 0; li < 2; ++li) {
		const int64_t dur = LEVEL_SECS[li + 1];
		for (uint32_t j = 0; j < GYS_LEVEL_RING; ++j)
			if (c->lvl_t_last >= 0 && level_bucket_start(tnow, dur, j) > c->lvl_t_last) p.mask[li] |= 1u << j;
	}
	c->lvl_t_last = tnow;
	if (!c->nsvc) return GYS_OK;
	const bool keep_last = c->cfg.enable_levels == 1; // enable_levels = 2: no 5-s level (nothing per key unless a ring boundary was crossed)
	if (!keep_last && !(p.mask[0] | p.mask[1])) {
		// no snapshot due: only the time of a service's first window close (firstTime_ of its series) is kept up
		ProfScope ps(c, "level_roll");
		hipLaunchKernelGGL(k_level_first, dim3(grid_for(c->nsvc, 256, (uint32_t)c->ncu * 8)), dim3(256), 0, c->stream, c->lvl_first, c->nsvc, tnow);
		HIPCHK(hipGetLastError());
		return GYS_OK;
	}
	// every service's closing-window record must be complete.  With lazily folded records (t-digest on) and the 5-s level, level 0 costs no pass
	// of its own: the fold leaves per service which window its record in hist_win belongs to (lvl_last_tag) and the two arrays change places --
	// the window records ARE the level-0 records, a key's first fold of the next window rewrites its (now stale) record in the other array
	// without reading it.  (Rounds 2 - 4 copied 256 B per service and close, k_level_roll: 1.1 ms at 10^7 services; writing the copy from the
	// fold pass was slower still, profiles/r5i_levels_fused_vs_separate.txt.)  k_level_roll runs when a ring boundary was crossed, for the
	// snapshots, or for the copy when the records are kept eagerly.
	const bool swap_last = keep_last && c->cfg.enable_tdigest;
	{
		const int rcf = swap_last ? fold_close_levels(c, tnow) : fold_range(c, 0, c->nsvc);
		if (rcf) return rcf;
	}
	if (!swap_last || (p.mask[0] | p.mask[1])) {
		p.win = c->hist_win;
		p.all = c->hist_all;
		p.meta = c->cfg.enable_tdigest ? c->td_meta : nullptr;
		p.epoch = c->epoch;
		p.nsvc = c->nsvc;
		p.snap = c->lvl_snap;
		p.last = keep_last && !swap_last ? c->lvl_last : nullptr;
		p.stride = c->cfg.max_services;
		p.first_sec = c->lvl_first;
		p.tnow = tnow;
		ProfScope ps(c, "level_roll");
		hipLaunchKernelGGL(k_level_roll, dim3(grid_for((uint64_t)c->nsvc * 16, 256, (uint32_t)c->ncu * 8)), dim3(256), 0, c->stream, p);
		HIPCHK(hipGetLastError());
	}
	if (swap_last && c->lvl_last_epoch != c->epoch) { // (once per window: a gys_window_prepare that is retried after a failure further down must not swap back)
		std::swap(c->hist_win, c->lvl_last);
		c->lvl_last_epoch = c->epoch;
	}
	return GYS_OK;
}

// the array that holds the records of window c->epoch (what the window views read, each record behind its hw_epoch check): hist_win -- except
// between gys_window_prepare and gys_window_finish when the close has already swapped it with the level-0 array (level_roll)
inline const gys_hist_rec *window_records(gys_ctx *c)
{
	// (the swap itself is the test, not `prepared`: it is skipped without services, and it stays in force when the rest of the prepare step failed)
	return c->cfg.enable_levels == 1 && c->cfg.enable_tdigest && c->lvl_last_epoch == c->epoch ? c->lvl_last : c->hist_win;
}

// where a level's records come from at time tq (s): mode 0 = cumulative - *sub (nullptr: nothing to subtract), 1 = empty, 2 = copy of *sub
void level_source(gys_ctx *c, int level, int64_t tq, int *mode, const gys_hist_rec **sub)
{
	*sub = nullptr;
	if (level == 3) {
		*mode = 0;
	} else if (level == 0) {
		// a 5-s ring keeps an add for 5 s: the window closed last, until a window's length has passed without another close
		if (c->cfg.enable_levels == 1 && c->lvl_t_last >= 0 && tq - c->lvl_t_last < LEVEL_SECS[0]) {
			*mode = 2;
			*sub = c->lvl_last;
		} else {
			*mode = 1;
		}
	} else {
		const int64_t dur = LEVEL_SECS[level];
		const uint32_t oldest = (level_bucket_idx(tq, dur) + 1u) % GYS_LEVEL_RING;
		if (c->lvl_t_last < 0 || level_bucket_start(tq, dur, oldest) > c->lvl_t_last) {
			*mode = 1; // every add is older than the ring's oldest live bucket
		} else {
			*mode = 0;
			*sub = c->lvl_snap + ((uint64_t)(level - 1) * GYS_LEVEL_RING + oldest) * c->cfg.max_services;
		}
	}
}

// device records of one level at time tusec for slots [first, first + n) into d_out
int level_view(gys_ctx *c, int level, uint64_t tusec, uint32_t first, uint32_t n, gys_hist_rec *d_out)
{
	int64_t tq = (int64_t)(tusec / 1000000ull);
	if (tq < c->lvl_t_last) tq = c->lvl_t_last;
	{
		const int rcf = fold_range(c, first, n); // max_val_seen is reported over everything ingested, the open window included
		if (rcf) return rcf;
	}
	LevelViewP p{};
	p.win = c->hist_win;
	p.all = c->hist_all;
	p.meta = c->cfg.enable_tdigest ? c->td_meta : nullptr;
	p.epoch_open = c->epoch + (c->prepared ? 1u : 0u);
	p.first = first;
	p.n = n;
	p.out = d_out;
	level_source(c, level, tq, &p.mode, &p.sub);
	p.last_tag = c->cfg.enable_tdigest ? c->lvl_last_tag : nullptr;
	p.last_epoch = c->lvl_last_epoch;
	hipLaunchKernelGGL(k_level_view, dim3((uint32_t)(((uint64_t)n * 16 + 255) / 256)), dim3(256), 0, c->stream, p);
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

// The plan of TIME_HISTOGRAM::get_stats_for_period_with_flush (common/gy_statistics.h:1378-1413) at tusec: the level that answers, its
// overlapping ring buckets with their scales and boundary snapshots, and the sources of the records -- everything that is the same for every
// service (first / n / out stay the caller's).  start / end are the reference's starttime / endtime + 1 (:1383).  Shared by level_period and
// the group records of a period (gys_rollup_host.hpp); the caller folds the services it reads first (fold_range).
void period_plan(gys_ctx *c, int64_t start, int64_t end, uint64_t tusec, LevelPeriodP &p, int *plevel)
{
	int64_t tq = (int64_t)(tusec / 1000000ull);
	if (tq < c->lvl_t_last) tq = c->lvl_t_last; // the flush: latestTime_ of every level
	p = LevelPeriodP{};
	p.win = c->hist_win;
	p.all = c->hist_all;
	p.meta = c->cfg.enable_tdigest ? c->td_meta : nullptr;
	p.epoch_open = c->epoch + (c->prepared ? 1u : 0u);
	int level = GYS_NLEVELS - 1; // MultiLevelTimeSeries::getLevel(start): the first level that reaches back to start
	for (int l = c->cfg.enable_levels == 1 ? 0 : 1; l < GYS_NLEVELS - 1; ++l) // (enable_levels = 2: no 5-s level, the 300-s ring answers)
		if (tq - LEVEL_SECS[l] <= start) {
			level = l;
			break;
		}
	if (plevel) *plevel = level;
	if (level == 3) {
		p.mode = 3;
		p.first_sec = c->lvl_first;
		p.start = start;
		p.end = end;
		p.latest = tq;
	} else if (level == 0) {
		// the 5-s ring has 1-s buckets: the window closed last sits in [t_last, t_last + 1) for 5 s, inside the interval or not
		const bool held = c->lvl_t_last >= 0 && tq - c->lvl_t_last < LEVEL_SECS[0];
		p.mode = held && start <= c->lvl_t_last && end > c->lvl_t_last ? 2 : 1;
		p.last = c->lvl_last;
		p.last_tag = c->cfg.enable_tdigest ? c->lvl_last_tag : nullptr;
		p.last_epoch = c->lvl_last_epoch;
	} else {
		const int64_t dur = LEVEL_SECS[level], w = dur / GYS_LEVEL_RING;
		const int64_t cur_start = level_bucket_start(tq, dur, level_bucket_idx(tq, dur));
		auto cum_before = [&](int64_t s) -> const gys_hist_rec * { // C(s); nullptr = the cumulative record now
			if (c->lvl_t_last < 0 || s > c->lvl_t_last) return nullptr;
			const uint32_t j = (uint32_t)((s % dur) / w);
			return c->lvl_snap + ((uint64_t)(level - 1) * GYS_LEVEL_RING + j) * c->cfg.max_services;
		};
		p.mode = 0;
		for (int k = 0; k < GYS_LEVEL_RING; ++k) { // BucketedTimeSeries::forEachBucket(start, end, fn), oldest first
			const int64_t bs = cur_start - (int64_t)(GYS_LEVEL_RING - 1 - k) * w;
			int64_t bn = bs + w;
			if (start >= bn) continue;
			if (end <= bs) break;
			if (bs <= tq && bn > tq) bn = tq + 1; // rangeAdjust: the bucket that holds latestTime_ ends there
			const uint32_t i = p.nrb++;
			if (i == 0) p.bnd[0] = cum_before(bs);
			p.bnd[i + 1] = cum_before(bs + w);
			if (start <= bs && end >= bn) {
				p.whole_mask |= 1u << i;
				p.scale[i] = 1.f;
			} else {
				const int64_t is = start > bs ? start : bs, ie = end < bn ? end : bn;
				p.scale[i] = (float)(ie - is) * 1.f / (float)(bn - bs);
			}
		}
		if (!p.nrb) p.mode = 1;
	}
}

// the interval's {count, sum} per histogram bucket for slots [first, first + n) into d_out
int level_period(gys_ctx *c, int64_t start, int64_t end, uint64_t tusec, uint32_t first, uint32_t n, gys_hist_rec *d_out, int *plevel)
{
	{
		const int rcf = fold_range(c, first, n);
		if (rcf) return rcf;
	}
	LevelPeriodP p;
	period_plan(c, start, end, tusec, p, plevel);
	p.first = first;
	p.n = n;
	p.out = d_out;
	hipLaunchKernelGGL(k_level_period, dim3((uint32_t)(((uint64_t)n * 16 + 255) / 256)), dim3(256), 0, c->stream, p);
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

// walk a variable-stride batch on the host (what COMM validate + the reference loops do) and produce record offsets
template <typename SizeFn>
int walk_batch(const uint8_t *batch, uint32_t n, const uint8_t *pend, uint32_t fixed, SizeFn elem_size, std::vector<uint32_t> &offs)
{
	const uint8_t *p = batch;
	offs.clear();
	if (!pend || pend < batch) {
		set_err("batch without an end pointer");
		return GYS_ERR_INVAL;
	}
	if ((uint64_t)n * fixed > (uint64_t)(pend - batch)) { // (before anything is sized by n: every record is at least its fixed part)
		set_err("%u records cannot lie in a batch of %zu bytes", n, (size_t)(pend - batch));
		return GYS_ERR_INVAL;
	}
	offs.reserve(n);
	// the L1 validators' rule (TCP_CONN_NOTIFY::validate / LISTENER_STATE_NOTIFY::validate, common/gy_comm_proto.cc:859-880, :974-995):
	// every one of the n announced records lies complete before pend and has a size that is a multiple of 8; the L2 loop
	// `i < n && p < pend` (gy_mconnhdlr.cc:9130, :11175) only ever sees messages that passed it
	for (uint32_t i = 0; i < n; ++i) {
		if ((size_t)(pend - p) < fixed) {
			set_err("batch ends before record %u of %u", i, n);
			return GYS_ERR_INVAL;
		}
		const uint32_t sz = elem_size(p);
		if ((sz & 7u) || (size_t)(pend - p) < sz) {
			set_err("record %u: bad element size %u", i, sz);
			return GYS_ERR_INVAL;
		}
		offs.push_back((uint32_t)(p - batch));
		p += sz;
	}
	return GYS_OK;
}

int run_conn(gys_ctx *c, const uint8_t *d_batch, const uint32_t *d_offsets, uint32_t n)
{
	if (!n) return GYS_OK;
	ConnP p{};
	p.batch = d_batch;
	p.offsets = d_offsets;
	p.n = n;
	p.gid = c->gid_tbl;
	p.hll32 = c->hll32;
	p.cms32 = (uint32_t *)(c->arena + c->al.off_u32) + c->al.u32_cms;
	p.cms64 = (unsigned long long *)(c->arena + c->al.off_i64sum) + c->al.i64_cms;
	p.svc_win = c->svc_win;
	if (c->cfg.conn_pair_cms) {
		p.pair32 = (uint32_t *)(c->arena + c->al.off_u32) + c->al.u32_cpair;
		p.pair64 = (unsigned long long *)(c->arena + c->al.off_i64sum) + c->al.i64_cpair;
		p.cpair32 = p.pair32 + (uint64_t)GYS_CMS_D * GYS_CMS_W;
		p.cpair64 = p.pair64 + (uint64_t)GYS_CMS_D * GYS_CMS_W;
	}
	c->conn_dirty = true;
	p.counters = c->counters;
	ProfScope ps(c, "conn");
	p.span = conn_span(n, c->ncu);
	hipLaunchKernelGGL(k_conn_ingest, dim3((n + p.span - 1) / p.span), dim3(GYS_CONN_THREADS), 0, c->stream, p);
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

// folds the connection path's per-service window accumulators (cumulative counters, Count-Min rows)
int conn_fold(gys_ctx *c)
{
	if (!c->conn_dirty || !c->nsvc) return GYS_OK;
	hipLaunchKernelGGL(k_conn_fold, dim3((c->nsvc + 255) / 256), dim3(256), 0, c->stream, c->svc_win, c->svc_ctr, c->svc_gid, c->nsvc,
			   (uint32_t *)(c->arena + c->al.off_u32) + c->al.u32_cms, (unsigned long long *)(c->arena + c->al.off_i64sum) + c->al.i64_cms);
	HIPCHK(hipGetLastError());
	c->conn_dirty = false;
	return GYS_OK;
}

int actp_ingest(gys_ctx *c, const uint8_t *d_batch, uint32_t n); // gys_actpairs_host.hpp

int run_actconn(gys_ctx *c, const uint8_t *d_batch, uint32_t n)
{
	if (!n) return GYS_OK;
	ActConnP p{};
	p.batch = d_batch;
	p.n = n;
	p.gid = c->gid_tbl;
	p.pair32 = (uint32_t *)(c->arena + c->al.off_u32) + c->al.u32_pair;
	p.pair64 = (unsigned long long *)(c->arena + c->al.off_i64sum) + c->al.i64_pair;
	p.svc_act = c->svc_act;
	p.counters = c->counters;
	p.win_rows = (uint32_t *)(c->arena + c->al.off_u32) + c->al.u32_misc;
	ProfScope ps(c, "actconn");
	hipLaunchKernelGGL(k_actconn_ingest, dim3((n + 255) / 256), dim3(256), 0, c->stream, p);
	HIPCHK(hipGetLastError());
	return c->ap_entries ? actp_ingest(c, d_batch, n) : GYS_OK;
}

// builds the window's Count-Min rows of the response path from the per-service event counts ("Count-Min rows of the window" in
// gys_kernels.hpp); the counts start the next window from zero
int resp_cms_fold(gys_ctx *c)
{
	if (!c->resp_dirty || !c->nsvc || !c->resp_win) return GYS_OK;
	const uint32_t nch = std::max(1u, std::min<uint32_t>(c->cms_nch, (c->nsvc + 65535u) / 65536u));
	uint32_t *cms32 = (uint32_t *)(c->arena + c->al.off_u32) + c->al.u32_cms;
	hipLaunchKernelGGL(k_cms_partial, dim3(nch, GYS_CMS_D * 2), dim3(1024), GYS_CMSF_CELLS * 4, c->stream, c->resp_win, c->svc_gid, c->nsvc, nch, c->cms_partial);
	hipLaunchKernelGGL(k_cms_reduce, dim3((GYS_CMS_D * GYS_CMS_W + 255) / 256), dim3(256), 0, c->stream, c->cms_partial, nch, cms32);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemsetAsync(c->resp_win, 0, (uint64_t)c->nsvc * 4, c->stream));
	c->resp_dirty = false;
	return GYS_OK;
}

int run_lstate(gys_ctx *c, const uint8_t *d_batch, const uint32_t *d_offsets, const uint32_t *d_host_slot, uint32_t single_host, uint32_t n)
{
	if (!n) return GYS_OK;
	LStateP p{};
	p.batch = d_batch;
	p.offsets = d_offsets;
	p.host_slot = d_host_slot;
	p.single_host = single_host;
	p.n = n;
	p.gid = c->gid_tbl;
	p.svc_state = c->svc_state;
	p.host_summ = c->host_summ_win;
	p.epoch = c->epoch;
	p.counters = c->counters;
	p.qps_hist = c->qps_hist;
	p.act_hist = c->act_hist;
	ProfScope ps(c, "lstate");
	p.claim = c->svc_claim;
	if (++c->lstate_launch == 0) { // (enq_mu or the exclusive call lock is held; 0 = the cleared claim table)
		// the call counter wrapped (2^32 calls: weeks of a large site's messages): claims of old calls would now outrank every new one
		c->lstate_launch = 1;
		HIPCHK(hipMemsetAsync(c->svc_claim, 0, (uint64_t)c->cfg.max_services * 8, c->stream));
	}
	p.launch = c->lstate_launch;
	if (n <= GYS_LSTATE_FUSED_MAX) { // a partha's message: one launch (the per-message path is launch-bound)
		hipLaunchKernelGGL(k_lstate_both, dim3(1), dim3(GYS_LSTATE_FUSED_MAX), 0, c->stream, p);
	} else {
		hipLaunchKernelGGL(k_lstate_ingest, dim3((n + 255) / 256), dim3(256), 0, c->stream, p);
		hipLaunchKernelGGL(k_lstate_keep, dim3((n + 255) / 256), dim3(256), 0, c->stream, p);
	}
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

// ---- host-pointer boundary (gys_subq.hpp: the queues' protocol and the staging ring are described there)
// the launch of a submission queue's copied batch (IngestEnv::launch; enq_mu is held)
int launch_batch(gys_ctx *c, SubQ::Kind kind, const uint8_t *dev, uint64_t fill, uint32_t nrec, const std::vector<gys_resp_seg> &segs)
{
	if (kind == SubQ::RESP) return run_resp_batch(c, segs.data(), (uint32_t)segs.size(), dev, fill);
	const SubQ &q = c->sq[kind];
	const uint32_t *d_offs = (const uint32_t *)(dev + q.cap);
	return kind == SubQ::CONN ? run_conn(c, dev, d_offs, nrec) : run_lstate(c, dev, d_offs, d_offs + q.cap_recs, 0, nrec);
}

// a record message: combined with the other callers' pending messages, unless it has many messages' size (a replayed backlog) -- then on
// its own through the staging ring, behind what the queue holds
int ingest_records(gys_ctx *c, SubQ &q, uint32_t host, const void *batch, const void *pend, const std::vector<uint32_t> &offs)
{
	const uint64_t bytes = (uint64_t)((const uint8_t *)pend - (const uint8_t *)batch);
	const uint32_t n = (uint32_t)offs.size();
	if (align_up(bytes, 8) <= q.cap / 2 && n <= q.cap_recs / 2) return subq_ingest(c->ingest, q, host, c->hosts.size(), batch, bytes, n, offs.data());
	const int rc = subq_flush(c->ingest, q);
	if (rc) return rc;
	// one pinned copy, one H2D copy on the copy stream (records, then the offsets behind them), the ingest kernel, no wait
	const uint64_t off_at = align_up(bytes, 8);
	return stage_call(
		c->ingest, c->ring, off_at + (uint64_t)n * 4,
		[&](uint8_t *pinned) {
			memcpy(pinned, batch, bytes);
			memcpy(pinned + off_at, offs.data(), (uint64_t)n * 4);
		},
		true, "ingest",
		[&](const uint8_t *dev) {
			const uint32_t *d_offs = (const uint32_t *)(dev + off_at);
			return q.kind == SubQ::CONN ? run_conn(c, dev, d_offs, n) : run_lstate(c, dev, d_offs, nullptr, host, n);
		});
}

// a response call as its own submission through the staging ring, behind whatever the response queue holds (same-host calls keep their
// order: a service's per-call value multisets keep the order of the calls); `fn`: the entry point, for the error text
int ingest_staged_resp(gys_ctx *c, uint32_t host, const void *ev, uint32_t nevents, uint32_t evsize, bool v6, const char *fn)
{
	const int rc = subq_flush(c->ingest, c->sq[SubQ::RESP]);
	if (rc) return rc;
	const uint64_t bytes = (uint64_t)nevents * evsize;
	return stage_call(
		c->ingest, c->ring, bytes, [&](uint8_t *pinned) { memcpy(pinned, ev, bytes); }, false, fn,
		[&](const uint8_t *dev) {
			gys_resp_seg seg{host, 0, 0};
			return run_resp_batch(c, &seg, 1, dev, nevents, v6);
		});
}

} // namespace

// ==================================================================================================== C ABI
// Every entry point makes the context's device the calling thread's current device first: the reference's L2 threads (and a process that
// holds one context per GPU) call in with whatever device they used last, and allocations / launches follow the CURRENT device.
#define GYS_ENTER_NOFLUSH(c)                                                   \
	do {                                                                   \
		if ((c) && hipSetDevice((c)->device) != hipSuccess) {          \
			set_err("hipSetDevice(%d) failed", (c)->device);      \
			return GYS_ERR_HIP;                                    \
		}                                                              \
	} while (0)
// ... and, except for the host-pointer ingest calls that may run concurrently, puts whatever the submission queues still hold on the
// stream first (stream order = call order for everything that reads or closes state)
#define GYS_ENTER(c)                                                           \
	do {                                                                   \
		GYS_ENTER_NOFLUSH(c);                                          \
		if (c)                                                         \
			for (auto &q_ : (c)->sq) {                             \
				const int rcq_ = subq_flush((c)->ingest, q_);  \
				if (rcq_) return rcq_;                         \
			}                                                      \
	} while (0)

// "Nothing throws across the boundary" (include/gysketch.h): the host side uses std::vector / std::string / std::thread, whose failures
// are C++ exceptions.  Every int-returning entry point is a function-try-block that turns them into an error code + gys_last_error() text.
#define GYS_CATCH_ALL                                                                                  \
	catch (const std::bad_alloc &)                                                                 \
	{                                                                                              \
		set_err("out of host memory");                                                         \
		return GYS_ERR_NOMEM;                                                                  \
	}                                                                                              \
	catch (const std::exception &ex_)                                                              \
	{                                                                                              \
		set_err("internal error: %s", ex_.what());                                             \
		return GYS_ERR_INTERNAL;                                                               \
	}                                                                                              \
	catch (...)                                                                                    \
	{                                                                                              \
		set_err("internal error");                                                             \
		return GYS_ERR_INTERNAL;                                                               \
	}


extern "C" {

uint32_t gys_abi_version(void) { return GYS_ABI_VERSION; }
const char *gys_last_error(void) { return g_err; }

uint32_t gys_machine_id_hash(const uint8_t machine_id[16]) { return (uint32_t)MachIdHash()(to_machid(machine_id)); }
uint32_t gys_shard_of(const uint8_t machine_id[16], uint32_t nshards) { return nshards ? gys_machine_id_hash(machine_id) % nshards : 0; }

uint64_t gys_reduce_arena_bytes(const gys_config *cfg) { return arena_layout(cfg ? cfg->max_clusters : 1, cfg && cfg->conn_pair_cms).total; }

int gys_create(const gys_config *cfg, gys_ctx **out)
try {
	if (!cfg || !out || cfg->struct_size != sizeof(gys_config)) {
		set_err("bad config (struct_size %u, expected %zu)", cfg ? cfg->struct_size : 0, sizeof(gys_config));
		return GYS_ERR_INVAL;
	}
	if (!cfg->max_hosts || !cfg->max_services || cfg->max_hosts > 65534 || !cfg->max_clusters || cfg->nranks == 0 || cfg->rank >= cfg->nranks ||
	    (cfg->svc_hll_p && (cfg->svc_hll_p < 4 || cfg->svc_hll_p > 10)) || cfg->svc_hll_levels > 1 || (cfg->svc_hll_levels && !cfg->svc_hll_p) ||
	    (cfg->td_pend_cap && (cfg->td_pend_cap < 64u || cfg->td_pend_cap > GYS_TD_PEND_CAP_MAX)) || cfg->actconn_pair_cap > (1u << 30) ||
	    (cfg->td_buf_values && (cfg->td_buf_values < (cfg->td_pend_cap ? cfg->td_pend_cap : GYS_TD_PEND_CAP) + 64u || cfg->td_buf_values > GYS_PCAP_MAX))) {
		set_err("bad config values");
		return GYS_ERR_INVAL;
	}
	int ndev = 0;
	HIPCHK(hipGetDeviceCount(&ndev)); // fails loudly when there is no GPU: there is no CPU path
	if (ndev <= 0) {
		set_err("no HIP device");
		return GYS_ERR_HIP;
	}
	// the context is destroyed on every early return below; released at `*out = c`.  A failed create also takes the runtime's "last error"
	// with it (an invalid device ordinal, say): the caller has the code and the text, and the thread's next HIP user -- whose launch
	// check reads hipGetLastError -- must not find this one
	std::unique_ptr<gys_ctx, void (*)(gys_ctx *)> guard(new gys_ctx(), [](gys_ctx *dead) {
		gys_destroy(dead);
		(void)hipGetLastError();
	});
	gys_ctx *c = guard.get();
	c->cfg = *cfg;
	if (cfg->device >= 0) {
		c->device = cfg->device;
		HIPCHK(hipSetDevice(c->device));
	} else {
		HIPCHK(hipGetDevice(&c->device));
	}
	hipDeviceProp_t prop;
	HIPCHK(hipGetDeviceProperties(&prop, c->device));
	c->ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	if (cfg->stream) {
		c->stream = (hipStream_t)cfg->stream;
	} else {
		HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
		c->own_stream = true;
	}
	HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking)); // H2D copies of the host-pointer submissions
	c->ingest.device = c->device;
	c->ingest.stream = c->stream;
	c->ingest.copy_stream = c->copy_stream;
	c->ingest.enq_mu = &c->enq_mu;
	c->ingest.max_batch_events = cfg->max_batch_events;
	c->ingest.launch = [c](SubQ::Kind kind, const uint8_t *dev, uint64_t fill, uint32_t nrec, const std::vector<gys_resp_seg> &segs) {
		return launch_batch(c, kind, dev, fill, nrec, segs);
	};
	for (SubQ::Kind k : {SubQ::RESP, SubQ::CONN, SubQ::LSTATE}) subq_init(c->ingest, c->sq[k], k);
	const uint64_t S = cfg->max_services, H = cfg->max_hosts;
	const uint32_t cap = next_pow2(S * 2);
	int rc;
#define ALLOC(buf, count) \
	if ((rc = buf.alloc(count)) != GYS_OK) return rc;
	ALLOC(c->lk_ent, cap);
	ALLOC(c->gid_ent, cap);
	c->lk_tbl.ent = c->lk_ent;
	c->gid_tbl.ent = c->gid_ent;
	c->lk_tbl.mask = c->gid_tbl.mask = cap - 1;
	HIPCHK(hipMemset(c->lk_tbl.ent, 0xFF, (uint64_t)cap * sizeof(TblEnt)));
	HIPCHK(hipMemset(c->gid_tbl.ent, 0xFF, (uint64_t)cap * sizeof(TblEnt)));
	ALLOC(c->svc_gid, S);
	ALLOC(c->hist_win, S);
	ALLOC(c->hist_all, S);
	ALLOC(c->bitmap, S * GYS_BM_WORDS);
	ALLOC(c->svc_ctr, S * 4);
	ALLOC(c->svc_win, S * 3);
	ALLOC(c->svc_state, S * 96);
	ALLOC(c->svc_claim, S);
	ALLOC(c->hll32, (uint64_t)1 << GYS_HLL_P);
	ALLOC(c->host_summ_win, H * 16);
	ALLOC(c->host_summ_last, H * 16);
	ALLOC(c->host_state, H);
	ALLOC(c->host_state_epoch, H);
	ALLOC(c->host_cluster, H);
	ALLOC(c->counters, 32);
	ALLOC(c->d_epoch, 4);
	ALLOC(c->misc, 16);
	ALLOC(c->svc_act, S * 4);
	ALLOC(c->topn_slot, S < 65536 ? S : 65536);
	ALLOC(c->topn_metric, S < 65536 ? S : 65536);
	ALLOC(c->dev_pcts, 64);
	c->htbl_cap = 16 * S + 64 * H; // every host's live sub-table (<= 8 L + 16 entries: a quarter full) plus its outgrown regions (< the live one)
	c->hlst_cap = 8 * S + 32 * H;
	ALLOC(c->htbl, c->htbl_cap);
	ALLOC(c->hlst, c->hlst_cap);
	c->hdesc_ext_cap = (uint32_t)(S / GYS_HOST_MAX_LOCAL) * 4u + 64u; // parts of many-listener hosts (incl. abandoned cuts)
	ALLOC(c->hdesc, H + c->hdesc_ext_cap);
	ALLOC(c->svc_host, S);
	ALLOC(c->host_spill, H);
	c->host_lst.reserve(H);
	// k_resp_host: up to 4096 sub-table entries (32 KiB) + 2048 x 24 B of per-key areas (48 KiB) + the tile image (48 or 96 KiB)
	c->resp_dyn_max = 160u * 1024u;
	HIPCHK((resp_host_lds_attr<8, false, false>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<8, true, false>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<8, true, true>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<16, false, false>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<16, true, false>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<16, true, true>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<12, false, false>(&c->resp_dyn_max))); // (half of the room per workgroup, two per CU)
	HIPCHK((resp_host_lds_attr<12, true, false>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<12, true, true>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<16, false, false, 1>(&c->resp_dyn_max))); // keys with candidates (bound-address listeners)
	HIPCHK((resp_host_lds_attr<16, true, false, 1>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<16, true, true, 1>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<16, false, false, 2>(&c->resp_dyn_max))); // IPv6 events
	HIPCHK((resp_host_lds_attr<16, true, false, 2>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<16, true, true, 2>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<8, false, false, 1>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<8, true, false, 1>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<8, true, true, 1>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<8, false, false, 2>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<8, true, false, 2>(&c->resp_dyn_max)));
	HIPCHK((resp_host_lds_attr<8, true, true, 2>(&c->resp_dyn_max)));
	c->host_seen.reserve(H);
	if (cfg->svc_hll_p) ALLOC(c->svc_hll, S << cfg->svc_hll_p);
	if (cfg->svc_hll_levels) ALLOC(c->hl_lvl, ((uint64_t)GYS_HLL_LVL_FILES * S) << cfg->svc_hll_p);
	if (cfg->actconn_pair_cap) {
		c->ap_entries = next_pow2(std::max<uint64_t>((uint64_t)cfg->actconn_pair_cap * 2, 16));
		for (int b = 0; b < 2; ++b) {
			ALLOC(c->ap_key[b], c->ap_entries);
			ALLOC(c->ap_ent[b], c->ap_entries);
			HIPCHK(hipMemset(c->ap_key[b].p, 0xFF, (uint64_t)c->ap_entries * sizeof(ActPairKey)));
		}
		ALLOC(c->ap_ctr, APC_NUM);
	}
	if (cfg->enable_levels) {
		ALLOC(c->lvl_snap, 2 * GYS_LEVEL_RING * S);
		ALLOC(c->lvl_last, cfg->enable_levels == 1 ? S : 1);
		ALLOC(c->lvl_last_tag, cfg->enable_levels == 1 && cfg->enable_tdigest ? S : 1);
		ALLOC(c->lvl_first, S);
		ALLOC(c->qps_hist, S);
		ALLOC(c->act_hist, S);
	}
	if (cfg->enable_tdigest) {
		const uint64_t B = cfg->max_batch_events ? cfg->max_batch_events : 1;
		// value buffer of a service: GYS_TD_PEND_CAP values wait for a merge, the rest is room for one batch's values of the service
		// (a batch that does not fit takes the slower spill path); sized to the services, within ~40 GiB unless the caller says otherwise
		c->pend_cap = cfg->td_pend_cap ? cfg->td_pend_cap : GYS_TD_PEND_CAP;
		// the fast merge class: the smallest k_digest_bins instance (merges of 1024 / 2048 / 4096 values) that leaves 128 values of room above the
		// buffer size (896 -> 1024 = GYS_TDIGEST_MERGE_FAST); a service is re-clustered early when another batch like its last would pass it
		c->merge_fast = c->pend_cap + 128u <= 1024u ? 1024u : c->pend_cap + 128u <= 2048u ? 2048u : 4096u;
		if (cfg->td_buf_values) {
			c->pcap = cfg->td_buf_values;
		} else {
			const uint64_t fit = ((40ull << 30) / (4 * S)) / 256 * 256;
			// (at least the fast merge size; with a larger buffer than the default also a quarter of the default's room on top: a service that
			// brings more values per batch than the room above td_pend_cap takes the predicted-run / spill paths every time it is nearly full)
			const uint64_t floor_cap = c->pend_cap > GYS_TD_PEND_CAP ? align_up(c->merge_fast, 256) + 256 : align_up(c->merge_fast, 256);
			c->pcap = (uint32_t)std::min<uint64_t>(GYS_PCAP_MAX, std::max<uint64_t>(floor_cap, fit));
		}
		ALLOC(c->td_sum, S * GYS_TD_NB);
		ALLOC(c->td_cnt, S * GYS_TD_NB);
		ALLOC(c->td_meta, S);
		ALLOC(c->td_minmax, S);
		ALLOC(c->td_cur, align_up(S, 64));
		ALLOC(c->td_run, S);
		if ((rc = c->td_pend.alloc(S * c->pcap, false)) != GYS_OK) return rc; // never read before written: no clear of (up to) tens of GB
		ALLOC(c->merge_list, std::min<uint64_t>(S, B) + 1);
		ALLOC(c->merge_list_slow, S + 1); // (the all-service scan may list any service)
		// a key lands in a larger merge size class only when the batch itself brought it more than CLASS0 - PEND_CAP values
		ALLOC(c->merge_list1, std::min<uint64_t>(S, B / (c->merge_fast - c->pend_cap) + 1) + 1);
		ALLOC(c->merge_list2, std::min<uint64_t>(S, B / (GYS_MERGE_CLASS1 - c->pend_cap) + 1) + 1);
		ALLOC(c->resp_win, S);
		c->cms_nch = (uint32_t)std::min<uint64_t>(32, (S + 65535) / 65536);
		ALLOC(c->cms_partial, (uint64_t)c->cms_nch * GYS_CMS_D * GYS_CMS_W);
		HIPCHK(hipFuncSetAttribute((const void *)k_cms_partial, hipFuncAttributeMaxDynamicSharedMemorySize, GYS_CMSF_CELLS * 4));
		// (entries above merge size class 1 take the several-workgroup path: the batch itself brought such a key more than CLASS1 - PEND_CAP values)
		c->huge_list_cap = std::min<uint64_t>(S, B / (GYS_MERGE_CLASS1 - c->pend_cap) + 1);
		ALLOC(c->huge_list, c->huge_list_cap + 1);
		ALLOC(c->query_list, 4);
		ALLOC(c->merge_count, FIN_NWORDS);
		ALLOC(c->query_sum, GYS_TD_NB);
		ALLOC(c->query_cnt, GYS_TD_NB);
		ALLOC(c->batch_cnt, align_up(S, 16));
		ALLOC(c->batch_off, align_up(S, 16));
		ALLOC(c->scan_block_sums, (S + GYS_SCAN_TILE - 1) / GYS_SCAN_TILE + 1);
		ALLOC(c->ev_kv, B);
		// `staged`: the runs of one batch.  With predicted runs (k_prespill) a batch may need the predicted runs (the last batch's counts
		// plus a quarter, + 64 per key) AND the exact runs of the keys the prediction missed (<= B): 5/2 B + slack, while indices stay 32-bit
		c->prespill = B * 5 / 2 + (1u << 24) < (1ull << 32);
		if ((rc = c->staged.alloc(c->prespill ? B * 5 / 2 + (1u << 24) : B, false)) != GYS_OK) return rc; // (runs are written before they are read)
		if (c->prespill) {
			ALLOC(c->td_run0, S);
			ALLOC(c->td_run1, S);
			ALLOC(c->td_prevm, S);
			ALLOC(c->pre_hot, 2);
			ALLOC(c->host_batch, H);
			// S + 1 entries (a key has at most one entry per batch; the keys of a batch are not bounded by its size: predictions come from EARLIER batches)
			ALLOC(c->append_list, S + 1);
		}
		c->huge_blocks = (int)std::min<uint64_t>(64, std::min<uint64_t>(S, B / GYS_MERGE_LDS_MAX + 1));
		if (c->huge_blocks < 1) c->huge_blocks = 1;
		// the several-workgroup path's pool shares the scratch: 64 KiB of bins per entry, up to 262 144 entries (16 GiB of 288) when the batches can
		// carry that many large keys; the one-workgroup fallback needs huge_blocks x 4 MiB of it
		c->huge_maxent = (uint32_t)std::max<uint64_t>((uint64_t)c->huge_blocks * GYS_HUGE_BINS / GYS_HB_BINS, std::min<uint64_t>(c->huge_list_cap, 262144)); // <= 16 GiB of bins: one round for a 2^29-event batch (167 773 possible entries) instead of eleven sets of empty launches
		const uint64_t scratch_entries = c->huge_maxent;
		if (const char *e = getenv("GYS_HUGE_MAXENT")) { // tests: a small pool, so that a modest batch walks its large keys in several rounds
			const long v = atol(e);
			if (v >= 1 && (uint64_t)v < c->huge_maxent) c->huge_maxent = (uint32_t)v;
		}
		ALLOC(c->huge_scratch, scratch_entries * GYS_HB_BINS);
		ALLOC(c->huge_acc, (uint64_t)c->huge_maxent * GYS_HB_ACC);
		ALLOC(c->huge_bm, (uint64_t)c->huge_maxent * GYS_BM_WORDS);
		ALLOC(c->huge_chunk_off, (uint64_t)c->huge_maxent + 1);
		ALLOC(c->huge_tail, (uint64_t)GYS_HB_TAIL_CAP);
		ALLOC(c->huge_tb_list, (uint64_t)c->huge_maxent);
		ALLOC(c->huge_fb_list, std::min<uint64_t>(S, B / (GYS_MERGE_CLASS1 - c->pend_cap) + 1) + 1);
		HIPCHK(hipFuncSetAttribute((const void *)k_huge_count, hipFuncAttributeMaxDynamicSharedMemorySize, GYS_HB_BINS * 4));
		HIPCHK(hipFuncSetAttribute((const void *)k_huge_merge<512, GYS_HB_TAIL_A, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (GYS_HB_BINS + GYS_HB_TAIL_A) * 4));
		HIPCHK(hipFuncSetAttribute((const void *)k_huge_merge<1024, GYS_HB_TAIL_LDS, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (GYS_HB_BINS + GYS_HB_TAIL_LDS) * 4));
	}
	ALLOC(c->last_act32, 2ull * GYS_CMS_D * GYS_CMS_W);
	ALLOC(c->last_act64, 2ull * GYS_CMS_D * GYS_CMS_W);
	ALLOC(c->ring_act32, 2ull * GYS_ACT_RING * GYS_CMS_D * GYS_CMS_W);
	ALLOC(c->ring_act64, 2ull * GYS_ACT_RING * GYS_CMS_D * GYS_CMS_W);
	ALLOC(c->act_live, 2);
#undef ALLOC
	// dev_alloc zeroes with hipMemset on the NULL stream, which may still be in flight; the context stream is non-blocking, so the
	// initialisation kernels / copies below must not start before every one of those clears has landed
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(c->d_epoch, &c->epoch, 4, hipMemcpyHostToDevice));
	if (cfg->enable_tdigest) {
		hipLaunchKernelGGL(k_minmax_init, dim3(grid_for(S, 256, 2048)), dim3(256), 0, c->stream, c->td_minmax, S);
		static const uint32_t one = 1; // static: the source of an async copy must outlive the call
		HIPCHK(hipMemcpyAsync(c->merge_count + FIN_QUERY_ONE, &one, 4, hipMemcpyHostToDevice, c->stream));
	}
	hipLaunchKernelGGL(k_hist_init, dim3(grid_for(S, 256, 2048)), dim3(256), 0, c->stream, c->hist_win, (uint64_t)0, S, (int64_t)INT64_MIN);
	hipLaunchKernelGGL(k_hist_init, dim3(grid_for(S, 256, 2048)), dim3(256), 0, c->stream, c->hist_all, (uint64_t)0, S, (int64_t)INT64_MIN);
	if (cfg->enable_levels) {
		if (cfg->enable_levels == 1) hipLaunchKernelGGL(k_hist_init, dim3(grid_for(S, 256, 2048)), dim3(256), 0, c->stream, c->lvl_last, (uint64_t)0, S, (int64_t)INT64_MIN);
		if (cfg->enable_levels == 1 && cfg->enable_tdigest) HIPCHK(hipMemsetAsync(c->lvl_last_tag, 0xFF, (size_t)S * 4, c->stream)); // (no window closed yet)
		c->lvl_last_epoch = 0xFFFFFFFEu;
		// GY_HISTOGRAM<int, ...>: max_val_seen_ starts at std::numeric_limits<int>::min()
		hipLaunchKernelGGL(k_hist_init, dim3(grid_for(S, 256, 2048)), dim3(256), 0, c->stream, c->qps_hist, (uint64_t)0, S, (int64_t)INT32_MIN);
		hipLaunchKernelGGL(k_hist_init, dim3(grid_for(S, 256, 2048)), dim3(256), 0, c->stream, c->act_hist, (uint64_t)0, S, (int64_t)INT32_MIN);
	}
	c->al = arena_layout(cfg->max_clusters, cfg->conn_pair_cms != 0);
	if (cfg->reduce_arena) {
		if (cfg->reduce_arena_bytes < c->al.total) {
			set_err("reduce_arena too small: %llu < %llu", (unsigned long long)cfg->reduce_arena_bytes, (unsigned long long)c->al.total);
			return GYS_ERR_INVAL;
		}
		c->arena = (uint8_t *)cfg->reduce_arena;
	} else {
		if ((rc = c->arena_own.alloc(c->al.total, false)) != GYS_OK) return rc;
		c->arena = c->arena_own;
	}
	if ((rc = c->last.alloc(c->al.total, false)) != GYS_OK) return rc;
	HIPCHK(hipMemsetAsync(c->arena, 0, c->al.total, c->stream));
	HIPCHK(hipMemsetAsync(c->last, 0, c->al.total, c->stream));
	{
		HIPCHK(hipMemcpyAsync(c->arena + c->al.off_i64max, &c->i64min, 8, hipMemcpyHostToDevice, c->stream));
	}
	HIPCHK(hipStreamSynchronize(c->stream));
	*out = guard.release();
	return GYS_OK;
} GYS_CATCH_ALL

void gys_destroy(gys_ctx *c)
{
	if (c) (void)hipSetDevice(c->device);
	if (!c) return;
	// the flushers joined, the stream drained, the graphs and then the events destroyed, the streams last
	ingest_teardown(c->sq, 3, c->ring, [c] {
		if (c->stream) hipStreamSynchronize(c->stream);
		if (c->win_graph_exec) hipGraphExecDestroy(c->win_graph_exec);
		if (c->win_graph) hipGraphDestroy(c->win_graph);
		for (auto &cg : c->close_graph) {
			if (cg.x) hipGraphExecDestroy(cg.x);
			if (cg.g) hipGraphDestroy(cg.g);
		}
		for (auto &sl : c->seg_ring) {
			if (sl.done) hipEventDestroy(sl.done);
		}
	});
	if (c->copy_stream) hipStreamDestroy(c->copy_stream);
	prof_resolve(c);
	if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
	delete c; // (frees all device and pinned memory: the members' destructors)
}

int gys_sync(gys_ctx *c)
try {
	GYS_ENTER(c);
	if (!c) return GYS_ERR_INVAL;
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ registration
int gys_register_cluster(gys_ctx *c, const char *cluster_name, uint32_t *cluster_idx)
try {
	GYS_ENTER(c);
	if (!c || !cluster_name) return GYS_ERR_INVAL;
	auto it = c->cluster_map.find(cluster_name);
	if (it == c->cluster_map.end()) {
		if (c->cluster_names.size() >= c->cfg.max_clusters) {
			set_err("max_clusters exhausted");
			return GYS_ERR_NOMEM;
		}
		const uint32_t idx = (uint32_t)c->cluster_names.size();
		c->cluster_names.emplace_back(cluster_name);
		c->registry_gen++; // (one more group, still empty)
		it = c->cluster_map.emplace(cluster_name, idx).first;
	}
	if (cluster_idx) *cluster_idx = it->second;
	return GYS_OK;
} GYS_CATCH_ALL

int gys_register_host(gys_ctx *c, const uint8_t machine_id[16], const char *cluster_name, uint32_t *host_slot)
try {
	GYS_ENTER(c);
	if (!c || !machine_id) return GYS_ERR_INVAL;
	int rc = check_owner(c, machine_id);
	if (rc) return rc;
	uint32_t cidx = 0;
	rc = gys_register_cluster(c, cluster_name ? cluster_name : "", &cidx);
	if (rc) return rc;
	const MachId m = to_machid(machine_id);
	auto it = c->host_map.find(m);
	uint32_t slot;
	if (it != c->host_map.end()) {
		slot = it->second;
	} else {
		if (c->hosts.size() >= c->cfg.max_hosts) {
			set_err("max_hosts exhausted");
			return GYS_ERR_NOMEM;
		}
		slot = (uint32_t)c->hosts.size();
		c->hosts.push_back(m);
		c->host_cluster_h.push_back(cidx);
		c->host_map.emplace(m, slot);
		c->host_lst.emplace_back();
		c->host_names.emplace_back();
		c->host_lst.back().tbl.assign(16, GYS_HOST_TBL_EMPTY);
		c->host_seen.push_back(0);
		c->registry_gen++;
		rc = host_lst_upload(c, slot);
		if (rc) return rc;
	}
	if (c->host_cluster_h[slot] != cidx) c->registry_gen++; // (a repeated registration that changes nothing leaves the cached groupings alone)
	c->host_cluster_h[slot] = cidx;
	HIPCHK(hipMemcpyAsync(c->host_cluster + slot, &cidx, 4, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (host_slot) *host_slot = slot;
	return GYS_OK;
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ deleting listeners (gys_svcdel.hpp)
// every per-service array of the context as k_svc_clear segments, with the contents gys_create leaves and what a service record does with
// the array (gys_svcpack.hpp: C carried, CH carried + host word, R reset by the unpack, K kept).  layout: also the arrays the configuration
// provides for but the context has not allocated yet (base nullptr) -- a record's layout depends on the configuration alone.
static void svc_clear_segments(gys_ctx *c, std::vector<SvcClearSeg> &segs, bool layout = false)
{
	const uint64_t S = c->cfg.max_services;
	const uint4 zero = make_uint4(0u, 0u, 0u, 0u), ones = make_uint4(~0u, ~0u, ~0u, ~0u);
	constexpr uint32_t C = GYS_SVCSEG_CARRY, CH = GYS_SVCSEG_CARRY_HOST, R = GYS_SVCSEG_RESET, K = GYS_SVCSEG_KEEP;
	auto add = [&](void *base, uint64_t bytes, uint4 fill, uint4 last, uint32_t kind) {
		if (base || layout) segs.push_back(SvcClearSeg{(uint8_t *)base, bytes, fill, last, kind, 0u});
	};
	auto hist = [&](gys_hist_rec *base, int64_t minval) { // zero, max_val_seen (the record's last 8 bytes) = minval
		add(base, sizeof(gys_hist_rec), zero, make_uint4(0u, 0u, (uint32_t)(uint64_t)minval, (uint32_t)((uint64_t)minval >> 32)), C);
	};
	add(c->svc_gid, 8, zero, zero, K);
	add(c->svc_host, 4, ones, ones, K);
	hist(c->hist_win, INT64_MIN);
	hist(c->hist_all, INT64_MIN);
	add(c->bitmap, GYS_BM_WORDS * 4, zero, zero, C);
	add(c->svc_ctr, 32, zero, zero, C);
	add(c->svc_win, 24, zero, zero, C);
	add(c->svc_state, 96, zero, zero, CH);
	add(c->svc_claim, 8, zero, zero, R);
	add(c->svc_act, 32, zero, zero, C);
	if (c->svc_hll) add(c->svc_hll, 1ull << c->cfg.svc_hll_p, zero, zero, C);
	if (c->hl_lvl)
		for (uint32_t f = 0; f < GYS_HLL_LVL_FILES; ++f) add(hll_level_array(c, f), 1ull << c->cfg.svc_hll_p, zero, zero, C);
	if (c->cfg.enable_levels) {
		for (uint32_t j = 0; j < 2 * GYS_LEVEL_RING; ++j) add(c->lvl_snap + (uint64_t)j * S, sizeof(gys_hist_rec), zero, zero, C);
		if (c->cfg.enable_levels == 1) hist(c->lvl_last, INT64_MIN);
		if (c->cfg.enable_levels == 1 && c->cfg.enable_tdigest) add(c->lvl_last_tag, 4, ones, ones, C);
		add(c->lvl_first, 8, zero, zero, C);
		hist(c->qps_hist, INT32_MIN);
		hist(c->act_hist, INT32_MIN);
	}
	if (c->cfg.enable_tdigest) {
		add(c->td_sum, GYS_TD_NB * 8ull, zero, zero, C);
		add(c->td_cnt, GYS_TD_NB * 4ull, zero, zero, C);
		add(c->td_meta, sizeof(TdMeta), zero, zero, C);
		const uint4 mm = make_uint4((uint32_t)INT32_MAX, (uint32_t)INT32_MIN, (uint32_t)INT32_MAX, (uint32_t)INT32_MIN);
		add(c->td_minmax, 8, mm, mm, C);
		add(c->td_cur, 4, zero, zero, C); // (the words of td_pend behind a zero cursor are never read)
		add(c->td_run, 4, zero, zero, R);
		add(c->td_run0, 4, zero, zero, R);
		add(c->td_run1, 4, zero, zero, R);
		add(c->td_prevm, 4, zero, zero, C);
		add(c->resp_win, 4, zero, zero, C);
	}
	add(c->svc_label, 4, ones, ones, K); // GYS_NO_GROUP
	add(c->svc_bithist, 2, zero, zero, C);
}

// the segment list and the device memory a clear of listed slots needs (staging_bytes: what the caller puts into dev_staging)
static int svc_clear_prepare(gys_ctx *c, std::vector<SvcClearSeg> &segs, uint64_t staging_bytes)
{
	svc_clear_segments(c, segs);
	if (segs.size() > GYS_SVCCLEAR_MAXSEG) {
		set_err("internal error: %zu clear segments", segs.size());
		return GYS_ERR_INTERNAL;
	}
	const int rc = c->clr_segs.p ? GYS_OK : c->clr_segs.alloc(GYS_SVCCLEAR_MAXSEG, false);
	return rc ? rc : ensure_staging(c, staging_bytes, 0);
}
// d_slots: nslots slot numbers on the device.  segs has to stay alive until the stream has been synchronised.
static int svc_clear_launch(gys_ctx *c, const std::vector<SvcClearSeg> &segs, const uint32_t *d_slots, uint32_t nslots)
{
	HIPCHK(hipMemcpyAsync(c->clr_segs, segs.data(), segs.size() * sizeof(SvcClearSeg), hipMemcpyHostToDevice, c->stream));
	ProfScope ps(c, "svc_clear");
	hipLaunchKernelGGL(k_svc_clear, dim3(std::min<uint32_t>(nslots, (uint32_t)c->ncu * 8u)), dim3(GYS_SVCCLEAR_NT), 0, c->stream, c->clr_segs, (uint32_t)segs.size(), d_slots,
			   nslots, c->cfg.max_services);
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

int gys_delete_listeners(gys_ctx *c, const uint64_t *glob_ids, uint32_t n, uint32_t *ndeleted)
try {
	GYS_ENTER(c); // whatever was ingested before the call is applied to the services before they go
	if (!c || (!glob_ids && n)) return GYS_ERR_INVAL;
	if (ndeleted) *ndeleted = 0;
	// every id is looked up before anything changes; unknown ids and repeats are not counted
	std::vector<uint32_t> del;
	{
		std::unordered_set<uint32_t> seen;
		for (uint32_t i = 0; i < n; ++i) {
			auto it = c->gid_map_h.find(glob_ids[i]);
			if (it != c->gid_map_h.end() && seen.insert(it->second).second) del.push_back(it->second);
		}
	}
	if (del.empty()) return GYS_OK;
	const uint32_t nd = (uint32_t)del.size();
	// ---- whatever can fail for want of memory comes first (at most one lk_tbl key per deleted listener), before the mirror changes
	std::vector<SvcClearSeg> segs;
	int rc = svc_clear_prepare(c, segs, 2ull * nd * 8 + (uint64_t)nd * 4);
	if (rc) return rc;
	// ---- host mirror: the listeners leave their hosts' chains, sub-tables and all_slots; lk_gone = the global-table keys that lose their last listener
	std::unordered_map<uint32_t, std::unordered_set<uint32_t>> by_host;
	for (uint32_t s : del) by_host[c->svc_host_h[s]].insert(s);
	// the touched hosts' mirrors as they were: an error before the device work is done puts them back, so that mirror and device never disagree
	struct MirrorUndo {
		gys_ctx *c;
		std::vector<std::pair<uint32_t, HostListeners>> was;
		bool armed = true;
		~MirrorUndo()
		{
			if (armed)
				for (auto &w : was) c->host_lst[w.first] = std::move(w.second);
		}
	} undo{c};
	undo.was.reserve(by_host.size());
	for (auto &hv : by_host) undo.was.emplace_back(hv.first, c->host_lst[hv.first]);
	std::vector<uint64_t> keys; // [gid_tbl keys: nd][lk_tbl keys]
	for (uint32_t s : del) keys.push_back(c->svc_gid_h[s]);
	for (auto &hv : by_host) {
		const uint32_t host = hv.first;
		std::vector<uint64_t> gone;
		host_lst_remove(c->host_lst[host], hv.second, c->svc_key_h.data(), gone);
		for (uint64_t k : gone) keys.push_back(listener_key(host, (uint32_t)(k >> 16), (uint16_t)(k & 0xFFFFu)));
	}
	// ---- device: the keys leave the tables, the hosts' sub-tables are rebuilt, the slots are cleared -- all behind the drained queues
	const uint32_t nlk = (uint32_t)keys.size() - nd;
	const uint64_t keys_bytes = keys.size() * 8;
	HIPCHK(hipMemcpyAsync(c->dev_staging, keys.data(), keys_bytes, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(c->dev_staging + keys_bytes, del.data(), (size_t)nd * 4, hipMemcpyHostToDevice, c->stream));
	{
		ProfScope ps(c, "table_erase");
		hipLaunchKernelGGL(k_table_erase, dim3(1), dim3(64), 0, c->stream, c->gid_tbl, (const uint64_t *)c->dev_staging.p, nd, (uint32_t *)nullptr);
		if (nlk) hipLaunchKernelGGL(k_table_erase, dim3(1), dim3(64), 0, c->stream, c->lk_tbl, (const uint64_t *)c->dev_staging.p + nd, nlk, (uint32_t *)nullptr);
	}
	rc = svc_clear_launch(c, segs, (const uint32_t *)(c->dev_staging + keys_bytes), nd);
	if (rc) return rc;
	HIPCHK(hipStreamSynchronize(c->stream)); // (keys / del / segs are locals; the staging buffer is reused by host_lst_flush)
	undo.armed = false; // the device has let the listeners go: the mirror follows
	for (uint32_t s : del) {
		c->gid_map_h.erase(c->svc_gid_h[s]);
		c->svc_gid_h[s] = 0;
		c->svc_comm[s] = std::array<char, 16>{};
		c->svc_port_h[s] = 0;
		c->svc_host_h[s] = GYS_NOSLOT;
		c->svc_key_h[s] = 0;
		c->svc_task_h[s] = 0;
		c->free_slots.insert(s);
	}
	c->registry_gen++;
	c->task_gen++;
	if (ndeleted) *ndeleted = nd;
	{
		// (a host whose upload fails here stays marked dirty: host_lst_add and the next delete rebuild its tables from the mirror first)
		ProfScope ps(c, "host_rebuild");
		for (auto &hv : by_host) {
			rc = host_lst_flush(c, hv.first);
			if (rc) return rc;
		}
	}
	return GYS_OK;
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ registering listeners
// The one registration path: the fresh (new, de-duplicated) listeners arr[0 .. n) of `host` take the service slots sl[i].  sl[0 .. nfree)
// are reused slots, the others the tail [nsvc, nsvc + n - nfree).  One staging copy, one synchronisation before the mirror follows.
static int register_fresh(gys_ctx *c, uint32_t host, const gys_listener_info *arr, uint32_t n, const std::vector<uint32_t> &sl, uint32_t nfree)
{
	std::vector<uint64_t> stage(2 * (size_t)n + ((size_t)n + 1) / 2); // [glob ids][listener keys][slot numbers, two to a word]
	for (uint32_t i = 0; i < n; ++i) {
		stage[i] = arr[i].glob_id;
		stage[n + i] = listener_key(host, arr[i].netns, arr[i].port);
	}
	memcpy(stage.data() + 2 * (size_t)n, sl.data(), (size_t)n * 4);
	std::vector<SvcClearSeg> segs;
	int rc = nfree ? svc_clear_prepare(c, segs, stage.size() * 8) : ensure_staging(c, stage.size() * 8, 0);
	if (rc) return rc;
	const uint64_t *d_keys = (const uint64_t *)c->dev_staging.p;
	const uint32_t *d_sl = (const uint32_t *)(d_keys + 2 * (size_t)n);
	HIPCHK(hipMemcpyAsync(c->dev_staging, stage.data(), stage.size() * 8, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemsetAsync(c->misc, 0, 4, c->stream));
	// A free slot is part of every pass over [0, nsvc): a window close that went by while it was free wrote for it what it writes for a
	// registered service without data (the first-close time of the since-start period, the level-0 tag, snapshots).  The slot is handed
	// out as gys_create left it -- a listener's series starts at ITS first close, like a tail slot's -- so it is cleared once more here.
	if (nfree) {
		rc = svc_clear_launch(c, segs, d_sl, nfree);
		if (rc) return rc;
	}
	const dim3 grid((n + 255) / 256), block(256);
	hipLaunchKernelGGL(k_scatter_u64, grid, block, 0, c->stream, c->svc_gid, d_sl, d_keys, n);
	hipLaunchKernelGGL(k_table_insert_vals, grid, block, 0, c->stream, c->gid_tbl, d_keys, d_sl, n, c->misc);
	hipLaunchKernelGGL(k_table_insert_vals, grid, block, 0, c->stream, c->lk_tbl, d_keys + n, d_sl, n, c->misc);
	hipLaunchKernelGGL(k_scatter_const_u32, grid, block, 0, c->stream, c->svc_host, d_sl, host, n);
	uint32_t nfail = 0;
	HIPCHK(hipMemcpyAsync(&nfail, c->misc, 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream)); // (stage / segs are locals)
	if (nfail) {
		set_err("key table full (%u inserts failed)", nfail);
		return GYS_ERR_NOMEM;
	}
	rc = host_lst_add(c, host, arr, n, sl.data());
	if (rc) return rc;
	const uint32_t top = c->nsvc + (n - nfree);
	c->svc_comm.resize(top);
	c->svc_gid_h.resize(top);
	c->svc_port_h.resize(top);
	c->svc_host_h.resize(top);
	c->svc_key_h.resize(top);
	c->svc_task_h.resize(top, 0ull);
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t s = sl[i];
		c->gid_map_h[arr[i].glob_id] = s;
		c->host_lst[host].all_slots.push_back(s);
		memcpy(c->svc_comm[s].data(), arr[i].comm, 16);
		c->svc_gid_h[s] = arr[i].glob_id;
		c->svc_port_h[s] = arr[i].port;
		c->svc_host_h[s] = host;
		c->svc_key_h[s] = host_key48(arr[i].netns, arr[i].port);
		c->svc_task_h[s] = 0;
		c->free_slots.erase(s);
	}
	c->nsvc = top;
	c->registry_gen++;
	c->task_gen++;
	return GYS_OK;
}

int gys_register_listeners(gys_ctx *c, const uint8_t machine_id[16], const gys_listener_info *arr_in, uint32_t n_in, uint32_t *first_slot)
try {
	GYS_ENTER(c);
	if (!c || !machine_id || (!arr_in && n_in)) return GYS_ERR_INVAL;
	uint32_t host;
	int rc = lookup_host(c, machine_id, &host);
	if (rc) return rc;
	// a partha resends NEW_LISTENER after a reconnect: a glob_id the engine already knows keeps its slot (and its histograms, digest,
	// counters); repeats inside one call are dropped as well, so that the device tables never see the same key twice
	std::vector<gys_listener_info> fresh;
	{
		std::unordered_set<uint64_t> seen;
		for (uint32_t i = 0; i < n_in; ++i)
			if (!c->gid_map_h.count(arr_in[i].glob_id) && seen.insert(arr_in[i].glob_id).second) fresh.push_back(arr_in[i]);
	}
	const uint32_t n = (uint32_t)fresh.size();
	if ((uint64_t)c->nsvc + n > c->cfg.max_services) { // (the tail only: this call never takes a free slot)
		set_err("max_services exhausted");
		return GYS_ERR_NOMEM;
	}
	if (first_slot) *first_slot = c->nsvc;
	if (!n) return GYS_OK;
	std::vector<uint32_t> sl(n);
	for (uint32_t i = 0; i < n; ++i) {
		if (fresh[i].glob_id == GYS_EMPTY_KEY) {
			set_err("glob_id ~0 is reserved");
			return GYS_ERR_INVAL;
		}
		sl[i] = c->nsvc + i;
	}
	return register_fresh(c, host, fresh.data(), n, sl, 0);
} GYS_CATCH_ALL

int gys_register_listeners_slots(gys_ctx *c, const uint8_t machine_id[16], const gys_listener_info *arr_in, uint32_t n_in, uint32_t *slots)
try {
	GYS_ENTER(c);
	if (!c || !machine_id || (!arr_in && n_in)) return GYS_ERR_INVAL;
	uint32_t host;
	int rc = lookup_host(c, machine_id, &host);
	if (rc) return rc;
	// known ids keep their slot, repeats inside the call share the first one's
	std::vector<gys_listener_info> fresh;
	std::vector<uint32_t> fresh_of(n_in, GYS_NOSLOT); // arr_in index -> index in fresh (new ids)
	{
		std::unordered_map<uint64_t, uint32_t> seen;
		for (uint32_t i = 0; i < n_in; ++i) {
			if (arr_in[i].glob_id == GYS_EMPTY_KEY) {
				set_err("glob_id ~0 is reserved");
				return GYS_ERR_INVAL;
			}
			if (c->gid_map_h.count(arr_in[i].glob_id)) continue;
			auto ins = seen.emplace(arr_in[i].glob_id, (uint32_t)fresh.size());
			if (ins.second) fresh.push_back(arr_in[i]);
			fresh_of[i] = ins.first->second;
		}
	}
	const uint32_t n = (uint32_t)fresh.size();
	const uint32_t nfree = (uint32_t)std::min<size_t>(n, c->free_slots.size()), ntail = n - nfree;
	if ((uint64_t)c->nsvc + ntail > c->cfg.max_services) {
		set_err("max_services exhausted (%zu free slots)", c->free_slots.size());
		return GYS_ERR_NOMEM;
	}
	std::vector<uint32_t> sl(n);
	{
		auto it = c->free_slots.begin();
		for (uint32_t i = 0; i < nfree; ++i, ++it) sl[i] = *it; // lowest slot number first
		for (uint32_t i = 0; i < ntail; ++i) sl[nfree + i] = c->nsvc + i;
	}
	if (n) {
		rc = register_fresh(c, host, fresh.data(), n, sl, nfree);
		if (rc) return rc;
	}
	if (slots)
		for (uint32_t i = 0; i < n_in; ++i) slots[i] = fresh_of[i] != GYS_NOSLOT ? sl[fresh_of[i]] : c->gid_map_h[arr_in[i].glob_id];
	return GYS_OK;
} GYS_CATCH_ALL

uint32_t gys_num_free_slots(gys_ctx *c) { return c ? (uint32_t)c->free_slots.size() : 0; }

uint64_t gys_svc_state_bytes(gys_ctx *c)
{
	if (!c) return 0;
	std::vector<SvcClearSeg> segs;
	svc_clear_segments(c, segs);
	uint64_t b = 0;
	for (const SvcClearSeg &sg : segs) b += sg.bytes;
	return b;
}

// ------------------------------------------------------------------------------------------------ service records (gys_svcpack.hpp)
namespace {

#define GYS_BLOB_MAGIC 0x42535947u // "GYSB"
#define GYS_BLOB_VERSION 1u
#define GYS_BLOB_PIECE (8ull << 20) // the host-pointer forms move the records through the staging buffer in pieces of about this size

// the 64-byte blob header ("service records" in include/gysketch.h gives the offsets)
struct SvcBlobHdr {
	uint32_t magic, version;
	uint32_t enable_tdigest, td_pend_cap, svc_hll_p, svc_hll_levels, enable_levels;
	uint16_t td_nb, level_ring;
	uint32_t bm_line_bytes, stride;
	uint32_t epoch, n;
	int64_t lvl_t_last, hl_t_last;
};
static_assert(sizeof(SvcBlobHdr) == 64, "the blob header is 64 bytes");

// the record layout of this context's configuration: segs with kind / rec_off filled in, and the kernel's parameters but for the list.
// Carried arrays whose size is a multiple of 16 come first, in list order, then the others (each rounded up to 4 bytes), a pad to 16
// bytes, the td_pend_cap buffered words (padded to 16 bytes).
struct SvcRecLayout {
	std::vector<SvcClearSeg> segs;
	SvcPackP p{};
};

int svc_rec_layout(gys_ctx *c, SvcRecLayout &L)
{
	L.segs.clear();
	L.p = SvcPackP{};
	svc_clear_segments(c, L.segs, true);
	if (L.segs.size() > GYS_SVCCLEAR_MAXSEG) {
		set_err("internal error: %zu record segments", L.segs.size());
		return GYS_ERR_INTERNAL;
	}
	uint64_t off = 0;
	uint32_t cur_off = ~0u;
	for (int pass = 0; pass < 2; ++pass)
		for (SvcClearSeg &sg : L.segs) {
			if (sg.kind < GYS_SVCSEG_CARRY || sg.kind > GYS_SVCSEG_KEEP) { // (an array named in svc_clear_segments without a kind)
				set_err("internal error: per-service array without a record kind");
				return GYS_ERR_INTERNAL;
			}
			if (sg.kind != GYS_SVCSEG_CARRY && sg.kind != GYS_SVCSEG_CARRY_HOST) continue;
			if (((sg.bytes & 15ull) == 0) != (pass == 0)) continue;
			sg.rec_off = (uint32_t)off;
			if (sg.base && sg.base == (uint8_t *)c->td_cur.p) cur_off = sg.rec_off;
			off += align_up(sg.bytes, 4);
		}
	SvcPackP &p = L.p;
	p.nsegs = (uint32_t)L.segs.size();
	p.max_services = c->cfg.max_services;
	p.pad_off = (uint32_t)off;
	p.pend_off = (uint32_t)align_up(off, 16);
	p.stride = p.pend_off;
	if (c->cfg.enable_tdigest) {
		if (cur_off == ~0u || c->pend_cap > c->pcap) {
			set_err("internal error: no cursor in the record layout");
			return GYS_ERR_INTERNAL;
		}
		p.td_pend = c->td_pend;
		p.td_cur = c->td_cur;
		p.pcap = c->pcap;
		p.pend_cap = c->pend_cap;
		p.cur_off = cur_off;
		p.stride = (uint32_t)align_up((uint64_t)p.pend_off + 4ull * c->pend_cap, 16);
	}
	return GYS_OK;
}

inline uint64_t blob_ids_bytes(uint32_t n) { return align_up((uint64_t)n * 8, 16); }

void blob_header(gys_ctx *c, const SvcRecLayout &L, uint32_t n, SvcBlobHdr &h)
{
	memset(&h, 0, sizeof(h));
	h.magic = GYS_BLOB_MAGIC;
	h.version = GYS_BLOB_VERSION;
	h.enable_tdigest = c->cfg.enable_tdigest ? 1u : 0u;
	h.td_pend_cap = c->cfg.enable_tdigest ? c->pend_cap : 0u;
	h.svc_hll_p = c->cfg.svc_hll_p;
	h.svc_hll_levels = c->cfg.svc_hll_levels ? 1u : 0u;
	h.enable_levels = c->cfg.enable_levels;
	h.td_nb = GYS_TD_NB;
	h.level_ring = GYS_LEVEL_RING;
	h.bm_line_bytes = GYS_BM_WORDS * 4;
	h.stride = L.p.stride;
	h.epoch = c->epoch;
	h.n = n;
	h.lvl_t_last = c->lvl_t_last;
	h.hl_t_last = c->hl_t_last;
}

// the slots of the ids: GYS_ERR_INVAL for an unknown (unless skip_unknown: GYS_NOSLOT) or repeated id
int blob_slots(gys_ctx *c, const uint64_t *ids, uint32_t n, bool skip_unknown, std::vector<uint32_t> &slots, uint32_t *nknown)
{
	std::unordered_set<uint64_t> seen;
	seen.reserve(n);
	slots.resize(n);
	uint32_t known = 0;
	for (uint32_t i = 0; i < n; ++i) {
		if (!seen.insert(ids[i]).second) {
			set_err("glob_id %016llx occurs twice", (unsigned long long)ids[i]);
			return GYS_ERR_INVAL;
		}
		auto it = c->gid_map_h.find(ids[i]);
		if (it == c->gid_map_h.end()) {
			if (!skip_unknown) {
				set_err("unknown glob_id %016llx", (unsigned long long)ids[i]);
				return GYS_ERR_INVAL;
			}
			slots[i] = GYS_NOSLOT;
		} else {
			slots[i] = it->second;
			known++;
		}
	}
	if (nknown) *nknown = known;
	return GYS_OK;
}

// records [first, first + cnt) of a call to / from d_recs (16-byte aligned): the slot (and host) words go through the head of the staging
// buffer, which the caller has sized (svc_rec_staging) -- d_recs may lie behind them in the same buffer.  Synchronises the stream.
inline uint64_t svc_rec_words_bytes(uint32_t cnt) { return align_up(2ull * cnt * 4, 256); }

int svc_rec_run(gys_ctx *c, SvcRecLayout &L, bool unpack, const uint32_t *slots, const uint32_t *hosts, uint32_t cnt, uint8_t *d_recs)
{
	if (!cnt) return GYS_OK;
	uint32_t *d_words = (uint32_t *)c->dev_staging.p;
	HIPCHK(hipMemcpyAsync(d_words, slots, (size_t)cnt * 4, hipMemcpyHostToDevice, c->stream));
	if (unpack) HIPCHK(hipMemcpyAsync(d_words + cnt, hosts, (size_t)cnt * 4, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(c->clr_segs, L.segs.data(), L.segs.size() * sizeof(SvcClearSeg), hipMemcpyHostToDevice, c->stream));
	SvcPackP p = L.p;
	p.segs = c->clr_segs;
	p.n = cnt;
	p.slots = d_words;
	p.hosts = d_words + cnt;
	p.recs = d_recs;
	{
		ProfScope ps(c, unpack ? "svc_unpack" : "svc_pack");
		const dim3 grid(std::min<uint32_t>(cnt, (uint32_t)c->ncu * 8u)), block(GYS_SVCPACK_NT);
		if (unpack) hipLaunchKernelGGL(k_svc_unpack, grid, block, 0, c->stream, p);
		else hipLaunchKernelGGL(k_svc_pack, grid, block, 0, c->stream, p);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipStreamSynchronize(c->stream)); // (slots / hosts / L.segs are the caller's locals)
	return GYS_OK;
}

// the device memory a run needs: the segment list's buffer and the staging buffer
int svc_rec_prepare(gys_ctx *c, uint64_t staging_bytes)
{
	const int rc = c->clr_segs.p ? GYS_OK : c->clr_segs.alloc(GYS_SVCCLEAR_MAXSEG, false);
	return rc ? rc : ensure_staging(c, staging_bytes, 0);
}

inline int svc_rec_not_prepared(gys_ctx *c)
{
	if (!c->prepared) return GYS_OK;
	set_err("window prepared: finish the close first");
	return GYS_ERR_STATE;
}

// the two history bytes become engine state with the first decision or the first unpack (as in gys_decide_listener_state_dev): allocated
// and zeroed, which is what a context without them stands for -- before the record layout is built, so that the layout is built once
int svc_bithist_ensure(gys_ctx *c)
{
	if (c->svc_bithist.p) return GYS_OK;
	const int rc = c->svc_bithist.alloc((size_t)c->cfg.max_services * 2, false);
	if (rc) return rc;
	const hipError_t e = hipMemsetAsync(c->svc_bithist, 0, (size_t)c->cfg.max_services * 2, c->stream);
	if (e != hipSuccess) {
		c->svc_bithist.release();
		HIPCHK(e);
	}
	return GYS_OK;
}

// records per piece of the host-pointer forms
inline uint32_t svc_rec_piece(const SvcRecLayout &L, uint32_t n) { return (uint32_t)std::min<uint64_t>(n, std::max<uint64_t>(1, GYS_BLOB_PIECE / L.p.stride)); }

// everything of an unpack that comes before the first store: header, size, fingerprint, the clock rule, the ids.  adopt: the destination
// takes the header's window number and close times.
int blob_validate(gys_ctx *c, const SvcRecLayout &L, const SvcBlobHdr &h, uint64_t blob_bytes, bool *adopt)
{
	if (h.magic != GYS_BLOB_MAGIC) {
		set_err("not a service blob (magic %08x)", h.magic);
		return GYS_ERR_INVAL;
	}
	if (h.version != GYS_BLOB_VERSION) {
		set_err("service blob of layout version %u, this library reads %u", h.version, GYS_BLOB_VERSION);
		return GYS_ERR_INVAL;
	}
	SvcBlobHdr mine;
	blob_header(c, L, h.n, mine);
#define GYS_BLOB_FIELD(f)                                                                                               \
	if (h.f != mine.f) {                                                                                            \
		set_err("service blob: " #f " is %llu, this context has %llu", (unsigned long long)h.f, (unsigned long long)mine.f); \
		return GYS_ERR_STATE;                                                                                   \
	}
	GYS_BLOB_FIELD(enable_tdigest)
	GYS_BLOB_FIELD(td_pend_cap)
	GYS_BLOB_FIELD(svc_hll_p)
	GYS_BLOB_FIELD(svc_hll_levels)
	GYS_BLOB_FIELD(enable_levels)
	GYS_BLOB_FIELD(td_nb)
	GYS_BLOB_FIELD(level_ring)
	GYS_BLOB_FIELD(bm_line_bytes)
	GYS_BLOB_FIELD(stride)
#undef GYS_BLOB_FIELD
	if (blob_bytes != 64ull + blob_ids_bytes(h.n) + (uint64_t)h.n * h.stride) {
		set_err("service blob of %llu bytes, %u records of %u bytes need %llu", (unsigned long long)blob_bytes, h.n, h.stride,
			(unsigned long long)(64ull + blob_ids_bytes(h.n) + (uint64_t)h.n * h.stride));
		return GYS_ERR_INVAL;
	}
	*adopt = false;
	if (h.epoch != c->epoch || h.lvl_t_last != c->lvl_t_last || h.hl_t_last != c->hl_t_last) {
		if (c->have_last || c->clock_adopted) {
			set_err("service blob of window %u (closes at %lld / %lld), this context is in window %u (%lld / %lld)", h.epoch, (long long)h.lvl_t_last,
				(long long)h.hl_t_last, c->epoch, (long long)c->lvl_t_last, (long long)c->hl_t_last);
			return GYS_ERR_STATE;
		}
		if (h.epoch == 0u) {
			set_err("service blob of window 0");
			return GYS_ERR_INVAL;
		}
		*adopt = true;
	}
	return GYS_OK;
}

// the restore case: a context that has not closed a window takes the source's clock
int blob_adopt_clock(gys_ctx *c, const SvcBlobHdr &h)
{
	HIPCHK(hipMemcpyAsync(c->d_epoch, &h.epoch, 4, hipMemcpyHostToDevice, c->stream)); // the captured close graphs read the window number here
	HIPCHK(hipStreamSynchronize(c->stream));
	c->epoch = h.epoch;
	c->lvl_t_last = h.lvl_t_last;
	c->hl_t_last = h.hl_t_last;
	c->hl_roll_epoch = h.epoch - 1u;                          // the window rolled last
	if (h.lvl_t_last >= 0) c->lvl_last_epoch = h.epoch - 1u;  // the window whose records the level-0 array holds (behind their tags)
	c->clock_adopted = true;
	return GYS_OK;
}

int blob_unpack_begin(gys_ctx *c, const SvcBlobHdr &h, bool adopt)
{
	if (adopt) {
		const int rc = blob_adopt_clock(c, h);
		if (rc) return rc;
	}
	// the carried window accumulators (connection path, response event counts) are folded at the next close like ingested ones
	c->conn_dirty = true;
	c->resp_dirty = true;
	return GYS_OK;
}

} // namespace

uint64_t gys_service_blob_bytes(gys_ctx *c, uint32_t n)
{
	if (!c) return 0;
	SvcRecLayout L;
	if (svc_rec_layout(c, L)) return 0;
	return 64ull + blob_ids_bytes(n) + (uint64_t)n * L.p.stride;
}

int gys_list_service_ids(gys_ctx *c, uint32_t first_slot, uint32_t nslots, uint64_t *glob_ids, uint32_t *nout)
try {
	GYS_ENTER_NOFLUSH(c);
	if (!c || !nout || (!glob_ids && nslots)) return GYS_ERR_INVAL;
	*nout = 0;
	const uint32_t end = (uint32_t)std::min<uint64_t>((uint64_t)first_slot + nslots, c->nsvc);
	for (uint32_t s = first_slot; s < end; ++s)
		if (c->svc_host_h[s] != GYS_NOSLOT) glob_ids[(*nout)++] = c->svc_gid_h[s];
	return GYS_OK;
} GYS_CATCH_ALL

int gys_list_host_service_ids(gys_ctx *c, const uint8_t machine_id[16], uint64_t *glob_ids, uint32_t cap, uint32_t *nfound)
try {
	GYS_ENTER_NOFLUSH(c);
	if (!c || !machine_id || !nfound || (!glob_ids && cap)) return GYS_ERR_INVAL;
	*nfound = 0;
	uint32_t host;
	const int rc = lookup_host(c, machine_id, &host);
	if (rc) return rc;
	std::vector<uint32_t> slots(c->host_lst[host].all_slots);
	std::sort(slots.begin(), slots.end());
	for (uint32_t s : slots) {
		if (*nfound < cap) glob_ids[*nfound] = c->svc_gid_h[s];
		++*nfound;
	}
	return GYS_OK;
} GYS_CATCH_ALL

static int pack_services(gys_ctx *c, const uint64_t *glob_ids, uint32_t n, uint8_t *blob, uint64_t blob_bytes, bool dev)
{
	if (!c || (!glob_ids && n) || !blob) return GYS_ERR_INVAL;
	int rc = svc_rec_not_prepared(c);
	if (rc) return rc;
	SvcRecLayout L;
	rc = svc_rec_layout(c, L);
	if (rc) return rc;
	const uint64_t need = 64ull + blob_ids_bytes(n) + (uint64_t)n * L.p.stride;
	if (blob_bytes < need) {
		set_err("blob buffer of %llu bytes, %u services need %llu", (unsigned long long)blob_bytes, n, (unsigned long long)need);
		return GYS_ERR_INVAL;
	}
	if (dev && ((uintptr_t)blob & 15u)) {
		set_err("the blob buffer must be 16-byte aligned");
		return GYS_ERR_INVAL;
	}
	std::vector<uint32_t> slots;
	rc = blob_slots(c, glob_ids, n, false, slots, nullptr);
	if (rc) return rc;
	const uint32_t piece = dev ? n : svc_rec_piece(L, n);
	rc = svc_rec_prepare(c, svc_rec_words_bytes(piece) + (dev ? 0ull : (uint64_t)piece * L.p.stride));
	if (rc) return rc;
	std::vector<uint8_t> head(64 + blob_ids_bytes(n), 0);
	SvcBlobHdr h;
	blob_header(c, L, n, h);
	memcpy(head.data(), &h, 64);
	if (n) memcpy(head.data() + 64, glob_ids, (size_t)n * 8);
	if (dev) {
		HIPCHK(hipMemcpyAsync(blob, head.data(), head.size(), hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipStreamSynchronize(c->stream)); // (head is a local; svc_rec_run synchronises only when there are records)
		return svc_rec_run(c, L, false, slots.data(), nullptr, n, blob + head.size());
	}
	memcpy(blob, head.data(), head.size());
	uint8_t *d_recs = c->dev_staging + svc_rec_words_bytes(piece);
	for (uint32_t first = 0; first < n; first += piece) {
		const uint32_t cnt = std::min(piece, n - first);
		rc = svc_rec_run(c, L, false, slots.data() + first, nullptr, cnt, d_recs);
		if (rc) return rc;
		HIPCHK(hipMemcpy(blob + head.size() + (uint64_t)first * L.p.stride, d_recs, (uint64_t)cnt * L.p.stride, hipMemcpyDeviceToHost));
	}
	return GYS_OK;
}

int gys_pack_services_dev(gys_ctx *c, const uint64_t *glob_ids, uint32_t n, void *d_blob, uint64_t blob_bytes)
try {
	GYS_ENTER(c);
	return pack_services(c, glob_ids, n, (uint8_t *)d_blob, blob_bytes, true);
} GYS_CATCH_ALL

int gys_pack_services(gys_ctx *c, const uint64_t *glob_ids, uint32_t n, void *blob, uint64_t blob_bytes)
try {
	GYS_ENTER(c);
	return pack_services(c, glob_ids, n, (uint8_t *)blob, blob_bytes, false);
} GYS_CATCH_ALL

static int unpack_services(gys_ctx *c, const uint8_t *blob, uint64_t blob_bytes, uint32_t *napplied, uint32_t *nskipped, bool dev)
{
	if (!c || !blob) return GYS_ERR_INVAL;
	if (napplied) *napplied = 0;
	if (nskipped) *nskipped = 0;
	if (blob_bytes < 64) {
		set_err("service blob of %llu bytes", (unsigned long long)blob_bytes);
		return GYS_ERR_INVAL;
	}
	if (dev && ((uintptr_t)blob & 15u)) {
		set_err("the blob buffer must be 16-byte aligned");
		return GYS_ERR_INVAL;
	}
	int rc = svc_rec_not_prepared(c);
	if (rc) return rc;
	SvcBlobHdr h;
	if (dev) HIPCHK(hipMemcpy(&h, blob, 64, hipMemcpyDeviceToHost));
	else memcpy(&h, blob, 64);
	rc = svc_bithist_ensure(c); // (no state: zeroes are what a context without the array stands for)
	if (rc) return rc;
	SvcRecLayout L;
	rc = svc_rec_layout(c, L); // once: the list names the arrays as they are now and nothing below moves them
	if (rc) return rc;
	bool adopt = false;
	rc = blob_validate(c, L, h, blob_bytes, &adopt);
	if (rc) return rc;
	const uint32_t n = h.n;
	std::vector<uint64_t> ids(n);
	if (n) {
		if (dev) HIPCHK(hipMemcpy(ids.data(), blob + 64, (size_t)n * 8, hipMemcpyDeviceToHost));
		else memcpy(ids.data(), blob + 64, (size_t)n * 8);
	}
	std::vector<uint32_t> slots, hosts(n, 0u);
	uint32_t known = 0;
	rc = blob_slots(c, ids.data(), n, true, slots, &known);
	if (rc) return rc;
	for (uint32_t i = 0; i < n; ++i)
		if (slots[i] != GYS_NOSLOT) hosts[i] = c->svc_host_h[slots[i]];
	const uint32_t piece = dev ? n : svc_rec_piece(L, n);
	rc = svc_rec_prepare(c, svc_rec_words_bytes(piece) + (dev ? 0ull : (uint64_t)piece * L.p.stride));
	if (rc) return rc;
	// ---- nothing has been modified so far
	rc = blob_unpack_begin(c, h, adopt);
	if (rc) return rc;
	const uint64_t recs_at = 64ull + blob_ids_bytes(n);
	if (dev) {
		rc = svc_rec_run(c, L, true, slots.data(), hosts.data(), n, const_cast<uint8_t *>(blob) + recs_at);
		if (rc) return rc;
	} else {
		uint8_t *d_recs = c->dev_staging + svc_rec_words_bytes(piece);
		for (uint32_t first = 0; first < n; first += piece) {
			const uint32_t cnt = std::min(piece, n - first);
			HIPCHK(hipMemcpyAsync(d_recs, blob + recs_at + (uint64_t)first * L.p.stride, (uint64_t)cnt * L.p.stride, hipMemcpyHostToDevice, c->stream));
			rc = svc_rec_run(c, L, true, slots.data() + first, hosts.data() + first, cnt, d_recs);
			if (rc) return rc;
		}
	}
	if (napplied) *napplied = known;
	if (nskipped) *nskipped = n - known;
	return GYS_OK;
}

int gys_unpack_services_dev(gys_ctx *c, const void *d_blob, uint64_t blob_bytes, uint32_t *napplied, uint32_t *nskipped)
try {
	GYS_ENTER(c);
	return unpack_services(c, (const uint8_t *)d_blob, blob_bytes, napplied, nskipped, true);
} GYS_CATCH_ALL

int gys_unpack_services(gys_ctx *c, const void *blob, uint64_t blob_bytes, uint32_t *napplied, uint32_t *nskipped)
try {
	GYS_ENTER(c);
	return unpack_services(c, (const uint8_t *)blob, blob_bytes, napplied, nskipped, false);
} GYS_CATCH_ALL

int gys_list_stale_listeners(gys_ctx *c, uint32_t flags, uint32_t max_age_windows, uint64_t *glob_ids, uint32_t cap, uint32_t *nfound)
try {
	GYS_ENTER(c);
	if (!c || !nfound || (!glob_ids && cap) || (flags & ~(GYS_STALE_DELETED | GYS_STALE_AGED))) return GYS_ERR_INVAL;
	*nfound = 0;
	if (!c->nsvc || !flags) return GYS_OK;
	SvcStaleP p{};
	p.svc_state = c->svc_state;
	p.nsvc = c->nsvc;
	p.ntiles = (c->nsvc + GYS_STALE_TILE - 1u) / GYS_STALE_TILE;
	p.epoch = c->epoch;
	p.flags = flags;
	p.max_age = max_age_windows;
	cap = std::min(cap, c->nsvc); // (there are no more hits than services: a caller's "everything" does not size the id buffer)
	p.cap = cap;
	int rc = GYS_OK;
	if (c->stale_tiles.cap < p.ntiles + 1u || c->stale_bits.cap < p.ntiles * 16ull) { // (16 words and a count per tile, + the total)
		const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(2ull * p.ntiles, 64), ((uint64_t)c->cfg.max_services + GYS_STALE_TILE - 1u) / GYS_STALE_TILE);
		rc = c->stale_bits.grow(want * 16, c->stream);
		if (!rc) rc = c->stale_tiles.grow(want + 1, c->stream);
	}
	if (!rc && c->stale_ids.cap < cap) rc = c->stale_ids.grow(cap, c->stream);
	if (rc) return rc;
	p.bits = c->stale_bits;
	p.tile_cnt = c->stale_tiles;
	p.ids = c->stale_ids;
	{
		ProfScope ps(c, "svc_stale");
		hipLaunchKernelGGL(k_svc_stale_mark, dim3(std::min<uint32_t>(p.ntiles, (uint32_t)c->ncu * 8u)), dim3(GYS_STALE_NT), 0, c->stream, p);
		hipLaunchKernelGGL(k_svc_stale_scan, dim3(1), dim3(GYS_STALE_NT), 0, c->stream, p);
		if (cap) hipLaunchKernelGGL(k_svc_stale_emit, dim3(grid_for((uint64_t)p.ntiles * 16, GYS_STALE_NT, (uint32_t)c->ncu * 8)), dim3(GYS_STALE_NT), 0, c->stream, p);
	}
	HIPCHK(hipGetLastError());
	uint32_t total = 0;
	HIPCHK(hipMemcpyAsync(&total, c->stale_tiles + p.ntiles, 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	const uint32_t nw = std::min(total, cap);
	if (nw) HIPCHK(hipMemcpy(glob_ids, c->stale_ids, (size_t)nw * 8, hipMemcpyDeviceToHost));
	*nfound = total;
	return GYS_OK;
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ ingest
int gys_ingest_resp_events_dev(gys_ctx *c, const gys_resp_seg *segs, uint32_t nsegs, const void *d_ev24, uint64_t nevents)
try {
	GYS_ENTER(c);
	if (!c || (!d_ev24 && nevents)) return GYS_ERR_INVAL;
	return run_resp_batch(c, segs, nsegs, d_ev24, nevents);
} GYS_CATCH_ALL

int gys_ingest_resp_events(gys_ctx *c, const uint8_t machine_id[16], const void *ev24, uint32_t nevents)
try {
	GYS_ENTER_NOFLUSH(c);
	if (!c || !machine_id || (!ev24 && nevents)) return GYS_ERR_INVAL;
	uint32_t host;
	int rc = lookup_host(c, machine_id, &host);
	if (rc) return rc;
	if (!nevents) return GYS_OK;
	if ((uint64_t)nevents <= std::min<uint64_t>(GYS_RQ_EVENTS, c->cfg.max_batch_events))
		return subq_ingest(c->ingest, c->sq[SubQ::RESP], host, c->hosts.size(), ev24, 0, nevents, nullptr); // combined with the other callers' pending calls
	return ingest_staged_resp(c, host, ev24, nevents, 24, false, "gys_ingest_resp_events"); // larger than a combined batch
} GYS_CATCH_ALL

int gys_ingest_resp_events_v6_dev(gys_ctx *c, const gys_resp_seg *segs, uint32_t nsegs, const void *d_ev48, uint64_t nevents)
try {
	GYS_ENTER(c);
	if (!c || (!d_ev48 && nevents) || ((uintptr_t)d_ev48 & 7u)) return GYS_ERR_INVAL;
	return run_resp_batch(c, segs, nsegs, d_ev48, nevents, true);
} GYS_CATCH_ALL

int gys_ingest_resp_events_v6(gys_ctx *c, const uint8_t machine_id[16], const void *ev48, uint32_t nevents)
try {
	GYS_ENTER_NOFLUSH(c);
	if (!c || !machine_id || (!ev48 && nevents)) return GYS_ERR_INVAL;
	uint32_t host;
	int rc = lookup_host(c, machine_id, &host);
	if (rc) return rc;
	if (!nevents) return GYS_OK;
	// its own submission, behind whatever the IPv4 queue holds
	return ingest_staged_resp(c, host, ev48, nevents, 48, true, "gys_ingest_resp_events_v6");
} GYS_CATCH_ALL

int gys_ingest_tcp_conn_dev(gys_ctx *c, const void *d_batch, const uint32_t *d_offsets, uint32_t nconns)
try {
	GYS_ENTER(c);
	if (!c || ((!d_batch || !d_offsets) && nconns)) return GYS_ERR_INVAL;
	return run_conn(c, (const uint8_t *)d_batch, d_offsets, nconns);
} GYS_CATCH_ALL

int gys_ingest_tcp_conn(gys_ctx *c, const uint8_t machine_id[16], const void *batch, uint32_t nconns, const void *pend)
try {
	GYS_ENTER_NOFLUSH(c);
	if (!c || !machine_id || (!batch && nconns) || ((uintptr_t)batch & 7u)) return GYS_ERR_INVAL;
	uint32_t host;
	int rc = lookup_host(c, machine_id, &host);
	if (rc) return rc;
	if (!nconns) return GYS_OK;
	std::vector<uint32_t> offs;
	// TCP_CONN_NOTIFY::get_elem_size common/gy_comm_proto.h:1721-1724
	rc = walk_batch((const uint8_t *)batch, nconns, (const uint8_t *)pend, 280, [](const uint8_t *p) {
		uint16_t cl;
		memcpy(&cl, p + 272, 2);
		return (uint32_t)(280u + cl + p[279]);
	}, offs);
	if (rc) return rc;
	if (offs.empty()) return GYS_OK;
	return ingest_records(c, c->sq[SubQ::CONN], host, batch, pend, offs);
} GYS_CATCH_ALL

int gys_ingest_listener_state_dev(gys_ctx *c, const void *d_batch, const uint32_t *d_offsets, const uint32_t *d_host_slot, uint32_t nrecs)
try {
	GYS_ENTER(c);
	if (!c || ((!d_batch || !d_offsets || !d_host_slot) && nrecs)) return GYS_ERR_INVAL;
	return run_lstate(c, (const uint8_t *)d_batch, d_offsets, d_host_slot, 0, nrecs);
} GYS_CATCH_ALL

int gys_ingest_active_conns_dev(gys_ctx *c, const void *d_batch, uint32_t nitems)
try {
	GYS_ENTER(c);
	if (!c || (!d_batch && nitems)) return GYS_ERR_INVAL;
	return run_actconn(c, (const uint8_t *)d_batch, nitems);
} GYS_CATCH_ALL

int gys_ingest_active_conns(gys_ctx *c, const uint8_t machine_id[16], const void *batch, uint32_t nitems, const void *pend)
try {
	GYS_ENTER_NOFLUSH(c);
	if (!c || !machine_id || (!batch && nitems) || ((uintptr_t)batch & 7u)) return GYS_ERR_INVAL;
	uint32_t host;
	int rc = lookup_host(c, machine_id, &host);
	if (rc) return rc;
	// fixed 104-byte stride; nitems is an upper bound as in the reference's loop over pconn (gy_mconnhdlr.cc:7842)
	const uint64_t avail = pend ? (uint64_t)((const uint8_t *)pend - (const uint8_t *)batch) / 104u : nitems;
	const uint32_t n = (uint32_t)std::min<uint64_t>(nitems, avail);
	if (!n) return GYS_OK;
	const uint64_t bytes = (uint64_t)n * 104u;
	return stage_call(
		c->ingest, c->ring, bytes, [&](uint8_t *pinned) { memcpy(pinned, batch, bytes); }, false, "gys_ingest_active_conns",
		[&](const uint8_t *dev) { return run_actconn(c, dev, n); });
} GYS_CATCH_ALL

int gys_ingest_listener_state(gys_ctx *c, const uint8_t machine_id[16], const void *batch, uint32_t nrecs, const void *pend)
try {
	GYS_ENTER_NOFLUSH(c);
	if (!c || !machine_id || (!batch && nrecs) || ((uintptr_t)batch & 7u)) return GYS_ERR_INVAL;
	uint32_t host;
	int rc = lookup_host(c, machine_id, &host);
	if (rc) return rc;
	if (!nrecs) return GYS_OK;
	std::vector<uint32_t> offs;
	// LISTENER_STATE_NOTIFY::get_elem_size common/gy_comm_proto.h:2229-2232
	rc = walk_batch((const uint8_t *)batch, nrecs, (const uint8_t *)pend, 88, [](const uint8_t *p) { return (uint32_t)(88u + p[85] + p[86]); }, offs);
	if (rc) return rc;
	if (offs.empty()) return GYS_OK;
	return ingest_records(c, c->sq[SubQ::LSTATE], host, batch, pend, offs);
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ wire front-end
// COMM_HEADER / EVENT_NOTIFY framing as an unmodified partha sends it to madhava (common/gy_comm_proto.h:336-420, :486-500).  The
// 16-byte message headers are validated on the host exactly like COMM_HEADER::validate (common/gy_comm_proto.cc:10-57); the records
// are walked, checked and indexed on the GPU (k_wire_*), then handed to the same ingest kernels as the batch entry points.
namespace {
constexpr uint32_t PM_HDR_MAGIC = 0x05666605u;      // COMM_HEADER::PM_HDR_MAGIC, partha to madhava
constexpr uint32_t COMM_EVENT_NOTIFY_T = 14;        // COMM_TYPE_E::COMM_EVENT_NOTIFY
constexpr uint32_t COMM_MIN_TYPE_T = 1, COMM_MAX_TYPE_T = 18;
constexpr uint32_t MAX_COMM_DATA_SZ_T = 16u << 20;  // gy_comm_proto.h:31
constexpr uint32_t NOTIFY_LISTENER_STATE_T = 0x309, NOTIFY_TCP_CONN_T = 0x30C; // NOTIFY_TYPE_E (0x301 + 8, + 11)
constexpr uint32_t MAX_NUM_CONNS_T = 2048, MAX_NUM_LISTENERS_T = 512;          // gy_comm_proto.h:1711, :2222

int wire_reserve(gys_ctx *c, uint64_t nslots, uint32_t nmsgs)
{
	if (nslots + 1 > c->wire_slots_cap) {
		const uint64_t cap = align_up(std::max<uint64_t>(nslots + 1, 1u << 16), 4096);
		c->wire_slots_cap = 0; // (a grow that fails leaves its array empty: no slot counts as reserved until all seven stand)
		int rc = GYS_OK;
		for (DevBuf<uint32_t> *b : {&c->wire_jump[0], &c->wire_jump[1], &c->wire_cnt, &c->wire_rank})
			if (!rc) rc = b->grow(cap, c->stream);
		if (!rc) rc = c->wire_bsums.grow(cap / GYS_SCAN_TILE + 2, c->stream);
		if (!rc) rc = c->wire_mark.grow(cap, c->stream);
		if (!rc) rc = c->wire_flags.grow(cap, c->stream);
		if (rc) return rc;
		c->wire_slots_cap = cap;
	}
	int rc = c->wire_status.p ? GYS_OK : c->wire_status.alloc(4, false);
	if (!rc && nmsgs > c->wire_msgs.cap) rc = c->wire_msgs.grow(std::max<uint32_t>(nmsgs, 1024), c->stream);
	return rc;
}

// d_buf: device copy of the stream (8-byte aligned); msgs: accepted messages of ONE record kind, sorted by position; fills
// c->dev_offsets[0 .. total records) with the records' byte offsets inside d_buf
int wire_decode(gys_ctx *c, const uint8_t *d_buf, uint64_t nbytes, std::vector<WireMsg> &msgs, uint32_t nrec_total)
{
	const uint32_t nslots = (uint32_t)(nbytes / 8) + 1; // + one terminal slot past the end
	const uint32_t nmsgs = (uint32_t)msgs.size();
	int rc = wire_reserve(c, nslots, nmsgs);
	if (rc) return rc;
	rc = ensure_staging(c, 0, nrec_total);
	if (rc) return rc;
	uint32_t maxev = 1;
	for (const WireMsg &m : msgs) maxev = std::max(maxev, m.nevents);
	HIPCHK(hipMemcpyAsync(c->wire_msgs, msgs.data(), (size_t)nmsgs * sizeof(WireMsg), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemsetAsync(c->wire_mark, 0, nslots, c->stream));
	HIPCHK(hipMemsetAsync(c->wire_status, 0, 16, c->stream));
	const dim3 gs((nslots + 255) / 256), gm((nmsgs + 255) / 256), b(256);
	ProfScope ps(c, "wire_decode");
	hipLaunchKernelGGL(k_wire_next, gs, b, 0, c->stream, (const uint64_t *)d_buf, c->wire_msgs, nmsgs, nslots, c->wire_jump[0], c->wire_flags);
	hipLaunchKernelGGL(k_wire_seed, gm, b, 0, c->stream, c->wire_msgs, nmsgs, c->wire_mark);
	int cur = 0;
	for (uint32_t span = 1; span < maxev; span <<= 1) { // after the round for span, the first 2 * span records of every chain are marked
		hipLaunchKernelGGL(k_wire_round, gs, b, 0, c->stream, nslots, c->wire_jump[cur], c->wire_jump[cur ^ 1], c->wire_mark);
		cur ^= 1;
	}
	hipLaunchKernelGGL(k_wire_count, gs, b, 0, c->stream, nslots, c->wire_mark, c->wire_flags, c->wire_cnt);
	const uint32_t nblk = (nslots + GYS_SCAN_TILE - 1) / GYS_SCAN_TILE;
	hipLaunchKernelGGL(k_scan_block_sums, dim3(nblk), b, 0, c->stream, c->wire_cnt, nslots, c->wire_bsums);
	hipLaunchKernelGGL(k_scan_top, dim3(1), b, 0, c->stream, c->wire_bsums, nblk);
	hipLaunchKernelGGL(k_scan_final, dim3(nblk), b, 0, c->stream, c->wire_cnt, nslots, c->wire_bsums, c->wire_rank);
	hipLaunchKernelGGL(k_wire_emit, gs, b, 0, c->stream, c->wire_msgs, nmsgs, nslots, c->wire_cnt, c->wire_rank, c->wire_flags, c->dev_offsets, c->wire_status);
	hipLaunchKernelGGL(k_wire_check, gm, b, 0, c->stream, c->wire_msgs, nmsgs, nslots, c->wire_cnt, c->wire_rank, c->wire_status);
	HIPCHK(hipGetLastError());
	uint32_t status = 0;
	HIPCHK(hipMemcpyAsync(&status, c->wire_status, 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (status) {
		set_err("malformed message: %s%s", (status & 1u) ? "record size / padding invalid or element overruns the message; " : "",
			(status & 2u) ? "fewer records than nevents_" : "");
		return GYS_ERR_INVAL;
	}
	return GYS_OK;
}
} // namespace

int gys_ingest_comm_stream(gys_ctx *c, const uint8_t machine_id[16], const void *buf, uint64_t nbytes, gys_comm_stats *out)
try {
	GYS_ENTER(c);
	if (!c || !machine_id || (!buf && nbytes) || ((uintptr_t)buf & 7u)) return GYS_ERR_INVAL; // COMM_HEADER::validate: 8-byte aligned data
	uint32_t host;
	int rc = lookup_host(c, machine_id, &host);
	if (rc) return rc;
	gys_comm_stats st{};
	if (nbytes >= (1ull << 32)) {
		set_err("stream too large (u32 offsets)");
		return GYS_ERR_INVAL;
	}
	std::vector<WireMsg> conn_msgs, lst_msgs;
	uint32_t nconn = 0, nlst = 0;
	const uint8_t *p = (const uint8_t *)buf, *pend = p + nbytes;
	while ((size_t)(pend - p) >= 16) {
		uint32_t magic, total_sz, data_type, padding_sz;
		memcpy(&magic, p, 4);
		memcpy(&total_sz, p + 4, 4);
		memcpy(&data_type, p + 8, 4);
		memcpy(&padding_sz, p + 12, 4);
		// COMM_HEADER::validate common/gy_comm_proto.cc:12-22
		if (!(magic == PM_HDR_MAGIC && total_sz < MAX_COMM_DATA_SZ_T && total_sz >= 16 && padding_sz < 8 && data_type > COMM_MIN_TYPE_T &&
		      data_type < COMM_MAX_TYPE_T) || (total_sz & 7u)) {
			st.nmsgs_invalid++;
			if (out) *out = st;
			set_err("invalid COMM_HEADER at byte %zu", (size_t)(p - (const uint8_t *)buf));
			return GYS_ERR_INVAL; // the reference terminates the connection
		}
		// a well-formed header whose body has not arrived yet (a recv() chunk ends inside the message): end of input, the whole
		// messages before it are ingested and bytes_consumed tells the caller where to resume (gysketch.h)
		if (total_sz > (uint64_t)(pend - p)) break;
		st.nmsgs++;
		const uint32_t act = total_sz - padding_sz;
		bool taken = false;
		if (data_type == COMM_EVENT_NOTIFY_T) {
			if (act < 16 + 8) {
				st.nmsgs_invalid++;
				if (out) *out = st;
				set_err("EVENT_NOTIFY message shorter than its headers");
				return GYS_ERR_INVAL;
			}
			uint32_t subtype, nevents;
			memcpy(&subtype, p + 16, 4);
			memcpy(&nevents, p + 20, 4);
			if (subtype == NOTIFY_TCP_CONN_T || subtype == NOTIFY_LISTENER_STATE_T) {
				const bool is_conn = subtype == NOTIFY_TCP_CONN_T;
				if (nevents > (is_conn ? MAX_NUM_CONNS_T : MAX_NUM_LISTENERS_T)) { // :853, :968
					st.nmsgs_invalid++;
					if (out) *out = st;
					set_err("nevents_ %u over the per-message limit", nevents);
					return GYS_ERR_INVAL;
				}
				// every record is at least its fixed part, so a message that announces more records than its payload can hold fails the
				// validators' walk (:859-880, :974-995) whatever its bytes say.  Rejected HERE, before any kernel: the offset list is sized by
				// the sum of the announced counts, and a long stream of header-only messages announcing 2 048 records each could wrap that sum
				if ((uint64_t)nevents * (is_conn ? 280u : 88u) > (uint64_t)act - 24u) {
					st.nmsgs_invalid++;
					if (out) *out = st;
					set_err("nevents_ %u records cannot lie in %u payload bytes", nevents, act - 24u);
					return GYS_ERR_INVAL;
				}
				WireMsg m{};
				m.pay_slot = (uint32_t)((p - (const uint8_t *)buf) + 24) / 8u;
				m.end_slot = (uint32_t)((p - (const uint8_t *)buf) + act) / 8u; // act_len is a multiple of 8 for well-formed messages
				m.nevents = nevents;
				m.kind = is_conn ? 0u : 1u;
				if (is_conn) {
					m.out_base = nconn;
					nconn += nevents;
					conn_msgs.push_back(m);
					st.nmsgs_tcp_conn++;
				} else {
					m.out_base = nlst;
					nlst += nevents;
					lst_msgs.push_back(m);
					st.nmsgs_listener_state++;
				}
				taken = true;
			}
		}
		if (!taken) st.nmsgs_skipped++; // registration, queries and the other notify subtypes belong to the control plane
		p += total_sz;
	}
	st.bytes_consumed = (uint64_t)(p - (const uint8_t *)buf);
	st.nrecords = (uint64_t)nconn + nlst;
	if (nconn || nlst) {
		rc = ensure_staging(c, nbytes + 8, 0);
		if (rc) return rc;
		HIPCHK(hipMemcpyAsync(c->dev_staging, buf, nbytes, hipMemcpyHostToDevice, c->stream));
		if (nconn) {
			rc = wire_decode(c, c->dev_staging, nbytes, conn_msgs, nconn);
			if (!rc) rc = run_conn(c, c->dev_staging, c->dev_offsets, nconn);
			if (rc) return rc;
		}
		if (nlst) {
			rc = wire_decode(c, c->dev_staging, nbytes, lst_msgs, nlst);
			if (!rc) rc = run_lstate(c, c->dev_staging, c->dev_offsets, nullptr, host, nlst);
			if (rc) return rc;
		}
		HIPCHK(hipStreamSynchronize(c->stream)); // the caller's buffer is only valid during the call
	}
	if (out) *out = st;
	return GYS_OK;
} GYS_CATCH_ALL

int gys_ingest_host_state(gys_ctx *c, const uint8_t machine_id[16], const gys_host_state *st)
try {
	GYS_ENTER(c);
	if (!c || !machine_id || !st) return GYS_ERR_INVAL;
	uint32_t host;
	int rc = lookup_host(c, machine_id, &host);
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(c->host_state + host, st, sizeof(*st), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(c->host_state_epoch + host, &c->epoch, 4, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ window boundary
int gys_reduce_sections(gys_ctx *c, gys_reduce_section out[4], uint32_t *nsections)
try {
	GYS_ENTER(c);
	if (!c || !out || !nsections) return GYS_ERR_INVAL;
	out[0] = {c->arena + c->al.off_hll8, (uint64_t)1 << GYS_HLL_P, 0, 0};
	out[1] = {c->arena + c->al.off_u32, c->al.n_u32, 1, 1};
	out[2] = {c->arena + c->al.off_i64sum, c->al.n_i64sum, 2, 1};
	out[3] = {c->arena + c->al.off_i64max, c->al.n_i64max, 2, 0};
	*nsections = 4;
	return GYS_OK;
} GYS_CATCH_ALL

// the kernels of the window boundary before the exchange (no level roll): folds of the per-service window accumulators into the
// Count-Min rows, cluster STATE_ONE sums + HLL pack, eager-mode record sweep.  dev_epoch: read the window number from device memory
// (captured graph) instead of the launch parameter.
static int enqueue_prepare(gys_ctx *c, bool dev_epoch)
{
	PrepP p{};
	p.host_summ = c->host_summ_win;
	p.host_state = c->host_state;
	p.host_state_epoch = c->host_state_epoch;
	p.host_cluster = c->host_cluster;
	p.nhosts = (uint32_t)c->hosts.size();
	p.epoch = c->epoch;
	p.d_epoch = dev_epoch ? c->d_epoch : nullptr;
	p.cluster_state = (uint32_t *)(c->arena + c->al.off_u32) + c->al.u32_cluster;
	p.hll32 = c->hll32;
	p.hll8 = c->arena + c->al.off_hll8;
	const uint32_t nthreads = std::max<uint32_t>(p.nhosts, (1u << GYS_HLL_P) / 4u);
	int rcf = conn_fold(c);
	if (!rcf) rcf = resp_cms_fold(c);
	if (rcf) return rcf;
	hipLaunchKernelGGL(k_window_prepare, dim3((nthreads + 255) / 256), dim3(256), 0, c->stream, p);
	if (c->nsvc && !c->cfg.enable_tdigest) {
		// eager mode (records updated per event): all-time += window (GY_HISTOGRAM::add_histogram), window cleared, and the all-service
		// histogram of the window reduced into the arena in the same pass over the records.  With the t-digest on, the records are
		// folded lazily from the value buffers ("per-key value buffers" in gys_kernels.hpp) and there is nothing to sweep here.
		long long *gh = (long long *)(c->arena + c->al.off_i64sum) + c->al.i64_ghist;
		hipLaunchKernelGGL(k_hist_fold, dim3(grid_for((uint64_t)c->nsvc * 16, 256, (uint32_t)c->ncu * 8)), dim3(256), 0, c->stream, c->hist_all,
				   c->hist_win, (uint64_t)c->nsvc, 1, gh, (long long *)(c->arena + c->al.off_i64max));
	}
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

int gys_window_prepare(gys_ctx *c, uint64_t tusec)
try {
	GYS_ENTER(c);
	if (!c) return GYS_ERR_INVAL;
	if (c->prepared) {
		set_err("window already prepared");
		return GYS_ERR_STATE;
	}
	c->hl_close_t = (int64_t)(tusec / 1000000ull); // (the per-service registers are rolled where they are cleared: gys_window_finish)
	if (c->cfg.enable_levels) {
		const int rcl = level_roll(c, tusec); // before the eager fold below: it needs the cumulative records WITHOUT the closing window
		if (rcl) return rcl;
	}
	{
		ProfScope ps(c, "window_prepare");
		const int rc = enqueue_prepare(c, false);
		if (rc) return rc;
	}
	c->prepared = true;
	return GYS_OK;
} GYS_CATCH_ALL

// the fixed sequence that ends a window: keep the (reduced) registers for queries, start the next window from zero
static hipError_t enqueue_finish(gys_ctx *c, hipStream_t st)
{
	hipError_t e;
	// ACTIVE_CONN_STATS tables: the window's tables enter a ring of the last three windows, the queries read the per-cell maximum (k_act_latch)
	hipLaunchKernelGGL(k_act_latch, dim3(64), dim3(256), 0, st, (const uint32_t *)(c->arena + c->al.off_u32) + c->al.u32_misc, c->d_epoch, c->act_live,
			   (const uint32_t *)(c->arena + c->al.off_u32) + c->al.u32_pair,
			   (const unsigned long long *)(c->arena + c->al.off_i64sum) + c->al.i64_pair, c->ring_act32, c->ring_act64, c->last_act32, c->last_act64);
	if (c->nsvc) {
		// CONN_BITMAP cleared every window (secs_to_reset_ = 5); lazily (per key, on its next touch) when the per-key pass runs
		if (!c->cfg.enable_tdigest && (e = hipMemsetAsync(c->bitmap, 0, (uint64_t)c->nsvc * GYS_BM_WORDS * 4, st)) != hipSuccess) return e;
		// (with svc_hll_levels the roll that runs in front of this sequence has cleared them: hll_level_roll)
		if (c->svc_hll && !c->hl_lvl && (e = hipMemsetAsync(c->svc_hll, 0, (uint64_t)c->nsvc << c->cfg.svc_hll_p, st)) != hipSuccess) return e;
	}
	const uint64_t hb = (uint64_t)c->hosts.size() * 16 * 4;
	if (((uintptr_t)c->arena & 15u) == 0) { // (a caller's reduce_arena is torch / hipMalloc memory: always; the plain sequence below otherwise)
		WinFinishP p{};
		p.arena = (uint4 *)c->arena;
		p.last = (uint4 *)c->last.p;
		p.n16 = c->al.total / 16;
		p.i64max_at = c->al.off_i64max;
		p.hll32 = (uint4 *)c->hll32.p;
		p.hll16 = ((uint64_t)4 << GYS_HLL_P) / 16;
		p.hs_win = (uint4 *)c->host_summ_win.p;
		p.hs_last = (uint4 *)c->host_summ_last.p;
		p.hs16 = hb / 16;
		p.d_epoch = c->d_epoch; // the device copy of the window number follows the host's
		hipLaunchKernelGGL(k_window_finish, dim3(grid_for(std::max<uint64_t>(p.n16, p.hs16), 256, (uint32_t)c->ncu * 4)), dim3(256), 0, st, p);
		return hipGetLastError();
	}
	if ((e = hipMemcpyAsync(c->last, c->arena, c->al.total, hipMemcpyDeviceToDevice, st)) != hipSuccess) return e;
	if ((e = hipMemsetAsync(c->arena, 0, c->al.total, st)) != hipSuccess) return e;
	if ((e = hipMemcpyAsync(c->arena + c->al.off_i64max, &c->i64min, 8, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
	if ((e = hipMemsetAsync(c->hll32, 0, (uint64_t)4 << GYS_HLL_P, st)) != hipSuccess) return e;
	if (hb) {
		if ((e = hipMemcpyAsync(c->host_summ_last, c->host_summ_win, hb, hipMemcpyDeviceToDevice, st)) != hipSuccess) return e;
		if ((e = hipMemsetAsync(c->host_summ_win, 0, hb, st)) != hipSuccess) return e;
	}
	hipLaunchKernelGGL(k_epoch_inc, dim3(1), dim3(1), 0, st, c->d_epoch);
	return hipGetLastError();
}

int gys_window_finish(gys_ctx *c)
try {
	GYS_ENTER(c);
	if (!c) return GYS_ERR_INVAL;
	if (!c->prepared) {
		set_err("gys_window_finish without gys_window_prepare");
		return GYS_ERR_STATE;
	}
	if (c->hl_lvl) {
		// once per window, whatever was retried before: the roll happens here, where the open registers used to be cleared, with the close
		// time of the prepare step.  In front of the captured sequence, not inside it (the bucket indices change from window to window).
		const int rcl = hll_level_roll(c);
		if (rcl) return rcl;
	}
	ProfScope ps(c, "window_finish");
	// keep the (reduced) registers of this window for queries, start the next window from zero.  The sequence is the same every
	// window for a given registry shape: it is captured into a hipGraph the first time and replayed afterwards (one launch instead
	// of seven); any capture problem falls back to plain stream operations.
	const uint64_t shape = ((uint64_t)c->hosts.size() << 32) | (uint64_t)c->nsvc;
	auto enqueue = [&](hipStream_t st) -> hipError_t { return enqueue_finish(c, st); };
	if (c->win_graph_state >= 0 && (c->win_graph_state == 0 || c->win_graph_shape != shape)) {
		if (c->win_graph_exec) hipGraphExecDestroy(c->win_graph_exec);
		if (c->win_graph) hipGraphDestroy(c->win_graph);
		c->win_graph_exec = nullptr;
		c->win_graph = nullptr;
		c->win_graph_state = -1;
		if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
			const hipError_t e1 = enqueue(c->stream);
			const hipError_t e2 = hipStreamEndCapture(c->stream, &c->win_graph);
			if (e1 == hipSuccess && e2 == hipSuccess && c->win_graph &&
			    hipGraphInstantiate(&c->win_graph_exec, c->win_graph, nullptr, nullptr, 0) == hipSuccess) {
				c->win_graph_state = 1;
				c->win_graph_shape = shape;
			}
		}
		(void)hipGetLastError();
	}
	if (c->win_graph_state == 1) {
		HIPCHK(hipGraphLaunch(c->win_graph_exec, c->stream));
		c->win_graph_launches++;
	} else {
		HIPCHK(enqueue(c->stream));
	}
	HIPCHK(hipGetLastError());
	c->epoch++;
	c->prepared = false;
	c->have_last = true;
	return GYS_OK;
} GYS_CATCH_ALL

// The whole single-rank window boundary as ONE captured hipGraph (BASELINE config 5: "hipGraph-captured window"): the fold kernels that
// are due (connection accumulators, Count-Min rows of the response path), k_window_prepare, the eager-mode sweep, the copy / clear
// sequence and the window-number increment -- captured once per (registry shape, which folds are due) and replayed with one launch.
// Not capturable, and therefore run as gys_window_prepare + gys_window_finish: multi-level windows (the snapshot masks depend on the
// close time) and more than one rank (the exchange sits between the two halves; gys_window_close_rccl).  With svc_hll_levels the graph
// is kept: the roll of the per-service registers (hll_level_roll, its bucket indices depend on the close time) is launched in front of
// it, and the graph then holds no clear of those registers.
int gys_window_close(gys_ctx *c, uint64_t tusec)
try {
	GYS_ENTER(c);
	if (!c) return GYS_ERR_INVAL;
	if (c->prepared) {
		set_err("window already prepared");
		return GYS_ERR_STATE;
	}
	static const bool no_graph = getenv("GYS_NO_CLOSE_GRAPH") != nullptr;
	if (c->cfg.enable_levels || c->cfg.nranks > 1 || no_graph) {
		const int rc = gys_window_prepare(c, tusec);
		return rc ? rc : gys_window_finish(c);
	}
	const uint32_t key = (c->conn_dirty && c->nsvc ? 1u : 0u) | (c->resp_dirty && c->nsvc && c->resp_win ? 2u : 0u);
	const uint64_t shape = ((uint64_t)c->hosts.size() << 32) | (uint64_t)c->nsvc;
	gys_ctx::CloseGraph &cg = c->close_graph[key];
	if (cg.state >= 0 && (cg.state == 0 || cg.shape != shape)) {
		if (cg.x) hipGraphExecDestroy(cg.x);
		if (cg.g) hipGraphDestroy(cg.g);
		cg.x = nullptr;
		cg.g = nullptr;
		cg.state = -1;
		const bool cd = c->conn_dirty, rd = c->resp_dirty;
		if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
			const int r1 = enqueue_prepare(c, true);
			const hipError_t e1 = enqueue_finish(c, c->stream);
			const hipError_t e2 = hipStreamEndCapture(c->stream, &cg.g);
			if (r1 == GYS_OK && e1 == hipSuccess && e2 == hipSuccess && cg.g && hipGraphInstantiate(&cg.x, cg.g, nullptr, nullptr, 0) == hipSuccess) {
				cg.state = 1;
				cg.shape = shape;
			}
		}
		(void)hipGetLastError();
		c->conn_dirty = cd; // (the folds were only recorded, not run)
		c->resp_dirty = rd;
	}
	if (cg.state == 1) {
		if (c->hl_lvl) {
			c->hl_close_t = (int64_t)(tusec / 1000000ull);
			const int rcl = hll_level_roll(c); // (nothing in the graph reads the per-service registers)
			if (rcl) return rcl;
		}
		ProfScope ps(c, "window_close_graph");
		HIPCHK(hipGraphLaunch(cg.x, c->stream));
		c->conn_dirty = false;
		c->resp_dirty = false;
		c->close_graph_launches++;
		c->win_graph_launches++;
	} else {
		const int rc = gys_window_prepare(c, tusec);
		return rc ? rc : gys_window_finish(c);
	}
	c->epoch++;
	c->prepared = false;
	c->have_last = true;
	return GYS_OK;
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ queries
int gys_query_svcsumm(gys_ctx *c, const uint8_t machine_id[16], gys_svcsumm *out)
try {
	GYS_ENTER(c);
	if (!c || !machine_id || !out) return GYS_ERR_INVAL;
	uint32_t host;
	int rc = lookup_host(c, machine_id, &host);
	if (rc) return rc;
	int32_t s[16];
	HIPCHK(hipMemcpyAsync(s, c->host_summ_last + (size_t)host * 16, sizeof(s), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	for (int i = 0; i < GYS_NSTATES; ++i) out->nstates[i] = s[i];
	out->tot_qps = s[6];
	out->tot_act_conn = s[7];
	out->tot_kb_inbound = s[8];
	out->tot_kb_outbound = s[9];
	out->tot_ser_errors = s[10];
	out->nlisteners = s[11];
	out->nactive = s[12];
	return GYS_OK;
} GYS_CATCH_ALL

int gys_query_clusterstate(gys_ctx *c, const char *cluster_name, gys_cluster_state *out)
try {
	GYS_ENTER(c);
	if (!c || !cluster_name || !out) return GYS_ERR_INVAL;
	auto it = c->cluster_map.find(cluster_name);
	if (it == c->cluster_map.end()) {
		set_err("unknown cluster");
		return GYS_ERR_NOTFOUND;
	}
	uint32_t v[12];
	const uint32_t *src = (const uint32_t *)(c->last + c->al.off_u32) + c->al.u32_cluster + (size_t)it->second * 12;
	HIPCHK(hipMemcpyAsync(v, src, sizeof(v), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	memcpy(out, v, sizeof(*out));
	return GYS_OK;
} GYS_CATCH_ALL

int gys_lookup_service(gys_ctx *c, uint64_t glob_id, uint32_t *slot)
try {
	GYS_ENTER(c);
	if (!c || !slot) return GYS_ERR_INVAL;
	auto it = c->gid_map_h.find(glob_id);
	if (it == c->gid_map_h.end()) {
		set_err("unknown glob_id %016llx", (unsigned long long)glob_id);
		return GYS_ERR_NOTFOUND;
	}
	*slot = it->second;
	return GYS_OK;
} GYS_CATCH_ALL

int gys_query_hist_percentiles(gys_ctx *c, uint64_t glob_id, int which, gys_hist_data *pdata, uint32_t npct, uint64_t *total_count, int64_t *max_val,
			       float *pavg)
try {
	GYS_ENTER(c);
	if (!c || !pdata || which < 0 || which > 1) return GYS_ERR_INVAL;
	uint32_t slot;
	int rc = gys_lookup_service(c, glob_id, &slot);
	if (rc) return rc;
	gys_hist_rec h;
	rc = gys_export_hist(c, which, slot, 1, &h);
	if (rc) return rc;
	const HashDef &d = hash_def(GYS_RESP_TIME_HASH);
	if (total_count) *total_count = h.total_count;
	if (max_val) *max_val = h.max_val_seen;
	if (pavg) { // common/gy_statistics.h:734-750
		int64_t total_sum = 0;
		const int64_t cnt = h.total_count ? (int64_t)h.total_count : 1;
		for (int i = 0; i < d.nthr + 2; ++i) total_sum += h.stats[i].sum;
		*pavg = (total_sum * 1.0f) / cnt;
	}
	for (uint32_t i = 0; i < npct; ++i) hist_percentile(d, h, pdata[i].percentile, &pdata[i].data_value, &pdata[i].sum, &pdata[i].count);
	return GYS_OK;
} GYS_CATCH_ALL

// quantile of an exact-integer digest: interpolation between cluster centres; only + - * / on doubles (matches oracle bit-for-bit)
static double td_quantile_interp(const int64_t *sum, const uint32_t *cnt, int32_t vmin, int32_t vmax, double q)
{
	uint64_t N = 0;
	for (int k = 0; k < GYS_TD_NB; ++k) N += cnt[k];
	if (!N) return 0.0;
	if (q < 0.0) q = 0.0;
	if (q > 1.0) q = 1.0;
	const double t = q * (double)N;
	double wbefore = 0.0, prev_c = 0.0, prev_mean = 0.0;
	bool have_prev = false;
	for (int k = 0; k < GYS_TD_NB; ++k) {
		if (!cnt[k]) continue;
		const double mean = (double)sum[k] / (double)cnt[k];
		const double c = wbefore + (double)cnt[k] * 0.5;
		if (t < c) {
			if (!have_prev) {
				const double lo = (double)vmin;
				if (c <= 0.0) return mean;
				return lo + (mean - lo) * (t / c);
			}
			return prev_mean + (mean - prev_mean) * ((t - prev_c) / (c - prev_c));
		}
		wbefore += (double)cnt[k];
		prev_c = c;
		prev_mean = mean;
		have_prev = true;
	}
	const double hi = (double)vmax, span = (double)N - prev_c;
	if (span <= 0.0) return hi;
	return prev_mean + (hi - prev_mean) * ((t - prev_c) / span);
}

// integer-millisecond data: the interpolated value rounded half-up to the value domain (same definition as the oracle)
static double td_quantile_host(const int64_t *sum, const uint32_t *cnt, int32_t vmin, int32_t vmax, double q)
{
	return std::floor(td_quantile_interp(sum, cnt, vmin, vmax, q) + 0.5);
}

// merged view of one service's digest = its clusters re-clustered with its buffered values (k_digest_merge in query mode: the state
// is not modified)
static int td_merged_view(gys_ctx *c, uint32_t slot, int64_t *sum, uint32_t *cnt, int32_t *vmin, int32_t *vmax)
{
	int rc = fold_range(c, slot, 1); // min / max must cover the buffered values
	if (rc) return rc;
	TdMeta mt;
	HIPCHK(hipMemcpyAsync(&mt, c->td_meta + slot, sizeof(mt), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	const MergeEnt ent{slot, mt.npend, 0u, 0u};
	HIPCHK(hipMemcpyAsync(c->query_list, &ent, sizeof(ent), hipMemcpyHostToDevice, c->stream));
	MergeP mp{};
	mp.d = digest_params(c);
	mp.list = c->query_list;
	mp.count = c->merge_count + FIN_QUERY_ONE;
	mp.out_sum = c->query_sum;
	mp.out_cnt = c->query_cnt;
	if (mt.npend <= GYS_MERGE_CLASS0) hipLaunchKernelGGL((k_digest_merge<GYS_MERGE_CLASS0, 256u>), dim3(1), dim3(256), 0, c->stream, mp);
	else if (mt.npend <= GYS_MERGE_CLASS1) hipLaunchKernelGGL((k_digest_merge<GYS_MERGE_CLASS1, 256u>), dim3(1), dim3(256), 0, c->stream, mp);
	else hipLaunchKernelGGL((k_digest_merge<GYS_MERGE_LDS_MAX, 1024u>), dim3(1), dim3(1024), 0, c->stream, mp);
	HIPCHK(hipGetLastError());
	int2 mm;
	HIPCHK(hipMemcpyAsync(sum, c->query_sum, sizeof(int64_t) * GYS_TD_NB, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(cnt, c->query_cnt, sizeof(uint32_t) * GYS_TD_NB, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(&mm, c->td_minmax + slot, sizeof(mm), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	*vmin = mm.x;
	*vmax = mm.y;
	return GYS_OK;
}

#define TDIGEST_CHECK()                         \
	if (!c->cfg.enable_tdigest) {           \
		set_err("t-digest disabled");   \
		return GYS_ERR_STATE;           \
	}

int gys_query_quantiles(gys_ctx *c, uint64_t glob_id, const double *q, uint32_t nq, double *out)
try {
	GYS_ENTER(c);
	if (!c || !q || !out) return GYS_ERR_INVAL;
	TDIGEST_CHECK();
	uint32_t slot;
	int rc = gys_lookup_service(c, glob_id, &slot);
	if (rc) return rc;
	int64_t sum[GYS_TD_NB];
	uint32_t cnt[GYS_TD_NB];
	int32_t vmin, vmax;
	rc = td_merged_view(c, slot, sum, cnt, &vmin, &vmax);
	if (rc) return rc;
	for (uint32_t i = 0; i < nq; ++i) out[i] = td_quantile_host(sum, cnt, vmin, vmax, q[i]);
	return GYS_OK;
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ Postgres tdigest forms
// The reference aggregates percentiles in SQL with the tdigest extension (tvondra/tdigest, not in /root/reference and unpinned:
// "create extension if not exists tdigest" common/gy_query_common.cc:3387; public.tdigest(col, 100) / public.tdigest_percentile
// :1818-1855, common/gy_json_field_maps.h:2641).  These two calls hand a service's digest over in that type's own external forms so
// that '<text>'::public.tdigest (or the binary COPY / libpq form) can be fed to public.tdigest_percentile and unioned with row
// digests.  Restated from the extension's published I/O functions (tdigest_out / tdigest_send, format with the TDIGEST_STORES_MEAN
// flag, 1.2.0 and later); the extension is absent here => PARITY UNPINNED.
//   text:   flags 1 count <N> compression 100 centroids <K> (<mean %lf>, <count>) ...      (means ascending)
//   binary: int32 flags | int64 count | int32 compression | int32 ncentroids | K x { float8 mean, int64 count }, network byte order
static int td_sql_centroids(gys_ctx *c, uint64_t glob_id, double *mean, int64_t *count, int *k, int64_t *total)
{
	uint32_t slot;
	int rc = gys_lookup_service(c, glob_id, &slot);
	if (rc) return rc;
	int64_t sum[GYS_TD_NB];
	uint32_t cnt[GYS_TD_NB];
	int32_t vmin, vmax;
	rc = td_merged_view(c, slot, sum, cnt, &vmin, &vmax);
	if (rc) return rc;
	*k = 0;
	*total = 0;
	for (int i = 0; i < GYS_TD_NB; ++i)
		if (cnt[i]) {
			mean[*k] = (double)sum[i] / (double)cnt[i];
			count[*k] = (int64_t)cnt[i];
			*total += (int64_t)cnt[i];
			++*k;
		}
	if (*k == 0) { // tdigest_in rejects count <= 0: an empty digest has no literal (SQL NULL is the empty aggregate)
		set_err("service %016llx has no response values yet", (unsigned long long)glob_id);
		return GYS_ERR_NOTFOUND;
	}
	return GYS_OK;
}

int gys_tdigest_sql_text(gys_ctx *c, uint64_t glob_id, char *buf, size_t buflen, size_t *needed)
try {
	GYS_ENTER(c);
	if (!c || (!buf && buflen)) return GYS_ERR_INVAL;
	TDIGEST_CHECK();
	double mean[GYS_TD_NB];
	int64_t count[GYS_TD_NB], total;
	int k;
	const int rc = td_sql_centroids(c, glob_id, mean, count, &k, &total);
	if (rc) return rc;
	std::string out;
	char tmp[96];
	snprintf(tmp, sizeof(tmp), "flags 1 count %lld compression %d centroids %d", (long long)total, GYS_TD_NB, k);
	out = tmp;
	for (int i = 0; i < k; ++i) {
		snprintf(tmp, sizeof(tmp), " (%lf, %lld)", mean[i], (long long)count[i]);
		out += tmp;
	}
	if (needed) *needed = out.size();
	if (out.size() + 1 > buflen) return GYS_ERR_NOMEM;
	memcpy(buf, out.c_str(), out.size() + 1);
	return GYS_OK;
} GYS_CATCH_ALL

int gys_tdigest_sql_binary(gys_ctx *c, uint64_t glob_id, void *buf, size_t buflen, size_t *needed)
try {
	GYS_ENTER(c);
	if (!c || (!buf && buflen)) return GYS_ERR_INVAL;
	TDIGEST_CHECK();
	double mean[GYS_TD_NB];
	int64_t count[GYS_TD_NB], total;
	int k;
	const int rc = td_sql_centroids(c, glob_id, mean, count, &k, &total);
	if (rc) return rc;
	const size_t len = 4 + 8 + 4 + 4 + (size_t)k * 16;
	if (needed) *needed = len;
	if (len > buflen) return GYS_ERR_NOMEM;
	uint8_t *p = (uint8_t *)buf;
	auto be = [&p](uint64_t v, int nbytes) { // pq_sendint32 / pq_sendint64 / pq_sendfloat8: big endian
		for (int i = nbytes - 1; i >= 0; --i) *p++ = (uint8_t)(v >> (8 * i));
	};
	be(1u, 4);
	be((uint64_t)total, 8);
	be((uint64_t)GYS_TD_NB, 4);
	be((uint64_t)k, 4);
	for (int i = 0; i < k; ++i) {
		uint64_t bits;
		memcpy(&bits, &mean[i], 8);
		be(bits, 8);
		be((uint64_t)count[i], 8);
	}
	return GYS_OK;
} GYS_CATCH_ALL

static double hll_estimate_host(const uint8_t *regs, int p)
{
	const uint32_t m = 1u << p;
	double sum = 0.0;
	uint32_t zeros = 0;
	for (uint32_t i = 0; i < m; ++i) {
		sum += 1.0 / (double)(1ull << regs[i]);
		zeros += regs[i] == 0;
	}
	const double alpha = m == 16 ? 0.673 : (m == 32 ? 0.697 : (m == 64 ? 0.709 : 0.7213 / (1.0 + 1.079 / (double)m)));
	double e = alpha * (double)m * (double)m / sum;
	if (e <= 2.5 * (double)m && zeros) e = (double)m * std::log((double)m / (double)zeros);
	return e;
}

int gys_query_distinct_flows(gys_ctx *c, double *out)
try {
	GYS_ENTER(c);
	if (!c || !out) return GYS_ERR_INVAL;
	std::vector<uint8_t> regs((size_t)1 << GYS_HLL_P);
	HIPCHK(hipMemcpyAsync(regs.data(), c->last + c->al.off_hll8, regs.size(), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	*out = hll_estimate_host(regs.data(), GYS_HLL_P);
	return GYS_OK;
} GYS_CATCH_ALL

int gys_query_cms(gys_ctx *c, uint64_t glob_id, int which, uint64_t *out)
try {
	GYS_ENTER(c);
	if (!c || !out || which < 0 || which > 1) return GYS_ERR_INVAL;
	uint64_t best = ~0ull;
	for (uint32_t r = 0; r < GYS_CMS_D; ++r) {
		const uint32_t col = jhash2_u64(glob_id, GYS_SEED + r) & (GYS_CMS_W - 1);
		uint64_t v = 0;
		if (which == 0) {
			uint32_t v32;
			HIPCHK(hipMemcpyAsync(&v32, (const uint32_t *)(c->last + c->al.off_u32) + c->al.u32_cms + (size_t)r * GYS_CMS_W + col, 4,
					      hipMemcpyDeviceToHost, c->stream));
			HIPCHK(hipStreamSynchronize(c->stream));
			v = v32;
		} else {
			HIPCHK(hipMemcpyAsync(&v, (const uint64_t *)(c->last + c->al.off_i64sum) + c->al.i64_cms + (size_t)r * GYS_CMS_W + col, 8,
					      hipMemcpyDeviceToHost, c->stream));
			HIPCHK(hipStreamSynchronize(c->stream));
		}
		best = std::min(best, v);
	}
	*out = best;
	return GYS_OK;
} GYS_CATCH_ALL

// Count-Min estimate for a (listener, client task group) pair.  which 0 / 1: active connections / bytes of the ACTIVE_CONN_STATS reports of
// the last three windows (per-cell maximum, k_act_latch); which 2 / 3 and 4 / 5: closed connections / bytes of the TCP_CONN_NOTIFY roll-up
// in the last finished window, listener side (connlistenmap_) and client side (connclientmap_) (gys_config.conn_pair_cms); which 6 / 7: as 0 / 1
// for the ACTIVE_CONN_STATS rows whose listener lives on another madhava (is_remote_listen_: the reference's remoteconntbl rows).
static int pair_tables(gys_ctx *c, int which, const void **tbl)
{
	if (which < 0 || which > 7) return GYS_ERR_INVAL;
	if (which == 6) {
		*tbl = c->last_act32 + (uint64_t)GYS_CMS_D * GYS_CMS_W;
		return GYS_OK;
	}
	if (which == 7) {
		*tbl = c->last_act64 + (uint64_t)GYS_CMS_D * GYS_CMS_W;
		return GYS_OK;
	}
	if (which >= 2 && !c->cfg.conn_pair_cms) {
		set_err("gys_config.conn_pair_cms is off");
		return GYS_ERR_STATE;
	}
	switch (which) {
	case 0: *tbl = c->last_act32; break;
	case 1: *tbl = c->last_act64; break;
	case 2: *tbl = (const uint32_t *)(c->last + c->al.off_u32) + c->al.u32_cpair; break;
	case 3: *tbl = (const uint64_t *)(c->last + c->al.off_i64sum) + c->al.i64_cpair; break;
	case 4: *tbl = (const uint32_t *)(c->last + c->al.off_u32) + c->al.u32_cpair + (uint64_t)GYS_CMS_D * GYS_CMS_W; break;
	default: *tbl = (const uint64_t *)(c->last + c->al.off_i64sum) + c->al.i64_cpair + (uint64_t)GYS_CMS_D * GYS_CMS_W; break;
	}
	return GYS_OK;
}

int gys_query_pair_cms(gys_ctx *c, uint64_t listener_glob_id, uint64_t cli_aggr_task_id, int which, uint64_t *out)
try {
	GYS_ENTER(c);
	if (!c || !out) return GYS_ERR_INVAL;
	const void *tbl;
	const int rc = pair_tables(c, which, &tbl);
	if (rc) return rc;
	uint64_t best = ~0ull;
	for (uint32_t r = 0; r < GYS_CMS_D; ++r) {
		const uint32_t col = jhash2_4w((uint32_t)listener_glob_id, (uint32_t)(listener_glob_id >> 32), (uint32_t)cli_aggr_task_id,
					       (uint32_t)(cli_aggr_task_id >> 32), GYS_SEED + r) & (GYS_CMS_W - 1);
		uint64_t v = 0;
		if (!(which & 1)) {
			uint32_t v32;
			HIPCHK(hipMemcpyAsync(&v32, (const uint32_t *)tbl + (size_t)r * GYS_CMS_W + col, 4, hipMemcpyDeviceToHost, c->stream));
			HIPCHK(hipStreamSynchronize(c->stream));
			v = v32;
		} else {
			HIPCHK(hipMemcpyAsync(&v, (const uint64_t *)tbl + (size_t)r * GYS_CMS_W + col, 8, hipMemcpyDeviceToHost, c->stream));
			HIPCHK(hipStreamSynchronize(c->stream));
		}
		best = std::min(best, v);
	}
	*out = best;
	return GYS_OK;
} GYS_CATCH_ALL

int gys_export_pair_cms(gys_ctx *c, int which, void *out)
try {
	GYS_ENTER(c);
	if (!c || !out) return GYS_ERR_INVAL;
	const void *tbl;
	const int rc = pair_tables(c, which, &tbl);
	if (rc) return rc;
	const size_t n = (size_t)GYS_CMS_D * GYS_CMS_W;
	HIPCHK(hipMemcpyAsync(out, tbl, n * ((which & 1) ? 8 : 4), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
} GYS_CATCH_ALL

int gys_export_active_conn_counters(gys_ctx *c, uint32_t first_slot, uint32_t nslots, uint64_t *out)
try {
	GYS_ENTER(c);
	if (!c || !out || (uint64_t)first_slot + nslots > c->nsvc) return GYS_ERR_INVAL;
	if (!nslots) return GYS_OK;
	HIPCHK(hipMemcpyAsync(out, c->svc_act + (size_t)first_slot * 4, (size_t)nslots * 32, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
} GYS_CATCH_ALL

int gys_query_topn(gys_ctx *c, const uint8_t machine_id[16], int kind, gys_topn_entry out[GYS_TOPN], uint32_t *nout)
try {
	GYS_ENTER(c);
	if (!c || !machine_id || !out || !nout || kind < 0 || kind > 3) return GYS_ERR_INVAL;
	uint32_t host;
	int rc = lookup_host(c, machine_id, &host);
	if (rc) return rc;
	*nout = 0;
	if (!c->nsvc || c->epoch < 2) return GYS_OK;
	const uint32_t cap = (uint32_t)std::min<uint64_t>(c->cfg.max_services, 65536);
	HIPCHK(hipMemsetAsync(c->misc + 1, 0, 4, c->stream));
	hipLaunchKernelGGL(k_topn_filter, dim3((c->nsvc + 255) / 256), dim3(256), 0, c->stream, c->svc_state, c->nsvc, host, c->epoch - 1, kind, c->topn_slot,
			   c->topn_metric, c->misc + 1, cap);
	uint32_t cnt = 0;
	HIPCHK(hipMemcpyAsync(&cnt, c->misc + 1, 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	cnt = std::min(cnt, cap);
	if (!cnt) return GYS_OK;
	std::vector<uint32_t> slots(cnt);
	std::vector<uint64_t> metrics(cnt);
	HIPCHK(hipMemcpy(slots.data(), c->topn_slot, (size_t)cnt * 4, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(metrics.data(), c->topn_metric, (size_t)cnt * 8, hipMemcpyDeviceToHost));
	std::vector<uint32_t> order(cnt);
	for (uint32_t i = 0; i < cnt; ++i) order[i] = i;
	// BOUNDED_PRIO_QUEUE keeps the N largest (common/gy_statistics.h:385-414); ties resolved by lowest service slot for determinism
	std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return metrics[a] != metrics[b] ? metrics[a] > metrics[b] : slots[a] < slots[b]; });
	const uint32_t k = std::min<uint32_t>(cnt, GYS_TOPN);
	for (uint32_t i = 0; i < k; ++i) {
		const uint32_t s = slots[order[i]];
		uint8_t rec[96];
		HIPCHK(hipMemcpy(rec, c->svc_state + (size_t)s * 96, 96, hipMemcpyDeviceToHost));
		memcpy(out[i].state, rec, 88);
		memcpy(&out[i].glob_id, rec, 8);
		out[i].host_slot = host;
		out[i].metric = (uint32_t)metrics[order[i]];
	}
	*nout = k;
	return GYS_OK;
} GYS_CATCH_ALL

int gys_scan_percentiles_dev(gys_ctx *c, int which, const float *pcts, uint32_t npct, int64_t *d_out)
try {
	GYS_ENTER(c);
	if (!c || !pcts || !d_out || !npct || npct > 64 || which < 0 || which > 1) return GYS_ERR_INVAL;
	if (!c->nsvc) return GYS_OK;
	HIPCHK(hipMemcpyAsync(c->dev_pcts, pcts, (size_t)npct * 4, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream)); // pcts may be a short-lived host buffer
	{
		const int rcf = fold_range(c, 0, c->nsvc);
		if (rcf) return rcf;
	}
	ProfScope ps(c, "hist_percentiles");
	hipLaunchKernelGGL(k_hist_percentiles_view, dim3((c->nsvc + 255) / 256), dim3(256), 0, c->stream, window_records(c), c->hist_all,
			   c->cfg.enable_tdigest ? c->td_meta : nullptr, c->epoch, which, c->nsvc, c->dev_pcts, npct, d_out);
	HIPCHK(hipGetLastError());
	return GYS_OK;
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ exports
int gys_scan_quantiles_dev(gys_ctx *c, const double *q, uint32_t nq, double *d_out)
try {
	GYS_ENTER(c);
	if (!c || !q || !d_out || nq == 0 || nq > 16) return GYS_ERR_INVAL;
	TDIGEST_CHECK();
	if (!c->nsvc) return GYS_OK;
	DevBuf<double> d_q;
	int rc = d_q.alloc(nq, false);
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(d_q, q, sizeof(double) * nq, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemsetAsync(c->merge_count + FIN_SLOW, 0, 4, c->stream));
	MergeBP bp{};
	bp.d = digest_params(c);
	bp.slow_list = c->merge_list_slow;
	bp.slow_count = c->merge_count + FIN_SLOW;
	bp.qs = d_q;
	bp.nq = nq;
	bp.qout = d_out;
	{
		ProfScope ps(c, "scan_quantiles");
		const dim3 sgrid(std::max(1u, std::min<uint32_t>(c->nsvc, (uint32_t)c->ncu * 8)));
		if (c->pend_cap <= 1024u) hipLaunchKernelGGL((k_digest_bins<true, 4u>), sgrid, dim3(256), 0, c->stream, bp);
		else if (c->pend_cap <= 2048u) hipLaunchKernelGGL((k_digest_bins<true, 8u>), sgrid, dim3(256), 0, c->stream, bp);
		else hipLaunchKernelGGL((k_digest_bins<true, 16u>), sgrid, dim3(256), 0, c->stream, bp);
	}
	uint32_t nslow = 0;
	HIPCHK(hipMemcpyAsync(&nslow, c->merge_count + FIN_SLOW, 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (nslow) { // services whose digest weighs 2^31 or more (64-bit weights) or whose buffer holds more than GYS_MB_BIG_CAP values of a second or longer: one at a time through the general merge
		std::vector<MergeEnt> slow(nslow);
		HIPCHK(hipMemcpy(slow.data(), c->merge_list_slow, sizeof(MergeEnt) * nslow, hipMemcpyDeviceToHost));
		std::vector<double> out(nq);
		for (const MergeEnt &e : slow) {
			int64_t sum[GYS_TD_NB];
			uint32_t cnt[GYS_TD_NB];
			int32_t vmin, vmax;
			const int rc = td_merged_view(c, e.slot, sum, cnt, &vmin, &vmax);
			if (rc) return rc;
			for (uint32_t i = 0; i < nq; ++i) out[i] = td_quantile_host(sum, cnt, vmin, vmax, q[i]);
			HIPCHK(hipMemcpy(d_out + (size_t)e.slot * nq, out.data(), sizeof(double) * nq, hipMemcpyHostToDevice));
		}
	}
	return GYS_OK;
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ ranks (gys_tdrank.hpp)
// k_td_ranks over members [first, first + n): service slots (d_in == nullptr) or the slabs at d_in.  Asynchronous on the context stream.
static int td_ranks_launch(gys_ctx *c, const gys_tdigest_slab *d_in, uint32_t first, uint32_t n, const int64_t *thr, uint32_t nt, double *d_below, uint64_t *d_total)
{
	if (!n) return GYS_OK;
	TdRankP rp{};
	rp.d = digest_params(c);
	rp.in = d_in;
	rp.first = first;
	rp.n = n;
	rp.nt = nt;
	for (uint32_t i = 0; i < nt; ++i) rp.thr[i] = thr[i];
	rp.below = d_below;
	rp.total = (unsigned long long *)d_total;
	// a wave per member, four to a workgroup.  Up to 16 workgroups per CU: with 1 - 4 thresholds eight of them are resident at a time (8 waves per
	// SIMD; 5 - 8 thresholds: six, 9 - 16: five), the rest follow as those finish and even out the tail
	const dim3 grid(std::max(1u, std::min<uint32_t>((n + 3u) / 4u, (uint32_t)c->ncu * 16u))), block(GYS_TR_NT);
	ProfScope ps(c, d_in ? "slab_ranks" : "scan_ranks");
	if (d_in) hipLaunchKernelGGL((k_td_ranks<1, 1u>), grid, block, 0, c->stream, rp);
	else if (nt <= 2u) hipLaunchKernelGGL((k_td_ranks<0, 1u>), grid, block, 0, c->stream, rp);
	else if (nt <= 4u) hipLaunchKernelGGL((k_td_ranks<0, 2u>), grid, block, 0, c->stream, rp);
	else if (nt <= 8u) hipLaunchKernelGGL((k_td_ranks<0, 4u>), grid, block, 0, c->stream, rp);
	else hipLaunchKernelGGL((k_td_ranks<0, 8u>), grid, block, 0, c->stream, rp);
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

#define RANKS_NT_CHECK(name)                                                             \
	if (nt == 0 || nt > GYS_TR_MAXT) {                                               \
		set_err(name ": 1 .. %u thresholds per call", (unsigned)GYS_TR_MAXT);    \
		return GYS_ERR_INVAL;                                                    \
	}

int gys_scan_ranks_dev(gys_ctx *c, const int64_t *thr, uint32_t nt, double *d_below, uint64_t *d_total)
try {
	GYS_ENTER(c);
	if (!c || !thr || !d_below) return GYS_ERR_INVAL;
	TDIGEST_CHECK();
	RANKS_NT_CHECK("gys_scan_ranks_dev");
	return td_ranks_launch(c, nullptr, 0u, c->nsvc, thr, nt, d_below, d_total);
} GYS_CATCH_ALL

int gys_query_ranks(gys_ctx *c, uint64_t glob_id, const int64_t *thr, uint32_t nt, double *below, uint64_t *total)
try {
	GYS_ENTER(c);
	if (!c || !thr || !below) return GYS_ERR_INVAL;
	TDIGEST_CHECK();
	RANKS_NT_CHECK("gys_query_ranks");
	uint32_t slot;
	int rc = gys_lookup_service(c, glob_id, &slot);
	if (rc) return rc;
	// the scan's kernel on this one slot: nt doubles, then the total, in a row the context keeps
	if ((rc = c->rank_row.grow(GYS_TR_MAXT + 1u, c->stream)) != GYS_OK) return rc;
	double *const d_row = c->rank_row.p;
	if ((rc = td_ranks_launch(c, nullptr, slot, 1u, thr, nt, d_row, (uint64_t *)(d_row + nt))) != GYS_OK) return rc;
	double row[GYS_TR_MAXT + 1u];
	HIPCHK(hipMemcpyAsync(row, d_row, ((size_t)nt + 1u) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	memcpy(below, row, (size_t)nt * sizeof(double));
	if (total) memcpy(total, row + nt, sizeof(uint64_t));
	return GYS_OK;
} GYS_CATCH_ALL

int gys_tdigest_slab_ranks_dev(gys_ctx *c, const gys_tdigest_slab *d_slabs, uint32_t nslabs, const int64_t *thr, uint32_t nt, double *d_below, uint64_t *d_total)
try {
	GYS_ENTER(c);
	if (!c || !d_slabs || !thr || !d_below) return GYS_ERR_INVAL;
	TDIGEST_CHECK();
	RANKS_NT_CHECK("gys_tdigest_slab_ranks_dev");
	return td_ranks_launch(c, d_slabs, 0u, nslabs, thr, nt, d_below, d_total);
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ the cached groupings
#define GYS_RB_CHUNK_SERVICES 1024u // members a workgroup of k_rollup_accum adds up before it hands its bins to the group's
#define GYS_RB_CHUNK_SLABS 32u

// g, cut into chunks of GYS_RB_CHUNK_SERVICES members, becomes dg's lists on the host and on the device, as of the current generation
static int groups_install(gys_ctx *c, DeviceGroups &dg, GroupLists g, bool with_off)
{
	dg.gen = ~0ull;
	dg.h = std::move(g);
	groups_chunk(dg.h, GYS_RB_CHUNK_SERVICES);
	dg.nchunks = (uint32_t)dg.h.chunks.size();
	int rc = dg.members.upload(dg.h.members, c->stream);
	if (rc == GYS_OK) rc = dg.chunks.upload(dg.h.chunks, c->stream);
	if (rc == GYS_OK) rc = dg.gchunks.upload(dg.h.gchunks, c->stream);
	if (rc == GYS_OK && with_off) rc = dg.off.upload(dg.h.off, c->stream);
	if (rc) return rc;
	HIPCHK(hipStreamSynchronize(c->stream));
	dg.gen = c->registry_gen;
	return GYS_OK;
}

// host -> member services (10^7 services: 40 MB), ascending slot inside a host: the order in which the top-N breaks ties.  The roll-ups
// share the list: their kernels add integers and take maxima / minima per group (gys_rollup.hpp, gys_hllroll.hpp, gys_histroll.hpp), so
// neither the order of a group's members nor where its chunks are cut changes a bit of their results.
static int ensure_host_groups(gys_ctx *c)
{
	if (c->host_groups.gen == c->registry_gen) return GYS_OK;
	std::vector<std::vector<uint32_t>> lists(c->hosts.size());
	for (size_t h = 0; h < lists.size(); ++h) {
		lists[h] = c->host_lst[h].all_slots;
		std::sort(lists[h].begin(), lists[h].end());
	}
	return groups_install(c, c->host_groups, groups_from_lists(lists), true);
}

// cluster -> member hosts, ascending host slot inside a cluster
static int ensure_cluster_groups(gys_ctx *c)
{
	if (c->cluster_groups.gen == c->registry_gen) return GYS_OK;
	return groups_install(c, c->cluster_groups, groups_from_keys(c->host_cluster_h, (uint32_t)c->cluster_names.size()), false);
}


// the 10 best services of EVERY host for one kind (last closed window): slots[h * GYS_TOPN + r] (GYS_NOSLOT = none), metrics likewise
static int topn_all_hosts(gys_ctx *c, int kind, std::vector<uint32_t> &slots, std::vector<uint64_t> &metrics)
{
	const uint32_t nh = (uint32_t)c->hosts.size();
	slots.assign((size_t)nh * GYS_TOPN, GYS_NOSLOT);
	metrics.assign((size_t)nh * GYS_TOPN, 0);
	if (!nh || !c->nsvc || c->epoch < 2) return GYS_OK;
	int rc = ensure_host_groups(c);
	if (rc) return rc;
	DevBuf<uint32_t> d_slot;
	DevBuf<uint64_t> d_metric;
	if ((rc = d_slot.grow(slots.size(), c->stream)) != GYS_OK || (rc = d_metric.grow(metrics.size(), c->stream)) != GYS_OK) return rc;
	TopnHostsP tp{};
	tp.svc_state = c->svc_state;
	tp.off = c->host_groups.off.p;
	tp.members = c->host_groups.members.p;
	tp.nhosts = nh;
	tp.epoch = c->epoch - 1;
	tp.kind = kind;
	tp.out_slot = d_slot.p;
	tp.out_metric = d_metric.p;
	{
		ProfScope ps(c, "topn_hosts");
		hipLaunchKernelGGL(k_topn_hosts, dim3(std::min<uint32_t>(nh, (uint32_t)c->ncu * 8)), dim3(256), 0, c->stream, tp);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(slots.data(), d_slot.p, slots.size() * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(metrics.data(), d_metric.p, metrics.size() * 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream)); // (d_slot / d_metric go at scope exit)
	return GYS_OK;
}

int gys_tdigest_slab_quantiles(gys_ctx *c, const gys_tdigest_slab *d_slab, const double *q, uint32_t nq, double *out)
try {
	GYS_ENTER(c);
	if (!c || !d_slab || !q || !out) return GYS_ERR_INVAL;
	gys_tdigest_slab s;
	HIPCHK(hipMemcpyAsync(&s, d_slab, sizeof(s), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	// td_quantile_interp on the wide counters (same arithmetic: exact integer prefix weights as doubles, one division per centre)
	uint64_t N = 0;
	for (int k = 0; k < GYS_TD_NB; ++k) N += s.cnt[k];
	for (uint32_t i = 0; i < nq; ++i) {
		double r = 0.0;
		if (N) {
			double qq = q[i] < 0.0 ? 0.0 : (q[i] > 1.0 ? 1.0 : q[i]);
			const double t = qq * (double)N;
			double wbefore = 0.0, prev_c = 0.0, prev_mean = 0.0;
			bool have_prev = false, done = false;
			for (int k = 0; k < GYS_TD_NB && !done; ++k) {
				if (!s.cnt[k]) continue;
				const double mean = (double)s.sum[k] / (double)s.cnt[k];
				const double cc = wbefore + (double)s.cnt[k] * 0.5;
				if (t < cc) {
					if (!have_prev) {
						const double lo = (double)s.vmin;
						r = cc <= 0.0 ? mean : lo + (mean - lo) * (t / cc);
					} else {
						r = prev_mean + (mean - prev_mean) * ((t - prev_c) / (cc - prev_c));
					}
					done = true;
					break;
				}
				wbefore += (double)s.cnt[k];
				prev_c = cc;
				prev_mean = mean;
				have_prev = true;
			}
			if (!done) {
				const double hi = (double)s.vmax, span = (double)N - prev_c;
				r = span <= 0.0 ? hi : prev_mean + (hi - prev_mean) * ((t - prev_c) / span);
			}
			r = std::floor(r + 0.5);
		}
		out[i] = r;
	}
	return GYS_OK;
} GYS_CATCH_ALL

uint32_t gys_num_clusters(gys_ctx *c) { return c ? (uint32_t)c->cluster_names.size() : 0; }

// ------------------------------------------------------------------------------------------------ RCCL exchange in the library
// RCCL is bound at run time (dlopen), not at link time: a process that never joins a communicator (one madhava, one GPU) does not need
// the library at all, and a host process that already carries an RCCL of its own (PyTorch bundles one) can point the engine at THAT
// copy instead of running two different RCCL builds side by side.  GYS_RCCL_LIB = path or soname; default "librccl.so" (found through
// this library's RUNPATH /opt/rocm/lib).  tests/cpp/fakerccl is a stand-in with the same entry points (two ranks on one GPU).
namespace {
struct RcclApi {
	void *handle = nullptr;
	decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
	decltype(&ncclCommInitRank) CommInitRank = nullptr;
	decltype(&ncclCommDestroy) CommDestroy = nullptr;
	decltype(&ncclCommCount) CommCount = nullptr;
	decltype(&ncclCommUserRank) CommUserRank = nullptr;
	decltype(&ncclGetErrorString) GetErrorString = nullptr;
	decltype(&ncclGroupStart) GroupStart = nullptr;
	decltype(&ncclGroupEnd) GroupEnd = nullptr;
	decltype(&ncclAllReduce) AllReduce = nullptr;
	decltype(&ncclAllGather) AllGather = nullptr;
	std::string err, path;
};

RcclApi *rccl_api()
{
	static RcclApi api = [] {
		RcclApi a;
		const char *env = getenv("GYS_RCCL_LIB");
		a.path = env && *env ? env : "librccl.so";
		a.handle = dlopen(a.path.c_str(), RTLD_NOW | RTLD_LOCAL);
		if (!a.handle && !(env && *env)) a.handle = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
		if (!a.handle) {
			const char *e = dlerror();
			a.err = std::string("cannot load ") + a.path + ": " + (e ? e : "?");
			return a;
		}
#define GYS_RCCL_SYM(name)                                                        \
	a.name = (decltype(a.name))dlsym(a.handle, "nccl" #name);                 \
	if (!a.name && a.err.empty()) a.err = a.path + " has no nccl" #name;
		GYS_RCCL_SYM(GetUniqueId)
		GYS_RCCL_SYM(CommInitRank)
		GYS_RCCL_SYM(CommDestroy)
		GYS_RCCL_SYM(CommCount)
		GYS_RCCL_SYM(CommUserRank)
		GYS_RCCL_SYM(GetErrorString)
		GYS_RCCL_SYM(GroupStart)
		GYS_RCCL_SYM(GroupEnd)
		GYS_RCCL_SYM(AllReduce)
		GYS_RCCL_SYM(AllGather)
#undef GYS_RCCL_SYM
		return a;
	}();
	return &api;
}
} // namespace

#define RCCL_API(R)                                            \
	RcclApi *R = rccl_api();                               \
	if (!R->err.empty()) {                                 \
		set_err("RCCL unavailable: %s", R->err.c_str()); \
		return GYS_ERR_HIP;                            \
	}

#define NCCLCHK(expr)                                                                          \
	do {                                                                                   \
		const ncclResult_t r_ = (expr);                                                \
		if (r_ != ncclSuccess) {                                                       \
			set_err("%s failed: %s (%s:%d)", #expr, R->GetErrorString(r_), __FILE__, __LINE__); \
			return GYS_ERR_HIP;                                                    \
		}                                                                              \
	} while (0)

static_assert(sizeof(ncclUniqueId) == GYS_RCCL_UID_BYTES, "gysketch.h carries an ncclUniqueId as 128 opaque bytes");

int gys_rccl_unique_id(uint8_t uid[GYS_RCCL_UID_BYTES])
try {
	if (!uid) return GYS_ERR_INVAL;
	// The exchange is between the GPUs of ONE node: unless the caller chose an interface, the bootstrap rendezvous goes over
	// loopback -- RCCL otherwise takes the first non-loopback interface, and on hosts whose first interface is a tunnel / container
	// bridge the ranks' connect() to it never returns (seen on part of the MI355X pool).  Must be set before RCCL's first call.
	setenv("NCCL_SOCKET_IFNAME", "lo", 0);
	RCCL_API(R);
	ncclUniqueId id;
	NCCLCHK(R->GetUniqueId(&id));
	memcpy(uid, &id, sizeof(id));
	return GYS_OK;
} GYS_CATCH_ALL

int gys_rccl_comm_create(gys_ctx *c, const uint8_t uid[GYS_RCCL_UID_BYTES], int nranks, int rank, void **comm)
try {
	GYS_ENTER(c);
	if (!c || !uid || !comm || nranks < 1 || rank < 0 || rank >= nranks) return GYS_ERR_INVAL;
	if ((uint32_t)nranks != std::max<uint32_t>(c->cfg.nranks, 1) || (uint32_t)rank != c->cfg.rank) {
		set_err("communicator (%d of %d) does not match gys_config rank / nranks (%u of %u)", rank, nranks, c->cfg.rank, c->cfg.nranks);
		return GYS_ERR_INVAL;
	}
	HIPCHK(hipSetDevice(c->device));
	setenv("NCCL_SOCKET_IFNAME", "lo", 0); // (see gys_rccl_unique_id)
	ncclUniqueId id;
	memcpy(&id, uid, sizeof(id));
	RCCL_API(R);
	ncclComm_t cm = nullptr;
	NCCLCHK(R->CommInitRank(&cm, nranks, id, rank));
	*comm = (void *)cm;
	return GYS_OK;
} GYS_CATCH_ALL

int gys_rccl_comm_destroy(void *comm)
try {
	if (!comm) return GYS_ERR_INVAL;
	RCCL_API(R);
	NCCLCHK(R->CommDestroy((ncclComm_t)comm));
	return GYS_OK;
} GYS_CATCH_ALL

int gys_window_close_rccl(gys_ctx *c, void *comm, uint64_t tusec)
try {
	GYS_ENTER(c);
	if (!c || !comm) return GYS_ERR_INVAL;
	RCCL_API(R);
	int rc = GYS_OK;
	if (!c->prepared) rc = gys_window_prepare(c, tusec); // (a call that failed in the exchange below left the window prepared: the retry resumes here)
	if (rc) return rc;
	gys_reduce_section sec[4];
	uint32_t nsec = 0;
	rc = gys_reduce_sections(c, sec, &nsec);
	if (rc) return rc;
	{
		ProfScope ps(c, "window_rccl");
		NCCLCHK(R->GroupStart());
		// from here on the group is ALWAYS closed: an error between Start and End would leave every later RCCL call of this thread
		// inside a group that never launches
		ncclResult_t bad = ncclSuccess;
		for (uint32_t i = 0; i < nsec && bad == ncclSuccess; ++i) {
			const ncclDataType_t dt = sec[i].dtype == 0 ? ncclUint8 : (sec[i].dtype == 1 ? ncclUint32 : ncclInt64);
			const ncclRedOp_t op = sec[i].op == 0 ? ncclMax : ncclSum;
			bad = R->AllReduce(sec[i].dev_ptr, sec[i].dev_ptr, sec[i].nelems, dt, op, (ncclComm_t)comm, c->stream);
		}
		const ncclResult_t end = R->GroupEnd();
		if (bad == ncclSuccess) bad = end;
		if (bad != ncclSuccess) {
			// the window stays prepared (arena not cleared, nothing finished): the caller may retry this call -- it resumes at the
			// exchange -- or fall back to gys_reduce_sections + its own collective + gys_window_finish
			set_err("window exchange failed: %s", R->GetErrorString(bad));
			return GYS_ERR_HIP;
		}
	}
	return gys_window_finish(c);
} GYS_CATCH_ALL

int gys_tdigest_global_rccl(gys_ctx *c, void *comm, gys_tdigest_slab *d_out)
try {
	GYS_ENTER(c);
	if (!c || !comm || !d_out) return GYS_ERR_INVAL;
	TDIGEST_CHECK();
	int nranks = 1, rank = 0;
	RCCL_API(R);
	NCCLCHK(R->CommCount((ncclComm_t)comm, &nranks));
	NCCLCHK(R->CommUserRank((ncclComm_t)comm, &rank));
	DevBuf<gys_tdigest_slab> all;
	int rc = all.grow((size_t)nranks, c->stream);
	if (rc) return rc;
	gys_tdigest_slab *d_all = all.p;
	rc = gys_tdigest_rollup_dev(c, GYS_ROLLUP_GLOBAL, d_all + rank); // in place: this rank's slab sits at its own position
	if (rc == GYS_OK) {
		const ncclResult_t r = R->AllGather(d_all + rank, d_all, sizeof(gys_tdigest_slab), ncclUint8, (ncclComm_t)comm, c->stream);
		if (r != ncclSuccess) {
			set_err("ncclAllGather failed: %s", R->GetErrorString(r));
			rc = GYS_ERR_HIP;
		}
	}
	if (rc == GYS_OK) rc = gys_tdigest_merge_slabs_dev(c, d_all, (uint32_t)nranks, d_out);
	const hipError_t es = hipStreamSynchronize(c->stream); // d_all is freed at scope exit
	if (rc == GYS_OK) HIPCHK(es);
	return rc;
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ distinct counts (gys_hllroll.hpp)
#define HLL_CHECK()                                                                       \
	if (!c->svc_hll) {                                                                \
		set_err("per-service HyperLogLog is off (gys_config.svc_hll_p = 0)");     \
		return GYS_ERR_STATE;                                                     \
	}
#define HLL_ALIGNED(ptr) (((uintptr_t)(ptr) & 15u) == 0)

static void hll_estimate_launch(gys_ctx *c, const uint8_t *files, uint32_t n, double *d_out)
{
	const uint64_t pieces = (uint64_t)n << (c->cfg.svc_hll_p - 4);
	if (n) hipLaunchKernelGGL(k_hll_estimate, dim3((uint32_t)std::min<uint64_t>((pieces + GYS_HLL_NT - 1) / GYS_HLL_NT, (uint64_t)c->ncu * 16)), dim3(GYS_HLL_NT), 0, c->stream,
				  files, n, (uint32_t)c->cfg.svc_hll_p, d_out);
}
int gys_scan_distinct_dev(gys_ctx *c, double *d_out)
try {
	GYS_ENTER(c);
	if (!c || !d_out) return GYS_ERR_INVAL;
	HLL_CHECK();
	{
		ProfScope ps(c, "hll_scan");
		hll_estimate_launch(c, c->svc_hll, c->nsvc, d_out);
	}
	HIPCHK(hipGetLastError());
	return GYS_OK;
} GYS_CATCH_ALL

int gys_query_distinct(gys_ctx *c, uint64_t glob_id, double *out)
try {
	GYS_ENTER(c);
	if (!c || !out) return GYS_ERR_INVAL;
	HLL_CHECK();
	auto it = c->gid_map_h.find(glob_id);
	if (it == c->gid_map_h.end()) {
		set_err("unknown glob_id %016llx", (unsigned long long)glob_id);
		return GYS_ERR_INVAL;
	}
	{
		const int rcs = c->hl_buf.grow(sizeof(double), c->stream);
		if (rcs) return rcs;
	}
	uint8_t *d_tmp = c->hl_buf.p;
	// the scan's kernel on this one slot: the same code turns the same bytes into the same double
	hll_estimate_launch(c, c->svc_hll + ((size_t)it->second << c->cfg.svc_hll_p), 1u, (double *)d_tmp);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(out, d_tmp, sizeof(double), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
} GYS_CATCH_ALL

uint32_t gys_hll_file_bytes(gys_ctx *c) { return c && c->cfg.svc_hll_p ? 1u << c->cfg.svc_hll_p : 0u; }

int gys_hll_global_rccl(gys_ctx *c, void *comm, uint8_t *d_regs, double *d_est)
try {
	GYS_ENTER(c);
	if (!c || !comm || (!d_regs && !d_est)) return GYS_ERR_INVAL;
	HLL_CHECK();
	int nranks = 1, rank = 0;
	RCCL_API(R);
	NCCLCHK(R->CommCount((ncclComm_t)comm, &nranks));
	NCCLCHK(R->CommUserRank((ncclComm_t)comm, &rank));
	const size_t m = (size_t)1 << c->cfg.svc_hll_p;
	DevBuf<uint8_t> all;
	int rc = all.grow(m * (size_t)nranks, c->stream);
	if (rc) return rc;
	uint8_t *d_all = all.p;
	rc = gys_hll_rollup_dev(c, GYS_ROLLUP_GLOBAL, d_all + m * (size_t)rank, nullptr); // in place: this rank's file sits at its own position
	if (rc == GYS_OK) {
		const ncclResult_t r = R->AllGather(d_all + m * (size_t)rank, d_all, m, ncclUint8, (ncclComm_t)comm, c->stream);
		if (r != ncclSuccess) {
			set_err("ncclAllGather failed: %s", R->GetErrorString(r));
			rc = GYS_ERR_HIP;
		}
	}
	if (rc == GYS_OK) rc = gys_hll_merge_files_dev(c, d_all, (uint32_t)nranks, d_regs, d_est);
	const hipError_t es = hipStreamSynchronize(c->stream); // d_all is freed at scope exit
	if (rc == GYS_OK) HIPCHK(es);
	return rc;
} GYS_CATCH_ALL

// ---- the levels of the closed windows (gys_config.svc_hll_levels; definition in include/gysketch.h)
#define HLL_LEVEL_CHECK(level)                                                                   \
	if ((level) < 0 || (level) >= GYS_NLEVELS) {                                             \
		set_err("level %d outside 0 .. %d", (int)(level), GYS_NLEVELS - 1);              \
		return GYS_ERR_INVAL;                                                            \
	}                                                                                        \
	if (!c->hl_lvl) {                                                                        \
		set_err("distinct-count levels are off (gys_config.svc_hll_levels = 0)");        \
		return GYS_ERR_STATE;                                                            \
	}

// the level's files of slots [first, first + n) at time tusec into d_files and / or their estimates into d_est (k_hll_level_view)
static int hll_level_view(gys_ctx *c, int level, uint64_t tusec, uint32_t first, uint32_t n, uint8_t *d_files, double *d_est)
{
	if (!n) return GYS_OK;
	const int64_t tl = c->hl_t_last, tq = std::max((int64_t)(tusec / 1000000ull), tl);
	const uint32_t p = c->cfg.svc_hll_p;
	HllLevelViewP q{};
	uint32_t farr = GYS_HLL_LVL_LAST;
	if (level == 0) {
		q.mask = tl >= 0 && tq - tl < LEVEL_SECS[0] ? 1u : 0u; // the window closed last, until a window's length has passed without another close
	} else if (level == GYS_NLEVELS - 1) {
		farr = GYS_HLL_LVL_ALL;
		q.mask = 1u;
	} else {
		farr = GYS_HLL_LVL_RING + (uint32_t)(level - 1) * GYS_LEVEL_RING;
		for (uint32_t j = 0; j < GYS_LEVEL_RING; ++j) // a bucket whose start has been crossed since the last close has expired (it is cleared at the next close)
			if (tl >= 0 && !(level_bucket_start(tq, LEVEL_SECS[level], j) > tl)) q.mask |= 1u << j;
	}
	q.base = hll_level_array(c, farr);
	q.stride = (uint64_t)c->cfg.max_services << p;
	q.first = first;
	q.n = n;
	q.p = p;
	q.files = d_files;
	q.est = d_est;
	const uint64_t pieces = (uint64_t)n << (p - 4u);
	hipLaunchKernelGGL(k_hll_level_view, dim3((uint32_t)std::min<uint64_t>((pieces + GYS_HLL_NT - 1) / GYS_HLL_NT, (uint64_t)c->ncu * 16)), dim3(GYS_HLL_NT), 0, c->stream, q);
	HIPCHK(hipGetLastError());
	return GYS_OK;
}

int gys_scan_distinct_level_dev(gys_ctx *c, int level, uint64_t tusec, double *d_out)
try {
	GYS_ENTER(c);
	if (!c || !d_out) return GYS_ERR_INVAL;
	HLL_LEVEL_CHECK(level);
	ProfScope ps(c, "hll_level_scan");
	return hll_level_view(c, level, tusec, 0u, c->nsvc, nullptr, d_out);
} GYS_CATCH_ALL

int gys_query_distinct_level(gys_ctx *c, uint64_t glob_id, int level, uint64_t tusec, double *out)
try {
	GYS_ENTER(c);
	if (!c || !out) return GYS_ERR_INVAL;
	HLL_LEVEL_CHECK(level);
	auto it = c->gid_map_h.find(glob_id);
	if (it == c->gid_map_h.end()) {
		set_err("unknown glob_id %016llx", (unsigned long long)glob_id);
		return GYS_ERR_INVAL;
	}
	int rc = c->hl_buf.grow(sizeof(double), c->stream);
	if (rc) return rc;
	uint8_t *d_tmp = c->hl_buf.p;
	rc = hll_level_view(c, level, tusec, it->second, 1u, nullptr, (double *)d_tmp); // the scan's kernel on this one slot
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(out, d_tmp, sizeof(double), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
} GYS_CATCH_ALL

uint32_t gys_num_services(gys_ctx *c) { return c ? c->nsvc : 0; }
uint32_t gys_num_hosts(gys_ctx *c) { return c ? (uint32_t)c->hosts.size() : 0; }

#define RANGE_CHECK(first, n)                                       \
	if (!c || !out || (uint64_t)(first) + (n) > c->nsvc) {      \
		set_err("bad slot range");                          \
		return GYS_ERR_INVAL;                               \
	}

int gys_export_hist(gys_ctx *c, int which, uint32_t first_slot, uint32_t nslots, gys_hist_rec *out)
try {
	GYS_ENTER(c);
	RANGE_CHECK(first_slot, nslots);
	if (which < 0 || which > 1) return GYS_ERR_INVAL;
	if (!nslots) return GYS_OK;
	{
		const int rcf = fold_range(c, first_slot, nslots);
		if (rcf) return rcf;
	}
	DevBuf<gys_hist_rec> tmp; // window / all-time VIEW of the records (hist_view in gys_kernels.hpp)
	{
		const int rct = tmp.alloc(nslots, false);
		if (rct) return rct;
	}
	hipLaunchKernelGGL(k_hist_view, dim3((nslots + 255) / 256), dim3(256), 0, c->stream, window_records(c), c->hist_all,
			   c->cfg.enable_tdigest ? c->td_meta : nullptr, c->epoch, which, first_slot, nslots, tmp);
	HIPCHK(hipMemcpyAsync(out, tmp, (size_t)nslots * sizeof(gys_hist_rec), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
} GYS_CATCH_ALL

int gys_export_conn_bitmap(gys_ctx *c, uint32_t first_slot, uint32_t nslots, uint16_t *out)
try {
	GYS_ENTER(c);
	RANGE_CHECK(first_slot, nslots);
	{
		const int rcf = fold_range(c, first_slot, nslots);
		if (rcf) return rcf;
	}
	HIPCHK(hipMemcpyAsync(out, c->bitmap + (size_t)first_slot * GYS_BM_WORDS, (size_t)nslots * GYS_BM_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
	std::vector<TdMeta> meta;
	if (c->cfg.enable_tdigest) { // rows of a key that has not been touched in the current window are logically cleared
		meta.resize(nslots);
		HIPCHK(hipMemcpyAsync(meta.data(), c->td_meta + first_slot, (size_t)nslots * sizeof(TdMeta), hipMemcpyDeviceToHost, c->stream));
	}
	HIPCHK(hipStreamSynchronize(c->stream));
	for (size_t i = 0; i < meta.size(); ++i)
		if (meta[i].hw_epoch != c->epoch) memset(out + i * 2 * GYS_BM_WORDS, 0, GYS_BM_WORDS * 4);
	return GYS_OK;
} GYS_CATCH_ALL

int gys_export_hll(gys_ctx *c, uint8_t *out)
try {
	GYS_ENTER(c);
	if (!c || !out) return GYS_ERR_INVAL;
	HIPCHK(hipMemcpyAsync(out, c->last + c->al.off_hll8, (size_t)1 << GYS_HLL_P, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
} GYS_CATCH_ALL

int gys_export_cms(gys_ctx *c, int which, void *out)
try {
	GYS_ENTER(c);
	if (!c || !out || which < 0 || which > 1) return GYS_ERR_INVAL;
	const size_t n = (size_t)GYS_CMS_D * GYS_CMS_W;
	if (which == 0)
		HIPCHK(hipMemcpyAsync(out, (const uint32_t *)(c->last + c->al.off_u32) + c->al.u32_cms, n * 4, hipMemcpyDeviceToHost, c->stream));
	else
		HIPCHK(hipMemcpyAsync(out, (const int64_t *)(c->last + c->al.off_i64sum) + c->al.i64_cms, n * 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
} GYS_CATCH_ALL

int gys_export_global_hist(gys_ctx *c, gys_hist_rec *out)
try {
	GYS_ENTER(c);
	if (!c || !out) return GYS_ERR_INVAL;
	int64_t v[32];
	int64_t mx;
	HIPCHK(hipMemcpyAsync(v, (const int64_t *)(c->last + c->al.off_i64sum) + c->al.i64_ghist, sizeof(v), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(&mx, c->last + c->al.off_i64max, 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	for (int i = 0; i < 15; ++i) {
		out->stats[i].count = (uint64_t)v[2 * i];
		out->stats[i].sum = v[2 * i + 1];
	}
	out->total_count = (uint64_t)v[30];
	out->max_val_seen = mx;
	return GYS_OK;
} GYS_CATCH_ALL

int gys_export_tdigest(gys_ctx *c, uint32_t first_slot, uint32_t nslots, int64_t *sums, uint32_t *cnts, int32_t *minmax)
try {
	GYS_ENTER(c);
	void *out = sums;
	RANGE_CHECK(first_slot, nslots);
	if (!c->cfg.enable_tdigest || !cnts || !minmax) return GYS_ERR_INVAL;
	{
		const int rcf = fold_range(c, first_slot, nslots); // min / max cover the buffered values
		if (rcf) return rcf;
	}
	HIPCHK(hipMemcpyAsync(sums, c->td_sum + (size_t)first_slot * GYS_TD_NB, (size_t)nslots * GYS_TD_NB * 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(cnts, c->td_cnt + (size_t)first_slot * GYS_TD_NB, (size_t)nslots * GYS_TD_NB * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(minmax, c->td_minmax + first_slot, (size_t)nslots * sizeof(int2), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
} GYS_CATCH_ALL

uint32_t gys_td_pend_cap(gys_ctx *c) { return c ? c->pend_cap : 0u; }

int gys_export_tdigest_pending(gys_ctx *c, uint32_t first_slot, uint32_t nslots, uint32_t *npend, int32_t *pend)
try {
	GYS_ENTER(c);
	void *out = npend;
	RANGE_CHECK(first_slot, nslots);
	if (!c->cfg.enable_tdigest || !pend) return GYS_ERR_INVAL;
	std::vector<TdMeta> meta(nslots);
	HIPCHK(hipMemcpyAsync(meta.data(), c->td_meta + first_slot, (size_t)nslots * sizeof(TdMeta), hipMemcpyDeviceToHost, c->stream));
	// a service buffers at most td_pend_cap values between batches (the rest of its pcap-entry buffer is room for a batch)
	const size_t cap = c->pend_cap;
	HIPCHK(hipMemcpy2DAsync(pend, cap * 4, c->td_pend + (size_t)first_slot * c->pcap, (size_t)c->pcap * 4, cap * 4, nslots, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	for (uint32_t i = 0; i < nslots; ++i) {
		npend[i] = meta[i].npend;
		for (uint32_t k = 0; k < cap; ++k) // staged words: value << 6 | family << 5 | CONN_BITMAP row
			pend[(size_t)i * cap + k] = k < meta[i].npend ? (int32_t)((uint32_t)pend[(size_t)i * cap + k] >> GYS_ROW_BITS) : 0;
	}
	return GYS_OK;
} GYS_CATCH_ALL

int gys_export_svc_counters(gys_ctx *c, uint32_t first_slot, uint32_t nslots, uint64_t *out)
try {
	GYS_ENTER(c);
	RANGE_CHECK(first_slot, nslots);
	{
		// mid-window: the cumulative counters must include the window so far (its Count-Min share moves into the arena a little early,
		// which nothing can observe before the window closes)
		const int rcf = conn_fold(c);
		if (rcf) return rcf;
	}
	HIPCHK(hipMemcpyAsync(out, c->svc_ctr + (size_t)first_slot * 4, (size_t)nslots * 32, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
} GYS_CATCH_ALL

int gys_export_svc_hll(gys_ctx *c, uint32_t first_slot, uint32_t nslots, uint8_t *out)
try {
	GYS_ENTER(c);
	RANGE_CHECK(first_slot, nslots);
	if (!c->svc_hll) return GYS_ERR_STATE;
	HIPCHK(hipMemcpyAsync(out, c->svc_hll + ((size_t)first_slot << c->cfg.svc_hll_p), (size_t)nslots << c->cfg.svc_hll_p, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
} GYS_CATCH_ALL

int gys_export_svc_hll_level(gys_ctx *c, int level, uint64_t tusec, uint32_t first_slot, uint32_t nslots, uint8_t *out)
try {
	GYS_ENTER(c);
	RANGE_CHECK(first_slot, nslots);
	HLL_LEVEL_CHECK(level);
	if (!nslots) return GYS_OK;
	DevBuf<uint8_t> tmp;
	int rc = tmp.grow((size_t)nslots << c->cfg.svc_hll_p, c->stream);
	if (rc == GYS_OK) rc = hll_level_view(c, level, tusec, first_slot, nslots, tmp.p, nullptr);
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(out, tmp.p, (size_t)nslots << c->cfg.svc_hll_p, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream)); // (tmp goes at scope exit)
	return GYS_OK;
} GYS_CATCH_ALL

int gys_get_counters(gys_ctx *c, gys_counters *out)
try {
	GYS_ENTER(c);
	if (!c || !out) return GYS_ERR_INVAL;
	uint64_t v[32];
	static_assert(CTR_NUM <= 31, "counter block (the last word is the sink of k_read_events)");
	HIPCHK(hipMemcpyAsync(v, c->counters, sizeof(v), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
#ifdef GYS_RESP_TIMING
	{
		unsigned long long t[16];
		HIPCHK(hipMemcpyFromSymbol(t, HIP_SYMBOL(gys::g_resp_timing), sizeof(t)));
		unsigned long long tot = 0;
		for (int i = 0; i < 12; ++i) tot += t[i];
		static const char *nm[12] = {"loads", "probe2", "probe3+", "kept/atomics", "ghist+hash", "hllq/store", "barrier1", "scan1+b", "scan2+b", "image+b", "prologue", "flush"};
		fprintf(stderr, "GYS_RESP_TIMING waves %llu ticks %llu:", t[15], tot);
		for (int i = 0; i < 12; ++i) fprintf(stderr, " %s %.1f%%", nm[i], tot ? 100.0 * (double)t[i] / (double)tot : 0.0);
		fprintf(stderr, "\n");
	}
#endif
#ifdef GYS_HUGE_TIMING
	fprintf(stderr, "GYS_HUGE_TIMING ticks: load %llu words+tail %llu scan %llu assign %llu writeback %llu | entries %llu npend %llu nc %llu\n", (unsigned long long)v[20], (unsigned long long)v[21], (unsigned long long)v[22], (unsigned long long)v[23], (unsigned long long)v[24], (unsigned long long)v[25], (unsigned long long)v[26], (unsigned long long)v[27]);
#endif
	out->resp_events = v[CTR_RESP_EVENTS];
	out->resp_dropped_range = v[CTR_RESP_DROP_RANGE];
	out->resp_dropped_nolistener = v[CTR_RESP_DROP_NOLISTENER];
	out->conn_events = v[CTR_CONN_EVENTS];
	out->conn_unknown_service = v[CTR_CONN_UNKNOWN];
	out->conn_new = v[CTR_CONN_NEW];
	out->conn_closed = v[CTR_CONN_CLOSED];
	out->conn_closed_no_notify = v[CTR_CONN_CLOSED_NO_NOTIFY];
	out->conn_client_side = v[CTR_CONN_CLI_SIDE];
	out->resp_run_overflow = v[CTR_RESP_RUN_OVERFLOW];
	out->lstate_records = v[CTR_LSTATE_RECORDS];
	out->lstate_missed = v[CTR_LSTATE_MISSED];
	out->lstate_errors = v[CTR_LSTATE_ERRORS];
	out->lstate_deleted = v[CTR_LSTATE_DELETED];
	out->resp_batches_host_local = c->n_batches_host_local;
	out->resp_batches_general = c->n_batches_general;
	out->window_graph_launches = c->win_graph_launches;
	out->resp_batches_host_split = c->n_batches_host_split;
	out->td_merges = v[CTR_TD_MERGES];
	out->td_merge_values = v[CTR_TD_MERGE_VALUES];
	out->actconn_records = v[CTR_ACTCONN_RECORDS];
	out->actconn_remote_listen = v[CTR_ACTCONN_REMOTE_LISTEN];
	out->actconn_unknown_listener = v[CTR_ACTCONN_UNKNOWN];
	out->stage_waits = c->ring.waits.load();
	auto snap = [](SubQ &q, uint64_t *calls, uint64_t *submissions) {
		std::lock_guard<std::mutex> g(q.mu);
		*calls = q.calls;
		*submissions = q.submissions;
		return q.tail_flushes;
	};
	out->resp_tail_flushes = snap(c->sq[SubQ::RESP], &out->resp_calls_queued, &out->resp_submissions);
	out->rec_tail_flushes = snap(c->sq[SubQ::CONN], &out->conn_calls_queued, &out->conn_submissions);
	out->rec_tail_flushes += snap(c->sq[SubQ::LSTATE], &out->lstate_calls_queued, &out->lstate_submissions);
	return GYS_OK;
} GYS_CATCH_ALL

int gys_resp_queue_pending(gys_ctx *c, uint64_t *events)
try {
	if (!c || !events) return GYS_ERR_INVAL;
	SubQ &q = c->sq[SubQ::RESP];
	std::lock_guard<std::mutex> g(q.mu);
	uint64_t n = 0;
	if (q.open >= 0) n += q.b[q.open].fill;
	for (int bi : q.sealed) n += q.b[bi].fill;
	*events = n;
	return GYS_OK;
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ multi-level windows
#define LEVELS_CHECK()                                                        \
	if (!c->cfg.enable_levels) {                                          \
		set_err("gys_config.enable_levels was not set");              \
		return GYS_ERR_STATE;                                         \
	}
#define LEVEL0_CHECK(level)                                                                   \
	if ((level) == 0 && c->cfg.enable_levels != 1) {                                       \
		set_err("the 5-s level is not kept with gys_config.enable_levels = 2");        \
		return GYS_ERR_STATE;                                                          \
	}

int gys_export_hist_level(gys_ctx *c, int level, uint64_t tusec, uint32_t first_slot, uint32_t nslots, gys_hist_rec *out)
try {
	GYS_ENTER(c);
	RANGE_CHECK(first_slot, nslots);
	LEVELS_CHECK();
	if (level < 0 || level >= GYS_NLEVELS) return GYS_ERR_INVAL;
	LEVEL0_CHECK(level);
	if (!nslots) return GYS_OK;
	DevBuf<gys_hist_rec> tmp;
	int rc = tmp.grow(nslots, c->stream);
	if (rc == GYS_OK) rc = level_view(c, level, tusec, first_slot, nslots, tmp.p);
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(out, tmp.p, (size_t)nslots * sizeof(gys_hist_rec), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream)); // (tmp goes at scope exit)
	return GYS_OK;
} GYS_CATCH_ALL

int gys_query_hist_level_stats(gys_ctx *c, uint64_t glob_id, int level, uint64_t tusec, gys_time_hist_val *pstats, uint32_t nstats, int64_t *tcount,
			       int64_t *tsum, double *mean_val)
try {
	GYS_ENTER(c);
	if (!c || (!pstats && nstats)) return GYS_ERR_INVAL;
	uint32_t slot;
	int rc = gys_lookup_service(c, glob_id, &slot);
	if (rc) return rc;
	gys_hist_rec h;
	rc = gys_export_hist_level(c, level, tusec, slot, 1, &h);
	if (rc) return rc;
	const HashDef &d = hash_def(GYS_RESP_TIME_HASH);
	int64_t tc = 0, ts = 0;
	for (int b = 0; b < d.nthr + 2; ++b) { // slabhist.count(level) / sum(level), common/gy_statistics.h:1358-1359
		tc += (int64_t)h.stats[b].count;
		ts += h.stats[b].sum;
	}
	for (uint32_t i = 0; i < nstats; ++i) pstats[i].data_value = level_percentile(d, h, pstats[i].percentile);
	if (tcount) *tcount = tc;
	if (tsum) *tsum = ts;
	if (mean_val) *mean_val = (double)ts / (double)(tc != 0 ? tc : 1); // :1361
	return GYS_OK;
} GYS_CATCH_ALL

int gys_export_hist_period(gys_ctx *c, int64_t starttime, int64_t endtime, uint64_t tusec, uint32_t first_slot, uint32_t nslots, gys_hist_rec *out,
			   int *level_used)
try {
	GYS_ENTER(c);
	RANGE_CHECK(first_slot, nslots);
	LEVELS_CHECK();
	if (!nslots) return GYS_OK;
	DevBuf<gys_hist_rec> tmp;
	int rc = tmp.grow(nslots, c->stream);
	if (rc == GYS_OK) rc = level_period(c, starttime, endtime + 1, tusec, first_slot, nslots, tmp.p, level_used);
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(out, tmp.p, (size_t)nslots * sizeof(gys_hist_rec), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream)); // (tmp goes at scope exit)
	return GYS_OK;
} GYS_CATCH_ALL

int gys_query_hist_period_stats(gys_ctx *c, uint64_t glob_id, int64_t starttime, int64_t endtime, uint64_t tusec, gys_time_hist_val *pstats,
				uint32_t nstats, int64_t *tcount, int64_t *tsum, double *mean_val)
try {
	GYS_ENTER(c);
	if (!c || (!pstats && nstats)) return GYS_ERR_INVAL;
	uint32_t slot;
	int rc = gys_lookup_service(c, glob_id, &slot);
	if (rc) return rc;
	gys_hist_rec h;
	rc = gys_export_hist_period(c, starttime, endtime, tusec, slot, 1, &h, nullptr);
	if (rc) return rc;
	const HashDef &d = hash_def(GYS_RESP_TIME_HASH);
	int64_t tc = 0, ts = 0;
	for (int b = 0; b < d.nthr + 2; ++b) { // slabhist.count(start, end) / sum(start, end), common/gy_statistics.h:1395-1396
		tc += (int64_t)h.stats[b].count;
		ts += h.stats[b].sum;
	}
	for (uint32_t i = 0; i < nstats; ++i) pstats[i].data_value = level_percentile(d, h, pstats[i].percentile); // :1389-1393
	if (tcount) *tcount = tc;
	if (tsum) *tsum = ts;
	if (mean_val) *mean_val = (double)ts / (double)(tc != 0 ? tc : 1); // :1398
	return GYS_OK;
} GYS_CATCH_ALL

int gys_export_day_stats(gys_ctx *c, uint64_t tusec, uint32_t first_slot, uint32_t nslots, gys_listener_day_stats *out)
try {
	GYS_ENTER(c);
	RANGE_CHECK(first_slot, nslots);
	LEVELS_CHECK();
	if (!nslots) return GYS_OK;
	DevBuf<gys_hist_rec> lv;
	DevBuf<gys_listener_day_stats> d_out;
	int rc = lv.alloc(nslots, false);
	if (!rc) rc = d_out.alloc(nslots, false);
	if (!rc) rc = level_view(c, 2, tusec, first_slot, nslots, lv);
	if (rc) return rc;
	ProfScope ps(c, "day_stats");
	hipLaunchKernelGGL(k_day_stats, dim3((nslots + 255) / 256), dim3(256), 0, c->stream, lv, c->qps_hist, c->act_hist, c->svc_gid, first_slot, nslots,
			   d_out);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(out, d_out, (size_t)nslots * sizeof(gys_listener_day_stats), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
} GYS_CATCH_ALL

int gys_scan_listener_state_dev(gys_ctx *c, uint64_t tusec, float qps_multiple, uint32_t diffsec, void *d_notify, gys_listener_scan *d_scan)
try {
	GYS_ENTER(c);
	if (!c) return GYS_ERR_INVAL;
	LEVELS_CHECK();
	LEVEL0_CHECK(0);
	if (!c->nsvc || (!d_notify && !d_scan)) return GYS_OK;
	int64_t tq = (int64_t)(tusec / 1000000ull);
	if (tq < c->lvl_t_last) tq = c->lvl_t_last;
	ListenerScanP p{};
	p.win = c->hist_win;
	p.all = c->hist_all;
	p.meta = c->cfg.enable_tdigest ? c->td_meta : nullptr;
	p.epoch_open = c->epoch + (c->prepared ? 1u : 0u);
	p.epoch_last = p.epoch_open - 1u;
	p.nsvc = c->nsvc;
	for (int lv = 0; lv < GYS_NLEVELS; ++lv) level_source(c, lv, tq, &p.mode[lv], &p.sub[lv]);
	p.last_tag = c->cfg.enable_tdigest ? c->lvl_last_tag : nullptr;
	p.last_epoch = c->lvl_last_epoch;
	p.qps = c->qps_hist;
	p.act = c->act_hist;
	p.bitmap = c->bitmap;
	p.svc_gid = c->svc_gid;
	p.multiple = qps_multiple;
	p.diffsec = (float)diffsec;
	p.notify = (uint8_t *)d_notify;
	p.scan = d_scan;
	ProfScope ps(c, "listener_scan");
	hipLaunchKernelGGL(k_listener_scan, dim3((c->nsvc + 255) / 256), dim3(256), 0, c->stream, p);
	HIPCHK(hipGetLastError());
	return GYS_OK;
} GYS_CATCH_ALL

int gys_decide_listener_state_dev(gys_ctx *c, const gys_listener_scan *d_scan, const gys_listener_issue_in *d_issue_in, void *d_notify,
				  gys_listener_decision *d_out)
try {
	GYS_ENTER(c);
	if (!c || !d_scan) return GYS_ERR_INVAL;
	if (!c->nsvc) return GYS_OK;
	if (!c->svc_bithist.p) { // the listeners' two history bytes: engine state from the first decision on
		const int rc = c->svc_bithist.alloc((size_t)c->cfg.max_services * 2, false);
		if (rc) return rc;
		const hipError_t e = hipMemsetAsync(c->svc_bithist, 0, (size_t)c->cfg.max_services * 2, c->stream);
		if (e != hipSuccess) {
			c->svc_bithist.release(); // (an array that was not cleared must not pass for the history)
			HIPCHK(e);
		}
	}
	ListenerDecideP p{};
	p.scan = d_scan;
	p.in = d_issue_in;
	p.hist = c->svc_bithist;
	p.notify = (uint8_t *)d_notify;
	p.out = d_out;
	p.nsvc = c->nsvc;
	p.msec1_bucket = 1; // get_bucketid_from_threshold<RESP_TIME_HASH>(1): the bucket whose ceiling is 1 ms
	for (uint32_t b = 1; b < 14; ++b)
		if (bucket_max_threshold(hash_def(GYS_RESP_TIME_HASH), b) == 1) p.msec1_bucket = b;
	ProfScope ps(c, "listener_decide");
	hipLaunchKernelGGL(k_listener_decide, dim3((c->nsvc + 255) / 256), dim3(256), 0, c->stream, p);
	HIPCHK(hipGetLastError());
	return GYS_OK;
} GYS_CATCH_ALL

int gys_export_svc_hist(gys_ctx *c, int which, uint32_t first_slot, uint32_t nslots, gys_hist_rec *out)
try {
	GYS_ENTER(c);
	RANGE_CHECK(first_slot, nslots);
	LEVELS_CHECK();
	if (which < 0 || which > 1) return GYS_ERR_INVAL;
	if (!nslots) return GYS_OK;
	const gys_hist_rec *src = (which ? c->act_hist : c->qps_hist) + first_slot;
	HIPCHK(hipMemcpyAsync(out, src, (size_t)nslots * sizeof(gys_hist_rec), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return GYS_OK;
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ standalone keyed histogram op
int gys_hist_init_dev(gys_ctx *c, int kind, gys_hist_rec *d_hist, uint32_t nkeys)
try {
	GYS_ENTER(c);
	if (!c || !d_hist || kind < 0 || kind >= GYS_NUM_HASH_KINDS) return GYS_ERR_INVAL;
	HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)nkeys * sizeof(gys_hist_rec), c->stream));
	const int64_t mn = hash_def(kind).t_bits == 64 ? INT64_MIN : (int64_t)INT32_MIN; // std::numeric_limits<T>::min() (:563)
	hipLaunchKernelGGL(k_hist_init, dim3(grid_for(nkeys, 256, 2048)), dim3(256), 0, c->stream, d_hist, (uint64_t)0, (uint64_t)nkeys, mn);
	HIPCHK(hipGetLastError());
	return GYS_OK;
} GYS_CATCH_ALL

int gys_hist_add_dev(gys_ctx *c, int kind, gys_hist_rec *d_hist, uint32_t nkeys, const uint32_t *d_keyidx, const int32_t *d_vals, uint64_t n)
try {
	GYS_ENTER(c);
	if (!c || !d_hist || kind < 0 || kind >= GYS_NUM_HASH_KINDS || ((!d_keyidx || !d_vals) && n)) return GYS_ERR_INVAL;
	if (!n) return GYS_OK;
	ProfScope ps(c, "hist_add");
	hipLaunchKernelGGL(k_hist_add, dim3(grid_for(n, 256, (uint32_t)c->ncu * 8)), dim3(256), 0, c->stream, kind, d_hist, nkeys, d_keyidx, d_vals, n);
	HIPCHK(hipGetLastError());
	return GYS_OK;
} GYS_CATCH_ALL

int gys_hist_merge_dev(gys_ctx *c, gys_hist_rec *d_dst, const gys_hist_rec *d_src, uint32_t nkeys)
try {
	GYS_ENTER(c);
	if (!c || !d_dst || !d_src) return GYS_ERR_INVAL;
	if (!nkeys) return GYS_OK;
	ProfScope ps(c, "hist_merge");
	hipLaunchKernelGGL(k_hist_fold, dim3(grid_for((uint64_t)nkeys * 16, 256, (uint32_t)c->ncu * 8)), dim3(256), 0, c->stream, d_dst,
			   (gys_hist_rec *)d_src, (uint64_t)nkeys, 0, (long long *)nullptr, (long long *)nullptr);
	HIPCHK(hipGetLastError());
	return GYS_OK;
} GYS_CATCH_ALL

int gys_hist_percentiles_dev(gys_ctx *c, int kind, const gys_hist_rec *d_hist, uint32_t nkeys, const float *pcts, uint32_t npct, int64_t *d_out)
try {
	GYS_ENTER(c);
	if (!c || !d_hist || !pcts || !d_out || !npct || npct > 64 || kind < 0 || kind >= GYS_NUM_HASH_KINDS) return GYS_ERR_INVAL;
	if (!nkeys) return GYS_OK;
	HIPCHK(hipMemcpyAsync(c->dev_pcts, pcts, (size_t)npct * 4, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream)); // pcts may be a short-lived host buffer
	ProfScope ps(c, "hist_percentiles");
	const uint64_t t = (uint64_t)nkeys * npct;
	hipLaunchKernelGGL(k_hist_percentiles, dim3((uint32_t)((t + 255) / 256)), dim3(256), 0, c->stream, kind, d_hist, nkeys, c->dev_pcts, npct, d_out);
	HIPCHK(hipGetLastError());
	return GYS_OK;
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ profiling
int gys_profile_enable(gys_ctx *c, int on)
try {
	GYS_ENTER(c);
	if (!c) return GYS_ERR_INVAL;
	c->profile = on != 0;
	return GYS_OK;
} GYS_CATCH_ALL

int gys_profile_reset(gys_ctx *c)
try {
	GYS_ENTER(c);
	if (!c) return GYS_ERR_INVAL;
	HIPCHK(hipStreamSynchronize(c->stream));
	prof_resolve(c);
	c->prof.clear();
	return GYS_OK;
} GYS_CATCH_ALL

int gys_profile_get(gys_ctx *c, const char *kernel, double *total_ms, uint64_t *launches)
try {
	GYS_ENTER(c);
	if (!c || !kernel) return GYS_ERR_INVAL;
	prof_resolve(c);
	auto it = c->prof.find(kernel);
	if (it == c->prof.end()) {
		if (total_ms) *total_ms = 0;
		if (launches) *launches = 0;
		return GYS_ERR_NOTFOUND;
	}
	if (total_ms) *total_ms = it->second.total_ms;
	if (launches) *launches = it->second.launches;
	return GYS_OK;
} GYS_CATCH_ALL

int gys_profile_names(gys_ctx *c, char *buf, size_t buflen)
try {
	GYS_ENTER(c);
	if (!c || !buf || !buflen) return GYS_ERR_INVAL;
	std::string s;
	for (auto &kv : c->prof) {
		if (!s.empty()) s += ",";
		s += kv.first;
	}
	snprintf(buf, buflen, "%s", s.c_str());
	return GYS_OK;
} GYS_CATCH_ALL

// ------------------------------------------------------------------------------------------------ synthetic generator
int gys_debug_read_events_dev(gys_ctx *c, const void *d_ev24, uint64_t nevents)
try {
	GYS_ENTER(c);
	if (!c || !d_ev24) return GYS_ERR_INVAL;
	if (!nevents) return GYS_OK;
	const uint64_t per_wg = 53248; // ~ a C3 host segment (13 tiles of 4096)
	hipLaunchKernelGGL(k_read_events, dim3((uint32_t)((nevents + per_wg - 1) / per_wg)), dim3(1024), 0, c->stream, (const uint64_t *)d_ev24, nevents, per_wg,
			   (uint64_t *)c->counters + 31);
	HIPCHK(hipGetLastError());
	return GYS_OK;
} GYS_CATCH_ALL

// the large-key path's list lengths as the last response batch left them (tests: which route did the entries take)
int gys_debug_huge_counts(gys_ctx *c, uint32_t out[8])
try {
	GYS_ENTER(c);
	if (!c || !out) return GYS_ERR_INVAL;
	memset(out, 0, 8 * sizeof(uint32_t));
	if (!c->merge_count.p) return GYS_OK; // (no t-digests: no merge lists)
	uint32_t w[FIN_NWORDS];
	HIPCHK(hipMemcpyAsync(w, c->merge_count, sizeof(w), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	out[0] = w[FIN_HUGE];
	out[1] = w[FIN_HUGE_FB];
	out[2] = w[FIN_HUGE_NENT];
	out[3] = w[FIN_HUGE_TAIL];
	out[4] = w[FIN_HUGE_TB];
	return GYS_OK;
} GYS_CATCH_ALL

int gys_gen_resp_events_dev(gys_ctx *c, void *d_ev24, uint64_t nevents, uint64_t seed, uint32_t first_host, uint32_t nhosts, uint32_t svcs_per_host,
			    uint32_t zipf_milli, gys_resp_seg *segs_out)
try {
	GYS_ENTER(c);
	if (!c || !d_ev24 || !nhosts || !svcs_per_host || !segs_out) return GYS_ERR_INVAL;
	const bool spread = zipf_milli == GYS_GEN_SPREAD; // per-service weights 0..255/256 instead of a Zipf law
	if (spread) zipf_milli = 0;
	if (zipf_milli && (c->zipf_n != svcs_per_host || c->zipf_milli != zipf_milli)) {
		std::vector<float> cdf(svcs_per_host);
		const double s = zipf_milli / 1000.0;
		double tot = 0;
		for (uint32_t k = 0; k < svcs_per_host; ++k) tot += 1.0 / std::pow((double)(k + 1), s);
		double run = 0;
		for (uint32_t k = 0; k < svcs_per_host; ++k) {
			run += 1.0 / std::pow((double)(k + 1), s) / tot;
			cdf[k] = (float)run;
		}
		cdf[svcs_per_host - 1] = 1.0f;
		c->zipf_n = 0; // (no table until the new one has landed)
		if (c->zipf_cdf.p) HIPCHK(hipStreamSynchronize(c->stream)); // a generator launch in flight reads the old table
		const int rc = c->zipf_cdf.grow(svcs_per_host, c->stream);
		if (rc) return rc;
		HIPCHK(hipMemcpy(c->zipf_cdf, cdf.data(), (size_t)svcs_per_host * 4, hipMemcpyHostToDevice));
		c->zipf_n = svcs_per_host;
		c->zipf_milli = zipf_milli;
	}
	GenP g{};
	g.ev = (uint64_t *)d_ev24;
	g.n = nevents;
	g.seed = seed;
	g.first_host = first_host;
	g.nhosts = nhosts;
	g.svcs_per_host = svcs_per_host;
	g.zipf_cdf = zipf_milli ? c->zipf_cdf : nullptr;
	g.spread = spread ? 1u : 0u;
	g.per_host = std::max<uint64_t>(1, nevents / nhosts);
	for (uint32_t h = 0; h < nhosts; ++h) {
		segs_out[h].host_slot = first_host + h;
		segs_out[h].reserved = 0;
		segs_out[h].first_event = std::min<uint64_t>((uint64_t)h * g.per_host, nevents);
	}
	if (nevents) hipLaunchKernelGGL(k_gen_resp, dim3(grid_for(nevents, 256, 4096)), dim3(256), 0, c->stream, g);
	HIPCHK(hipGetLastError());
	return GYS_OK;
} GYS_CATCH_ALL

} // extern "C"

#include "gys_actpairs_host.hpp"
#include "gys_svcdeps_engine.hpp"
#include "gys_svccomp_engine.hpp"
#include "gys_groupflow_engine.hpp"
#include "gys_svcresol_engine.hpp"
#include "gys_json.hpp"
#include "gys_regex.hpp"
#include "gys_svcquery_host.hpp"
#include "gys_rollup_host.hpp"
#include "gys_rollsel_host.hpp"
#include "gys_topk_host.hpp"
