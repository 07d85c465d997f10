// gys_mconn_shim.hpp -- C++17 host-side mirror of the reference's aggregation entry points on top of the C ABI.
//
// The reference has no plugin layer: the path under replacement is a handful of MCONN_HANDLER / SHCONN_HANDLER member functions
// invoked from the L2 dispatch switch (server/gy_mconnhdlr.cc:4756-4792).  This header gives a class with THOSE names, argument
// order and error behaviour (bool return, never throws across the boundary) so that the bodies of the reference functions can be
// replaced by one-line forwards (INTEGRATION.md shows the exact diff).  The reference types it cannot include here (comm::*,
// PARTHA_INFO) appear as opaque byte pointers with the same memory layout contract:
//
//   reference signature (server/gy_mconnhdlr.h)                                              -> shim
//   bool partha_tcp_conn_info(const std::shared_ptr<PARTHA_INFO>&, comm::TCP_CONN_NOTIFY*,      partha_tcp_conn_info(machine_id, pone, nconns, pendptr)
//                             int nconns, uint8_t *pendptr, POOL_ALLOC_ARRAY*)            :2091
//   bool partha_listener_state(const std::shared_ptr<PARTHA_INFO>&, const comm::LISTENER_STATE_NOTIFY*,  partha_listener_state(machine_id, pone, nconns, pendptr)
//                             int nconns, uint8_t *pendptr, POOL_ALLOC_ARRAY*, PGConnPool&, bool) :2129
//   void send_cluster_state() noexcept                                                    :2155  send_cluster_state_rccl(tusec) (RCCL inside the library) / send_cluster_state(tusec, reduce_cb)
//   TCP_SOCK_HANDLER::handle_ipv4_resp_event(tcp_ipv4_resp_event_t*, bool) (gy_socket_stat.cc:1517)  handle_ipv4_resp_events(machine_id, pevents, n)
//   TCP_SOCK_HANDLER::handle_ipv6_resp_event(tcp_ipv6_resp_event_t*, bool) (gy_socket_stat.cc:1535)  handle_ipv6_resp_events(machine_id, pevents, n)
//   web_curr_listener_summ (server/gy_mnodehandle.cc:1628)                                       get_listener_summ(machine_id, out)
//   bool handle_partha_active_conns(const std::shared_ptr<PARTHA_INFO>&, const comm::ACTIVE_CONN_STATS*,  handle_partha_active_conns(machine_id, pconn, nitems, pendptr)
//                             int nitems, uint8_t *pendptr, PGConnPool&)                 :2039 (.cc:7705, dispatch :5244)
//   bool web_curr_top_listeners(...) (server/gy_mnodehandle.cc:2706)                             web_curr_top_listeners(machine_id | nullptr, flags, madid, timestr, out)
//   TCP_SOCK_HANDLER::listener_stats_update(servshr, cpu_issue, mem_issue) (common/gy_socket_stat.cc:3895) listener_stats_update(tnow, qps_multiple, diffsec, d_notify, d_scan)
//
//   the re-seeding of a listener's statistics after a restart (handle_listener_req, gy_mconnhdlr.cc:14257)   save_all(path) / load_all(path); a partha that changes ranks: save_partha_services(machine_id, blob) / restore_services(blob, n)
//
// PARTHA_INFO is identified by its GY_MACHINE_ID (PARTHA_INFO::machine_id_, the key of partha_tbl_).
#pragma once

#include <cstdint>
#include <cstdio>
#include <ctime>
#include <functional>
#include <mutex>
#include <shared_mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/gysketch.h"

namespace gyeeta_amd {

class GYS_MCONN_HANDLER {
public:
	// cb: performs the cross-GPU reduce of every gys_reduce_section (RCCL ncclAllReduce with ncclMax / ncclSum on the section's
	// dev_ptr); empty for a single GPU.  It is the analogue of NOTIFY_MS_CLUSTER_STATE -> SHCONN_HANDLER::aggregate_cluster_state.
	using ReduceFn = std::function<bool(const gys_reduce_section *secs, uint32_t nsecs)>;

	explicit GYS_MCONN_HANDLER(const gys_config &cfg)
	{
		if (gys_create(&cfg, &ctx_) != GYS_OK) throw std::runtime_error(std::string("gys_create: ") + gys_last_error());
	}
	~GYS_MCONN_HANDLER()
	{
		if (comm_) {
			gys_sync(ctx_);
			gys_rccl_comm_destroy(comm_);
		}
		gys_destroy(ctx_);
	}
	GYS_MCONN_HANDLER(const GYS_MCONN_HANDLER &) = delete;
	GYS_MCONN_HANDLER &operator=(const GYS_MCONN_HANDLER &) = delete;

	gys_ctx *ctx() noexcept { return ctx_; }

	// partha registration (PM_CONNECT) and NOTIFY_NEW_LISTENER: the two control-plane facts the data path needs
	bool partha_register(const uint8_t machine_id[16], const char *cluster_name) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_register_host(ctx_, machine_id, cluster_name, nullptr) == GYS_OK;
	}
	bool partha_new_listeners(const uint8_t machine_id[16], const gys_listener_info *arr, uint32_t n) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_register_listeners(ctx_, machine_id, arr, n, nullptr) == GYS_OK;
	}

	// NOTIFY_NEW_LISTENER for a long-running process: new listeners take the slots deleted ones gave back before the tail
	bool partha_new_listeners_reuse(const uint8_t machine_id[16], const gys_listener_info *arr, uint32_t n, uint32_t *slots = nullptr) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_register_listeners_slots(ctx_, machine_id, arr, n, slots) == GYS_OK;
	}
	// NEW_LISTENER::ser_aggr_task_id_ (common/gy_comm_proto.h:1538; kept per listener by handle_listener_req, gy_mconnhdlr.cc:13912-13966): the
	// process group each listener runs in, 0 = none -- what the service dependency graph joins the active-connection rows' client ids to
	bool set_listener_tasks(const uint64_t *glob_ids, const uint64_t *ser_aggr_task_ids, uint32_t n) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_set_listener_tasks(ctx_, glob_ids, ser_aggr_task_ids, n) == GYS_OK;
	}
	// the service flow map's edges ("u calls v"; sel NULL = all), ordered by (src_slot, dst_slot, kind): a count, then the rows
	bool svc_edges(const gys_svc_edge_sel *sel, std::vector<gys_svc_edge> &out) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		try {
			uint32_t nout = 0, nmatch = 0;
			if (gys_svc_edges_dev(ctx_, sel, nullptr, 0, &nmatch) != GYS_OK) return false;
			out.resize(nmatch);
			if (gys_svc_edges(ctx_, sel, out.data(), nmatch, &nout, &nmatch) != GYS_OK) return false;
			out.resize(nout);
			return true;
		} catch (...) {
			return false;
		}
	}
	// what lies within max_hops (0 = any number) calls of the services `roots` in direction dir (GYS_DEP_CALLEES / _CALLERS / _BOTH): ids and
	// distances ordered by (hops, slot).  The ids go into gys_svc_filter.svcids for the roll-ups of "everything downstream of X".
	bool svc_deps(const uint64_t *roots, uint32_t nroots, uint32_t dir, uint32_t max_hops, std::vector<uint64_t> &glob_ids, std::vector<uint32_t> &hops) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		try {
			const uint32_t cap = gys_num_services(ctx_);
			uint32_t nout = 0, nreached = 0;
			glob_ids.resize(cap);
			hops.resize(cap);
			if (gys_svc_deps(ctx_, roots, nroots, dir, max_hops, glob_ids.data(), hops.data(), cap, &nout, &nreached) != GYS_OK) return false;
			glob_ids.resize(nout);
			hops.resize(nout);
			return true;
		} catch (...) {
			return false;
		}
	}
	bool svcgraph_stats(gys_svcgraph_stats_t *out) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_svcgraph_stats(ctx_, out) == GYS_OK;
	}
	// a LISTEN_FLAG_DELETE record's effect in the reference (gy_mconnhdlr.cc:11195-11248): the listeners leave the engine, their slots become free
	bool delete_listeners(const uint64_t *glob_ids, uint32_t n, uint32_t *ndeleted = nullptr) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_delete_listeners(ctx_, glob_ids, n, ndeleted) == GYS_OK;
	}
	// MCONN_HANDLER::cleanup_partha_unused_listeners (gy_mconnhdlr.cc:16284-16343) for every partha at once: the listeners whose state a
	// delete record marked and those that have not reported for max_age_windows windows (360 x 5 s = the reference's 30 minutes) are listed
	// by one device pass (at most 65536 per round) and deleted 512 at a time: gys_delete_listeners' table erase is one lane walking the
	// batch, sized for the hundreds of ids of a delete message.  Returns the number deleted, or -1 on an error.
	int64_t cleanup_unused_listeners(uint32_t max_age_windows = 360) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		int64_t total = 0;
		try {
			std::vector<uint64_t> ids(65536);
			for (;;) {
				uint32_t nfound = 0, nd = 0;
				if (gys_list_stale_listeners(ctx_, GYS_STALE_DELETED | GYS_STALE_AGED, max_age_windows, ids.data(), (uint32_t)ids.size(), &nfound) != GYS_OK) return -1;
				const uint32_t nw = nfound < ids.size() ? nfound : (uint32_t)ids.size();
				if (!nw) break;
				for (uint32_t at = 0; at < nw; at += 512u) {
					uint32_t part = 0;
					if (gys_delete_listeners(ctx_, ids.data() + at, nw - at < 512u ? nw - at : 512u, &part) != GYS_OK) return -1;
					nd += part;
				}
				total += nd;
				if (nfound <= ids.size() || !nd) break;
			}
		} catch (...) {
			return -1;
		}
		return total;
	}

	// ---- service records ("service records" in gysketch.h): what the reference keeps in Postgres and re-seeds after a restart
	// (handle_listener_req, server/gy_mconnhdlr.cc:14257) lives in device memory here; these calls copy it out and back in.
	// One partha's listeners as a blob: a partha that moves to another rank takes this with it (restore_services there, delete_listeners here).
	bool save_partha_services(const uint8_t machine_id[16], std::vector<uint8_t> &blob) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		try {
			uint32_t n = 0;
			if (gys_list_host_service_ids(ctx_, machine_id, nullptr, 0, &n) != GYS_OK) return false;
			std::vector<uint64_t> ids(n ? n : 1);
			if (gys_list_host_service_ids(ctx_, machine_id, ids.data(), n, &n) != GYS_OK) return false;
			blob.resize(gys_service_blob_bytes(ctx_, n));
			return gys_pack_services(ctx_, ids.data(), n, blob.data(), blob.size()) == GYS_OK;
		} catch (...) {
			return false;
		}
	}
	// a blob into the listeners registered here (the others are counted in *nskipped); the state of the applied ones is overwritten
	bool restore_services(const void *blob, size_t nbytes, uint32_t *napplied = nullptr, uint32_t *nskipped = nullptr) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_unpack_services(ctx_, blob, nbytes, napplied, nskipped) == GYS_OK;
	}
	// every registered listener to a file: blobs of at most 64 MB over ranges of slots, each behind its length (u64, little-endian).  The
	// file is written beside `path` (path + ".tmp") and renamed over it when it is complete and flushed: a crash or a failed pack in the
	// middle of a periodic save leaves the previous checkpoint as it was.  The exclusive lock is held for the whole save -- every blob of a
	// file has to carry the same window number and close times (a close between two ranges would make load_all refuse the later ones) -- so
	// ingest calls wait for its duration: save right behind send_cluster_state, to a local disk.
	bool save_all(const char *path, uint64_t *nservices = nullptr) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		FILE *f = nullptr;
		bool ok = false;
		std::string tmp;
		try {
			tmp = std::string(path) + ".tmp";
			const uint64_t one = gys_service_blob_bytes(ctx_, 1) - 64u, fit = ((64ull << 20) - 64u) / (one ? one : 1); // (header 64, id 8 + pad, record)
			const uint32_t per = (uint32_t)(fit ? fit : 1);
			std::vector<uint64_t> ids(per);
			std::vector<uint8_t> blob;
			uint64_t total = 0;
			f = fopen(tmp.c_str(), "wb");
			ok = f != nullptr;
			for (uint32_t first = 0, nsvc = gys_num_services(ctx_); ok && first < nsvc; first += per) {
				uint32_t n = 0;
				ok = gys_list_service_ids(ctx_, first, per, ids.data(), &n) == GYS_OK;
				if (!ok || !n) continue;
				blob.resize(gys_service_blob_bytes(ctx_, n));
				const uint64_t len = blob.size();
				ok = gys_pack_services(ctx_, ids.data(), n, blob.data(), len) == GYS_OK && fwrite(&len, 8, 1, f) == 1 && fwrite(blob.data(), 1, len, f) == len;
				total += n;
			}
			if (ok) ok = fflush(f) == 0;
			if (nservices) *nservices = total;
		} catch (...) {
			ok = false;
		}
		if (f && fclose(f) != 0) ok = false;
		if (ok) ok = rename(tmp.c_str(), path) == 0;
		if (!ok && !tmp.empty()) (void)remove(tmp.c_str());
		return ok;
	}
	// ... and back, after the hosts and listeners have been registered again; a fresh context continues the file's window count and ring times
	bool load_all(const char *path, uint64_t *napplied = nullptr, uint64_t *nskipped = nullptr) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		FILE *f = nullptr;
		bool ok = false;
		try {
			std::vector<uint8_t> blob;
			uint64_t na = 0, ns = 0, len = 0;
			f = fopen(path, "rb");
			ok = f != nullptr;
			while (ok && fread(&len, 8, 1, f) == 1) {
				ok = len >= 64u && len <= (64ull << 20) + 64u;
				if (!ok) break;
				blob.resize(len);
				uint32_t a = 0, s = 0;
				ok = fread(blob.data(), 1, len, f) == len && gys_unpack_services(ctx_, blob.data(), len, &a, &s) == GYS_OK;
				na += a;
				ns += s;
			}
			if (ok) ok = feof(f) != 0;
			if (napplied) *napplied = na;
			if (nskipped) *nskipped = ns;
		} catch (...) {
			ok = false;
		}
		if (f) fclose(f);
		return ok;
	}

	// MCONN_HANDLER::partha_tcp_conn_info: pone points into the L1 receive buffer, valid only during the call
	bool partha_tcp_conn_info(const uint8_t machine_id[16], const void *pone, int nconns, const uint8_t *pendptr) noexcept
	{
		if (!pone || nconns < 0) return false;
		std::shared_lock<std::shared_mutex> g(mu_); // up to 16 L2 threads call concurrently (gy_mconnhdlr.h:60); one context == one stream
		return gys_ingest_tcp_conn(ctx_, machine_id, pone, (uint32_t)nconns, pendptr) == GYS_OK;
	}

	// MCONN_HANDLER::partha_listener_state
	bool partha_listener_state(const uint8_t machine_id[16], const void *pone, int nconns, const uint8_t *pendptr) noexcept
	{
		if (!pone || nconns < 0) return false;
		std::shared_lock<std::shared_mutex> g(mu_);
		return gys_ingest_listener_state(ctx_, machine_id, pone, (uint32_t)nconns, pendptr) == GYS_OK;
	}

	// L1 + L2 in one step for a partha connection's receive buffer: COMM_HEADER-framed messages, records decoded on the GPU
	// (MCONN_HANDLER::handle_l1 -> handle_l2_misc dispatch, gy_mconnhdlr.cc:4700-4792).  nconsumed: whole messages consumed.
	bool handle_partha_stream(const uint8_t machine_id[16], const void *pbuf, uint64_t nbytes, uint64_t *nconsumed = nullptr) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		gys_comm_stats st{};
		const bool ok = gys_ingest_comm_stream(ctx_, machine_id, pbuf, nbytes, &st) == GYS_OK;
		if (nconsumed) *nconsumed = st.bytes_consumed;
		return ok;
	}

	// MCONN_HANDLER::handle_partha_active_conns (gy_mconnhdlr.cc:7705-7772, L2 dispatch :5244): a partha's 15-s ACTIVE_CONN_STATS rows
	bool handle_partha_active_conns(const uint8_t machine_id[16], const void *pconn, int nitems, const uint8_t *pendptr) noexcept
	{
		if (!pconn || nitems < 0) return false;
		std::shared_lock<std::shared_mutex> g(mu_);
		return gys_ingest_active_conns(ctx_, machine_id, pconn, (uint32_t)nitems, pendptr) == GYS_OK;
	}

	// comm::HOST_STATE_NOTIFY store read by send_cluster_state (gy_mconnhdlr.cc:16052-16075)
	bool partha_host_state(const uint8_t machine_id[16], const gys_host_state &st) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_ingest_host_state(ctx_, machine_id, &st) == GYS_OK;
	}

	// TCP_SOCK_HANDLER::handle_ipv4_resp_event for a batch of raw 24-byte events of one host
	bool handle_ipv4_resp_events(const uint8_t machine_id[16], const void *pevents, uint32_t nevents) noexcept
	{
		std::shared_lock<std::shared_mutex> g(mu_);
		return gys_ingest_resp_events(ctx_, machine_id, pevents, nevents) == GYS_OK;
	}

	// TCP_SOCK_HANDLER::handle_ipv6_resp_event (gy_socket_stat.cc:1535) for a batch of raw 48-byte tcp_ipv6_resp_event_t of one host
	bool handle_ipv6_resp_events(const uint8_t machine_id[16], const void *pevents, uint32_t nevents) noexcept
	{
		std::shared_lock<std::shared_mutex> g(mu_);
		return gys_ingest_resp_events_v6(ctx_, machine_id, pevents, nevents) == GYS_OK;
	}

	// MCONN_HANDLER::send_cluster_state (scheduled every 5000 ms, gy_mconnhdlr.cc:207-210) + the shyama-side aggregation
	void send_cluster_state(uint64_t tusec, const ReduceFn &reduce = {}) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		if (gys_window_prepare(ctx_, tusec) != GYS_OK) return;
		if (reduce) {
			gys_reduce_section secs[4];
			uint32_t n = 0;
			if (gys_reduce_sections(ctx_, secs, &n) == GYS_OK) (void)reduce(secs, n);
		}
		(void)gys_window_finish(ctx_);
	}

	// The multi-GPU form: one process per GPU, every rank joins the communicator once (rank 0 makes the id with gys_rccl_unique_id and
	// hands the 128 bytes to the others over whatever channel the deployment has) and then closes every window with the four
	// register families all-reduced over xGMI INSIDE the library (ncclAllReduce x 4 in one ncclGroup on the context stream).
	bool join_cluster(const uint8_t uid[GYS_RCCL_UID_BYTES], int nranks, int rank) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_rccl_comm_create(ctx_, uid, nranks, rank, &comm_) == GYS_OK;
	}
	void send_cluster_state_rccl(uint64_t tusec) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		if (comm_) (void)gys_window_close_rccl(ctx_, comm_, tusec);
	}

	// web_curr_listener_summ: LISTEN_SUMM_STATS<int> of one partha (fields map 1:1 onto svcsumm JSON, gy_mfields.h:768-790)
	bool get_listener_summ(const uint8_t machine_id[16], gys_svcsumm &out) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_query_svcsumm(ctx_, machine_id, &out) == GYS_OK;
	}
	bool get_cluster_state(const char *cluster, gys_cluster_state &out) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_query_clusterstate(ctx_, cluster, &out) == GYS_OK;
	}

	// RESP_TIME_HISTOGRAM::get_stats_with_flush of one listener on one time level (Level_5s_5min_5days_all index 0..3;
	// common/gy_statistics.h:1333-1374); needs gys_config.enable_levels
	int get_resp_level_stats(uint64_t glob_id, int level, time_t tnow, gys_time_hist_val *pstats, size_t nstats, int64_t &tcount, int64_t &tsum,
				 double &mean_val) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_query_hist_level_stats(ctx_, glob_id, level, (uint64_t)tnow * 1000000ull, pstats, (uint32_t)nstats, &tcount, &tsum, &mean_val) == GYS_OK
			       ? 0
			       : -1;
	}

	// RESP_TIME_HISTOGRAM::get_stats_for_period_with_flush of one listener (common/gy_statistics.h:1378-1413)
	int get_resp_period_stats(uint64_t glob_id, time_t starttime, time_t endtime, gys_time_hist_val *pstats, size_t nstats, int64_t &tcount, int64_t &tsum,
				  double &mean_val, time_t tnow = time(nullptr)) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_query_hist_period_stats(ctx_, glob_id, (int64_t)starttime, (int64_t)endtime, (uint64_t)tnow * 1000000ull, pstats, (uint32_t)nstats,
						   &tcount, &tsum, &mean_val) == GYS_OK
			       ? 0
			       : -1;
	}

	// the same question asked of every host / cluster / this madhava (scope: GYS_ROLLUP_*): the sum of the listeners' period records, one
	// record per group on the device (percentiles through gys_hist_percentiles_dev); *level_used = the level that answered (may be nullptr)
	bool aggr_resp_period_hist(int scope, time_t starttime, time_t endtime, gys_hist_rec *d_out, int *level_used = nullptr, time_t tnow = time(nullptr)) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_); // (a query: not concurrent with ingest calls)
		return gys_hist_rollup_period_dev(ctx_, scope, (int64_t)starttime, (int64_t)endtime, (uint64_t)tnow * 1000000ull, d_out, level_used) == GYS_OK;
	}

	// the NOTIFY_LISTENER_DAY_STATS payload (comm::LISTENER_DAY_STATS[], MAX_NUM_LISTENERS = 2048 per message) for service slots
	// [first_slot, first_slot + nslots), as TCP_LISTENER::get_curr_state fills it (common/gy_socket_stat.cc:2098-2112)
	bool listener_day_stats(time_t tnow, uint32_t first_slot, uint32_t nslots, gys_listener_day_stats *pout) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_export_day_stats(ctx_, (uint64_t)tnow * 1000000ull, first_slot, nslots, pout) == GYS_OK;
	}

	// LISTENER_DAY_STATS of every host / cluster / this madhava (scope: GYS_ROLLUP_*), glob_id_ = the group index; records on the device
	bool aggr_day_stats(int scope, time_t tnow, gys_listener_day_stats *d_out) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_day_stats_rollup_dev(ctx_, scope, (uint64_t)tnow * 1000000ull, d_out) == GYS_OK;
	}

	// the same answers as the reference's web JSON (web_curr_listener_summ / web_curr_listener_state / web_curr_clusterstate)
	bool web_curr_listener_summ(const uint8_t machine_id[16], const char *madid, const char *timestr, std::string &out) noexcept
	{
		return json_call(out, [&](char *b, size_t n, size_t *need) { return gys_json_svcsumm(ctx_, machine_id, madid, timestr, b, n, need); });
	}
	bool web_curr_listener_state(const uint8_t machine_id[16], const char *madid, const char *timestr, std::string &out) noexcept
	{
		return json_call(out, [&](char *b, size_t n, size_t *need) { return gys_json_svcstate(ctx_, machine_id, madid, timestr, b, n, need); });
	}
	// MCONN_HANDLER::web_curr_listener_state with QUERY_OPTIONS (server/gy_mnodehandle.cc:4650-4900; common/gy_query_common.h:24-140): the
	// multi-host form -- criteria on the numeric svcstate columns (filter: groups of terms as CRITERIA_SET holds them, nullptr = none),
	// one sort column (GYS_SVC_COL_*, -1 = service order), maxrecs; one pass over the kept states of every listener on the device
	bool web_curr_listener_state_multihost(const gys_svc_filter *filter, int sort_col, bool sort_desc, uint32_t maxrecs, const char *madid,
					       const char *timestr, std::string &out) noexcept
	{
		return json_call(out, [&](char *b, size_t n, size_t *need) {
			return gys_json_svcstate_multihost(ctx_, filter, sort_col, sort_desc ? 1 : 0, maxrecs, madid, timestr, b, n, need);
		});
	}
	// MCONN_HANDLER::web_curr_listener_summ, multi-host form (server/gy_mnodehandle.cc:1628-1690): every partha with a recent listener state
	// whose LISTEN_SUMM_STATS row passes the criteria (terms name GYS_SUMM_COL_*)
	bool web_curr_listener_summ_multihost(const gys_svc_filter *filter, int sort_col, bool sort_desc, uint32_t maxrecs, const char *madid,
					      const char *timestr, std::string &out) noexcept
	{
		return json_call(out, [&](char *b, size_t n, size_t *need) {
			return gys_json_svcsumm_multihost(ctx_, filter, sort_col, sort_desc ? 1 : 0, maxrecs, madid, timestr, b, n, need);
		});
	}
	// AOPER_PERCENTILE of one column over the matching listeners (discrete percentiles, exact)
	bool aggr_listener_state_percentiles(const gys_svc_filter *filter, int col, const double *pcts, uint32_t npcts, int64_t *out, uint64_t *nmatched) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_query_svcstate_percentiles(ctx_, filter, col, pcts, npcts, out, nmatched) == GYS_OK;
	}
	// a string criterion on the service name ({ svcstate.name like 'post' }: CRITERION_ONE::match_str_criterian common/gy_query_criteria.h:1335-1383)
	// resolved into the service ids a filter's `svcids` takes; comp = GYS_COMP_EQ / NEQ / SUBSTR / NOTSUBSTR / LIKE / NOTLIKE / IN / NOTIN
	bool svc_ids_by_name(int comp, const std::vector<std::string> &patterns, std::vector<uint64_t> &ids) noexcept
	{
		try {
			std::shared_lock<std::shared_mutex> g(mu_);
			std::vector<const char *> p;
			for (const auto &s : patterns) p.push_back(s.c_str());
			uint32_t n = 0;
			ids.resize(1024);
			int rc = gys_svc_ids_by_name(ctx_, comp, p.data(), (uint32_t)p.size(), ids.data(), (uint32_t)ids.size(), &n);
			if (rc == GYS_ERR_NOMEM) {
				ids.resize(n);
				rc = gys_svc_ids_by_name(ctx_, comp, p.data(), (uint32_t)p.size(), ids.data(), (uint32_t)ids.size(), &n);
			}
			if (rc != GYS_OK) return false;
			ids.resize(n);
			return true;
		} catch (...) {
			return false;
		}
	}
	// ... on the host name ({ svcstate.host substr 'db' }): the machine ids (16 bytes each) a filter's `machine_ids` takes
	bool machine_ids_by_hostname(int comp, const std::vector<std::string> &patterns, std::vector<uint8_t> &ids16) noexcept
	{
		try {
			std::shared_lock<std::shared_mutex> g(mu_);
			std::vector<const char *> p;
			for (const auto &s : patterns) p.push_back(s.c_str());
			uint32_t n = 0;
			ids16.resize(16 * 256);
			int rc = gys_machine_ids_by_hostname(ctx_, comp, p.data(), (uint32_t)p.size(), ids16.data(), (uint32_t)(ids16.size() / 16), &n);
			if (rc == GYS_ERR_NOMEM) {
				ids16.resize((size_t)16 * n);
				rc = gys_machine_ids_by_hostname(ctx_, comp, p.data(), (uint32_t)p.size(), ids16.data(), n, &n);
			}
			if (rc != GYS_OK) return false;
			ids16.resize((size_t)16 * n);
			return true;
		} catch (...) {
			return false;
		}
	}
	// the aggregation operators (AGGR_OPER_E, common/gy_json_field_maps.h:114-129) over the matching listeners: group_by 0 all / 1 host / 2 cluster
	bool aggr_listener_state(const gys_svc_filter *filter, int group_by, const uint8_t *cols, uint32_t ncols, gys_svc_aggr_row *out, uint32_t maxrows,
				 uint32_t *nrows) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_); // (a query: not concurrent with ingest calls)
		return gys_query_svcstate_aggr(ctx_, filter, group_by, cols, ncols, out, maxrows, nrows) == GYS_OK;
	}
	// the aggregated response-time digest / distinct-flow count of the listeners a filter selects, per group (the WHERE + GROUP BY of
	// public.tdigest_percentile over listeners' rows, common/gy_query_common.cc:1818-1855): rows on the host, slabs / files / estimates on the device
	bool aggr_listener_sketches(const gys_svc_filter *filter, uint32_t flags, int group_by, int hll_level, time_t tnow, gys_rollup_row *rows, uint32_t maxrows,
				    uint32_t *nrows, gys_tdigest_slab *d_slabs, uint8_t *d_regs, double *d_est) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_); // (a query: not concurrent with ingest calls)
		return gys_rollup_filtered_dev(ctx_, filter, flags, group_by, hll_level, (uint64_t)tnow * 1000000ull, rows, maxrows, nrows, d_slabs, d_regs, d_est) == GYS_OK;
	}
	// the response-time histogram of every host / cluster / this madhava at one of the 5 s / 5 min / 5 days / all levels (the sum of the
	// listeners' level records: GY_HISTOGRAM::add_histogram, common/gy_statistics.h:625-660), and of the listeners a filter selects, per group;
	// records on the device, percentiles through gys_hist_percentiles_dev
	bool aggr_resp_hist_level(int scope, int level, time_t tnow, gys_hist_rec *d_out) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_); // (a query: not concurrent with ingest calls)
		return gys_hist_rollup_level_dev(ctx_, scope, level, (uint64_t)tnow * 1000000ull, d_out) == GYS_OK;
	}
	bool aggr_listener_resp_hist(const gys_svc_filter *filter, uint32_t flags, int group_by, int level, time_t tnow, gys_rollup_row *rows, uint32_t maxrows, uint32_t *nrows,
				     gys_hist_rec *d_recs) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_hist_rollup_filtered_dev(ctx_, filter, flags, group_by, level, (uint64_t)tnow * 1000000ull, rows, maxrows, nrows, d_recs) == GYS_OK;
	}
	// MCONN_HANDLER::web_curr_top_listeners (server/gy_mnodehandle.cc:2706-3190): machine_id = one partha's four top-10 queues,
	// nullptr = every host's queues merged into MAX_MULTI_TOPN = 50 slots per kind; flags: GYS_TOP_* (which arrays to send)
	bool web_curr_top_listeners(const uint8_t *machine_id, uint32_t flags, const char *madid, const char *timestr, std::string &out) noexcept
	{
		return json_call(out, [&](char *b, size_t n, size_t *need) { return gys_json_toplisteners(ctx_, machine_id, flags, madid, timestr, b, n, need); });
	}
	// TCP_SOCK_HANDLER::listener_stats_update (common/gy_socket_stat.cc:3895-4380): the 5-s walk over every listener, from the engine's
	// own state: d_notify = device buffer of 88 B x services (LISTENER_STATE_NOTIFY records, ready for partha_listener_state's device
	// form), d_scan = gys_listener_scan x services; either may be nullptr.  Needs gys_config.enable_levels.
	bool listener_stats_update(time_t tnow, float qps_multiple, uint32_t diffsec, void *d_notify, gys_listener_scan *d_scan) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_scan_listener_state_dev(ctx_, (uint64_t)tnow * 1000000ull, qps_multiple, diffsec, d_notify, d_scan) == GYS_OK;
	}
	// TCP_LISTENER::get_curr_state for every listener (common/gy_socket_stat.cc:2020-2870, called at :4241) + the caller's history byte and
	// "just started" rule (:4244-4266): d_scan as listener_stats_update left it, d_issue_in = the task / host inputs per service slot (nullptr:
	// none), curr_state_ / curr_issue_ / issue_bit_hist_ / high_resp_bit_hist_ patched into d_notify, the decisions into d_out (either may be nullptr)
	bool listener_curr_states(const gys_listener_scan *d_scan, const gys_listener_issue_in *d_issue_in, void *d_notify, gys_listener_decision *d_out) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		return gys_decide_listener_state_dev(ctx_, d_scan, d_issue_in, d_notify, d_out) == GYS_OK;
	}
	bool web_curr_clusterstate(const char *shyamaid, const char *timestr, std::string &out) noexcept
	{
		return json_call(out, [&](char *b, size_t n, size_t *need) { return gys_json_clusterstate(ctx_, shyamaid, timestr, b, n, need); });
	}

private:
	template <typename F>
	bool json_call(std::string &out, F &&f) noexcept
	{
		std::unique_lock<std::shared_mutex> g(mu_);
		try {
			size_t need = 0;
			int rc = f(nullptr, 0, &need);
			if (rc != GYS_OK && rc != GYS_ERR_NOMEM) return false;
			out.resize(need + 1);
			rc = f(out.data(), out.size(), &need);
			out.resize(need);
			return rc == GYS_OK;
		} catch (...) {
			return false;
		}
	}

	gys_ctx *ctx_ = nullptr;
	void *comm_ = nullptr; // ncclComm_t
	std::shared_mutex mu_; // ingest calls share it (thread-safe among themselves inside the library); registration, window close and queries are exclusive
};

} // namespace gyeeta_amd
